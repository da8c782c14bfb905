"""Poseidon P128Pow5T3 over the Pasta fields in bulk (halo2_amd/csrc/poseidon.hip): the hash a circuit's user reaches for outside the
circuit too -- the leaves and nodes of a Merkle tree, nullifiers, commitments to a witness -- and the witness of the Pow5 chip.

Every argument is an array of (..., 4) uint64 Montgomery limbs: a CUDA int64 tensor is used in place and a CUDA tensor comes back;
a numpy array is uploaded and a numpy array comes back.  `field` is FP or FQ.  The constants are `halo2_amd.poseidon_spec`'s.

Any other specification is a `Spec(field, width, rate, ...)` (halo2_amd/poseidon_spec.py, halo2_amd/csrc/poseidon_spec.hip) with the same
four as methods and the same array conventions, `width` words a state; its table of constants is uploaded once per device and kept
by the Spec."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import fields
from ._lib import PoseidonSpec, check, lib
from .arithmetic import _is_torch, _stream_ptr
from .poseidon_spec import ROWS, WIDTH, Spec

__all__ = ["permute", "hash", "trace", "merkle_root", "Spec"]


def _device(a, tail, what):
    """-> (contiguous int64 CUDA tensor of shape (n,) + tail, came from numpy?); None in `tail` is any length"""
    import torch
    host = not _is_torch(a)
    if host:
        a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(fields.current_device())
    shape_ok = a.ndim == 1 + len(tail) and all(want in (None, got) for want, got in zip(tail, a.shape[1:]))
    if a.dtype != torch.int64 or not a.is_cuda or not shape_ok:
        raise ValueError(f"{what}: expected an (n, {', '.join('len' if t is None else str(t) for t in tail)}) array of Montgomery limbs")
    return a.contiguous(), host


def _back(t, host):
    return t.cpu().numpy().view(np.uint64) if host else t


def _ptr(t):
    return t.data_ptr() if t.numel() else None


def permute(states, field: int, out=None):
    """The permutation of n states: (n, 3, 4) -> (n, 3, 4).  torch: `out` may be `states` itself (in place)."""
    import torch
    s, host = _device(states, (WIDTH, 4), "poseidon.permute")
    res = torch.empty_like(s) if out is None else out
    if out is not None and (not _is_torch(out) or out.shape != s.shape or out.dtype != torch.int64 or not out.is_contiguous()):
        raise ValueError("poseidon.permute: out is a contiguous int64 tensor of the states' shape")
    check(lib().h2_poseidon_permute_device(field, _ptr(s), s.shape[0], _ptr(res), _stream_ptr()), "h2_poseidon_permute_device")
    return _back(res, host)


def hash(messages, field: int):                                               # noqa: A001 -- the reference's name
    """Hash<_, P128Pow5T3, ConstantLength<len>, 3, 2> of n messages of `len` elements: (n, len, 4) -> (n, 4)."""
    import torch
    m, host = _device(messages, (None, 4), "poseidon.hash")
    if m.shape[1] == 0:
        raise ValueError("poseidon.hash: a message has at least one element")
    res = torch.empty((m.shape[0], 4), dtype=torch.int64, device=m.device)
    check(lib().h2_poseidon_hash_device(field, _ptr(m), m.shape[0], m.shape[1], _ptr(res), _stream_ptr()), "h2_poseidon_hash_device")
    return _back(res, host)


def trace(states, field: int):
    """The Pow5 chip's witness of `count` permutations: (count, 3, 4) -> (4, 37 * count, 4), the columns state0, state1, state2 and
    partial_sbox.  Permutation i owns rows 37 i .. 37 i + 36: its input on row 0, its output on row 36 (see include/halo2_mi355x.h)."""
    import torch
    s, host = _device(states, (WIDTH, 4), "poseidon.trace")
    res = torch.empty((WIDTH + 1, ROWS * s.shape[0], 4), dtype=torch.int64, device=s.device)
    check(lib().h2_poseidon_trace_device(field, _ptr(s), s.shape[0], _ptr(res), _stream_ptr()), "h2_poseidon_trace_device")
    return _back(res, host)


def merkle_root(leaves, field: int):
    """The root of the binary tree over a power-of-two number of leaves, a node being hash(left, right): (n, 4) -> (4,).  One `hash`
    launch per layer; every layer stays on the device."""
    t, host = _device(leaves, (4,), "poseidon.merkle_root")
    n = t.shape[0]
    if n == 0 or n & (n - 1):
        raise ValueError("poseidon.merkle_root: a power-of-two number of leaves")
    while t.shape[0] > 1:
        t = hash(t.view(t.shape[0] // 2, 2, 4), field)
    return _back(t[0], host)


# ---- any Spec (halo2_amd/csrc/poseidon_spec.hip): the bodies of Spec.permute / hash / trace / merkle_root --------------------------------------
def spec_constants(spec: Spec, device):
    """The table the spec kernels read, on `device`: (rounds * width + width * width, 4) Montgomery limbs, the round constants and then
    the MDS matrix row-major.  Uploaded once per device and kept by the Spec; the library holds none of it."""
    import torch
    device = torch.device(device)
    table = spec._device_constants.get(device)
    if table is None:
        flat = [c for row in spec.round_constants for c in row] + [c for row in spec.mds for c in row]
        table = torch.from_numpy(fields.to_limbs(flat, spec.field, True).view(np.int64)).to(device)
        spec._device_constants[device] = table
    return table


def spec_descriptor(spec: Spec, device, stream=None) -> PoseidonSpec:
    """h2_poseidon_spec_t for `spec` with its table on `device`; the stream is torch's current one unless given."""
    return PoseidonSpec(spec.field, spec.width, spec.rate, spec.full_rounds, spec.partial_rounds,
                        spec_constants(spec, device).data_ptr(), _stream_ptr().value if stream is None else stream)


def spec_permute(spec: Spec, states, out=None):
    import torch
    s, host = _device(states, (spec.width, 4), "Spec.permute")
    res = torch.empty_like(s) if out is None else out
    if out is not None and (not _is_torch(out) or out.shape != s.shape or out.dtype != torch.int64 or not out.is_contiguous()):
        raise ValueError("Spec.permute: out is a contiguous int64 tensor of the states' shape")
    d = spec_descriptor(spec, s.device)
    check(lib().h2_poseidon_spec_permute_device(C.byref(d), _ptr(s), s.shape[0], _ptr(res)), "h2_poseidon_spec_permute_device")
    return _back(res, host)


def spec_hash(spec: Spec, messages):
    import torch
    m, host = _device(messages, (None, 4), "Spec.hash")
    if m.shape[1] == 0:
        raise ValueError("Spec.hash: a message has at least one element")
    res = torch.empty((m.shape[0], 4), dtype=torch.int64, device=m.device)
    d = spec_descriptor(spec, m.device)
    check(lib().h2_poseidon_spec_hash_device(C.byref(d), _ptr(m), m.shape[0], m.shape[1], _ptr(res)), "h2_poseidon_spec_hash_device")
    return _back(res, host)


def spec_trace(spec: Spec, states):
    import torch
    if spec.partial_rounds % 2:
        raise ValueError("Spec.trace: the Pow5 chip lays two partial rounds on a row; partial_rounds is even")
    s, host = _device(states, (spec.width, 4), "Spec.trace")
    res = torch.empty((spec.width + 1, spec.rows * s.shape[0], 4), dtype=torch.int64, device=s.device)
    d = spec_descriptor(spec, s.device)
    check(lib().h2_poseidon_spec_trace_device(C.byref(d), _ptr(s), s.shape[0], _ptr(res)), "h2_poseidon_spec_trace_device")
    return _back(res, host)


def spec_merkle_root(spec: Spec, leaves, arity=None):
    """One `hash` launch per layer; every layer stays on the device."""
    arity = spec.rate if arity is None else arity
    t, host = _device(leaves, (4,), "Spec.merkle_root")
    n = t.shape[0]
    if arity < 2:
        raise ValueError("Spec.merkle_root: an arity of at least 2")
    size = 1
    while size < n:
        size *= arity
    if n == 0 or size != n:
        raise ValueError("Spec.merkle_root: a power of the arity as the number of leaves")
    while t.shape[0] > 1:
        t = spec_hash(spec, t.view(t.shape[0] // arity, arity, 4))
    return _back(t[0], host)
