"""Variable-base scalar multiplication over Pallas in bulk (halo2_amd/csrc/ecc.hip): n independent products [k_i]P_i, and the
witness of the ECC chip's variable-base `mul` (halo2_gadgets ecc/chip/mul.rs) for many multiplications at once.

Points are arrays of uint64 Montgomery limbs, (..., 8), the identity (0, 0); scalars of `mul` are CANONICAL integers of 4 limbs below
2^255; the alphas of `mul_trace` are Montgomery elements of Fp, as cells are.  A CUDA int64 tensor is used in place and a CUDA tensor
comes back; a numpy array is uploaded and a numpy array comes back."""
from __future__ import annotations

import numpy as np

from . import fields
from ._lib import check, lib
from .arithmetic import _is_torch, _stream_ptr

__all__ = ["ROWS", "AUX", "mul", "mul_trace", "OffCurve", "Vanishing"]

ROWS = 137                                      # rows of the region "variable-base scalar mul" (mul.rs:164-293)
AUX = 16                                        # s, the 14 running sums of its range check, eta (mul/overflow.rs:101-208)


class OffCurve(ValueError):
    """A base of `mul` is neither the identity nor a point of the curve."""


class Vanishing(ValueError):
    """A multiplication of `mul_trace` has no witness: its base is the identity, or a denominator of the incomplete range vanished
    (the reference's Error::Synthesis; no point of the curve does that)."""


def _ptr(t):
    return t.data_ptr() if t.numel() else None


def _device(a, width, what):
    import torch
    host = not _is_torch(a)
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(fields.current_device()) if host else a.contiguous()
    if t.ndim != 2 or t.shape[1] != width or t.dtype != torch.int64 or not t.is_cuda:
        raise ValueError(f"{what}: an (n, {width}) array of uint64 limbs")
    return t, host


def _raise(status, error, what):
    bad = status.nonzero().flatten()
    if bad.numel():
        raise error(f"{what}: entry {int(bad[0])} ({bad.numel()} of {status.numel()})")


def mul(bases, scalars, with_status: bool = False):
    """[k_i]P_i: bases (n, 8) Montgomery affine, scalars (n, 4) canonical and below 2^255 -> (n, 8).  Complete: k = 0, k = q and the
    identity base give the identity.  A base off the curve raises `OffCurve`; with_status: returns (points, status) instead."""
    import torch
    b, host = _device(bases, 8, "ecc.mul bases")
    k, host_k = _device(scalars, 4, "ecc.mul scalars")
    if b.shape[0] != k.shape[0] or host != host_k:
        raise ValueError("ecc.mul: as many scalars as bases, both of one kind")
    n = b.shape[0]
    out = torch.empty((n, 8), dtype=torch.int64, device=b.device)
    status = torch.empty((n,), dtype=torch.uint8, device=b.device)
    check(lib().h2_ecc_mul_device(_ptr(b), _ptr(k), n, _ptr(out), _ptr(status), _stream_ptr()), "h2_ecc_mul_device")
    if with_status:
        return (out.cpu().numpy().view(np.uint64), status.cpu().numpy()) if host else (out, status)
    _raise(status, OffCurve, "ecc.mul: a base off the curve")
    return out.cpu().numpy().view(np.uint64) if host else out


def mul_trace(bases, alphas, with_status: bool = False):
    """What EccChip.mul witnesses for `count` pairs: bases (count, 8), alphas (count, 4) Montgomery elements of Fp ->
    (columns, aux): columns (10, ROWS * count, 4), the chip's ten advice columns with multiplication i in rows ROWS i .., zero where the
    reference assigns nothing; aux (count, 16, 4) (see include/halo2_mi355x.h).  A multiplication without a witness raises `Vanishing`;
    with_status: returns (columns, aux, status) instead."""
    import torch
    b, host = _device(bases, 8, "ecc.mul_trace bases")
    a, host_a = _device(alphas, 4, "ecc.mul_trace alphas")
    if b.shape[0] != a.shape[0] or host != host_a:
        raise ValueError("ecc.mul_trace: as many alphas as bases, both of one kind")
    count = b.shape[0]
    columns = torch.empty((10, ROWS * count, 4), dtype=torch.int64, device=b.device)
    aux = torch.empty((count, AUX, 4), dtype=torch.int64, device=b.device)
    status = torch.empty((count,), dtype=torch.uint8, device=b.device)
    check(lib().h2_ecc_mul_trace_device(_ptr(b), _ptr(a), count, _ptr(columns), _ptr(aux), _ptr(status), _stream_ptr()),
          "h2_ecc_mul_trace_device")
    if host:
        columns, aux = columns.cpu().numpy().view(np.uint64), aux.cpu().numpy().view(np.uint64)
    if with_status:
        return columns, aux, status.cpu().numpy() if host else status
    _raise(status, Vanishing, "ecc.mul_trace: no witness for")
    return columns, aux
