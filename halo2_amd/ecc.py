"""Scalar multiplication over Pallas in bulk.  Variable base (halo2_amd/csrc/ecc.hip): n independent products [k_i]P_i, and the
witness of the ECC chip's variable-base `mul` (halo2_gadgets ecc/chip/mul.rs) for many multiplications at once.  Fixed base
(halo2_amd/csrc/ecc_fixed.hip): `FixedBase` builds a base's window table, Lagrange coefficients, z and u on the device
(ecc/chip/constants.rs), `mul_fixed`, `mul_fixed_short` and `mul_fixed_trace` multiply and witness over them (ecc/chip/mul_fixed.rs).

Points are arrays of uint64 Montgomery limbs, (..., 8), the identity (0, 0); scalars of `mul` are CANONICAL integers of 4 limbs below
2^255; the alphas of `mul_trace` are Montgomery elements of Fp, as cells are.  A CUDA int64 tensor is used in place and a CUDA tensor
comes back; a numpy array is uploaded and a numpy array comes back.

`mul_fixed_short_trace` and `mul_fixed_base_field_trace` (halo2_amd/csrc/ecc_fixed_sum.hip) witness the two fixed-base forms whose
scalar is a running sum (mul_fixed/short.rs, mul_fixed/base_field_elem.rs); their inputs are CANONICAL elements of Fp and the
inverses' scratch is a tensor of the call's own.

`add` and `add_trace` are the group's complete addition in bulk (halo2_amd/csrc/sinsemilla_commit.hip, ecc/chip/add.rs): n sums
P_i + Q_i, and the nine cells the chip witnesses for each."""
from __future__ import annotations

import numpy as np

from . import fields
from ._lib import check, lib
from .arithmetic import _is_torch, _stream_ptr, scale_add

__all__ = ["ROWS", "AUX", "mul", "mul_trace", "OffCurve", "Vanishing",
           "NUM_WINDOWS", "NUM_WINDOWS_SHORT", "FIXED_AUX", "FixedBase", "mul_fixed", "mul_fixed_short", "mul_fixed_trace",
           "add", "add_trace", "SHORT_AUX", "BASE_FIELD_AUX", "SUM_SCRATCH_LANES", "mul_fixed_short_trace", "mul_fixed_base_field_trace"]

ROWS = 137                                      # rows of the region "variable-base scalar mul" (mul.rs:164-293)
AUX = 16                                        # s, the 14 running sums of its range check, eta (mul/overflow.rs:101-208)
NUM_WINDOWS, NUM_WINDOWS_SHORT = 85, 22         # 3-bit windows of a full-width and of a 64-bit scalar (constants.rs:18-23)
FIXED_AUX = 11                                  # the complete addition's nine cells and the product (add.rs:213-295)
SHORT_AUX, BASE_FIELD_AUX = 12, 15              # FIXED_AUX and the signed y; FIXED_AUX and alpha_0', alpha_1, alpha_2, alpha_0' canonical
SUM_SCRATCH_LANES = 1 << 16                     # multiplications per chunk of a running-sum trace: 174 MB of inverses at 85 windows


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


class FixedBase:
    """The four tables of a fixed base over its 3-bit windows (constants.rs: compute_window_table, compute_lagrange_coeffs,
    find_zs_and_us), built once on the device and kept there: `points` (num_windows, 8, 8) Montgomery affine, `lagrange`
    (num_windows, 8, 4), `zs` (num_windows,) and `us` (num_windows, 8, 4), int64 CUDA tensors.  base_xy: 8 uint64 Montgomery limbs,
    a point of the curve.  z_limit: the exclusive bound on the z searched, 0 for the reference's 1000 * 2^16; a window without one
    raises `_lib.NotFound`.  The integer views -- generator(), window_table(), lagrange_coeffs(), z(), u() -- read each table back once."""

    def __init__(self, base_xy, num_windows: int = NUM_WINDOWS, z_limit: int = 0):
        import ctypes as C

        import torch
        base = np.ascontiguousarray(base_xy, dtype=np.uint64).reshape(-1)
        if base.shape != (8,):
            raise ValueError("FixedBase: a base of 8 uint64 limbs")
        self.num_windows, self._base, self._host = int(num_windows), base, {}
        nw, dev = max(self.num_windows, 0), fields.current_device()
        self.points = torch.zeros((nw, 8, 8), dtype=torch.int64, device=dev)
        self.lagrange = torch.zeros((nw, 8, 4), dtype=torch.int64, device=dev)
        self.zs = torch.zeros((nw,), dtype=torch.int64, device=dev)
        self.us = torch.zeros((nw, 8, 4), dtype=torch.int64, device=dev)
        check(lib().h2_ecc_fixed_tables_device(base.ctypes.data_as(C.POINTER(C.c_uint64)), self.num_windows, int(z_limit),
                                               self.points.data_ptr(), self.lagrange.data_ptr(), self.zs.data_ptr(), self.us.data_ptr(),
                                               _stream_ptr()), "h2_ecc_fixed_tables_device")

    def _ints(self, name, tensor):
        if name not in self._host:
            flat = fields.from_limbs(tensor.cpu().numpy().view(np.uint64).reshape(-1, 4), fields.FP, True)
            self._host[name] = flat
        return self._host[name]

    def generator(self):
        """the base as (x, y)"""
        return tuple(fields.from_limbs(self._base.reshape(2, 4), fields.FP, True))

    def window_table(self):
        """[w][k] = (x, y)"""
        v = self._ints("points", self.points)
        return [[(v[16 * w + 2 * k], v[16 * w + 2 * k + 1]) for k in range(8)] for w in range(self.num_windows)]

    def lagrange_coeffs(self):
        """[w][c]: the coefficient of X^c of window w's interpolation polynomial"""
        v = self._ints("lagrange", self.lagrange)
        return [v[8 * w:8 * w + 8] for w in range(self.num_windows)]

    def z(self):
        if "z" not in self._host:
            self._host["z"] = [int(v) for v in self.zs.cpu().numpy().view(np.uint64)]
        return self._host["z"]

    def u(self):
        """[w][k] with u^2 = y + z"""
        v = self._ints("u", self.us)
        return [v[8 * w:8 * w + 8] for w in range(self.num_windows)]


def mul_fixed(fixed_base: FixedBase, scalars):
    """[k_i]B: scalars (n, 4) canonical, of which the low 3 * num_windows bits are read -> (n, 8).  k = 0 gives the identity."""
    import torch
    k, host = _device(scalars, 4, "ecc.mul_fixed scalars")
    n = k.shape[0]
    out = torch.empty((n, 8), dtype=torch.int64, device=k.device)
    check(lib().h2_ecc_mul_fixed_device(fixed_base.points.data_ptr(), fixed_base.num_windows, _ptr(k), n, _ptr(out), _stream_ptr()),
          "h2_ecc_mul_fixed_device")
    return out.cpu().numpy().view(np.uint64) if host else out


def mul_fixed_short(fixed_base: FixedBase, magnitudes, signs):
    """[sign_i magnitude_i]B (mul_fixed/short.rs): magnitudes (n, 4) canonical, signs n values of 1 or -1; the product of the magnitude,
    negated here where the sign is -1."""
    import torch
    out = mul_fixed(fixed_base, magnitudes)
    host = not _is_torch(out)
    pts = torch.from_numpy(out.view(np.int64)).to(fields.current_device()) if host else out
    s = torch.as_tensor(np.asarray(signs.cpu() if _is_torch(signs) else signs, dtype=np.int64), device=pts.device)
    if s.shape != (pts.shape[0],) or not bool(((s == 1) | (s == -1)).all()):
        raise ValueError("ecc.mul_fixed_short: one sign of 1 or -1 per magnitude")
    y = pts[:, 4:].contiguous()
    neg_y = scale_add(y.clone(), fields.scalar_limbs(fields.P - 1, fields.FP), torch.zeros_like(y), fields.FP) if y.shape[0] else y
    pts = torch.cat([pts[:, :4], torch.where((s == -1)[:, None], neg_y, pts[:, 4:])], dim=1)
    return pts.cpu().numpy().view(np.uint64) if host else pts


def mul_fixed_trace(fixed_base: FixedBase, scalars):
    """What the chip's full-width `mul_fixed` witnesses for `count` scalars (as `mul_fixed`) -> (columns, aux): columns
    (6, num_windows * count, 4), the advice columns x_p, y_p, x_qr, y_qr, window, u with multiplication i in rows num_windows i ..,
    zero where the reference assigns nothing; aux (count, FIXED_AUX, 4), the closing complete addition and the product (see
    include/halo2_mi355x.h)."""
    import torch
    k, host = _device(scalars, 4, "ecc.mul_fixed_trace scalars")
    count, nw = k.shape[0], fixed_base.num_windows
    columns = torch.empty((6, nw * count, 4), dtype=torch.int64, device=k.device)
    aux = torch.empty((count, FIXED_AUX, 4), dtype=torch.int64, device=k.device)
    check(lib().h2_ecc_mul_fixed_trace_device(fixed_base.points.data_ptr(), fixed_base.us.data_ptr(), nw, _ptr(k), count, _ptr(columns),
                                              _ptr(aux), _stream_ptr()), "h2_ecc_mul_fixed_trace_device")
    if host:
        return columns.cpu().numpy().view(np.uint64), aux.cpu().numpy().view(np.uint64)
    return columns, aux


def _sum_scratch(nw: int, count: int, device):
    """the inverses' scratch of a running-sum trace: nw - 2 elements per lane, for every lane up to SUM_SCRATCH_LANES of them, beyond
    which the call goes through in chunks"""
    import torch
    lanes = max(1, min(count, SUM_SCRATCH_LANES))
    return torch.empty((lanes * (nw - 2), 4), dtype=torch.int64, device=device)


def _sum_descriptor(fixed_base: FixedBase, nw: int, scratch, what: str):
    from ._lib import EccFixedSum
    if fixed_base.num_windows != nw:
        raise ValueError(f"{what}: the tables of a base at {nw} windows")
    return EccFixedSum(nw, fixed_base.points.data_ptr(), fixed_base.us.data_ptr(), scratch.data_ptr(), scratch.shape[0], _stream_ptr())


def mul_fixed_short_trace(fixed_base: FixedBase, magnitudes, signs):
    """What the chip's `mul_fixed_short` witnesses for `count` pairs (mul_fixed/short.rs): magnitudes, signs (count, 4) CANONICAL
    elements of Fp, a valid magnitude below 2^64 and a valid sign 1 or p - 1 -> (columns, aux): columns (6, 23 * count, 4), the advice
    columns x_p, y_p, x_qr, y_qr, window, u with multiplication i in rows 23 i .., `window` holding the running sum z_0 .. z_22; aux
    (count, SHORT_AUX, 4), the closing complete addition, the magnitude's product and the signed y (see include/halo2_mi355x.h).  An
    invalid pair gets the cells the reference assigns for it, which its gates then reject.  The inverses' scratch is allocated here,
    per call, and is at most SUM_SCRATCH_LANES multiplications wide."""
    import ctypes as C

    import torch
    m, host = _device(magnitudes, 4, "ecc.mul_fixed_short_trace magnitudes")
    s, host_s = _device(signs, 4, "ecc.mul_fixed_short_trace signs")
    if m.shape[0] != s.shape[0] or host != host_s:
        raise ValueError("ecc.mul_fixed_short_trace: as many signs as magnitudes, both of one kind")
    count, nw = m.shape[0], NUM_WINDOWS_SHORT
    scratch = _sum_scratch(nw, count, m.device)
    d = _sum_descriptor(fixed_base, nw, scratch, "ecc.mul_fixed_short_trace")
    columns = torch.empty((6, (nw + 1) * count, 4), dtype=torch.int64, device=m.device)
    aux = torch.empty((count, SHORT_AUX, 4), dtype=torch.int64, device=m.device)
    check(lib().h2_ecc_mul_fixed_short_trace_device(C.byref(d), _ptr(m), _ptr(s), count, _ptr(columns), _ptr(aux)),
          "h2_ecc_mul_fixed_short_trace_device")
    if host:
        return columns.cpu().numpy().view(np.uint64), aux.cpu().numpy().view(np.uint64)
    return columns, aux


def mul_fixed_base_field_trace(fixed_base: FixedBase, alphas):
    """What the chip's `mul_fixed_base_field_elem` witnesses for `count` elements (mul_fixed/base_field_elem.rs): alphas (count, 4)
    CANONICAL elements of Fp -> (columns, aux): columns (6, 86 * count, 4) as `mul_fixed_short_trace`'s with the running sum
    z_0 .. z_85; aux (count, BASE_FIELD_AUX, 4): the closing complete addition and the product, alpha_0', alpha_1, alpha_2, and
    alpha_0' again as canonical limbs, the `values=` of `range_check_many` (see include/halo2_mi355x.h)."""
    import ctypes as C

    import torch
    a, host = _device(alphas, 4, "ecc.mul_fixed_base_field_trace alphas")
    count, nw = a.shape[0], NUM_WINDOWS
    scratch = _sum_scratch(nw, count, a.device)
    d = _sum_descriptor(fixed_base, nw, scratch, "ecc.mul_fixed_base_field_trace")
    columns = torch.empty((6, (nw + 1) * count, 4), dtype=torch.int64, device=a.device)
    aux = torch.empty((count, BASE_FIELD_AUX, 4), dtype=torch.int64, device=a.device)
    check(lib().h2_ecc_mul_fixed_base_field_trace_device(C.byref(d), _ptr(a), count, _ptr(columns), _ptr(aux)),
          "h2_ecc_mul_fixed_base_field_trace_device")
    if host:
        return columns.cpu().numpy().view(np.uint64), aux.cpu().numpy().view(np.uint64)
    return columns, aux


def add_trace(p, q):
    """What the chip's complete addition witnesses for n pairs (add.rs:213-295): p, q (n, 8) Montgomery affine, the identity (0, 0) ->
    (n, FIXED_AUX, 4): x_p, y_p, x_qr, y_qr, lambda, alpha, beta, gamma, delta and the sum's x and y, the order of `mul_fixed_trace`'s
    aux.  Every branch is the reference's: P + P, P + (-P) and the identity on either side."""
    import torch
    a, host = _device(p, 8, "ecc.add_trace p")
    b, host_b = _device(q, 8, "ecc.add_trace q")
    if a.shape[0] != b.shape[0] or host != host_b:
        raise ValueError("ecc.add_trace: as many q as p, both of one kind")
    n = a.shape[0]
    aux = torch.empty((n, FIXED_AUX, 4), dtype=torch.int64, device=a.device)
    check(lib().h2_ecc_add_trace_device(_ptr(a), _ptr(b), n, _ptr(aux), _stream_ptr()), "h2_ecc_add_trace_device")
    return aux.cpu().numpy().view(np.uint64) if host else aux


def add(p, q):
    """P_i + Q_i, complete: (n, 8) and (n, 8) -> (n, 8)."""
    aux = add_trace(p, q)
    out = aux[:, 9:11].reshape(-1, 8)
    return np.ascontiguousarray(out) if isinstance(out, np.ndarray) else out.contiguous()
