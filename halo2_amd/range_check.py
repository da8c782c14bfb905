"""The witness of the K = 10 lookup range check in bulk (halo2_amd/csrc/range_check.hip; halo2_gadgets
utilities/lookup_range_check.rs): `decompose` gives the running sums z_0 .. z_W of many values at once, `short` the three rows of
many short range checks.

Values are CANONICAL: a sequence of integers (reduced here), an (n, 4) array of uint64 limbs, or an (n, 4) CUDA int64 tensor, which is
used in place.  What comes back is Montgomery limbs, as cells are: a CUDA tensor for a CUDA tensor, a numpy array otherwise."""
from __future__ import annotations

import numpy as np

from . import fields
from ._lib import FP, check, lib
from .arithmetic import _is_torch, _stream_ptr

__all__ = ["K", "MAX_WORDS", "decompose", "short"]

K = 10
MAX_WORDS = 25                                  # floor(CAPACITY / K) = floor(254 / 10)


def _ptr(t):
    return t.data_ptr() if t.numel() else None


def _values(values, field, what):
    import torch
    host = not _is_torch(values)
    if host:
        a = np.asarray(values) if isinstance(values, np.ndarray) else None
        if a is None or a.dtype == object:
            m = fields.MODULUS[field]
            a = fields.to_limbs([int(v) % m for v in values], field, montgomery=False)
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4).view(np.int64)).to(fields.current_device())
    else:
        t = values.contiguous()
    if t.ndim != 2 or t.shape[1] != 4 or t.dtype != torch.int64 or not t.is_cuda:
        raise ValueError(f"{what}: integers or an (n, 4) array of uint64 limbs")
    return t, host


def _run(entry, name, values, parameter, rows, field, with_status):
    import torch
    v, host = _values(values, field, name)
    count = v.shape[0]
    out = torch.empty((count, rows, 4), dtype=torch.int64, device=v.device)
    status = torch.empty((count,), dtype=torch.uint8, device=v.device) if with_status else None
    check(entry(field, _ptr(v), count, parameter, _ptr(out), None if status is None else _ptr(status), _stream_ptr()), name)
    if host:
        out = out.cpu().numpy().view(np.uint64)
        status = None if status is None else status.cpu().numpy()
    return (out, status) if with_status else out


def decompose(values, num_words: int, field: int = FP, with_status: bool = False):
    """The running sums of `range_check` over num_words K-bit words: -> (count, num_words + 1, 4), row j of value i its z_j =
    value >> K j.  with_status: -> (rows, status), status[i] = 1 where z_W != 0 (the value does not fit K num_words bits).
    num_words outside 1 .. 25 raises ValueError."""
    if not 0 <= int(num_words) < 1 << 32:
        raise ValueError("range_check.decompose: bad arguments")
    return _run(lib().h2_range_check_trace_device, "h2_range_check_trace_device", values, int(num_words), int(num_words) + 1, field,
                with_status)


def short(values, num_bits: int, field: int = FP, with_status: bool = False):
    """The rows of `short_range_check`: -> (count, 3, 4): value, value 2^(K - num_bits) in the field, 2^-num_bits.  with_status:
    -> (rows, status), status[i] = 1 where value >= 2^num_bits.  num_bits above 10 raises ValueError."""
    if not 0 <= int(num_bits) < 1 << 32:
        raise ValueError("range_check.short: bad arguments")
    return _run(lib().h2_short_range_check_trace_device, "h2_short_range_check_trace_device", values, int(num_bits), 3, field, with_status)
