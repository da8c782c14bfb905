"""Every plan of the registered commit on the device: each case of tests/commit_plans.py's SWEEP is run through its entry point, the plan the
library took is read back through h2_commit_last_plan and held, field by field, to the host replica, and the result to the C oracle as
affine integers.

One base array and three columns per curve serve every table: a table of n points is registered from the first n bases (an identity and a
repeated point among the first eight), a call over n_used scalars reads the first n_used of a column.  The oracle's answer for a prefix is
the sum of the oracle's multiexps over the pieces between the lengths the sweep uses (a multiexp is linear in its terms), so the 2^19-point
columns cost one pass per curve and column instead of one per case.  Tables are registered once per (curve, points, bits) and freed when
the module ends; the curve of a case follows its table's width, and the width sweep runs on both."""
import ctypes as C

import numpy as np
import pytest

import commit_plans as cp
import halo2_amd as h
from halo2_amd import _lib
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

MONT, JAC = h.FORM_MONTGOMERY, 0
MAX_N = max(c.points for c in cp.SWEEP)
CUTS = sorted({0, MAX_N} | {v for c in cp.SWEEP for v in (c.n_used, c.n_used - 4) if 0 < v <= MAX_N})
KINDS = ("dense", "skewed", "sparse")          # random; all scalars equal (one heavy bucket per window); 90 % zeros
_cache = {}
_tables = {}
_lanes = {}
_faulted = []


def curve_of(case):
    return (case.bits or case.points) % 2


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to("cuda:0")


def _p(a):
    return a.ctypes.data_as(_lib.u64p)


def ok(rc):
    if rc == _lib.H2_ERR_HIP:
        raise RuntimeError(f"HIP failure: {h.lib().h2_last_error()}")
    assert rc == 0, (rc, h.lib().h2_last_error())


def bases(curve):
    """MAX_N points: index 5 holds the identity and 7 repeats 6 (every table of eight points or more has both)"""
    if ("b", curve) not in _cache:
        g = co.generate_bases(curve, 0xC100 + curve, MAX_N)
        g[5] = 0
        g[7] = g[6]
        _cache["b", curve] = g
    return _cache["b", curve]


def blind_base(curve):
    return co.generate_bases(curve, 0xC200 + curve, 1)[0]


def column(curve, kind):
    """(host limbs, device tensor) of one MAX_N-scalar column"""
    if ("s", curve, kind) not in _cache:
        sf = co.field_of_curve(curve, "scalar")
        s = co.random_field(sf, 0xC300 + curve, MAX_N)
        if kind == "skewed":
            s[:] = s[11]
        elif kind == "sparse":
            keep = np.random.default_rng(0xC400 + curve).random(MAX_N) < 0.1
            s[~keep] = 0
        _cache["s", curve, kind] = (s, _dev(s))
    return _cache["s", curve, kind]


def blinds(curve):
    if ("bl", curve) not in _cache:
        bl = co.random_field(co.field_of_curve(curve, "scalar"), 0xC500 + curve, cp.MAX_COLS + 2)
        _cache["bl", curve] = (bl, _dev(bl))
    return _cache["bl", curve]


def one(curve):
    return co.to_mont(co.field_of_curve(curve, "scalar"), co.ints_to_limbs([1]))


def _affine(curve, jac):
    return co.points_to_mont(curve, [co.jac_to_affine_ints(curve, jac)])[0]


def pieces(curve, kind, parity):
    """The oracle's multiexp over every piece [CUTS[i], CUTS[i + 1]) of a column as affine points; parity 0 / 1: only the scalars at even /
    odd indices (the two sides of a paired commit with shift 0)"""
    key = ("p", curve, kind, parity)
    if key not in _cache:
        s = column(curve, kind)[0]
        if parity is not None:
            s = s.copy()
            s[1 - parity::2] = 0
        g = bases(curve)
        _cache[key] = np.stack([_affine(curve, co.best_multiexp(curve, s[a:b], g[a:b])) for a, b in zip(CUTS, CUTS[1:])])
    return _cache[key]


def prefix_sum(curve, kind, n, extra=(), parity=None):
    """sum over i < n of column[i] * base[i], plus the (scalar, affine point) terms of `extra`, as affine integers"""
    key = ("w", curve, kind, n, parity, tuple((sc.tobytes(), pt.tobytes()) for sc, pt in extra))
    if key not in _cache:
        k = CUTS.index(n)
        pts = [pieces(curve, kind, parity)[:k]] + [pt.reshape(1, 8) for _, pt in extra]
        scs = [np.repeat(one(curve), k, axis=0)] + [sc.reshape(1, 4) for sc, _ in extra]
        pts, scs = np.ascontiguousarray(np.concatenate(pts)), np.ascontiguousarray(np.concatenate(scs))
        _cache[key] = co.jac_to_affine_ints(curve, co.best_multiexp(curve, scs, pts)) if len(pts) else None
    return _cache[key]


def table(curve, points, bits):
    key = (curve, points, bits)
    if key not in _tables:
        hd = C.c_uint64(0)
        g = np.ascontiguousarray(bases(curve)[:points])
        ok(h.lib().h2_bases_register_ex(curve, _p(g), points, MONT, bits, C.byref(hd)))
        ok(h.lib().h2_bases_set_blind_base(hd, _p(blind_base(curve)), MONT))
        _tables[key] = hd
    return _tables[key]


@pytest.fixture(scope="module", autouse=True)
def _free_tables():
    yield
    import torch
    torch.cuda.synchronize()
    for hd in _tables.values():
        h.lib().h2_bases_free(hd)
    _tables.clear()
    _cache.clear()


def read_plan(stream):
    rec = _lib.CommitPlan()
    ok(h.lib().h2_commit_last_plan(C.c_void_p(stream), C.byref(rec)))
    return rec.as_dict()


def got_of(curve, out):
    return co.jac_to_affine_ints(curve, np.ascontiguousarray(out.cpu().numpy().view(np.uint64)))


def run_case(case, curve, kinds):
    """The case's call once per column kind on a fresh stream; the read-back against the replica and the result against the oracle.  After a
    HIP error nothing more is enqueued: every later case fails at once."""
    assert not _faulted, f"not run: an earlier case met a HIP error ({_faulted[0]})"
    try:
        _run_case(case, curve, kinds)
    except Exception as e:
        if "HIP" in str(e) or "hip" in type(e).__name__.lower() or isinstance(e, RuntimeError):
            _faulted.append(f"{case}: {str(e)[:200]}")
        raise


def _run_case(case, curve, kinds):
    import torch
    lib = h.lib()
    n = case.n_used
    if cp.table_bits(case.points, case.bits) is None:
        hd = C.c_uint64(0)
        assert lib.h2_bases_register_ex(curve, _p(np.ascontiguousarray(bases(curve)[:case.points])), case.points, MONT, case.bits, C.byref(hd)) == _lib.H2_ERR_ARGS
        return
    hd = table(curve, case.points, case.bits)
    lanes = resident_lanes(curve)
    bl_h, bl_d = blinds(curve)
    w = blind_base(curve)
    stream = torch.cuda.Stream()
    for kind in kinds:
        s_h, s_d = column(curve, kind)
        with torch.cuda.stream(stream):
            st = C.c_void_p(stream.cuda_stream)
            blind_ptr = bl_d[0].data_ptr() if case.blind else None
            extra = [(bl_h[0], w)] if case.blind else []
            wants = None
            if case.entry == "device":
                out = torch.zeros(12, dtype=torch.int64, device="cuda:0")
                rc = lib.h2_commit_device(hd, s_d.data_ptr(), n, None, blind_ptr, MONT, JAC, out.data_ptr(), st)
                outs = [out]
            elif case.entry == "range":
                out = torch.zeros(12, dtype=torch.int64, device="cuda:0")
                rc = lib.h2_commit_range_device(hd, s_d.data_ptr(), case.first, n, blind_ptr, MONT, JAC, out.data_ptr(), st)
                outs = [out]
                g = bases(curve)[case.first:case.first + n]
                terms_s = np.concatenate([s_h[:n]] + [sc.reshape(1, 4) for sc, _ in extra])
                terms_p = np.concatenate([g] + [pt.reshape(1, 8) for _, pt in extra])
                wants = [co.jac_to_affine_ints(curve, co.best_multiexp(curve, np.ascontiguousarray(terms_s), np.ascontiguousarray(terms_p))) if len(terms_s) else None]
            elif case.entry == "host":
                res = np.zeros(12, dtype=np.uint64)
                try:
                    ok(lib.h2_set_option(b"host_commit_chunk", float(case.chunk)))
                    rc = lib.h2_commit(hd, _p(s_h), n, None, _p(bl_h[0]) if case.blind else None, MONT, JAC, _p(res))
                finally:
                    ok(lib.h2_set_option(b"host_commit_chunk", 0.0))
                outs = [torch.from_numpy(res.view(np.int64))]
                st = C.c_void_p(None)
            elif case.entry == "batch":
                K = case.K
                vpk = C.c_void_p * K
                out = torch.zeros((K, 12), dtype=torch.int64, device="cuda:0")
                cols = [column(curve, KINDS[(KINDS.index(kind) + k) % 2]) for k in range(K)]      # dense and skewed columns alternate
                rc = lib.h2_commit_batch_device(hd, vpk(*[c_[1].data_ptr() for c_ in cols]), K, n, None,
                                                vpk(*[bl_d[k].data_ptr() for k in range(K)]) if case.blind else None, MONT, JAC,
                                                vpk(*[out[k].data_ptr() for k in range(K)]), st)
                outs = list(out)
                wants = [prefix_sum(curve, KINDS[(KINDS.index(kind) + k) % 2], n, [(bl_h[k], w)] if case.blind else []) for k in range(K)]
            else:
                assert case.entry == "pair" and n == case.points
                out = torch.zeros((2, 12), dtype=torch.int64, device="cuda:0")
                rc = lib.h2_commit_pair_device(hd, s_d.data_ptr(), n, case.pair_shift, MONT, JAC, out.data_ptr(), st)
                outs = list(out)
            plan_stream = st.value
        got = read_plan(plan_stream) if rc == 0 else None
        exp = cp.expected(case, lanes)
        if isinstance(exp, str):
            assert rc == _lib.H2_ERR_ARGS, (case, rc)
            return
        ok(rc)
        torch.cuda.synchronize()
        diff = {f: (got[f], exp[f]) for f in cp.FIELDS if got[f] != exp[f]}
        assert not diff, f"{case} ({kind}): read-back against replica, (device, replica) per field: {diff}"
        if wants is None:
            if case.entry == "pair":
                wants = pair_wants(case, curve, kind)
            else:
                wants = [prefix_sum(curve, kind, n, extra)]
        for i, (o_, want) in enumerate(zip(outs, wants)):
            assert got_of(curve, o_) == want, f"{case} ({kind}), output {i}: result differs from the oracle; plan {got}"


def resident_lanes(curve):
    """The lanes of the accumulate the device holds at once: the replica's input, taken from the device's first answer for the curve (a
    tiny commit of its own) and checked to be whole workgroups."""
    import torch
    if curve not in _lanes:
        hd = table(curve, 8, 8)
        out = torch.zeros(12, dtype=torch.int64, device="cuda:0")
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            ok(h.lib().h2_commit_device(hd, column(curve, "dense")[1].data_ptr(), 8, None, None, MONT, JAC, out.data_ptr(), C.c_void_p(st.cuda_stream)))
        torch.cuda.synchronize()
        _lanes[curve] = read_plan(st.cuda_stream)["lanes"]
        assert _lanes[curve] > 0 and _lanes[curve] % 256 == 0, _lanes
    return _lanes[curve]


def pair_wants(case, curve, kind):
    """both outputs of a paired commit: column i < n - 4 feeds output (i >> shift) & 1, the last four feed 0, 1, 0, 1"""
    n, shift = case.points, case.pair_shift
    s, g = column(curve, kind)[0], bases(curve)
    tail = lambda side: [(s[i], g[i]) for i in range(n - 4, n) if (i - (n - 4)) & 1 == side]
    if shift == 0:
        return [prefix_sum(curve, kind, n - 4, tail(side), parity=side) for side in (0, 1)]
    idx = np.arange(n)
    sides = np.where(idx < n - 4, (idx >> shift) & 1, (idx - (n - 4)) & 1)
    wants = []
    for side in (0, 1):
        part = s[:n].copy()
        part[sides != side] = 0
        wants.append(co.jac_to_affine_ints(curve, co.best_multiexp(curve, part, np.ascontiguousarray(g[:n]))))
    return wants


def kinds_of(case):
    return KINDS if case.note in ("max_big off", "max_big on", "lane_div 8", "lane_div 16") else KINDS[:2]


WIDTH_SWEEP = [c for c in cp.SWEEP if c.note == "width sweep"]
OTHERS = [c for c in cp.SWEEP if c.note != "width sweep"]
GROUPS = sorted({(c.points, c.bits) for c in OTHERS})


def test_the_query_refuses_a_stream_without_a_registered_commit():
    import torch
    s = torch.cuda.Stream(priority=-1)          # (a fresh stream: see tests/test_gpu_generic_paths.py)
    rec = _lib.CommitPlan()
    assert h.lib().h2_commit_last_plan(C.c_void_p(s.cuda_stream), C.byref(rec)) == _lib.H2_ERR_ARGS
    assert h.lib().h2_commit_last_plan(None, None) == _lib.H2_ERR_ARGS


@pytest.mark.parametrize("curve", [h.PALLAS, h.VESTA])
@pytest.mark.parametrize("bits", range(4, 21))
def test_every_width_over_one_small_table(bits, curve):
    """Widths 4 to 20 over 2^13 + 3 points: the full column, one scalar less with a blind, both sides of the one-pass / two-pass edge at
    8192 digit columns, two scalars, one blind alone, and nothing with and without a blind."""
    for case in WIDTH_SWEEP:
        if case.bits == bits:
            run_case(case, curve, KINDS[:2])


@pytest.mark.parametrize("points,bits", GROUPS)
def test_the_sweep_by_table(points, bits):
    """Every other case of the sweep, grouped by the table it registers."""
    for case in OTHERS:
        if (case.points, case.bits) == (points, bits):
            run_case(case, curve_of(case), kinds_of(case))
