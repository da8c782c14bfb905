"""The exceptional point additions (P + P, P - P, the identity) on every multiexp path, against closed-form answers.

The input families of tests/exceptional_points.py put equal and opposite points into the same bucket, fold, chain and range on purpose; each
answer is (sum_i s_i c_i + blind c_w) G, so the sizes can reach the grouped and slice-split forms without an oracle multiexp.  Where the
library reports the form a call took (h2_msm_last_path, h2_bases_info) the test asserts it, with the thresholds of
tests/test_gpu_generic_paths.py.  The formula-level counterpart (every addition form on rescaled and formula-made operands) is the
"exc" section of tests/native/field_check.hip."""
import ctypes as C

import numpy as np
import pytest

import exceptional_points as xp
import halo2_amd as h
from halo2_amd import _lib, fields
from oracle import c_oracle as co
from oracle import pasta as o
from test_gpu_generic_paths import LATENCY, LATENCY_MAX, ONE_PASS, SLICE_SPLIT, THROUGHPUT, TWO_PASS, last_path

pytestmark = pytest.mark.gpu
CURVES = [h.PALLAS, h.VESTA]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def affine_of(curve, out):
    if not isinstance(out, np.ndarray):
        out = np.ascontiguousarray(out.cpu().numpy().view(np.uint64))
    return co.jac_to_affine_ints(curve, out)


def families(curve, n, w, seed):
    return [xp.palette(curve, n, seed), xp.cancelling(curve, n, seed + 1), xp.uniform_buckets(curve, n, w, seed + 2),
            xp.uniform_buckets(curve, n, w, seed + 3, "alternating", phi=True), xp.heavy(curve, n, seed + 4)]


def msm_device(inp, n=None):
    n = inp.n if n is None else n
    out = h.best_multiexp(_dev(inp.scalars[:n]), _dev(inp.bases[:n]), inp.curve)
    return out, last_path()


# ---- the generic multiexp --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n,form,bits", [(1024, ONE_PASS, 10), (4096, ONE_PASS, 13), (65536, TWO_PASS, 13), ((1 << 18) + 1, LATENCY, 16)])
def test_generic_forms(curve, n, form, bits):
    import torch
    with torch.cuda.stream(torch.cuda.Stream()):
        for inp in families(curve, n, bits, 100 + n % 1000 + curve):
            out, path = msm_device(inp)
            torch.cuda.synchronize()
            assert (path[0], path[3]) == (form, bits), (inp.name, path)
            assert affine_of(curve, out) == inp.want(), inp.name
            if inp.name == "cancelling":
                assert not out.cpu().numpy().any()                         # the identity is all-zero Jacobian limbs


@pytest.mark.parametrize("curve", CURVES)
def test_generic_slice_split(curve):
    import torch
    n = LATENCY_MAX + 1
    with torch.cuda.stream(torch.cuda.Stream()):
        for inp in (xp.palette(curve, n, 200 + curve), xp.cancelling(curve, n, 210 + curve)):
            out, path = msm_device(inp)
            torch.cuda.synchronize()
            assert path[:2] == (SLICE_SPLIT, 2), (inp.name, path)
            assert affine_of(curve, out) == inp.want(), inp.name


@pytest.mark.parametrize("curve", CURVES)
def test_generic_throughput_form(curve):
    """the throughput form: a call on a fresh stream while a 2^22 latency-form call is in flight on another"""
    import torch
    big = xp.palette(curve, 1 << 22, 300 + curve)
    small = [xp.cancelling(curve, (1 << 20) + 1, 310 + curve), xp.uniform_buckets(curve, (1 << 20) + 1, 16, 320 + curve),
             xp.palette(curve, (1 << 20) + 1, 330 + curve)]
    x = torch.cuda.Stream()
    d_big = (_dev(big.scalars), _dev(big.bases))
    with torch.cuda.stream(x):
        h.best_multiexp(*d_big, curve)                                     # warm-up: X's workspaces exist
    torch.cuda.synchronize()
    for inp in small:
        d = (_dev(inp.scalars), _dev(inp.bases))
        torch.cuda.synchronize()
        y = torch.cuda.Stream()
        with torch.cuda.stream(x):
            out_x = h.best_multiexp(*d_big, curve)
            path_x = last_path()
        with torch.cuda.stream(y):
            out_y = h.best_multiexp(*d, curve)
            path_y = last_path()
        torch.cuda.synchronize()
        assert path_x[:2] == (LATENCY, 3) and path_y[:2] == (THROUGHPUT, 1), (inp.name, path_x, path_y)
        assert affine_of(curve, out_x) == big.want()
        assert affine_of(curve, out_y) == inp.want(), inp.name


@pytest.mark.parametrize("curve", CURVES)
def test_host_msm_and_ragged_batch(curve):
    """h2_msm from host memory, and h2_msm_batch_device over ragged entries of every family"""
    import torch
    for inp in families(curve, 5000, 13, 400 + curve):
        assert affine_of(curve, h.best_multiexp(inp.scalars, inp.bases, curve)) == inp.want(), inp.name
    sizes = [1, 7, 600, 4096, 70000]
    inps = [fam for n in sizes for fam in families(curve, n, 13 if n > 2048 else 10, 410 + n + curve)]
    pairs = [(_dev(i.scalars), _dev(i.bases)) for i in inps]
    outs = h.arithmetic.best_multiexp_batch(pairs, curve)
    torch.cuda.synchronize()
    for i, inp in enumerate(inps):
        assert affine_of(curve, outs[i]) == inp.want(), (inp.name, inp.n)


# ---- registered tables -------------------------------------------------------------------------------------------------------------
class Table:
    def __init__(self, curve, n, wb, c_w, seed):
        """n palette bases registered at window width wb (0: the library's choice) with blind base c_w G"""
        self.curve, self.n, self.c_w = curve, n, c_w
        self.inp = xp.palette(curve, n, seed)
        self.handle = C.c_uint64(0)
        lib = h.lib()
        if wb:
            assert lib.h2_bases_register_ex(curve, self.inp.bases.ctypes.data_as(_lib.u64p), n, h.FORM_MONTGOMERY, wb, C.byref(self.handle)) == 0
        else:
            assert lib.h2_bases_register(curve, self.inp.bases.ctypes.data_as(_lib.u64p), n, h.FORM_MONTGOMERY, C.byref(self.handle)) == 0
        nn, bits, cv = C.c_size_t(), C.c_int(), C.c_int()
        assert lib.h2_bases_info(self.handle, C.byref(nn), C.byref(bits), C.byref(cv)) == 0
        assert (nn.value, cv.value) == (n, curve) and bits.value == (wb or lib.h2_commit_window_bits(n)), (wb, bits.value)
        self.bits = bits.value
        self.w = xp.point(curve, c_w)
        assert lib.h2_bases_set_blind_base(self.handle, self.w.ctypes.data_as(_lib.u64p), h.FORM_MONTGOMERY) == 0

    def close(self):
        h.lib().h2_bases_free(self.handle)


def commit_device(t, scalars, blind=None):
    import torch
    out = torch.empty(12, dtype=torch.int64, device="cuda")
    d_sc = _dev(scalars)
    d_bl = None if blind is None else _dev(fields.scalar_limbs(blind, fields.CURVE_FIELDS[t.curve][1], True))
    rc = h.lib().h2_commit_device(t.handle, d_sc.data_ptr(), scalars.shape[0], None, None if d_bl is None else d_bl.data_ptr(),
                                  h.FORM_MONTGOMERY, _lib.OUT_JACOBIAN, out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, h.lib().h2_last_error()
    torch.cuda.synchronize()
    return out


def registered_cases(t, seed):
    """scalar columns over t's palette bases (c_i in [-8, 8]) that meet the exceptional additions: the palette itself, one scalar
    everywhere (heavy), rows c / -c under equal scalars (the column sums to the identity), rows c / c under equal scalars (doublings),
    and uniform buckets: bucket j < 2^(w-1) holds a pair of rows x / 5 - x, so every bucket sums to 5 G"""
    sf = fields.CURVE_FIELDS[t.curve][1]
    c, n = t.inp.coeffs, t.n
    rand = co.random_field(sf, seed, n)
    canc, dbl, uni = np.zeros_like(rand), np.zeros_like(rand), np.zeros_like(rand)
    canc[c == 0] = rand[c == 0]
    for v in range(1, 9):
        pos, neg = np.flatnonzero(c == v), np.flatnonzero(c == -v)
        m = min(pos.size, neg.size)
        canc[pos[:m]] = canc[neg[:m]] = rand[pos[:m]]
    for v in range(-8, 9):
        rows = np.flatnonzero(c == v)
        m = rows.size // 2
        dbl[rows[:m]] = dbl[rows[m:2 * m]] = rand[rows[:m]]
    pairs = []
    for x in range(-3, 3):
        a, b = np.flatnonzero(c == x), np.flatnonzero(c == 5 - x)
        pairs += list(zip(a[:min(a.size, b.size)], b[:min(a.size, b.size)]))
    pa = np.array(pairs[:(1 << (min(t.bits, 16) - 1)) - 1])
    uni[pa[:, 0]] = uni[pa[:, 1]] = fields.to_limbs(range(1, pa.shape[0] + 1), sf, True)
    return [("palette", t.inp.scalars), ("heavy", np.ascontiguousarray(np.repeat(rand[:1], n, axis=0))), ("cancelling", canc),
            ("doubling", dbl), ("uniform buckets", uni)]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n,wb", [(4096, 0), (4096, 8), (4096, 13), (4096, 16), (1 << 18, 17)])
def test_registered_commit_device(curve, n, wb):
    """h2_commit_device over tables of every width: the families' columns with no blind, a palette blind and a cancelling blind"""
    import torch
    t = Table(curve, n, wb, -3, 500 + curve + wb)
    try:
        with torch.cuda.stream(torch.cuda.Stream()):
            cases = registered_cases(t, 510 + curve + wb)
            for name, sc in cases:
                want = xp.closed_form(curve, sc, t.inp.coeffs)
                assert affine_of(curve, commit_device(t, sc)) == want, (name, t.bits)
                kb = xp.closed_form_scalar(curve, sc, t.inp.coeffs)
                blind = (-kb * pow(t.c_w, -1, o.CURVES[curve][1])) % o.CURVES[curve][1]
                out = commit_device(t, sc, blind)
                assert affine_of(curve, out) is None and not out.cpu().numpy().any(), (name, t.bits)
                assert affine_of(curve, commit_device(t, sc, 77)) == xp.closed_form(curve, sc, t.inp.coeffs, 77, t.c_w), (name, t.bits)
    finally:
        t.close()


@pytest.mark.parametrize("curve", CURVES)
def test_registered_commit_host_ranges(curve):
    """h2_commit from host memory in ranges of 4096 scalars: the cancelling column's pairs lie in different ranges, so the range
    partials cancel each other"""
    n = 1 << 15
    t = Table(curve, n, 0, 5, 600 + curve)
    lib = h.lib()
    try:
        assert lib.h2_set_option(b"host_commit_chunk", 4096.0) == 0
        sf = fields.CURVE_FIELDS[curve][1]
        for name, sc in registered_cases(t, 610 + curve):
            kb = xp.closed_form_scalar(curve, sc, t.inp.coeffs)
            for blind in (None, 11, (-kb * pow(t.c_w, -1, o.CURVES[curve][1])) % o.CURVES[curve][1]):
                out = np.zeros(12, dtype=np.uint64)
                bl = None if blind is None else fields.scalar_limbs(blind, sf, True)
                rc = lib.h2_commit(t.handle, np.ascontiguousarray(sc).ctypes.data_as(_lib.u64p), n, None,
                                   None if bl is None else bl.ctypes.data_as(_lib.u64p), h.FORM_MONTGOMERY, _lib.OUT_JACOBIAN,
                                   out.ctypes.data_as(_lib.u64p))
                assert rc == 0, lib.h2_last_error()
                assert affine_of(curve, out) == xp.closed_form(curve, sc, t.inp.coeffs, blind or 0, t.c_w), (name, blind)
    finally:
        lib.h2_set_option(b"host_commit_chunk", 0.0)
        t.close()


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [8192, 1 << 19])
def test_commit_batch_both_forms(curve, n):
    """h2_commit_batch_device: four columns of 8192 take the column-batched form, four of 2^19 one commit per column"""
    import torch
    t = Table(curve, n, 0, -7, 700 + curve + n % 97)
    try:
        cases = registered_cases(t, 710 + curve)[1:]
        sm = o.CURVES[curve][1]
        sf = fields.CURVE_FIELDS[curve][1]
        cancel = lambda sc: (-xp.closed_form_scalar(curve, sc, t.inp.coeffs) * pow(t.c_w, -1, sm)) % sm
        blinds = [cancel(cases[0][1]), 5, cancel(cases[2][1]), 9]          # heavy and doubling: nonzero columns cancelled by the blind
        d_sc = [_dev(sc) for _, sc in cases]
        d_bl = [_dev(fields.scalar_limbs(b, sf, True)) for b in blinds]
        out = torch.empty((4, 12), dtype=torch.int64, device="cuda")
        arr = C.c_void_p * 4
        with torch.cuda.stream(torch.cuda.Stream()):
            rc = h.lib().h2_commit_batch_device(t.handle, arr(*[d.data_ptr() for d in d_sc]), 4, n, None, arr(*[d.data_ptr() for d in d_bl]),
                                                h.FORM_MONTGOMERY, _lib.OUT_JACOBIAN, arr(*[out[i].data_ptr() for i in range(4)]),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, h.lib().h2_last_error()
        torch.cuda.synchronize()
        for i, (name, sc) in enumerate(cases):
            assert affine_of(curve, out[i]) == xp.closed_form(curve, sc, t.inp.coeffs, blinds[i], t.c_w), (name, i)
        assert xp.closed_form(curve, cases[0][1], t.inp.coeffs) is not None and affine_of(curve, out[0]) is None
        assert xp.closed_form(curve, cases[2][1], t.inp.coeffs) is not None and affine_of(curve, out[2]) is None
    finally:
        t.close()


@pytest.mark.parametrize("curve", CURVES)
def test_commit_pair(curve):
    """h2_commit_pair_device: column i < n - 4 feeds output (i >> shift) & 1, the last four feed 0, 1, 0, 1"""
    import torch
    n, shift = 8192, 3
    assert h.lib().h2_commit_pair_supported(n) == 1
    t = Table(curve, n, 0, 3, 800 + curve)
    try:
        sel = (np.arange(n) >> shift) & 1
        sel[n - 4:] = [0, 1, 0, 1]
        for name, sc in registered_cases(t, 810 + curve):
            out = torch.empty(24, dtype=torch.int64, device="cuda")
            d = _dev(sc)
            rc = h.lib().h2_commit_pair_device(t.handle, d.data_ptr(), n, shift, h.FORM_MONTGOMERY, _lib.OUT_JACOBIAN, out.data_ptr(),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, h.lib().h2_last_error()
            torch.cuda.synchronize()
            for k in (0, 1):
                m = sel == k
                assert affine_of(curve, out[12 * k:12 * k + 12]) == xp.closed_form(curve, sc[m], t.inp.coeffs[m]), (name, k)
    finally:
        t.close()


# ---- point kernels -------------------------------------------------------------------------------------------------------------------
def jacobian_of(curve, coeffs, lams=(1,)):
    """(len, 12) Jacobian limbs of c G: row i as (l^2 x, l^3 y, l) with l = lams[i % len(lams)] (l = 1: Z = 1), the identity all zeros"""
    bf = fields.CURVE_FIELDS[curve][0]
    coeffs = np.asarray(coeffs)
    aff = xp.multiples(curve)[coeffs + xp.CMAX]
    out = np.zeros((coeffs.size, 12), dtype=np.uint64)
    zero = np.zeros((1, 4), dtype=np.uint64)
    m = fields.MODULUS[bf]
    for r, lam in enumerate(lams):
        rows = np.flatnonzero((np.arange(coeffs.size) % len(lams) == r) & (coeffs != 0))
        if not rows.size:
            continue
        sc = lambda a, e: co.scale_add(bf, np.ascontiguousarray(a), fields.scalar_limbs(pow(lam, e, m), bf, True), np.repeat(zero, rows.size, 0))
        out[rows, 0:4], out[rows, 4:8] = sc(aff[rows, 0:4], 2), sc(aff[rows, 4:8], 3)
        out[rows, 8:12] = fields.scalar_limbs(lam, bf, True)
    return out


@pytest.mark.parametrize("curve", CURVES)
def test_points_sum(curve):
    sm = o.CURVES[curve][1]
    rng = np.random.default_rng(900 + curve)
    for coeffs in ([3, 3], [3, -3], [0, 0, 5], [5, 0, -5, 5, 5, -10], [1, 1, 2, 4, 8, -16], list(rng.integers(-8, 9, 1000)),
                   [4, -4] * 500 + [0] * 24):
        want = o.ec_mul(sum(int(c) for c in coeffs) % sm, xp.generator(curve), o.CURVES[curve][0])
        for lams in ((1,), (1, 0x1234567890abcdef, 3 << 200)):             # equal points with equal and with different Z
            assert affine_of(curve, h.points_sum(jacobian_of(curve, coeffs, lams), curve)) == want, (coeffs[:8], len(lams))


@pytest.mark.parametrize("curve", CURVES)
def test_generator_collapse(curve):
    """g_lo + u g_hi with g_lo = +-g_hi (and identities) and u = +-1: doublings and cancellations in every lane"""
    sm = o.CURVES[curve][1]
    sf = fields.CURVE_FIELDS[curve][1]
    half = 2048
    rng = np.random.default_rng(950 + curve)
    hi = rng.integers(-8, 9, half)
    sign = np.where(rng.integers(0, 2, half) == 1, 1, -1)
    lo = hi * sign
    g = np.ascontiguousarray(np.concatenate([xp.multiples(curve)[lo + xp.CMAX], xp.multiples(curve)[hi + xp.CMAX]]))
    for u in (1, -1):
        got = h.parallel_generator_collapse(g, fields.scalar_limbs(u % sm, sf, True), curve)
        want = xp.multiples(curve)[lo + u * hi + xp.CMAX]
        assert np.array_equal(got, want), u


@pytest.mark.parametrize("curve", CURVES)
def test_lagrange_basis(curve):
    """the point iFFT on palette generators against the oracle (k = 8), and closed forms at k = 10 and 16: a constant vector c G gives
    (c G, O, ..., O), a delta gives 2^-k G everywhere, an alternating +-A gives A at n / 2 and O elsewhere"""
    sm = o.CURVES[curve][1]
    rng = np.random.default_rng(980 + curve)
    k = 8
    g = np.ascontiguousarray(xp.multiples(curve)[rng.integers(-8, 9, 1 << k) + xp.CMAX])
    assert np.array_equal(h.lagrange_basis(g, curve, k), co.lagrange_basis(curve, g, k))
    tab = xp.multiples(curve)
    for k in (10, 16):
        n = 1 << k
        got = h.lagrange_basis(np.ascontiguousarray(np.repeat(tab[3 + xp.CMAX][None], n, axis=0)), curve, k)
        assert np.array_equal(got[0], tab[3 + xp.CMAX]) and not got[1:].any(), k
        delta = np.zeros((n, 8), dtype=np.uint64)
        delta[0] = tab[1 + xp.CMAX]
        got = h.lagrange_basis(delta, curve, k)
        assert (got == xp.point(curve, pow(n, -1, sm))[None]).all(), k
        alt = np.ascontiguousarray(tab[np.where(np.arange(n) % 2 == 0, 5, -5) + xp.CMAX])
        got = h.lagrange_basis(alt, curve, k)
        assert np.array_equal(got[n // 2], tab[5 + xp.CMAX]) and not np.delete(got, n // 2, axis=0).any(), k


# ---- partials that meet each other: host slices, device ranges, the split over devices -------------------------------------------------
def thirds(curve, m, signs, seed):
    """3 m rows: one palette column repeated in each third with its coefficients times signs[t] and the same scalars, so the range
    partials of a three-way cut are X, +-X, ... exactly"""
    rng = np.random.default_rng(seed)
    c = rng.integers(-8, 9, m)
    s = co.random_field(fields.CURVE_FIELDS[curve][1], seed, m)
    return xp.Inputs(curve, f"thirds {signs}", np.concatenate([s] * len(signs)), np.concatenate([c * t for t in signs]))


@pytest.mark.parametrize("curve", CURVES)
def test_host_slice_pipeline(curve):
    """h2_msm from host memory from 2^19 points on: three ranges whose slice sums are added on the device.  The thirds make the range
    partials X, -X, X and X, X, -2X; the 2^20 + 1 families put cancelling pairs and uniform buckets across the ranges"""
    m = 1 << 18
    inps = [thirds(curve, m, (1, -1, 1), 1000 + curve), thirds(curve, m, (1, 1, -2), 1010 + curve),
            xp.cancelling(curve, (1 << 20) + 1, 1020 + curve), xp.uniform_buckets(curve, (1 << 20) + 1, 16, 1030 + curve)]
    for inp in inps:
        assert affine_of(curve, h.best_multiexp(inp.scalars, inp.bases, curve)) == inp.want(), inp.name


@pytest.mark.parametrize("curve", CURVES)
def test_commit_ranges_and_points_sum_device(curve):
    """h2_commit_range_device over the two halves of a registered table and an all-zero range, then h2_points_sum_device over the three
    partials: columns whose half partials are opposite (the sum is O), equal (a doubling), and a blind that cancels the second half"""
    import torch
    n = 1 << 14
    t = Table(curve, n, 0, 7, 1100 + curve)
    sf = fields.CURVE_FIELDS[curve][1]
    sm = o.CURVES[curve][1]
    lib = h.lib()
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    try:
        c, half = t.inp.coeffs, n // 2
        rand = co.random_field(sf, 1110 + curve, n)
        cols = {}
        for name, sign in (("opposite", -1), ("equal", 1)):
            sc = np.zeros_like(rand)
            for v in range(-8, 9):
                a, b = np.flatnonzero(c[:half] == v), half + np.flatnonzero(c[half:] == sign * v)
                k = min(a.size, b.size)
                sc[a[:k]] = sc[b[:k]] = rand[a[:k]]
            cols[name] = sc
        for name, sc in cols.items():
            second = xp.closed_form_scalar(curve, sc[half:], c[half:])
            for blind in (None, (-second * pow(t.c_w, -1, sm)) % sm):
                d_sc = _dev(sc)
                d_bl = None if blind is None else _dev(fields.scalar_limbs(blind, sf, True))
                parts = torch.zeros((3, 12), dtype=torch.int64, device="cuda")
                for i, (first, cnt, bl) in enumerate(((0, half, None), (half, half, d_bl), (64, 64, None))):
                    src = d_sc[first:first + cnt] if i < 2 else torch.zeros((cnt, 4), dtype=torch.int64, device="cuda")
                    rc = lib.h2_commit_range_device(t.handle, src.data_ptr(), first, cnt, None if bl is None else bl.data_ptr(), h.FORM_MONTGOMERY,
                                                    _lib.OUT_JACOBIAN, parts[i].data_ptr(), st())
                    assert rc == 0, lib.h2_last_error()
                out = torch.empty(12, dtype=torch.int64, device="cuda")
                rc = lib.h2_points_sum_device(curve, parts.data_ptr(), 3, h.FORM_MONTGOMERY, _lib.OUT_JACOBIAN, out.data_ptr(), st())
                assert rc == 0, lib.h2_last_error()
                torch.cuda.synchronize()
                assert affine_of(curve, parts[2]) is None
                want = xp.closed_form(curve, sc, c, blind or 0, t.c_w)
                assert affine_of(curve, out) == want, (name, blind)
                if name == "opposite" and blind is None:
                    assert want is None and affine_of(curve, parts[0]) is not None
                if name == "equal" and blind is None:
                    assert affine_of(curve, parts[0]) == affine_of(curve, parts[1]) is not None
    finally:
        t.close()


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("m", [4096, 1 << 18])
def test_msm_split_multi_on_one_device_twice(curve, m):
    """h2_msm_split_multi over devices [0, 0]: two halves whose partials are X and -X (the sum is O) or X and X (a doubling)"""
    for signs in ((1, -1), (1, 1)):
        inp = thirds(curve, m, signs, 1200 + curve + m % 7)
        out = np.zeros(12, dtype=np.uint64)
        devs = (C.c_int * 2)(0, 0)
        rc = h.lib().h2_msm_split_multi(curve, inp.scalars.ctypes.data, inp.bases.ctypes.data, inp.n, devs, 2, h.FORM_MONTGOMERY,
                                        _lib.OUT_JACOBIAN, out.ctypes.data)
        assert rc == 0, h.lib().h2_last_error()
        assert affine_of(curve, out) == inp.want(), signs
        assert (inp.want() is None) == (signs == (1, -1))


# ---- the opening argument ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,rounds,challenges", [(h.PALLAS, 1, (2,)), (h.VESTA, 3, (2, -1, 3)), (h.PALLAS, 3, (-1, -1, 2))])
def test_collapsed_generators_of_palette_bases(curve, rounds, challenges):
    """h2_ipa_collapsed_generators_device (the IPA read-out) over a palette table: with small integer challenges every output is a small
    multiple of G, so all 2^(k - rounds) outputs are checked; its running sums over the digit buckets meet equal and opposite points"""
    import torch
    from halo2_amd._lib import FORM_MONTGOMERY, check, lib
    k = 13
    n, nj = 1 << k, 1 << (k - rounds)
    sf = fields.CURVE_FIELDS[curve][1]
    sm = o.CURVES[curve][1]
    c = np.random.default_rng(1300 + curve + rounds).integers(-8, 9, n)
    g = np.ascontiguousarray(xp.multiples(curve)[c + xp.CMAX])
    params = h.Params(curve, k, g, g, xp.point(curve, 3), xp.point(curve, -5))
    try:
        handle = params._opening_basis(True)
        ch = fields.to_limbs([v % sm for v in challenges], sf, True)
        d_out = torch.empty((nj, 8), dtype=torch.int64, device="cuda:0")
        check(lib().h2_ipa_collapsed_generators_device(handle, k, rounds, ch.ctypes.data_as(C.POINTER(C.c_uint64)), FORM_MONTGOMERY,
                                                       d_out.data_ptr(), None), "h2_ipa_collapsed_generators_device")
        torch.cuda.synchronize()
        s_h = []                                                           # s(h): bit rounds-1-r of h picks challenge r
        for hh in range(1 << rounds):
            v = 1
            for r in range(rounds):
                if (hh >> (rounds - 1 - r)) & 1:
                    v *= challenges[r]
            s_h.append(v)
        kk = sum(s_h[hh] * c[hh * nj:(hh + 1) * nj] for hh in range(1 << rounds))
        cmax = 8 * sum(abs(v) for v in s_h)
        want = xp.multiples(curve, cmax)[kk + cmax]
        got = d_out.cpu().numpy().view(np.uint64)
        assert (kk == 0).any() and np.array_equal(got, want)
    finally:
        params.close()


def _rng(sf, seed):
    ctr = [seed]

    def rng(count):
        ctr[0] += 1
        return co.random_field(sf, ctr[0], count)
    return rng


@pytest.mark.parametrize("curve,k,schedule", [(h.PALLAS, 6, "collapse"), (h.PALLAS, 6, "original"), (h.VESTA, 6, "collapse"),
                                              (h.VESTA, 6, "original"), (h.PALLAS, 13, "collapse"), (h.VESTA, 13, "original"),
                                              (h.PALLAS, 13, "paired"), (h.VESTA, 13, "paired")])
def test_opening_with_palette_generators(curve, k, schedule):
    """create_proof (h2_open*) over palette generators (identities included) and palette w, u: the proof bytes equal oracle/ipa.py's
    and its verifier accepts them, as in tests/test_gpu_opening.py"""
    from halo2_amd.opening import create_proof
    from halo2_amd.transcript import Blake2bWrite
    from oracle import ipa
    n = 1 << k
    sf = fields.CURVE_FIELDS[curve][1]
    c = np.random.default_rng(1400 + curve + k).integers(-8, 9, n)
    g = np.ascontiguousarray(xp.multiples(curve)[c + xp.CMAX])
    w, u = xp.point(curve, -3), xp.point(curve, 5)
    params = h.Params.from_generators(curve, k, g, None, w, u)
    try:
        px = fields.to_limbs(range(n), sf, True)
        blind = h.Blind(co.random_field(sf, 1410, 1)[0])
        p = params.commit(px, blind, affine=True)
        tr = Blake2bWrite(curve)
        tr.write_point(p)
        x = tr.squeeze_challenge_scalar()
        v = h.eval_polynomial(px, x, sf)
        tr.write_scalar(v)
        create_proof(params, _rng(sf, 1420), tr, px, blind, x, schedule=schedule)
        proof = tr.finalize()
        p_int = co.affine_to_ints(curve, p)
        ot = ipa.Transcript(curve)
        ot.write_point(p_int)
        ox = ot.squeeze_challenge()
        ov = co.limbs_to_ints(co.from_mont(sf, co.eval_polynomial(sf, px, x)))[0]
        ot.write_scalar(ov)
        ipa.create_proof(curve, k, g, w, u, _rng(sf, 1420), ot, px, blind.value, x)
        assert bytes(ot.out) == proof
        vt = ipa.Transcript(curve, proof)
        vt.read_point(), vt.squeeze_challenge(), vt.read_scalar()
        assert ipa.verify_proof(curve, k, g, w, u, vt, p_int, ox, ov)
    finally:
        params.close()
