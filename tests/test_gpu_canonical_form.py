"""H2_FORM_CANONICAL through every single-GPU entry point of the C ABI that takes a form (tests/form_cases.py is the table,
tests/test_form_coverage.py holds it to the header).

The reference is always the oracle (oracle/c_oracle.py, oracle/pasta.py and their siblings; Montgomery in and out) or the operation's
definition over Python integers -- never the library's own Montgomery arm.  The canonical inputs are `co.from_mont` of the oracle's
inputs; field outputs must equal `co.from_mont(oracle result)` at every index, points are compared as canonical affine (x, y), and
an affine output also by its raw bytes.  Every case then runs the library's Montgomery arm on the Montgomery inputs against the same
oracle value: that only tells the two arms apart when a case fails.

0 and the all-zero point read the same in both forms, so every field vector is oracle-random with 1, 2, p - 1, 2^255 mod p, R mod p
(canonical bytes = Montgomery one), R^-1 mod p (Montgomery bytes = canonical one) and 0 planted at fixed indices (`planted`), and point
vectors are `co.generate_bases` with one identity where the entry point takes it.  Sizes are the smallest that reach each kernel; where
the library says which path a call took (h2_commit_window_bits, h2_commit_column_window_bits, h2_bases_info, h2_msm_last_path,
h2_commit_pair_supported) the case asserts it.  Runs only on a real MI355X (`-m gpu`)."""
import contextlib
import ctypes as C
import random

import numpy as np
import pytest

import halo2_amd as h
import mock_prover_cases as cases
import mock_prover_model as model
import ntt_shapes as ns
from halo2_amd import fields
from halo2_amd._lib import ConstraintSystemFailure, u64p
from halo2_amd.arithmetic import (assigned_to_field, best_multiexp_batch, ipa_round_scalars, ipa_s_combine, permute_expression_pair,
                                  sort_field)
from halo2_amd.commitment import hash_to_curve, lagrange_basis, points_from_bytes, points_to_bytes
from oracle import c_oracle as co
from oracle import hash_to_curve as oh
from oracle import lookup as olk
from oracle import pasta as o

pytestmark = pytest.mark.gpu

CAN, MONT = h.FORM_CANONICAL, h.FORM_MONTGOMERY
FORMS = (CAN, MONT)                    # the check first, the arm that localises a failure second
FIELDS = [h.FP, h.FQ]
CURVES = [h.PALLAS, h.VESTA]
JAC, AFF = 0, 1                        # H2_OUT_JACOBIAN, H2_OUT_AFFINE
PROF_NTT_PASS = 1                      # H2_PROF_NTT_PASS
PATH_ONE_PASS, PATH_TWO_PASS, PATH_GROUPED_LATENCY = 1, 2, 4       # H2_MSM_PATH_*


# ---------------------------------------------------------------------------------------------------- forms and inputs
def can(field, a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return co.from_mont(field, a.reshape(-1, 4)).reshape(a.shape)


def mont(field, a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return co.to_mont(field, a.reshape(-1, 4)).reshape(a.shape)


def conv(form, field, a):
    """the oracle's Montgomery limbs in the form a call is made with"""
    return can(field, a) if form == CAN else np.ascontiguousarray(a, dtype=np.uint64)


def special_values(field):
    m = fields.MODULUS[field]
    return [0, 1, 2, m - 1, (1 << 255) % m, pow(fields.R, -1, m), fields.R % m]


def planted(field, seed, n, zero_at=None):
    """n oracle-random elements (Montgomery limbs) with the special canonical values at the fixed indices (1 + 37 i) mod n; the zero
    goes to `zero_at` instead where a zero at its usual place would wipe out what the case computes."""
    a = co.random_field(field, seed, n)
    sp = co.to_mont(field, co.ints_to_limbs(special_values(field)))
    for i in range(len(sp)):
        if i == 0 and zero_at is not None:
            if 0 <= zero_at < n:
                a[zero_at] = sp[0]
            continue
        a[(1 + 37 * i) % n] = sp[i]
    return a


# where the special values land in a vector of 8: index -> value (index 4 keeps its random element)
PLANTED_8 = {0: "p - 1", 1: "0", 2: "R^-1", 3: "2", 5: "2^255", 6: "1", 7: "R"}


def fe(field, v):
    """one element given as an integer: Montgomery limbs"""
    return fields.scalar_limbs(v % fields.MODULUS[field], field, True)


def bases_with_identity(curve, seed, n):
    g = co.generate_bases(curve, seed, n)
    if n > 2:
        g[n // 2] = 0
    return g


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to("cuda:0")


def host(t):
    return np.ascontiguousarray(t.cpu().numpy().view(np.uint64))


def sync():
    import torch
    torch.cuda.synchronize()


def _p(a):
    return a.ctypes.data_as(u64p)


def ok(rc):
    assert rc == 0, (rc, h.lib().h2_last_error())


def same(got, form, field, want):
    """bit-exact at every index against the oracle's result in the form of the call"""
    got = host(got) if hasattr(got, "cpu") else np.ascontiguousarray(got, dtype=np.uint64)
    want = conv(form, field, want)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got.reshape(-1, 4) != want.reshape(-1, 4)).any(axis=1))
        raise AssertionError(f"form {form}: {bad.size} of {got.size // 4} elements differ, first at index {bad[0]}")


def check_point(curve, form, out, want_jac):
    """A 12- or 8-limb output in `form` against the oracle's Jacobian result: the same canonical affine point; an affine output
    also byte for byte; the identity as Z = 0 / 64 zero bytes."""
    bf = co.field_of_curve(curve, "base")
    out = host(out) if hasattr(out, "cpu") else np.ascontiguousarray(out, dtype=np.uint64)
    want = co.jac_to_affine_ints(curve, np.ascontiguousarray(want_jac, dtype=np.uint64))
    as_mont = conv(MONT, bf, out) if form == MONT else mont(bf, out)
    if out.shape[0] == 12:
        assert co.jac_to_affine_ints(curve, as_mont) == want, f"form {form}, Jacobian"
        if want is None:
            assert not out[8:].any()
    else:
        assert out.shape[0] == 8
        assert co.affine_to_ints(curve, as_mont) == want, f"form {form}, affine"
        assert np.array_equal(out, conv(form, bf, co.points_to_mont(curve, [want])[0])), f"form {form}, affine bytes"


def last_path():
    import torch
    p, g, t, c = C.c_int(), C.c_int(), C.c_uint(), C.c_int()
    ok(h.lib().h2_msm_last_path(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(p), C.byref(g), C.byref(t), C.byref(c)))
    return p.value, c.value


def table_bits(handle):
    n, c = C.c_size_t(0), C.c_int(0)
    ok(h.lib().h2_bases_info(handle, C.byref(n), C.byref(c), None))
    return n.value, c.value


@contextlib.contextmanager
def ntt_passes_launched(expect):
    """The body's transforms launched exactly `expect` pass kernels (profiling never changes an NTT)."""
    lib = h.lib()
    ok(lib.h2_profile_enable(1))
    ms, cnt = C.c_double(0), C.c_uint64(0)
    try:
        yield
        sync()
        ok(lib.h2_profile_read(PROF_NTT_PASS, C.byref(ms), C.byref(cnt)))
    finally:
        lib.h2_profile_enable(0)
    assert cnt.value == expect, (cnt.value, expect)


# ---------------------------------------------------------------------------------------------------- a. registered commits
def _size_for_window(bits):
    """(n, column table) with the smallest n = 2^i + 3 whose registered table has `bits`-bit windows; 17 bits are a column table's
    (h2_commit_column_window_bits), at the first power of two that gets them."""
    lib = h.lib()
    if bits == 17:
        return next(1 << i for i in range(4, 22) if lib.h2_commit_column_window_bits(1 << i) == 17), True
    return next((1 << i) + 3 for i in range(4, 22) if lib.h2_commit_window_bits((1 << i) + 3) == bits), False


def test_registered_window_widths_are_the_documented_ones():
    """8 / 13 / 16 bits, 17 for column tables from 2^18 points; the cases below take one size of each."""
    lib = h.lib()
    assert sorted({lib.h2_commit_window_bits((1 << i) + 3) for i in range(4, 22)}) == [8, 13, 16]
    assert _size_for_window(17) == (1 << 18, True)


@pytest.mark.parametrize("curve,bits", [(c, b) for b in (8, 13, 16) for c in CURVES] + [(h.VESTA, 17)])
def test_registered_commits(curve, bits):
    """h2_bases_register with canonical points, h2_bases_set_blind_base with a canonical w, then h2_commit, h2_commit_device,
    h2_commit_batch_device (three unequal columns, one all zero) and h2_commit_range_device (two uneven ranges, summed by
    h2_points_sum_device) with canonical scalars and blinds, Jacobian and affine, against the oracle's Params::commit."""
    import torch
    lib = h.lib()
    n, column_table = _size_for_window(bits)
    sf, bf = co.field_of_curve(curve, "scalar"), co.field_of_curve(curve, "base")
    g = bases_with_identity(curve, 0xA100 + bits + curve, n)
    w = co.generate_bases(curve, 0xA200 + curve, 1)[0]
    cols = [planted(sf, 0xA300 + bits, n), np.zeros((n, 4), dtype=np.uint64), co.random_field(sf, 0xA301 + bits, n)]
    cols[2][::3] = 0
    blinds = planted(sf, 0xA400, 8)[[7, 4, 5]]                           # R mod p, a random element, 2^255 mod p (PLANTED_8)
    wants = [co.commit(curve, g, w, cols[i], blinds[i]) for i in range(3)]
    cut = n // 3 + 1
    want_lo = co.best_multiexp(curve, cols[0][:cut], g[:cut])
    want_hi = co.commit(curve, np.ascontiguousarray(g[cut:]), w, np.ascontiguousarray(cols[0][cut:]), blinds[0])
    zero_jac = np.zeros(12, dtype=np.uint64)
    vp3 = C.c_void_p * 3
    for form in FORMS:
        hd = C.c_uint64(0)
        g_f = conv(form, bf, g)
        if column_table:
            ok(lib.h2_bases_register_ex(curve, _p(g_f), n, form, 17, C.byref(hd)))
        else:
            ok(lib.h2_bases_register(curve, _p(g_f), n, form, C.byref(hd)))
        assert table_bits(hd) == (n, bits)
        ok(lib.h2_bases_set_blind_base(hd, _p(conv(form, bf, w)), form))
        cols_f = [conv(form, sf, c_) for c_ in cols]
        blinds_f = conv(form, sf, blinds)
        d_cols, d_bl = [dev(c_) for c_ in cols_f], dev(blinds_f)
        for kind in (JAC, AFF):
            width = 8 if kind else 12
            out = np.zeros(width, dtype=np.uint64)
            ok(lib.h2_commit(hd, _p(cols_f[0]), n, None, _p(blinds_f[0]), form, kind, _p(out)))
            check_point(curve, form, out, wants[0])
            d_out = torch.zeros(width, dtype=torch.int64, device="cuda:0")
            ok(lib.h2_commit_device(hd, d_cols[0].data_ptr(), n, None, d_bl[0].data_ptr(), form, kind, d_out.data_ptr(), None))
            sync()
            check_point(curve, form, d_out, wants[0])
            d_outs = torch.zeros((3, width), dtype=torch.int64, device="cuda:0")
            ok(lib.h2_commit_batch_device(hd, vp3(*[t.data_ptr() for t in d_cols]), 3, n, None, vp3(*[d_bl[i].data_ptr() for i in range(3)]),
                                          form, kind, vp3(*[d_outs[i].data_ptr() for i in range(3)]), None))
            sync()
            for i in range(3):
                check_point(curve, form, d_outs[i], wants[i])
            # two uneven ranges: Jacobian partials (what a split commit gathers), their sum in the form and kind of the call
            parts = torch.zeros((2, 12), dtype=torch.int64, device="cuda:0")
            ok(lib.h2_commit_range_device(hd, d_cols[0].data_ptr(), 0, cut, None, form, JAC, parts[0].data_ptr(), None))
            ok(lib.h2_commit_range_device(hd, d_cols[0][cut:].data_ptr(), cut, n - cut, d_bl[0].data_ptr(), form, JAC, parts[1].data_ptr(), None))
            total = torch.zeros(width, dtype=torch.int64, device="cuda:0")
            ok(lib.h2_points_sum_device(curve, parts.data_ptr(), 2, form, kind, total.data_ptr(), None))
            one = torch.zeros(width, dtype=torch.int64, device="cuda:0")
            ok(lib.h2_commit_range_device(hd, d_cols[0][cut:].data_ptr(), cut, n - cut, d_bl[0].data_ptr(), form, kind, one.data_ptr(), None))
            sync()
            check_point(curve, form, parts[0], want_lo)
            check_point(curve, form, parts[1], want_hi)
            check_point(curve, form, total, wants[0])
            check_point(curve, form, one, want_hi)
            # an all-zero column without a blind is the identity in the form asked for: 64 zero bytes / Z = 0
            ok(lib.h2_commit_device(hd, d_cols[1].data_ptr(), n, None, None, form, kind, d_out.data_ptr(), None))
            sync()
            check_point(curve, form, d_out, zero_jac)
            assert not host(d_out)[-4:].any() and (kind == JAC or not host(d_out).any())
        ok(lib.h2_bases_free(hd))


@pytest.mark.parametrize("curve", CURVES)
def test_registration_from_device_memory_and_with_a_chosen_width(curve):
    """One size through h2_bases_register_device (canonical points in HBM) and h2_bases_register_ex (a width that is not the default),
    with the blind base presented to the commit as a canonical device point (msm_blind_install's form on the commit's stream)."""
    import torch
    lib = h.lib()
    n = (1 << 13) + 3
    default = lib.h2_commit_window_bits(n)
    chosen = 13 if default != 13 else 16
    sf, bf = co.field_of_curve(curve, "scalar"), co.field_of_curve(curve, "base")
    g = bases_with_identity(curve, 0xA500 + curve, n)
    w = co.generate_bases(curve, 0xA501 + curve, 1)[0]
    col, blind = planted(sf, 0xA502, n), planted(sf, 0xA503, 8)[7]
    want = co.commit(curve, g, w, col, blind)
    for form in FORMS:
        g_f = conv(form, bf, g)
        d_g, d_w = dev(g_f), dev(conv(form, bf, w))
        d_col, d_bl = dev(conv(form, sf, col)), dev(conv(form, sf, blind))
        for how in ("device", "ex"):
            hd = C.c_uint64(0)
            if how == "device":
                ok(lib.h2_bases_register_device(curve, d_g.data_ptr(), n, form, C.byref(hd)))
                assert table_bits(hd) == (n, default)
            else:
                ok(lib.h2_bases_register_ex(curve, _p(g_f), n, form, chosen, C.byref(hd)))
                assert table_bits(hd) == (n, chosen)
            for kind in (JAC, AFF):
                d_out = torch.zeros(8 if kind else 12, dtype=torch.int64, device="cuda:0")
                ok(lib.h2_commit_device(hd, d_col.data_ptr(), n, d_w.data_ptr(), d_bl.data_ptr(), form, kind, d_out.data_ptr(), None))
                sync()
                check_point(curve, form, d_out, want)
            ok(lib.h2_bases_free(hd))
        assert np.array_equal(host(d_g), g_f)                               # the caller's points are not converted in place


def _pair_size(kind):
    """A table size n (g || u || u || w || w) for h2_commit_pair_device.  The sub-digit form takes tables of up to 2^16 + 4 points with
    16-bit windows (csrc/msm_subdigit.hip); any other supported table takes the general form."""
    lib = h.lib()
    sub = lambda n: n <= (1 << 16) + 4 and lib.h2_commit_window_bits(n) == 16
    sizes = [(1 << i) + 4 for i in range(12, 18)]
    return next(n for n in sizes if lib.h2_commit_pair_supported(n) and sub(n) == (kind == "sub_digit"))


@pytest.mark.parametrize("kind", ["sub_digit", "general"])
@pytest.mark.parametrize("curve", CURVES)
def test_paired_commit(curve, kind):
    """h2_commit_pair_device over a table registered from canonical points, canonical scalars: both outputs against the oracle's
    multiexp over g || u || u || w || w with the other side's scalars zeroed, for two shifts, Jacobian and affine."""
    import torch
    lib = h.lib()
    n = _pair_size(kind)
    assert lib.h2_commit_pair_supported(n) == 1
    sf, bf = co.field_of_curve(curve, "scalar"), co.field_of_curve(curve, "base")
    g = co.generate_bases(curve, 0xA600 + curve, n - 4)
    u, w = co.generate_bases(curve, 0xA601, 1)[0], co.generate_bases(curve, 0xA602, 1)[0]
    basis = np.ascontiguousarray(np.concatenate([g, np.stack([u, u, w, w])]))
    col = planted(sf, 0xA603, n)
    idx = np.arange(n)
    shifts = (0, 5)
    wants = {}
    for shift in shifts:
        side = np.where(idx < n - 4, (idx >> shift) & 1, (idx - (n - 4)) & 1)
        for s_ in (0, 1):
            part = col.copy()
            part[side != s_] = 0
            wants[shift, s_] = co.best_multiexp(curve, part, basis)
    for form in FORMS:
        hd = C.c_uint64(0)
        ok(lib.h2_bases_register(curve, _p(conv(form, bf, basis)), n, form, C.byref(hd)))
        bits = table_bits(hd)[1]
        assert (bits == 16 and n <= (1 << 16) + 4) == (kind == "sub_digit"), (n, bits)
        d_col = dev(conv(form, sf, col))
        for shift in shifts:
            for out_kind in (JAC, AFF):
                d_out = torch.zeros((2, 8 if out_kind else 12), dtype=torch.int64, device="cuda:0")
                ok(lib.h2_commit_pair_device(hd, d_col.data_ptr(), n, shift, form, out_kind, d_out.data_ptr(), None))
                sync()
                for s_ in (0, 1):
                    check_point(curve, form, d_out[s_], wants[shift, s_])
        ok(lib.h2_bases_free(hd))


# ---------------------------------------------------------------------------------------------------- b. the blind-base cache
SEARCH_BOUND = 256


@pytest.mark.parametrize("curve", CURVES)
def test_blind_base_cache_is_keyed_by_bytes_and_form(curve):
    """set_blind_base_host skips the install when (bytes, form) repeat.  Forms alternate on ONE handle and every commit must use the
    w of the latest install.

    The sharpest input would be 64 bytes B that are a curve point under both readings.  No such point exists: (x, y) and
    (x / R, y / R) both on y^2 = x^3 + 5 force x^3 = 5 R (R + 1), and then on Pallas x^3 + 5 is not a square while on Vesta 5 R (R + 1)
    is not a cube (both asserted below, with a search of the first SEARCH_BOUND = 256 multiples of the generator that finds none).  So
    two different byte strings are used: B1, the canonical bytes of P1, and B2, the Montgomery bytes of P2; and also the Montgomery
    bytes of P1, the same point arriving in the other form."""
    import torch
    lib = h.lib()
    bm, _ = o.CURVES[curve]
    r_inv = pow(o.R, -1, bm)
    both = lambda pt: o.on_curve(pt, bm) and o.on_curve((pt[0] * r_inv % bm, pt[1] * r_inv % bm), bm)
    pt, found = None, []
    for k in range(1, SEARCH_BOUND + 1):
        pt = o.ec_add(pt, (bm - 1, 2), bm) if pt else (bm - 1, 2)
        if both(pt):
            found.append(k)
    assert not found
    x3 = 5 * o.R * (o.R + 1) % bm
    assert pow(x3, (bm - 1) // 3, bm) != 1 or pow((x3 + 5) % bm, (bm - 1) // 2, bm) != 1
    n = 600
    sf, bf = co.field_of_curve(curve, "scalar"), co.field_of_curve(curve, "base")
    g = co.generate_bases(curve, 0xB100 + curve, n)
    col, blind = planted(sf, 0xB101, n), planted(sf, 0xB102, 8)[7]
    p1, p2 = co.points_to_mont(curve, [o.ec_mul(0x1234567, (bm - 1, 2), bm), o.ec_mul(0x89ABCD, (bm - 1, 2), bm)])
    want = {1: co.commit(curve, g, p1, col, blind), 2: co.commit(curve, g, p2, col, blind)}
    hd = C.c_uint64(0)
    ok(lib.h2_bases_register(curve, _p(can(bf, g)), n, CAN, C.byref(hd)))
    d_col, d_bl = dev(can(sf, col)), dev(can(sf, blind))
    d_out = torch.zeros(8, dtype=torch.int64, device="cuda:0")
    b1_can, b1_mont, b2_mont = can(bf, p1), p1, p2
    for step, (bytes_, form, which) in enumerate([(b1_can, CAN, 1), (b2_mont, MONT, 2), (b1_can, CAN, 1), (b1_mont, MONT, 1), (b1_can, CAN, 1),
                                                  (b1_can, CAN, 1), (can(bf, p2), CAN, 2), (b2_mont, MONT, 2)]):
        ok(lib.h2_bases_set_blind_base(hd, _p(np.ascontiguousarray(bytes_)), form))
        ok(lib.h2_commit_device(hd, d_col.data_ptr(), n, None, d_bl.data_ptr(), CAN, AFF, d_out.data_ptr(), None))
        sync()
        try:
            check_point(curve, CAN, d_out, want[which])
        except AssertionError as e:
            raise AssertionError(f"step {step}: w installed in form {form}") from e
    ok(lib.h2_bases_free(hd))


# ---------------------------------------------------------------------------------------------------- c. generic multiexp
GENERIC = [(2048, PATH_ONE_PASS, 10), (2049, PATH_ONE_PASS, 13), (65536, PATH_TWO_PASS, 13), ((1 << 18) + 1, PATH_GROUPED_LATENCY, 16)]


@pytest.mark.parametrize("n,path,bits", GENERIC)
@pytest.mark.parametrize("curve", CURVES)
def test_generic_multiexp(curve, n, path, bits):
    """h2_msm (host pointers) and h2_msm_device with canonical scalars AND canonical bases, Jacobian and affine, one size per form of
    the dispatch (read back with h2_msm_last_path); and the empty multiexp, the identity in the form asked for."""
    lib = h.lib()
    sf, bf = co.field_of_curve(curve, "scalar"), co.field_of_curve(curve, "base")
    g = bases_with_identity(curve, 0xC100 + curve, n)
    s = planted(sf, 0xC101 + n % 89, n)
    want = co.best_multiexp(curve, s, g)
    for form in FORMS:
        s_f, g_f = conv(form, sf, s), conv(form, bf, g)
        d_s, d_g = dev(s_f), dev(g_f)
        for affine in (False, True):
            check_point(curve, form, h.best_multiexp(s_f, g_f, curve, form, affine), want)            # h2_msm
            sync()
            out = h.best_multiexp(d_s, d_g, curve, form, affine)                                       # h2_msm_device
            assert last_path() == (path, bits)
            sync()
            check_point(curve, form, out, want)
            if n == GENERIC[0][0]:
                check_point(curve, form, h.best_multiexp(d_s[:0], d_g[:0], curve, form, affine), np.zeros(12, dtype=np.uint64))
                check_point(curve, form, h.best_multiexp(s_f[:0], g_f[:0], curve, form, affine), np.zeros(12, dtype=np.uint64))
        assert np.array_equal(host(d_g), g_f) and np.array_equal(host(d_s), s_f)                       # converted on a private copy
    assert lib.h2_msm_window_bits(n) == bits


@pytest.mark.parametrize("curve", CURVES)
def test_generic_multiexp_batch(curve):
    """h2_msm_batch_device with two pairs of unequal length, canonical scalars and bases."""
    sf, bf = co.field_of_curve(curve, "scalar"), co.field_of_curve(curve, "base")
    sizes = (2049, 300)
    gs = [bases_with_identity(curve, 0xC200 + i + curve, n) for i, n in enumerate(sizes)]
    ss = [planted(sf, 0xC210 + i, n) for i, n in enumerate(sizes)]
    wants = [co.best_multiexp(curve, s, g) for s, g in zip(ss, gs)]
    for form in FORMS:
        pairs = [(dev(conv(form, sf, s)), dev(conv(form, bf, g))) for s, g in zip(ss, gs)]
        for affine in (False, True):
            out = best_multiexp_batch(pairs, curve, form, affine)                                      # h2_msm_batch_device
            sync()
            for i in range(2):
                check_point(curve, form, out[i], wants[i])


# ---------------------------------------------------------------------------------------------------- d. poly.hip
POLY_SIZES = [1, 2, 8, 9, 2047, 2048, 2049, (1 << 19) + 3]          # the tile edges; 2^19 + 3: the carry kernels' per = 2 arm


def eval_points(field, seed):
    """x in {0, 1, p - 1, random}, Montgomery limbs"""
    return [fe(field, 0), fe(field, 1), fe(field, -1), co.random_field(field, seed, 1)[0]]


@pytest.mark.parametrize("n", POLY_SIZES)
@pytest.mark.parametrize("field", FIELDS)
def test_eval_polynomial_and_inner_product(field, n):
    a, b = planted(field, 0xD100 + n % 97, n), planted(field, 0xD101 + n % 97, n)[::-1].copy()
    for x in eval_points(field, 0xD102):
        want = co.eval_polynomial(field, a, x)
        for form in FORMS:
            a_f, x_f = conv(form, field, a), conv(form, field, x)
            same(h.eval_polynomial(a_f, x_f, field, form), form, field, want)                 # h2_eval_polynomial
            same(h.eval_polynomial(dev(a_f), x_f, field, form), form, field, want)            # h2_eval_polynomial_device
    want = co.inner_product(field, a, b)
    for form in FORMS:
        a_f, b_f = conv(form, field, a), conv(form, field, b)
        same(h.compute_inner_product(a_f, b_f, field, form), form, field, want)               # h2_inner_product
        same(h.compute_inner_product(dev(a_f), dev(b_f), field, form), form, field, want)     # h2_inner_product_device


@pytest.mark.parametrize("n", POLY_SIZES)
@pytest.mark.parametrize("field", FIELDS)
def test_kate_division_powers_scale_add(field, n):
    import torch
    a, b = planted(field, 0xD200 + n % 97, n), planted(field, 0xD201 + n % 97, n)[::-1].copy()
    for x in eval_points(field, 0xD202):
        want_q, want_p, want_s = co.kate_division(field, a, x), co.powers(field, x, n), co.scale_add(field, a, x, b)
        for form in FORMS:
            a_f, b_f, x_f = conv(form, field, a), conv(form, field, b), conv(form, field, x)
            same(h.kate_division(a_f, x_f, field, form), form, field, want_q)                 # h2_kate_division
            same(h.kate_division(dev(a_f), x_f, field, form), form, field, want_q)            # h2_kate_division_device
            same(h.powers(x_f, n, field, form), form, field, want_p)                          # h2_powers
            same(h.powers(x_f, n, field, form, device=torch.device("cuda:0")), form, field, want_p)     # h2_powers_device
            same(h.scale_add(a_f, x_f, b_f, field, form), form, field, want_s)                # h2_scale_add
            same(h.scale_add(dev(a_f), x_f, dev(b_f), field, form), form, field, want_s)      # h2_scale_add_device


def _with_zeros(a, pattern):
    """BatchInvert leaves zeros alone: a lane's 8 consecutive elements, a whole 64-element group and a whole 2048-element tile
    ("runs"), or everything up to the first tile's end ("first_tile")."""
    a, n = a.copy(), a.shape[0]
    if pattern == "first_tile":
        a[:2048] = 0
        return a
    for lo, hi in ((8, 16), (64, 128), (2048, 4096)):
        if n >= hi:
            a[lo:hi] = 0
    return a


@pytest.mark.parametrize("pattern", ["runs", "first_tile"])
@pytest.mark.parametrize("n", POLY_SIZES)
@pytest.mark.parametrize("field", FIELDS)
def test_batch_invert(field, n, pattern):
    a = _with_zeros(planted(field, 0xD300 + n % 97, n), pattern)
    want = co.batch_invert(field, a)
    for form in FORMS:
        a_f = conv(form, field, a)
        same(h.batch_invert(a_f, field, form), form, field, want)                             # h2_batch_invert
        same(h.batch_invert(dev(a_f), field, form), form, field, want)                        # h2_batch_invert_device


@pytest.mark.parametrize("n", POLY_SIZES)
@pytest.mark.parametrize("field", FIELDS)
def test_grand_product(field, n):
    m_ = planted(field, 0xD400 + n % 97, n, zero_at=n - 2)                # a zero factor only where it leaves z[0 .. n-2] alone
    for init in (fe(field, 1), co.random_field(field, 0xD401, 1)[0]):
        want = co.grand_product(field, m_, n, init)
        for form in FORMS:
            m_f, i_f = conv(form, field, m_), conv(form, field, init)
            same(h.grand_product(m_f, n, i_f, field, form), form, field, want)                # h2_grand_product
            same(h.grand_product(dev(m_f), n, i_f, field, form), form, field, want)           # h2_grand_product_device


def _inverses(vals, m):
    """1 / v mod m over integers, 0 for 0: one modular inversion for the whole list (prefix products), so that half a million
    elements cost half a second"""
    prefix, acc = [], 1
    for v in vals:
        prefix.append(acc)
        if v:
            acc = acc * v % m
    inv, out = pow(acc, -1, m), [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        if vals[i]:
            out[i] = inv * prefix[i] % m
            inv = inv * vals[i] % m
    return out


@pytest.mark.parametrize("n", POLY_SIZES)
@pytest.mark.parametrize("field", FIELDS)
def test_assigned_to_field(field, n):
    """num / den with x / 0 = 0 and a denominator ONE kept out of the inversion -- canonical 1 and Montgomery 1 are different bytes,
    and both are among the planted denominators -- against the quotient over Python integers."""
    m = fields.MODULUS[field]
    num, den = planted(field, 0xD500 + n % 97, n), planted(field, 0xD501 + n % 97, n)[::-1].copy()
    den[5::7] = fe(field, 1)
    den[3::11] = 0
    ni, di = co.limbs_to_ints(can(field, num)), co.limbs_to_ints(can(field, den))
    want = mont(field, co.ints_to_limbs([a * d_inv % m for a, d_inv in zip(ni, _inverses(di, m))]))
    for form in FORMS:
        n_f, d_f = conv(form, field, num), conv(form, field, den)
        same(assigned_to_field(n_f, d_f, field, form), form, field, want)                     # h2_assigned_to_field
        same(assigned_to_field(dev(n_f), dev(d_f), field, form), form, field, want)           # h2_assigned_to_field_device
        same(assigned_to_field(n_f, None, field, form), form, field, num)
        same(assigned_to_field(dev(n_f), None, field, form), form, field, num)


# ---------------------------------------------------------------------------------------------------- e. NTT family
def _sizes_by_passes(kind):
    """k = 1, the largest single-pass size and the smallest two-pass size of the default plan of `kind` (tests/ntt_shapes.py)."""
    one = max(L for L in range(2, 23) if len(ns.passes(L, kind)) == 1)
    two = min(L for L in range(2, 23) if len(ns.passes(L, kind)) == 2)
    return [1, one, two]


def _inverse_factors(field, L):
    m = fields.MODULUS[field]
    return fe(field, pow(o.omega_for(m, L), -1, m)), fe(field, pow(1 << L, -1, m))


@pytest.mark.parametrize("L", _sizes_by_passes(0))
@pytest.mark.parametrize("field", FIELDS)
def test_ntt_and_ifft(field, L):
    """h2_ntt / h2_ntt_device with a canonical omega, h2_ifft / h2_ifft_device with canonical omega^-1 and 1 / n: the kernels are the
    Montgomery ones and the host converts the factors (ntt.hip), so this is the linearity claim under test."""
    lib = h.lib()
    n = 1 << L
    a = planted(field, 0xE100 + L, n)
    omega = co.random_field(field, 0xE101 + L, 1)[0]
    omega_inv, divisor = _inverse_factors(field, L)
    want_f, want_i = co.best_fft(field, a, omega, L), co.ifft(field, a, omega_inv, L, divisor)
    passes = len(ns.passes(L, 0))
    for form in FORMS:
        a_f, w_f, wi_f, dv_f = (conv(form, field, v) for v in (a, omega, omega_inv, divisor))
        same(h.best_fft(a_f.copy(), w_f, L, field, form), form, field, want_f)                # h2_ntt
        d = dev(a_f)
        with ntt_passes_launched(passes):
            h.best_fft(d, w_f, L, field, form)                                                # h2_ntt_device
        same(d, form, field, want_f)
        b = a_f.copy()
        ok(lib.h2_ifft(field, _p(b), L, _p(wi_f), _p(dv_f), form))
        same(b, form, field, want_i)
        d = dev(a_f)
        with ntt_passes_launched(passes):
            ok(lib.h2_ifft_device(field, d.data_ptr(), L, _p(wi_f), _p(dv_f), form, None))
        same(d, form, field, want_i)


@pytest.mark.parametrize("L", _sizes_by_passes(1))
@pytest.mark.parametrize("field", FIELDS)
def test_batched_ntt_and_ifft(field, L):
    """h2_ntt_batch_device / h2_ifft_batch_device over three columns (the batched plan), canonical columns and factors."""
    lib = h.lib()
    n = 1 << L
    cols = [planted(field, 0xE200 + 4 * L + i, n) for i in range(3)]
    omega = co.random_field(field, 0xE201 + L, 1)[0]
    omega_inv, divisor = _inverse_factors(field, L)
    wants_f = [co.best_fft(field, c_, omega, L) for c_ in cols]
    wants_i = [co.ifft(field, c_, omega_inv, L, divisor) for c_ in cols]
    passes = 3 * len(ns.passes(L, 1))
    for form in FORMS:
        w_f, wi_f, dv_f = (conv(form, field, v) for v in (omega, omega_inv, divisor))
        d = [dev(conv(form, field, c_)) for c_ in cols]
        with ntt_passes_launched(passes):
            h.best_fft_batch(d, w_f, L, field, form)                                          # h2_ntt_batch_device
        for t, want in zip(d, wants_f):
            same(t, form, field, want)
        d = [dev(conv(form, field, c_)) for c_ in cols]
        arr = (C.c_void_p * 3)(*[t.data_ptr() for t in d])
        with ntt_passes_launched(passes):
            ok(lib.h2_ifft_batch_device(field, arr, 3, L, _p(wi_f), _p(dv_f), form, None))
        for t, want in zip(d, wants_i):
            same(t, form, field, want)


def _extended_pairs():
    two = min(L for L in range(2, 23) if len(ns.passes(L, 0)) == 2)
    return [(5, 7), (two - 2, two)]


@pytest.mark.parametrize("k,ext_k", _extended_pairs())
@pytest.mark.parametrize("field", FIELDS)
def test_extended_domain_transforms(field, k, ext_k):
    """h2_coeff_to_extended, h2_extended_to_coeff and h2_divide_by_vanishing_poly, host and device, with g_coset, g_coset^-1, the
    extended omega, the divisor and the nt = 2^(ext_k - k) t_evaluations of EvaluationDomain(5, k) all passed in canonical form."""
    import torch
    lib = h.lib()
    ref = o.EvaluationDomain(5, k, fields.MODULUS[field])
    assert ref.extended_k == ext_k and len(ns.passes(ext_k, 0)) == (1 if k == 5 else 2)
    a, e = planted(field, 0xE300 + k, 1 << k), planted(field, 0xE301 + k, 1 << ext_k)
    c = lambda v: fe(field, v)
    t_evals = mont(field, co.ints_to_limbs(ref.t_evaluations))
    want_ext = co.coeff_to_extended(field, a, k, ext_k, c(ref.g_coset), c(ref.g_coset_inv), c(ref.extended_omega))
    want_back = co.extended_to_coeff(field, e, ext_k, c(ref.g_coset), c(ref.g_coset_inv), c(ref.extended_omega_inv), c(ref.extended_ifft_divisor))
    want_div = co.divide_by_vanishing_poly(field, e, ext_k, t_evals)
    for form in FORMS:
        f = lambda v: conv(form, field, c(v))
        a_f, e_f, t_f = conv(form, field, a), conv(form, field, e), conv(form, field, t_evals)
        gc, gci, eo, eoi, edv = f(ref.g_coset), f(ref.g_coset_inv), f(ref.extended_omega), f(ref.extended_omega_inv), f(ref.extended_ifft_divisor)
        out = np.zeros((1 << ext_k, 4), dtype=np.uint64)
        ok(lib.h2_coeff_to_extended(field, _p(a_f), _p(out), k, ext_k, _p(gc), _p(gci), _p(eo), form))
        same(out, form, field, want_ext)
        d_a, d_out = dev(a_f), torch.zeros((1 << ext_k, 4), dtype=torch.int64, device="cuda:0")
        ok(lib.h2_coeff_to_extended_device(field, d_a.data_ptr(), d_out.data_ptr(), k, ext_k, _p(gc), _p(gci), _p(eo), form, None))
        same(d_out, form, field, want_ext)
        b = e_f.copy()
        ok(lib.h2_extended_to_coeff(field, _p(b), ext_k, _p(gc), _p(gci), _p(eoi), _p(edv), form))
        same(b, form, field, want_back)
        d_e = dev(e_f)
        ok(lib.h2_extended_to_coeff_device(field, d_e.data_ptr(), ext_k, _p(gc), _p(gci), _p(eoi), _p(edv), form, None))
        same(d_e, form, field, want_back)
        b = e_f.copy()
        ok(lib.h2_divide_by_vanishing_poly(field, _p(b), ext_k, _p(t_f), t_f.shape[0], form))
        same(b, form, field, want_div)
        d_e = dev(e_f)
        ok(lib.h2_divide_by_vanishing_poly_device(field, d_e.data_ptr(), ext_k, _p(t_f), t_f.shape[0], form, None))
        same(d_e, form, field, want_div)


# ---------------------------------------------------------------------------------------------------- f. IPA pieces
@pytest.mark.parametrize("half", [1, 255, 256, 257])
@pytest.mark.parametrize("field", FIELDS)
def test_fold_scalars(field, half):
    a = planted(field, 0xF100 + half, 2 * half)
    for factor in (co.random_field(field, 0xF101, 1)[0], fe(field, fields.R), fe(field, -1)):
        want = co.fold_scalars(field, a, factor)
        for form in FORMS:
            a_f, x_f = conv(form, field, a), conv(form, field, factor)
            same(h.fold_scalars(a_f, x_f, field, form), form, field, want)                    # h2_fold_scalars
            same(h.fold_scalars(dev(a_f), x_f, field, form).contiguous(), form, field, want)  # h2_fold_scalars_device


@pytest.mark.parametrize("half", [1, 4, 300, 32768 + 5])
@pytest.mark.parametrize("curve", CURVES)
def test_generator_collapse(curve, half):
    """h2_generator_collapse / _device on canonical points with a canonical challenge in {1, p - 1, lambda, random}: the narrow arm
    (1, 4), the wide arm (300) and the lane-per-point arm (above 32768).  Affine in, affine out: raw canonical bytes are compared."""
    sf, bf = co.field_of_curve(curve, "scalar"), co.field_of_curve(curve, "base")
    g = co.generate_bases(curve, 0xF200 + half % 97 + curve, 2 * half)
    if half > 2:
        g[1] = 0                                                          # an identity in each half
        g[half + 2] = 0
    for u in (fe(sf, 1), fe(sf, -1), fe(sf, fields.zeta(sf)), co.random_field(sf, 0xF201, 1)[0]):
        want = co.generator_collapse(curve, g, u)
        for form in FORMS:
            g_f, u_f = conv(form, bf, g), conv(form, sf, u)
            same(h.parallel_generator_collapse(g_f, u_f, curve, form), form, bf, want)                    # h2_generator_collapse
            same(h.parallel_generator_collapse(dev(g_f), u_f, curve, form).contiguous(), form, bf, want)  # h2_generator_collapse_device


def _s_of(h_bits, us, m):
    """the product of the challenges u_r picked by the bits of h (bit len(us)-1-r <-> u_r)"""
    v = 1
    for r, u in enumerate(us):
        if (h_bits >> (len(us) - 1 - r)) & 1:
            v = v * u % m
    return v


@pytest.mark.parametrize("k,j", [(1, 0), (5, 2), (9, 5)])
@pytest.mark.parametrize("field", FIELDS)
def test_ipa_round_scalars(field, k, j):
    """h2_ipa_round_scalars_device with a canonical p' and canonical challenges: cl / cr against the definition over integers,
    compared as limbs of the form of the call."""
    import torch
    m = fields.MODULUS[field]
    n, blk = 1 << k, k - j
    half = 1 << (blk - 1)
    p_l = planted(field, 0xF300 + k, 1 << blk)
    u_l = planted(field, 0xF301 + k, 8, zero_at=-1)[[7, 4, 0, 2, 5]][:j]            # R, a random element, p - 1, R^-1, 2^255 (PLANTED_8)
    p_i, u_i = co.limbs_to_ints(can(field, p_l)), co.limbs_to_ints(can(field, u_l)) if j else []
    want_l, want_r = [], []
    for idx in range(n):
        hh, i = idx >> blk, idx & ((1 << blk) - 1)
        v = p_i[i ^ half] * _s_of(hh, u_i, m) % m
        want_l.append(v if i < half else 0)
        want_r.append(0 if i < half else v)
    want_l, want_r = mont(field, co.ints_to_limbs(want_l)), mont(field, co.ints_to_limbs(want_r))
    for form in FORMS:
        d_p = dev(conv(form, field, p_l))
        d_l = torch.full((n, 4), -1, dtype=torch.int64, device="cuda:0")
        d_r = torch.full((n, 4), -1, dtype=torch.int64, device="cuda:0")
        ipa_round_scalars(d_p, k, j, [conv(form, field, u_l[r]) for r in range(j)], field, d_l, d_r, form)
        same(d_l, form, field, want_l)
        same(d_r, form, field, want_r)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("field", FIELDS)
def test_ipa_s_combine(field, accumulate):
    """h2_ipa_s_combine / _device with canonical challenges, coefficients and output (and a canonical vector to add to): the sum of
    coeffs[b] * compute_s(u_b, 1) over integers."""
    m = fields.MODULUS[field]
    k, batch = 6, 3
    ch = planted(field, 0xF400, batch * k, zero_at=-1)
    cf = planted(field, 0xF401, 8, zero_at=-1)[[7, 0, 4]]                 # R, p - 1, a random element (PLANTED_8)
    init = planted(field, 0xF402, 1 << k)
    ch_i, cf_i, init_i = (co.limbs_to_ints(can(field, v)) for v in (ch, cf, init))
    want = []
    for idx in range(1 << k):
        s = sum(cf_i[b] * _s_of(idx, ch_i[b * k:(b + 1) * k], m) for b in range(batch))
        want.append((s + (init_i[idx] if accumulate else 0)) % m)
    want = mont(field, co.ints_to_limbs(want))
    for form in FORMS:
        ch_f, cf_f = conv(form, field, ch), conv(form, field, cf)
        start = conv(form, field, init) if accumulate else np.full((1 << k, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        out = start.copy()
        ipa_s_combine(k, ch_f, cf_f, field, out, form, bool(accumulate))                      # h2_ipa_s_combine
        same(out, form, field, want)
        d_out = dev(start)
        ipa_s_combine(k, ch_f, cf_f, field, d_out, form, bool(accumulate))                    # h2_ipa_s_combine_device
        same(d_out, form, field, want)


@pytest.mark.parametrize("curve", CURVES)
def test_collapsed_generators(curve):
    """h2_ipa_collapsed_generators_device at k = 16, rounds 1 and 3, with canonical challenges (the table and the output are Montgomery
    either way): G'[i] = sum_h s(h) G[i + h 2^(k - rounds)] against the oracle's multiexp at sampled i, and the whole output of the
    canonical call equal to the Montgomery call's."""
    import torch
    lib = h.lib()
    k = 16
    n = 1 << k
    sf = co.field_of_curve(curve, "scalar")
    m = fields.MODULUS[sf]
    g = co.generate_bases(curve, 0xF500 + curve, n)
    hd = C.c_uint64(0)
    ok(lib.h2_bases_register(curve, _p(g), n, MONT, C.byref(hd)))
    assert table_bits(hd) == (n, 16)
    for rounds in (1, 3):
        nj = 1 << (k - rounds)
        ch = planted(sf, 0xF501, 8, zero_at=-1)[[7, 0, 4]][:rounds]                 # R mod p, p - 1, a random element (PLANTED_8)
        u_i = co.limbs_to_ints(can(sf, ch))
        s_l = mont(sf, co.ints_to_limbs([_s_of(hh, u_i, m) for hh in range(1 << rounds)]))
        outs = {}
        for form in FORMS:
            d_out = torch.zeros((nj, 8), dtype=torch.int64, device="cuda:0")
            ok(lib.h2_ipa_collapsed_generators_device(hd, k, rounds, _p(conv(form, sf, ch)), form, d_out.data_ptr(), None))
            sync()
            outs[form] = host(d_out)
            for i in sorted({0, 1, nj - 1, nj // 2, (12345 * 7) % nj}):
                want = co.jac_to_affine_ints(curve, co.best_multiexp(curve, s_l, np.ascontiguousarray(g[i::nj])))
                assert co.affine_to_ints(curve, outs[form][i]) == want, (form, rounds, i)
        assert np.array_equal(outs[CAN], outs[MONT])
    ok(lib.h2_bases_free(hd))


# ---------------------------------------------------------------------------------------------------- g. points and lookups
@pytest.mark.parametrize("k", [1, 5, 9])
@pytest.mark.parametrize("curve", CURVES)
def test_lagrange_basis(curve, k):
    """h2_lagrange_basis / _device: canonical g in, canonical g_lagrange out (ec_load_bitrev and the store kernel of ecfft.hip)."""
    import torch
    lib = h.lib()
    bf = co.field_of_curve(curve, "base")
    g = co.generate_bases(curve, 0x6100 + k + curve, 1 << k)
    want = co.lagrange_basis(curve, g, k)
    for form in FORMS:
        g_f = conv(form, bf, g)
        same(lagrange_basis(g_f, curve, k, form), form, bf, want)                             # h2_lagrange_basis
        d_g, d_out = dev(g_f), torch.zeros((1 << k, 8), dtype=torch.int64, device="cuda:0")
        ok(lib.h2_lagrange_basis_device(curve, d_g.data_ptr(), d_out.data_ptr(), k, form, None))
        same(d_out, form, bf, want)
        assert np.array_equal(host(d_g), g_f)


@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("curve", CURVES)
def test_points_compress_and_decompress(curve, n):
    """h2_points_compress* of canonical points and h2_points_decompress* into canonical points, the identity among them, against
    pasta_curves' encoding restated in oracle/pasta.py."""
    import torch
    lib = h.lib()
    bf = co.field_of_curve(curve, "base")
    bm = o.CURVES[curve][0]
    pts = np.concatenate([bases_with_identity(curve, 0x6200 + n + curve, n), np.zeros((1, 8), dtype=np.uint64)])      # n points, then the identity
    ints = [co.affine_to_ints(curve, p_) for p_ in pts]
    raw = b"".join(o.point_to_bytes(p_, bm) for p_ in ints)
    assert [o.point_from_bytes(raw[32 * i:32 * i + 32], bm) for i in range(n + 1)] == ints
    for count in (n, n + 1):
        want_raw, want_pts = raw[:32 * count], pts[:count]
        for form in FORMS:
            p_f = conv(form, bf, want_pts)
            assert points_to_bytes(p_f, curve, form) == want_raw                              # h2_points_compress
            d_bytes = torch.zeros(32 * count, dtype=torch.uint8, device="cuda:0")
            ok(lib.h2_points_compress_device(curve, dev(p_f).data_ptr(), count, form, d_bytes.data_ptr(), None))
            sync()
            assert d_bytes.cpu().numpy().tobytes() == want_raw
            same(points_from_bytes(want_raw, curve, form), form, bf, want_pts)                # h2_points_decompress
            d_in = torch.from_numpy(np.frombuffer(want_raw, dtype=np.uint8).copy()).to("cuda:0")
            d_xy = torch.full((count, 8), -1, dtype=torch.int64, device="cuda:0")
            ok(lib.h2_points_decompress_device(curve, d_in.data_ptr(), count, form, d_xy.data_ptr(), None))
            same(d_xy, form, bf, want_pts)


@pytest.mark.parametrize("curve", CURVES)
def test_hash_to_curve(curve):
    """h2_hash_to_curve / _device with canonical output (the h2c_kernel epilogue) against oracle/hash_to_curve.py."""
    import torch
    lib = h.lib()
    bf = co.field_of_curve(curve, "base")
    prefix = "Halo2-Parameters"
    msgs = [bytes([0]) + i.to_bytes(4, "little") for i in (0, 1, 2, 77, 1 << 20)]
    hasher = oh.hash_to_curve("vesta" if curve else "pallas", prefix)
    want = co.points_to_mont(curve, [hasher(m_) for m_ in msgs])
    flat = np.frombuffer(b"".join(msgs), dtype=np.uint8).copy()
    for form in FORMS:
        same(hash_to_curve(curve, prefix, msgs, form), form, bf, want)                        # h2_hash_to_curve
        d_msgs = torch.from_numpy(flat).to("cuda:0")
        d_out = torch.full((len(msgs), 8), -1, dtype=torch.int64, device="cuda:0")
        ok(lib.h2_hash_to_curve_device(curve, prefix.encode(), d_msgs.data_ptr(), 5, len(msgs), form, d_out.data_ptr(), None))
        same(d_out, form, bf, want)


@pytest.mark.parametrize("n", [3, 2049])
@pytest.mark.parametrize("field", FIELDS)
def test_sort(field, n):
    """h2_sort_device orders by CANONICAL value in either form: canonical limbs in, the sorted integers out."""
    a = planted(field, 0x6300 + n, n)
    a[n // 2] = a[0]                                                       # a repeated value
    want = mont(field, co.ints_to_limbs(sorted(co.limbs_to_ints(can(field, a)))))
    for form in FORMS:
        same(sort_field(dev(conv(form, field, a)), field, form), form, field, want)


def _lookup_case(usable, table_size, dup_heavy, field):
    from test_gpu_lookup import _lookup_case as make
    m = fields.MODULUS[field]
    inputs, table = make(random.Random(usable * 7 + table_size + field), m, usable, table_size, dup_heavy)
    sp = special_values(field)                                            # the planted values, in the table and looked up
    for i, v in enumerate(sp[:usable]):
        table[(1 + 37 * i) % usable] = v
    present = sorted(set(table))
    rnd = random.Random(usable)
    inputs = [v if v in present else rnd.choice(present) for v in inputs]
    for i, v in enumerate(sp[:usable]):
        if v in present:
            inputs[(3 + 41 * i) % usable] = v
    return inputs, table


@pytest.mark.parametrize("usable,table_size,dup_heavy", [(2, 1, False), (26, 4, False), (4090, 100, True)])
@pytest.mark.parametrize("field", FIELDS)
def test_permute_expression_pair(field, usable, table_size, dup_heavy):
    """h2_permute_expression_pair_device on canonical columns (lk_prepare / lk_finish / lk_assemble) against the sequential walk of
    oracle/lookup.py; a missing value is still H2_ERR_LOOKUP."""
    inputs, table = _lookup_case(usable, table_size, dup_heavy, field)
    want = olk.permute_expression_pair(inputs, table, usable)
    assert want is not None
    up = lambda ints, form: dev(fields.to_limbs(ints, field, form == MONT))
    for form in FORMS:
        a, s = permute_expression_pair(up(inputs, form), up(table, form), usable, field, form)
        assert fields.from_limbs(host(a), field, form == MONT) == want[0], form
        assert fields.from_limbs(host(s), field, form == MONT) == want[1], form
    if usable == 26:
        bad_in, bad_tab = [5, 7, 7, 9], [5, 7, 8, 8]
        assert olk.permute_expression_pair(bad_in, bad_tab, 4) is None
        for form in FORMS:
            with pytest.raises(ConstraintSystemFailure):
                permute_expression_pair(up(bad_in, form), up(bad_tab, form), 4, field, form)


def _plane_rows(plane, n):
    bits = np.unpackbits(plane.cpu().numpy().view(np.uint8), bitorder="little")
    return [int(r) for r in np.flatnonzero(bits[:n])]


@pytest.mark.parametrize("faults", [0, 12])
@pytest.mark.parametrize("field", FIELDS)
def test_mock_prover_lookup_check(field, faults):
    """h2_lookup_check_device over canonical columns: the nine-component lookup of mock_prover_cases.wide_lookup_case (its inputs are
    plain advice columns, its tables plain fixed columns, no rotation: no poison plane), satisfied and with 12 planted faults; the
    failing rows are the host model's."""
    import torch
    lib = h.lib()
    m = fields.MODULUS[field]
    k, cs, fixed, advice, instance, mapping = cases.wide_lookup_case(m, faults=faults)
    want = [f[2] for f in model.verify(k, cs, fixed, advice, instance, mapping, m) if f[0] == "Lookup"]
    assert bool(want) == bool(faults)
    n, w = 1 << k, len(advice)
    usable = n - (cs.blinding_factors + 1)
    arr = lambda ts: (C.c_void_p * w)(*[t.data_ptr() for t in ts])
    for form in FORMS:
        d_in = [dev(fields.to_limbs(col, field, form == MONT)) for col in advice]
        d_tab = [dev(fields.to_limbs(col, field, form == MONT)) for col in fixed]
        fail = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device="cuda:0")
        count = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
        ok(lib.h2_lookup_check_device(field, arr(d_in), None, arr(d_tab), None, w, n, usable, form, fail.data_ptr(), count.data_ptr(), None))
        sync()
        assert _plane_rows(fail, n) == want and count.cpu().tolist() == [len(want)], form


@pytest.mark.parametrize("broken", [False, True])
@pytest.mark.parametrize("field", FIELDS)
def test_mock_prover_permutation_check(field, broken):
    """h2_permutation_check_device over canonical columns: the copy constraints of the shared test circuit at k = 8, satisfied and with
    two broken copies (mock_prover_cases.seeded_faults); the failing cells are the host model's."""
    import torch
    lib = h.lib()
    m = fields.MODULUS[field]
    k = 8
    n = 1 << k
    k_, cs, fixed, advice, instance, mapping = cases.variant_case("full", m, k, cases.seeded_faults(m, k, "copy", 2) if broken else None)
    want = [(f[1], f[2]) for f in model.verify(k_, cs, fixed, advice, instance, mapping, m) if f[0] == "Permutation"]
    assert bool(want) == broken
    usable = n - (cs.blinding_factors + 1)
    by_kind = {"fixed": fixed, "advice": advice, "instance": instance}
    columns = [tuple(c_) for c_ in cs.permutation_columns]
    pad = lambda col: list(col) + [0] * (n - len(col))
    flat = np.asarray(mapping, dtype=np.int64)
    if flat.ndim == 3:
        flat = flat[:, :, 0] * n + flat[:, :, 1]
    d_map = torch.from_numpy(np.ascontiguousarray(flat)).to("cuda:0")
    assert tuple(d_map.shape) == (len(columns), n)
    flags = (C.c_uint8 * len(columns))(*[1 if kind == "advice" else 0 for kind, _ in columns])
    for form in FORMS:
        d_cols = [dev(fields.to_limbs(pad(by_kind[kind][idx]), field, form == MONT)) for kind, idx in columns]
        ptrs = (C.c_void_p * len(columns))(*[t.data_ptr() for t in d_cols])
        fail = torch.full((len(columns), (n + 63) // 64), -1, dtype=torch.int64, device="cuda:0")
        counts = torch.full((len(columns),), -1, dtype=torch.int32, device="cuda:0")
        ok(lib.h2_permutation_check_device(field, ptrs, flags, len(columns), d_map.data_ptr(), k, usable, form, fail.data_ptr(), counts.data_ptr(), None))
        sync()
        got = [(columns[c_], r) for c_ in range(len(columns)) for r in _plane_rows(fail[c_], n)]
        assert got == want, form
        assert counts.cpu().tolist() == [sum(1 for col, _ in want if col == columns[c_]) for c_ in range(len(columns))]
