"""Every pass shape of the default NTT plans, through every transform entry point, bit-exact against the C oracle at every index.

tests/test_ntt_shape_coverage.py proves on the CPU which shapes (plan kind, first, last, r, logT) the size lists of tests/ntt_shapes.py
reach; this file runs them: h2_ntt_device / h2_ifft_device at every size 2^0 .. 2^22 (plan 0), h2_ntt_batch_device /
h2_ifft_batch_device at the same sizes (plan 1: at most 8 stages and 64 KiB per pass -- the 4-stage later passes of 2^9 and 2^10 with
32 and 64 columns, the three-pass transforms from 2^17 whose middle pass writes and re-reads the packed signed intermediate), the
EvaluationDomain transforms (coset factors on a zero-padded first-pass load, the 1/n store, the {1, zeta^2, zeta} store) at every
k = 1 .. 14 with extensions of 1, 2 and 3 bits, structured vectors (zeros, p - 1 everywhere, single entries, alternating, small
values) with omega in {root of unity, 1, p - 1, random}, and the 8 x 32 kernel family on the laboratory build.  Around every call the
NTT pass counter of the event profiler says which plan ran: columns x the passes of the plan file.  No tolerance and no sampling
anywhere: outputs are compared as limbs."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import halo2_amd as h
import ntt_shapes as ns
from halo2_amd import fields
from oracle import c_oracle as co
from oracle import pasta as o

pytestmark = pytest.mark.gpu

PROF_NTT_PASS = 1                     # H2_PROF_NTT_PASS (include/halo2_mi355x.h)
FIELDS = [h.FP, h.FQ]


def mont(field, v):
    return fields.scalar_limbs(v, field, True)


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


@contextlib.contextmanager
def ntt_passes_launched(expect):
    """The body's transforms launched exactly `expect` pass kernels (profiling never changes an NTT: halo2_mi355x.h)."""
    import torch
    lib = h.lib()
    assert lib.h2_profile_enable(1) == 0
    ms, cnt = C.c_double(0), C.c_uint64(0)
    try:
        yield
        torch.cuda.synchronize()
        assert lib.h2_profile_read(PROF_NTT_PASS, C.byref(ms), C.byref(cnt)) == 0
    finally:
        lib.h2_profile_enable(0)
    assert cnt.value == expect, (cnt.value, expect)


def inverse_factors(field, L):
    m = fields.MODULUS[field]
    return mont(field, pow(o.omega_for(m, L), -1, m)), mont(field, pow(1 << L, -1, m))


def run_forward(field, cols, omega, L, form=h.FORM_MONTGOMERY):
    """One device tensor: h2_ntt_device in place; a list: h2_ntt_batch_device."""
    if isinstance(cols, list):
        h.best_fft_batch(cols, omega, L, field, form)
    else:
        h.best_fft(cols, omega, L, field, form)


def run_inverse(field, cols, omega_inv, divisor, L, form=h.FORM_MONTGOMERY):
    from halo2_amd._lib import check, lib
    from halo2_amd.arithmetic import _p, _stream_ptr
    if isinstance(cols, list):
        arr = (C.c_void_p * len(cols))(*[a.data_ptr() for a in cols])
        check(lib().h2_ifft_batch_device(field, arr, len(cols), L, _p(omega_inv), _p(divisor), form, _stream_ptr()), "h2_ifft_batch_device")
    else:
        check(lib().h2_ifft_device(field, cols.data_ptr(), L, _p(omega_inv), _p(divisor), form, _stream_ptr()), "h2_ifft_device")


# ------------------------------------------------------------------ (a) one transform, plan 0
def check_one_transform(field, L, inverse, form=h.FORM_MONTGOMERY):
    a = co.random_field(field, 8100 + 2 * L + inverse, 1 << L)
    conv = (lambda x: co.from_mont(field, x)) if form == h.FORM_CANONICAL else (lambda x: x)
    d = to_dev(conv(a))
    if inverse:
        omega_inv, divisor = inverse_factors(field, L)
        want = co.ifft(field, a, omega_inv, L, divisor)
        with ntt_passes_launched(len(ns.passes(L, 0))):
            run_inverse(field, d, conv(omega_inv.reshape(1, 4))[0], conv(divisor.reshape(1, 4))[0], L, form)
    else:
        omega = co.random_field(field, 8200 + L, 1)[0]                    # any field element: the butterfly network itself must match
        want = co.best_fft(field, a, omega, L)
        with ntt_passes_launched(len(ns.passes(L, 0))):
            run_forward(field, d, conv(omega.reshape(1, 4))[0], L, form)
    assert np.array_equal(to_host(d), conv(want))


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("L", ns.SWEEP_PLAN0)
def test_ntt_device_every_size(field, L):
    """h2_ntt_device on a device vector in place (more than one pass: through the stream's scratch vector), a random omega."""
    check_one_transform(field, L, inverse=False)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("L", ns.SWEEP_PLAN0)
def test_ifft_device_every_size(field, L):
    """h2_ifft_device with the domain's omega^-1 and 1/n: the last pass's store multiplies."""
    check_one_transform(field, L, inverse=True)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("L", [4, 12, 15])
@pytest.mark.parametrize("inverse", [False, True])
def test_one_transform_canonical_form(field, L, inverse):
    check_one_transform(field, L, inverse, form=h.FORM_CANONICAL)


# ------------------------------------------------------------------ (b) batched columns, plan 1
def check_batch(field, L, inverse, alone=False):
    ncols = 4 if L < 19 else 2           # four: three internal streams, and the fourth column reuses stream 0's scratch vector
    cols = [co.random_field(field, 8300 + 8 * L + 4 * inverse + i, 1 << L) for i in range(ncols)]
    if inverse:
        omega_inv, divisor = inverse_factors(field, L)
        wants = [co.ifft(field, c, omega_inv, L, divisor) for c in cols]
        run = lambda d: run_inverse(field, d, omega_inv, divisor, L)
    else:
        omega = co.random_field(field, 8400 + L, 1)[0]
        wants = [co.best_fft(field, c, omega, L) for c in cols]
        run = lambda d: run_forward(field, d, omega, L)
    d = [to_dev(c) for c in cols]
    with ntt_passes_launched(ncols * len(ns.passes(L, 1))):
        run(d)
    for i, (t, want) in enumerate(zip(d, wants)):
        assert np.array_equal(to_host(t), want), f"column {i}"
    if alone:                            # a batch of one column takes plan 0 and gives the same vector
        d = [to_dev(cols[0])]
        with ntt_passes_launched(len(ns.passes(L, 0))):
            run(d)
        assert np.array_equal(to_host(d[0]), wants[0])


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("L", ns.SWEEP_PLAN1)
def test_ntt_batch_device_every_size(field, L):
    check_batch(field, L, inverse=False, alone=L in (9, 17))


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("L", ns.SWEEP_PLAN1)
def test_ifft_batch_device_every_size(field, L):
    check_batch(field, L, inverse=True, alone=L in (9, 17))


def test_pass_counts_tell_the_plans_apart():
    """What the launch counts above rest on: 2^9 is one pass alone and two batched, 2^17 two alone and three batched."""
    assert [len(ns.passes(L, kind)) for L in (9, 17) for kind in (0, 1)] == [1, 2, 2, 3]


# ------------------------------------------------------------------ (d) domain transforms
def check_domain(field, j, k, a, e):
    """lagrange_to_coeff of `a`, coeff_to_extended of the result, divide_by_vanishing_poly of that, and extended_to_coeff of the GENERIC
    extended vector `e` (not the image of a low-degree polynomial: every output index carries information) and of the extension."""
    dom = h.EvaluationDomain(j, k, field)
    ref = o.EvaluationDomain(j, k, fields.MODULUS[field])
    assert dom.extended_k == ref.extended_k and a.shape[0] == dom.n and e.shape[0] == 1 << ref.extended_k
    c = lambda v: mont(field, v)
    coeff_want = co.ifft(field, a, c(ref.omega_inv), k, c(ref.ifft_divisor))
    assert np.array_equal(dom.lagrange_to_coeff(a.copy()), coeff_want)
    ext_want = co.coeff_to_extended(field, coeff_want, k, ref.extended_k, c(ref.g_coset), c(ref.g_coset_inv), c(ref.extended_omega))
    ext = dom.coeff_to_extended(coeff_want.copy())
    assert np.array_equal(ext, ext_want)
    t = co.to_mont(field, co.ints_to_limbs(ref.t_evaluations))
    assert np.array_equal(dom.divide_by_vanishing_poly(e.copy()), co.divide_by_vanishing_poly(field, e, ref.extended_k, t))
    keep = dom.n * dom.quotient_poly_degree
    for vec in (e, ext_want):
        back_want = co.extended_to_coeff(field, vec, ref.extended_k, c(ref.g_coset), c(ref.g_coset_inv), c(ref.extended_omega_inv),
                                         c(ref.extended_ifft_divisor))
        assert np.array_equal(dom.extended_to_coeff(vec.copy()), back_want[:keep])
    return dom.extended_k


def check_domain_random(field, j, k):
    ext_k = k + {2: 0, 3: 1, 5: 2, 9: 3}[j]
    a = co.random_field(field, 8500 + 16 * k + j, 1 << k)
    e = co.random_field(field, 8600 + 16 * k + j, 1 << ext_k)
    assert check_domain(field, j, k, a, e) == ext_k


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("j", [3, 5, 9])
@pytest.mark.parametrize("k", range(1, 15))
def test_domain_transforms_every_k(field, j, k):
    """Extensions of 1, 2 and 3 bits (extended k at most 17): the first pass's `j < n_in` test meets every first-pass shape."""
    check_domain_random(field, j, k)


@pytest.mark.parametrize("field", FIELDS)
def test_domain_transforms_without_extension(field):
    """j = 2: a quotient of degree 1, the extended domain IS the domain (no index is padded)."""
    check_domain_random(field, 2, 4)


# ------------------------------------------------------------------ (e) structured inputs
def structured_vectors(field, n):
    """The values are the limbs the kernels read (the transform is linear in them and the comparison is of limbs): p - 1 is the
    largest residue a pass can be handed, zeros and small values the smallest."""
    top = co.ints_to_limbs([fields.MODULUS[field] - 1])[0]
    z = np.zeros((n, 4), dtype=np.uint64)
    out = {"zero": z, "all p-1": np.tile(top, (n, 1))}
    out["p-1 at 0"] = z.copy()
    out["p-1 at 0"][0] = top
    out["1 at n-1"] = z.copy()
    out["1 at n-1"][n - 1, 0] = 1
    out["0, p-1 alternating"] = z.copy()
    out["0, p-1 alternating"][1::2] = top
    out["i mod 3"] = z.copy()
    out["i mod 3"][:, 0] = np.arange(n, dtype=np.uint64) % 3
    out["20 bits"] = z.copy()
    out["20 bits"][:, 0] = np.random.default_rng(8700 + n).integers(0, 1 << 20, n, dtype=np.uint64)
    return out


def structured_omegas(field, L):
    m = fields.MODULUS[field]
    return {"root of unity": mont(field, o.omega_for(m, L)), "1": mont(field, 1), "p-1": mont(field, m - 1),
            "random": co.random_field(field, 8800 + L, 1)[0]}


def check_structured(field, L, batched):
    m, n = fields.MODULUS[field], 1 << L
    vecs = structured_vectors(field, n)
    for wname, omega in structured_omegas(field, L).items():
        wants = {name: co.best_fft(field, v, omega, L) for name, v in vecs.items()}
        if wname == "1":                 # the network with omega = 1 sums: n (p - 1) mod p at index 0, zero elsewhere
            s = co.limbs_to_ints(wants["all p-1"])
            assert s[0] == n * (m - 1) % m and not any(s[1:])
        for name, v in vecs.items():
            d = to_dev(v)
            with ntt_passes_launched(len(ns.passes(L, 0))):
                run_forward(field, d, omega, L)
            assert np.array_equal(to_host(d), wants[name]), (name, wname)
        if batched:                      # seven columns over three streams
            d = [to_dev(v) for v in vecs.values()]
            with ntt_passes_launched(len(d) * len(ns.passes(L, 1))):
                run_forward(field, d, omega, L)
            for (name, want), t in zip(wants.items(), d):
                assert np.array_equal(to_host(t), want), (name, wname, "batched")


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("L", [1, 2, 4, 9, 10, 11, 13, 16, 17])
def test_structured_inputs(field, L):
    """The carry-free passes are correct by a bounds argument (|value| < 2^260, RAW limbs, q in [-64, 64]: ntt_pass.cuh): here it meets
    the extreme residues, in every position at once and alone, under twiddles that never reduce anything (omega = 1) or only negate."""
    check_structured(field, L, batched=L in (9, 10, 17))


def check_structured_domain(field, j, k):
    ext_n = (1 << k) * {3: 2, 5: 4, 9: 8}[j]
    va, ve = structured_vectors(field, 1 << k), structured_vectors(field, ext_n)
    for name in va:
        check_domain(field, j, k, va[name], ve[name])


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k", [3, 9, 12])
def test_structured_inputs_through_the_domain(field, k):
    check_structured_domain(field, 5, k)


# ------------------------------------------------------------------ the 8 x 32 family (the product runs it beyond 2^28)
def eight_by_thirty_two(field, name):
    """The body runs in a child on the laboratory build with H2_NTT_FE9=0: the same plans on the 8 x 32 kernels -- single passes of every
    stage count 1 .. 10, two passes up to 10 + 10, the three-pass 2^21 with a middle pass, plan 1, the load and store modes, the
    structured vectors."""
    if not os.environ.get("H2_AB_CHILD"):
        from conftest import run_test_in_ab_child
        run_test_in_ab_child(__file__, name, H2_NTT_FE9="0")
        return
    from halo2_amd import _lib
    assert os.environ.get("H2_NTT_FE9") == "0" and _lib.LIB_PATH.endswith("libhalo2_mi355x_ab.so"), _lib.LIB_PATH
    for L in list(range(1, 17)) + [20, 21]:
        check_one_transform(field, L, inverse=False)
        check_one_transform(field, L, inverse=True)
    for L in (9, 10, 13, 17):
        check_batch(field, L, inverse=False)
        check_batch(field, L, inverse=True)
    for k in (3, 9, 12):
        check_domain_random(field, 5, k)
    for L in (4, 11, 13):
        check_structured(field, L, batched=False)


def test_eight_by_thirty_two_family_fp():
    eight_by_thirty_two(h.FP, "test_eight_by_thirty_two_family_fp")


def test_eight_by_thirty_two_family_fq():
    eight_by_thirty_two(h.FQ, "test_eight_by_thirty_two_family_fq")
