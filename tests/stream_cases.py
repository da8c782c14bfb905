"""One call of every entry point of the C ABI that takes a `void *stream`, cut into the pieces a stream-order test needs (a helper:
nothing here is collected).

Every prototype of include/halo2_mi355x.h whose parameter list holds `void *stream` is a key of CASES.  Its value is a Case, a tuple of
Cases where the entry point has several forms (the dispatch of the generic multiexp, the two forms of the batched commit), or an
Excluded with the one-line reason.  A Case separates what the probes of tests/call_sequences.py fuse:

    inputs(seed)                -> {name: host array} of every DEVICE input of the call; axis 0 of an array counts its elements
    outputs()                   -> {name: bytes of a fresh device buffer | ("in", input name, bytes of its prefix) for a call in place}
    call(ins, outs, stream_ptr) -> the one library call on device buffers (anything with data_ptr()), on that hipStream_t; a call
                                   whose result reaches the host (a proof, a transcript) returns those bytes, any other None
    expected(seed)              -> the oracle's bytes: the outputs in the order of outputs(), then the host bytes
    valid(arrays)               -> asserts that the arrays are valid input (ranges, curve membership, the lookup's table)
    post(name, bytes)           -> the form an output is compared in, applied to the device's bytes and to the oracle's alike (the square of a
                                   root whose sign the library is free to pick)

Host-pointer arguments (points, challenges, omegas, programs, transcripts) are consumed at call time and are the same under every
seed.  Registered bases, Params, FixedBase and CommitDomain are set-up objects: they are built at the first call, which the GPU test
makes on the default stream with a device-wide synchronise behind it.

Seeds: REAL and DECOY give arrays of the same shapes and different bytes, both valid, and so is every element-wise mixture of the two
(tests/test_stream_case_coverage.py checks all three): a mis-ordered run computes a wrong answer from valid data, never a fault or a
refusal.  THIRD is the second stream's data of the shared-cache test.  Three entry points have no device input at all (NO_DEVICE_INPUT):
their inputs() is empty and only their outputs can show a misplaced launch.

Shapes are the smallest that still take more than one launch or leave the caller's stream; tests/test_stream_case_coverage.py holds
each claim to the plan replicas the suite already has.  Two choices are larger than the smallest, on purpose: the generator collapse,
the scalar fold, the round scalars and the s vector take the LARGE shapes of tests/call_sequences.py (2^11 points, (11, 3), (12, 64)),
because its small ones are a single workgroup in a single launch; and the batched transforms take two columns, although one column
already rides one internal stream, because two are the fewest that use a second internal stream and the batched plan."""
import contextlib
import ctypes as C
import functools
import os
import random
import re

import numpy as np

import call_sequences as cs
import commit_plans as cp
import ntt_shapes as ns
import scan_sort_cases as ssc
from oracle import c_oracle as co
from oracle import hash_to_curve as oh
from oracle import ipa as oipa
from oracle import lookup as olk
from oracle import pasta as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "halo2_mi355x.h")

REAL, DECOY, THIRD = 1, 2, 3
SEEDS = (REAL, DECOY, THIRD)
FP, FQ, PALLAS, VESTA = 0, 1, 0, 1
MONT, AFFINE = 1, 1                                               # H2_FORM_MONTGOMERY, H2_OUT_AFFINE
P = o.P
MODULUS = {FP: o.P, FQ: o.Q}


class Excluded(str):
    """The reason an entry point has no stream-order case."""


def prototypes_with_stream(header=HEADER):
    """Names of the functions declared in the header whose parameter list holds `void *stream`."""
    text = re.sub(r"/\*.*?\*/", " ", open(header).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    found = re.findall(r"\bint\s+(h2_\w+)\s*\(([^()]*)\)\s*;", text)
    return {name for name, params in found if re.search(r"\bvoid\s*\*\s*stream\b", params)}


MAY_BE_EXCLUDED = {"h2_msm_last_path", "h2_commit_last_plan", "h2_msm_split_rccl_device", "h2_commit_split_rccl_device"}
NO_DEVICE_INPUT = {"h2_powers_device", "h2_ipa_collapsed_generators_device", "h2_ecc_fixed_tables_device"}


class Case:
    def __init__(self, name, entry, shape, inputs, outputs, call, expected, valid, post=None, mode_c=False, host_bytes=0):
        self.name, self.entry, self.shape, self.mode_c, self.host_bytes = name, entry, shape, mode_c, host_bytes
        self.inputs = functools.lru_cache(maxsize=None)(inputs)
        self.expected = functools.lru_cache(maxsize=None)(expected)
        self.outputs, self.call, self.valid, self._post = outputs, call, valid, post

    def post(self, name, raw: bytes) -> bytes:
        return self._post(name, raw) if self._post else raw

    def output_bytes(self):
        return [(name, spec if isinstance(spec, int) else spec[2]) for name, spec in self.outputs().items()]

    def __repr__(self):
        return self.name


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------
def _lib():
    import halo2_amd as h
    return h.lib()


def ok(rc):
    assert rc == 0, (rc, _lib().h2_last_error())


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _vp(*tensors):
    return (C.c_void_p * len(tensors))(*[t if isinstance(t, int) else t.data_ptr() for t in tensors])


def _st(stream_ptr):
    return C.c_void_p(stream_ptr)


@contextlib.contextmanager
def on_stream(stream_ptr):
    """torch's current stream set to the hipStream_t: what a halo2_amd wrapper passes to the library."""
    import torch
    stream = torch.cuda.ExternalStream(stream_ptr) if stream_ptr else torch.cuda.default_stream()
    with torch.cuda.stream(stream):
        yield stream


def rf(field, base, seed, n):
    """n oracle-random field elements, Montgomery limbs; another vector per seed"""
    return co.random_field(field, base + 0x101 * seed, n)


def fe(field, v):
    return co.to_mont(field, co.ints_to_limbs([v % MODULUS[field]]))[0]


def limbs(ints, field=FP, montgomery=True) -> np.ndarray:
    a = co.ints_to_limbs([int(v) for v in ints])
    return co.to_mont(field, a) if montgomery else a


def ints_of(a, field=FP, montgomery=True):
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    return co.limbs_to_ints(co.from_mont(field, a) if montgomery else a)


def point_limbs(points, curve=PALLAS) -> np.ndarray:
    """[(x, y)] with the identity as (0, 0) or None -> (n, 8) Montgomery limbs"""
    flat = [c for pt in points for c in (pt if pt is not None else (0, 0))]
    return limbs(flat, co.field_of_curve(curve, "base")).reshape(-1, 8)


def _b(*arrays) -> bytes:
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def below_modulus(a, field, montgomery=True):
    """every 4-limb element is a reduced residue (a Montgomery limb vector of one is one as well)"""
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    m = [(MODULUS[field] >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    less, equal = np.zeros(a.shape[0], dtype=bool), np.ones(a.shape[0], dtype=bool)
    for i in (3, 2, 1, 0):
        less |= equal & (a[:, i] < np.uint64(m[i]))
        equal &= a[:, i] == np.uint64(m[i])
    assert bool(less.all()), "an element is not below the modulus"


def on_the_curve(a, curve, identity_ok=True):
    bm = o.CURVES[curve][0]
    v = ints_of(a, co.field_of_curve(curve, "base"))
    for x, y in zip(v[0::2], v[1::2]):
        if (x, y) == (0, 0):
            assert identity_ok
        else:
            assert (y * y - x * x * x - 5) % bm == 0, "a point is off the curve"


def fields_valid(field, *names, montgomery=True):
    def valid(arrays):
        for name in names:
            below_modulus(arrays[name], field, montgomery)
    return valid


def nothing_to_check(arrays):
    assert not arrays


def mixture(a, b):
    """Elements of a and b in turn (axis 0 counts the elements)."""
    out = np.array(a, copy=True)
    out[1::2] = b[1::2]
    return out


# ---- a. multiexps ----------------------------------------------------------------------------------------------------------------------
MSM_CURVE = PALLAS
GROUPED = (1 << 18) + 1
MSM_SIZES = {300: 1, 70000: 2, GROUPED: 4}                       # n -> H2_MSM_PATH_*: one pass, two passes, GROUPED_LATENCY (the library's own streams)


@functools.lru_cache(maxsize=None)
def _msm_inputs(n, seed):
    return {"scalars": rf(co.field_of_curve(MSM_CURVE, "scalar"), 0x7000 + n % 89, seed, n),
            "bases": co.generate_bases(MSM_CURVE, 0x7100 + n % 89 + 0x101 * seed, n)}


@functools.lru_cache(maxsize=None)
def _msm_wanted(n, seed):
    """one cache for every test that needs the oracle's 2^18 + 1 multiexp"""
    a = _msm_inputs(n, seed)
    return cs._affine_limbs(MSM_CURVE, co.best_multiexp(MSM_CURVE, a["scalars"], a["bases"]))


def last_msm_path(stream_ptr):
    path = C.c_int(0)
    ok(_lib().h2_msm_last_path(_st(stream_ptr), C.byref(path), None, None, None))
    return path.value


def _points_valid(curve, scalars=(), points=()):
    def valid(arrays):
        for name in scalars:
            below_modulus(arrays[name], co.field_of_curve(curve, "scalar"))
        for name in points:
            below_modulus(arrays[name], co.field_of_curve(curve, "base"))
            on_the_curve(arrays[name], curve)
    return valid


def _msm_case(n):
    def call(ins, outs, sp):
        ok(_lib().h2_msm_device(MSM_CURVE, ins["scalars"].data_ptr(), ins["bases"].data_ptr(), n, MONT, AFFINE, outs["out"].data_ptr(), _st(sp)))
        assert last_msm_path(sp) == MSM_SIZES[n], (n, last_msm_path(sp))
    return Case(f"msm-{n}", "h2_msm_device", n, lambda seed: _msm_inputs(n, seed), lambda: {"out": 64}, call,
                lambda seed: _msm_wanted(n, seed), _points_valid(MSM_CURVE, ["scalars"], ["bases"]))


MSM_BATCH = (2049, 300)


def _msm_batch_case():
    def inputs(seed):
        out = {}
        for i, n in enumerate(MSM_BATCH):
            a = _msm_inputs(n, seed + 8 * (i + 1))
            out[f"scalars{i}"], out[f"bases{i}"] = a["scalars"], a["bases"]
        return out

    def call(ins, outs, sp):
        ok(_lib().h2_msm_batch_device(MSM_CURVE, _vp(ins["scalars0"], ins["scalars1"]), _vp(ins["bases0"], ins["bases1"]),
                                      (C.c_size_t * 2)(*MSM_BATCH), 2, MONT, AFFINE, _vp(outs["out0"], outs["out1"]), _st(sp)))

    def expected(seed):
        a = inputs(seed)
        return b"".join(cs._affine_limbs(MSM_CURVE, co.best_multiexp(MSM_CURVE, a[f"scalars{i}"], a[f"bases{i}"])) for i in range(2))
    return Case("msm-batch-2", "h2_msm_batch_device", MSM_BATCH, inputs, lambda: {"out0": 64, "out1": 64}, call, expected,
                _points_valid(MSM_CURVE, ["scalars0", "scalars1"], ["bases0", "bases1"]))


# ---- b. registered commits: the tables are set-up objects, the columns and blinds the inputs ----------------------------------------------
COMMIT_CURVE = VESTA
COMMIT_SF = co.field_of_curve(COMMIT_CURVE, "scalar")
COMMIT_TABLE = cp.SMALL                                           # 2^13 + 3 points: 16-bit windows
ALTERNATING = (1 << 10, cp.MAX_COLS + 1)                          # (table, columns): two column-batched groups on two internal streams
SPREAD = (300, 3)                                                 # 8-bit windows decline the batched form: one commit per column, three streams
PAIR_TABLE = next(n for n in range(8, 1 << 14) if cp.pair_supported(n))
_handles = {}


@functools.lru_cache(maxsize=None)
def _table_points(points):
    return co.generate_bases(COMMIT_CURVE, 0x7200 + points % 89, points), co.generate_bases(COMMIT_CURVE, 0x7201, 1)[0]


def commit_handle(points):
    """The registered table of `points` seeded points with the blind base installed (registered once, freed by nobody)."""
    if points not in _handles:
        g, w = _table_points(points)
        hd = C.c_uint64(0)
        ok(_lib().h2_bases_register(COMMIT_CURVE, _p(g), points, MONT, C.byref(hd)))
        ok(_lib().h2_bases_set_blind_base(hd, _p(w), MONT))
        _handles[points] = hd
    return _handles[points]


def last_commit_plan(stream_ptr):
    from halo2_amd import _lib as hl
    plan = hl.CommitPlan()
    ok(_lib().h2_commit_last_plan(_st(stream_ptr), C.byref(plan)))
    return plan.as_dict()


def _commit_case():
    n = COMMIT_TABLE

    def call(ins, outs, sp):
        ok(_lib().h2_commit_device(commit_handle(n), ins["scalars"].data_ptr(), n, None, ins["blind"].data_ptr(), MONT, AFFINE,
                                   outs["out"].data_ptr(), _st(sp)))

    def inputs(seed):
        return {"scalars": rf(COMMIT_SF, 0x7300, seed, n), "blind": rf(COMMIT_SF, 0x7301, seed, 1)}

    def expected(seed):
        a, (g, w) = inputs(seed), _table_points(n)
        return cs._affine_limbs(COMMIT_CURVE, co.commit(COMMIT_CURVE, g, w, a["scalars"], a["blind"][0]))
    return Case("commit-device-blind", "h2_commit_device", n, inputs, lambda: {"out": 64}, call, expected, fields_valid(COMMIT_SF, "scalars", "blind"))


def _commit_range_case():
    first = COMMIT_TABLE // 3 + 1
    n = COMMIT_TABLE - first

    def call(ins, outs, sp):
        ok(_lib().h2_commit_range_device(commit_handle(COMMIT_TABLE), ins["scalars"].data_ptr(), first, n, ins["blind"].data_ptr(), MONT, AFFINE,
                                         outs["out"].data_ptr(), _st(sp)))

    def inputs(seed):
        return {"scalars": rf(COMMIT_SF, 0x7310, seed, n), "blind": rf(COMMIT_SF, 0x7311, seed, 1)}

    def expected(seed):
        a, (g, w) = inputs(seed), _table_points(COMMIT_TABLE)
        return cs._affine_limbs(COMMIT_CURVE, co.commit(COMMIT_CURVE, np.ascontiguousarray(g[first:]), w, a["scalars"], a["blind"][0]))
    return Case("commit-range", "h2_commit_range_device", (first, n), inputs, lambda: {"out": 64}, call, expected,
                fields_valid(COMMIT_SF, "scalars", "blind"))


PAIR_SHIFT = 5


def _commit_pair_case():
    n = PAIR_TABLE

    def call(ins, outs, sp):
        ok(_lib().h2_commit_pair_device(commit_handle(n), ins["scalars"].data_ptr(), n, PAIR_SHIFT, MONT, AFFINE, outs["out"].data_ptr(), _st(sp)))
        assert last_commit_plan(sp)["caller"] == cp.PAIR_SUBDIGIT

    def inputs(seed):
        return {"scalars": rf(COMMIT_SF, 0x7320, seed, n)}

    def expected(seed):
        col, (g, _) = inputs(seed)["scalars"], _table_points(n)
        idx = np.arange(n)
        side = np.where(idx < n - 4, (idx >> PAIR_SHIFT) & 1, (idx - (n - 4)) & 1)
        out = b""
        for s in (0, 1):
            part = col.copy()
            part[side != s] = 0
            out += cs._affine_limbs(COMMIT_CURVE, co.best_multiexp(COMMIT_CURVE, part, g))
        return out
    return Case("commit-pair-subdigit", "h2_commit_pair_device", n, inputs, lambda: {"out": 128}, call, expected, fields_valid(COMMIT_SF, "scalars"))


def _commit_batch_case(name, points, count, caller, groups):
    def call(ins, outs, sp):
        cols, blinds = [ins[f"col{i}"] for i in range(count)], [ins[f"blind{i}"] for i in range(count)]
        ok(_lib().h2_commit_batch_device(commit_handle(points), _vp(*cols), count, points, None, _vp(*blinds), MONT, AFFINE,
                                         _vp(*[outs[f"out{i}"] for i in range(count)]), _st(sp)))
        plan = last_commit_plan(sp)
        assert (plan["caller"], plan["caller_count"]) == (caller, groups), plan

    def inputs(seed):
        out = {}
        for i in range(count):
            out[f"col{i}"], out[f"blind{i}"] = rf(COMMIT_SF, 0x7400 + 2 * i + points % 89, seed, points), rf(COMMIT_SF, 0x7401 + 2 * i, seed, 1)
        return out

    def expected(seed):
        a, (g, w) = inputs(seed), _table_points(points)
        return b"".join(cs._affine_limbs(COMMIT_CURVE, co.commit(COMMIT_CURVE, g, w, a[f"col{i}"], a[f"blind{i}"][0])) for i in range(count))
    names = [f"col{i}" for i in range(count)] + [f"blind{i}" for i in range(count)]
    return Case(name, "h2_commit_batch_device", (points, count), inputs, lambda: {f"out{i}": 64 for i in range(count)}, call, expected,
                fields_valid(COMMIT_SF, *names))


POINTS_SUM = 65


def _points_sum_case():
    bf = co.field_of_curve(MSM_CURVE, "base")

    def inputs(seed):
        """Jacobian points (x z^2, y z^3, z) with a z of their own each"""
        xy = ints_of(co.generate_bases(MSM_CURVE, 0x7500 + 0x101 * seed, POINTS_SUM), bf)
        zs = ints_of(rf(bf, 0x7501, seed, POINTS_SUM), bf)
        m = MODULUS[bf]
        flat = [c for i, z in enumerate(zs) for c in (xy[2 * i] * z * z % m, xy[2 * i + 1] * z * z * z % m, z)]
        return {"points": limbs(flat, bf).reshape(-1, 12)}

    def affine(a):
        m = MODULUS[bf]
        v = ints_of(a, bf)
        pts = []
        for i in range(len(v) // 3):
            zi = pow(v[3 * i + 2], -1, m)
            pts.append((v[3 * i] * zi * zi % m, v[3 * i + 1] * zi * zi * zi % m))
        return pts

    def valid(arrays):
        below_modulus(arrays["points"], bf)
        assert all(z for z in ints_of(arrays["points"], bf)[2::3])
        on_the_curve(point_limbs(affine(arrays["points"]), MSM_CURVE), MSM_CURVE, identity_ok=False)

    def call(ins, outs, sp):
        ok(_lib().h2_points_sum_device(MSM_CURVE, ins["points"].data_ptr(), POINTS_SUM, MONT, AFFINE, outs["out"].data_ptr(), _st(sp)))

    def expected(seed):
        total = None
        for pt in affine(inputs(seed)["points"]):
            total = o.ec_add(total, pt, MODULUS[bf])
        return _b(point_limbs([total], MSM_CURVE))
    return Case("points-sum", "h2_points_sum_device", POINTS_SUM, inputs, lambda: {"out": 64}, call, expected, valid)


# ---- c. NTT family: the smallest two-pass size of the default plan, one root of unity for every seed ----------------------------------------
NTT_FIELD = FP
NTT_LOG = min(L for L in range(2, 23) if len(ns.passes(L, 0)) == 2)               # a transform alone
NTT_BATCH_LOG = min(L for L in range(2, 23) if len(ns.passes(L, 1)) == 2)         # the batched plan
# ntt_batch forks from one column on (a lone column rides one internal stream with the lone plan); two columns are the fewest that take the
# batched plan and two internal streams
NTT_BATCH_COLUMNS = 2


def _ntt_factors(L):
    m = MODULUS[NTT_FIELD]
    w = o.omega_for(m, L)
    return fe(NTT_FIELD, w), fe(NTT_FIELD, pow(w, -1, m)), fe(NTT_FIELD, pow(1 << L, -1, m))


def _ntt_case(name, entry, inverse):
    L = NTT_LOG
    omega, omega_inv, divisor = _ntt_factors(L)

    def call(ins, outs, sp):
        if inverse:
            ok(_lib().h2_ifft_device(NTT_FIELD, ins["a"].data_ptr(), L, _p(omega_inv), _p(divisor), MONT, _st(sp)))
        else:
            ok(_lib().h2_ntt_device(NTT_FIELD, ins["a"].data_ptr(), L, _p(omega), MONT, _st(sp)))

    def inputs(seed):
        return {"a": rf(NTT_FIELD, 0x7600 + inverse, seed, 1 << L)}

    def expected(seed):
        a = inputs(seed)["a"]
        return _b(co.ifft(NTT_FIELD, a, omega_inv, L, divisor) if inverse else co.best_fft(NTT_FIELD, a, omega, L))
    return Case(name, entry, L, inputs, lambda: {"a": ("in", "a", 32 << L)}, call, expected, fields_valid(NTT_FIELD, "a"), mode_c=True)


def _ntt_batch_case(name, entry, inverse):
    L, count = NTT_BATCH_LOG, NTT_BATCH_COLUMNS
    omega, omega_inv, divisor = _ntt_factors(L)
    names = [f"a{i}" for i in range(count)]

    def call(ins, outs, sp):
        arr = _vp(*[ins[n] for n in names])
        if inverse:
            ok(_lib().h2_ifft_batch_device(NTT_FIELD, arr, count, L, _p(omega_inv), _p(divisor), MONT, _st(sp)))
        else:
            ok(_lib().h2_ntt_batch_device(NTT_FIELD, arr, count, L, _p(omega), MONT, _st(sp)))

    def inputs(seed):
        return {n: rf(NTT_FIELD, 0x7610 + 2 * i + inverse, seed, 1 << L) for i, n in enumerate(names)}

    def expected(seed):
        a = inputs(seed)
        return b"".join(_b(co.ifft(NTT_FIELD, a[n], omega_inv, L, divisor) if inverse else co.best_fft(NTT_FIELD, a[n], omega, L)) for n in names)
    return Case(name, entry, (L, count), inputs, lambda: {n: ("in", n, 32 << L) for n in names}, call, expected, fields_valid(NTT_FIELD, *names),
                mode_c=True)


EXT_K = NTT_LOG
DOMAIN_K = EXT_K - 2                                              # EvaluationDomain(5, k): the extended domain has 2^(k + 2) elements


@functools.lru_cache(maxsize=None)
def _domain():
    ref = o.EvaluationDomain(5, DOMAIN_K, MODULUS[NTT_FIELD])
    assert ref.extended_k == EXT_K
    return ref


def _dm(name):
    return fe(NTT_FIELD, getattr(_domain(), name))


def _coeff_to_extended_case():
    def call(ins, outs, sp):
        ok(_lib().h2_coeff_to_extended_device(NTT_FIELD, ins["a"].data_ptr(), outs["out"].data_ptr(), DOMAIN_K, EXT_K, _p(_dm("g_coset")),
                                              _p(_dm("g_coset_inv")), _p(_dm("extended_omega")), MONT, _st(sp)))

    def inputs(seed):
        return {"a": rf(NTT_FIELD, 0x7620, seed, 1 << DOMAIN_K)}

    def expected(seed):
        return _b(co.coeff_to_extended(NTT_FIELD, inputs(seed)["a"], DOMAIN_K, EXT_K, _dm("g_coset"), _dm("g_coset_inv"), _dm("extended_omega")))
    return Case("coeff-to-extended", "h2_coeff_to_extended_device", (DOMAIN_K, EXT_K), inputs, lambda: {"out": 32 << EXT_K}, call, expected,
                fields_valid(NTT_FIELD, "a"), mode_c=True)


def _extended_to_coeff_case():
    def call(ins, outs, sp):
        ok(_lib().h2_extended_to_coeff_device(NTT_FIELD, ins["a"].data_ptr(), EXT_K, _p(_dm("g_coset")), _p(_dm("g_coset_inv")),
                                              _p(_dm("extended_omega_inv")), _p(_dm("extended_ifft_divisor")), MONT, _st(sp)))

    def inputs(seed):
        return {"a": rf(NTT_FIELD, 0x7621, seed, 1 << EXT_K)}

    def expected(seed):
        return _b(co.extended_to_coeff(NTT_FIELD, inputs(seed)["a"], EXT_K, _dm("g_coset"), _dm("g_coset_inv"), _dm("extended_omega_inv"),
                                       _dm("extended_ifft_divisor")))
    return Case("extended-to-coeff", "h2_extended_to_coeff_device", EXT_K, inputs, lambda: {"a": ("in", "a", 32 << EXT_K)}, call, expected,
                fields_valid(NTT_FIELD, "a"), mode_c=True)


def _divide_by_vanishing_case():
    def t_evals():
        return limbs(_domain().t_evaluations, NTT_FIELD)

    def call(ins, outs, sp):
        t = t_evals()
        ok(_lib().h2_divide_by_vanishing_poly_device(NTT_FIELD, ins["a"].data_ptr(), EXT_K, _p(t), t.shape[0], MONT, _st(sp)))

    def inputs(seed):
        return {"a": rf(NTT_FIELD, 0x7622, seed, 1 << EXT_K)}

    def expected(seed):
        return _b(co.divide_by_vanishing_poly(NTT_FIELD, inputs(seed)["a"], EXT_K, t_evals()))
    return Case("divide-by-vanishing-poly", "h2_divide_by_vanishing_poly_device", EXT_K, inputs, lambda: {"a": ("in", "a", 32 << EXT_K)}, call,
                expected, fields_valid(NTT_FIELD, "a"), mode_c=True)


LAGRANGE_K = 9                                                    # ec_stage, ec_stage_glv per lane and per wave (ecfft.hip: t + 7 <= k needs k >= 9)
LAGRANGE_CURVE = PALLAS


def _lagrange_basis_case():
    n = 1 << LAGRANGE_K

    def call(ins, outs, sp):
        ok(_lib().h2_lagrange_basis_device(LAGRANGE_CURVE, ins["g"].data_ptr(), outs["out"].data_ptr(), LAGRANGE_K, MONT, _st(sp)))

    def inputs(seed):
        return {"g": co.generate_bases(LAGRANGE_CURVE, 0x7630 + 0x101 * seed, n)}
    return Case("lagrange-basis", "h2_lagrange_basis_device", LAGRANGE_K, inputs, lambda: {"out": 64 * n}, call,
                lambda seed: _b(co.lagrange_basis(LAGRANGE_CURVE, inputs(seed)["g"], LAGRANGE_K)), _points_valid(LAGRANGE_CURVE, points=["g"]),
                mode_c=True)


# ---- d. poly.hip: two tiles and one element -----------------------------------------------------------------------------------------------
POLY_FIELD = FQ
POLY_N = ssc.K_TILE + 1


def _poly_x():
    return rf(POLY_FIELD, 0x7700, 0, 1)[0]


POLY_ENTRIES = ("eval-polynomial", "inner-product", "kate-division", "powers", "scale-add", "batch-invert", "assigned-to-field", "grand-product")


def _poly_case(name, entry, names, out_spec, call, oracle, mode_c=True):
    def inputs(seed):
        return {n: rf(POLY_FIELD, 0x7710 + 4 * POLY_ENTRIES.index(name) + i, seed, POLY_N) for i, n in enumerate(names)}
    return Case(name, entry, POLY_N, inputs, lambda: dict(out_spec), call, lambda seed: _b(oracle(*[inputs(seed)[n] for n in names])),
                fields_valid(POLY_FIELD, *names) if names else nothing_to_check, mode_c=mode_c)


def _poly_cases():
    f, n, x = POLY_FIELD, POLY_N, _poly_x()
    L = _lib
    return {
        "h2_eval_polynomial_device": _poly_case(
            "eval-polynomial", "h2_eval_polynomial_device", ["a"], {"out": 32},
            lambda i, u, sp: ok(L().h2_eval_polynomial_device(f, i["a"].data_ptr(), n, _p(x), MONT, u["out"].data_ptr(), _st(sp))),
            lambda a: co.eval_polynomial(f, a, x)),
        "h2_inner_product_device": _poly_case(
            "inner-product", "h2_inner_product_device", ["a", "b"], {"out": 32},
            lambda i, u, sp: ok(L().h2_inner_product_device(f, i["a"].data_ptr(), i["b"].data_ptr(), n, MONT, u["out"].data_ptr(), _st(sp))),
            lambda a, b: co.inner_product(f, a, b)),
        "h2_kate_division_device": _poly_case(
            "kate-division", "h2_kate_division_device", ["a"], {"out": 32 * (n - 1)},
            lambda i, u, sp: ok(L().h2_kate_division_device(f, i["a"].data_ptr(), n, _p(x), MONT, u["out"].data_ptr(), _st(sp))),
            lambda a: co.kate_division(f, a, x)),
        "h2_powers_device": _poly_case(
            "powers", "h2_powers_device", [], {"out": 32 * n},
            lambda i, u, sp: ok(L().h2_powers_device(f, _p(x), n, MONT, u["out"].data_ptr(), _st(sp))),
            lambda: co.powers(f, x, n), mode_c=False),
        "h2_scale_add_device": _poly_case(
            "scale-add", "h2_scale_add_device", ["a", "b"], {"a": ("in", "a", 32 * n)},
            lambda i, u, sp: ok(L().h2_scale_add_device(f, i["a"].data_ptr(), _p(x), i["b"].data_ptr(), n, MONT, _st(sp))),
            lambda a, b: co.scale_add(f, a, x, b)),
        "h2_batch_invert_device": _poly_case(
            "batch-invert", "h2_batch_invert_device", ["a"], {"a": ("in", "a", 32 * n)},
            lambda i, u, sp: ok(L().h2_batch_invert_device(f, i["a"].data_ptr(), n, MONT, _st(sp))),
            lambda a: co.batch_invert(f, a)),
        "h2_assigned_to_field_device": _poly_case(
            "assigned-to-field", "h2_assigned_to_field_device", ["num", "den"], {"out": 32 * n},
            lambda i, u, sp: ok(L().h2_assigned_to_field_device(f, i["num"].data_ptr(), i["den"].data_ptr(), u["out"].data_ptr(), n, MONT, _st(sp))),
            _assigned_oracle),
        "h2_grand_product_device": _poly_case(
            "grand-product", "h2_grand_product_device", ["m"], {"z": 32 * n},
            lambda i, u, sp: ok(L().h2_grand_product_device(f, i["m"].data_ptr(), n, _p(x), MONT, u["z"].data_ptr(), _st(sp))),
            lambda m: co.grand_product(f, m, n, x)),
    }


def _assigned_oracle(num, den):
    """num / den over Python integers (no denominator of a random vector is zero or one)"""
    m = MODULUS[POLY_FIELD]
    inv = ints_of(co.batch_invert(POLY_FIELD, den), POLY_FIELD)
    return limbs([a * b % m for a, b in zip(ints_of(num, POLY_FIELD), inv)], POLY_FIELD)


# ---- e. the opening argument ---------------------------------------------------------------------------------------------------------------
IPA_CURVE = cs.IPA_CURVE
IPA_SF = co.field_of_curve(IPA_CURVE, "scalar")
IPA_SMALL_K, IPA_LARGE_K = cs.IPA_KS
ROUND_SCALARS = cs.ROUND_SCALARS[1]
S_COMBINE = cs.S_COMBINE[1]
COLLAPSED = (13, 3)                                               # (k, rounds): the smallest table with 16-bit windows is 2^13 points


def _generator_collapse_case():
    k = IPA_LARGE_K
    half, bf = 1 << (k - 1), co.field_of_curve(IPA_CURVE, "base")

    def call(ins, outs, sp):
        ok(_lib().h2_generator_collapse_device(IPA_CURVE, ins["g"].data_ptr(), half, _p(cs._ipa_challenge()), MONT, _st(sp)))

    def inputs(seed):
        return {"g": co.generate_bases(IPA_CURVE, 0x7800 + 0x101 * seed, 2 * half)}

    def expected(seed):
        return _b(np.ascontiguousarray(co.generator_collapse(IPA_CURVE, inputs(seed)["g"], cs._ipa_challenge())[:half]))
    return Case("generator-collapse", "h2_generator_collapse_device", k, inputs, lambda: {"g": ("in", "g", 64 * half)}, call, expected,
                _points_valid(IPA_CURVE, points=["g"]))


def _fold_scalars_case():
    half = 1 << (IPA_LARGE_K - 1)

    def call(ins, outs, sp):
        ok(_lib().h2_fold_scalars_device(IPA_SF, ins["a"].data_ptr(), half, _p(cs._ipa_challenge()), MONT, _st(sp)))

    def inputs(seed):
        return {"a": rf(IPA_SF, 0x7810, seed, 2 * half)}
    return Case("fold-scalars", "h2_fold_scalars_device", half, inputs, lambda: {"a": ("in", "a", 32 * half)}, call,
                lambda seed: _b(np.ascontiguousarray(co.fold_scalars(IPA_SF, inputs(seed)["a"], cs._ipa_challenge())[:half])),
                fields_valid(IPA_SF, "a"))


def _round_scalars_case():
    k, j = ROUND_SCALARS
    field, _, u = cs._round_inputs(k, j)

    def call(ins, outs, sp):
        ok(_lib().h2_ipa_round_scalars_device(field, ins["p"].data_ptr(), k, j, _p(np.ascontiguousarray(u)), MONT, outs["cl"].data_ptr(),
                                              outs["cr"].data_ptr(), _st(sp)))

    def inputs(seed):
        return {"p": rf(field, 0x7820, seed, 1 << (k - j))}

    def expected(seed):
        """p'[i ^ half] times the challenges picked by the bits of the block number, placed by the half i falls in"""
        m = MODULUS[field]
        p_i, u_i = ints_of(inputs(seed)["p"], field), ints_of(u, field)
        blk = k - j
        half = 1 << (blk - 1)
        left, right = [], []
        for row in range(1 << k):
            block, i = row >> blk, row & ((1 << blk) - 1)
            s = 1
            for r in range(j):
                if (block >> (j - 1 - r)) & 1:
                    s = s * u_i[r] % m
            v = p_i[i ^ half] * s % m
            left.append(v if i < half else 0)
            right.append(0 if i < half else v)
        return _b(limbs(left, field), limbs(right, field))
    return Case("ipa-round-scalars", "h2_ipa_round_scalars_device", (k, j), inputs, lambda: {"cl": 32 << k, "cr": 32 << k}, call, expected,
                fields_valid(field, "p"))


def _s_combine_case():
    k, batch = S_COMBINE
    us, coeffs = cs._s_combine_inputs(k, batch)
    ch, cf = limbs([v for u in us for v in u], FP), limbs(coeffs, FP)

    def call(ins, outs, sp):
        ok(_lib().h2_ipa_s_combine_device(FP, k, batch, _p(ch), _p(cf), MONT, 1, ins["out"].data_ptr(), _st(sp)))

    def inputs(seed):
        """accumulate = 1: the vector added to is the call's device input"""
        return {"out": rf(FP, 0x7830, seed, 1 << k)}

    def expected(seed):
        m = MODULUS[FP]
        total = ints_of(inputs(seed)["out"], FP)
        for u, c in zip(us, coeffs):
            s = [c % m]
            for u_j in reversed(u):
                s += [v * u_j % m for v in s]
            total = [(a + b) % m for a, b in zip(total, s)]
        return _b(limbs(total, FP))
    return Case("ipa-s-combine-accumulate", "h2_ipa_s_combine_device", (k, batch), inputs, lambda: {"out": ("in", "out", 32 << k)}, call, expected,
                fields_valid(FP, "out"))


def _collapsed_generators_case():
    k, rounds = COLLAPSED
    n, nj = 1 << k, 1 << (k - rounds)
    ch = rf(co.field_of_curve(COMMIT_CURVE, "scalar"), 0x7840, 0, rounds)

    def call(ins, outs, sp):
        ok(_lib().h2_ipa_collapsed_generators_device(commit_handle(n), k, rounds, _p(ch), MONT, outs["out"].data_ptr(), _st(sp)))

    def expected(seed):
        sf = co.field_of_curve(COMMIT_CURVE, "scalar")
        m, u = MODULUS[sf], ints_of(ch, sf)
        s = []
        for hh in range(1 << rounds):
            v = 1
            for r in range(rounds):
                if (hh >> (rounds - 1 - r)) & 1:
                    v = v * u[r] % m
            s.append(v)
        s_l, g = limbs(s, sf), _table_points(n)[0]
        return b"".join(cs._affine_limbs(COMMIT_CURVE, co.best_multiexp(COMMIT_CURVE, s_l, np.ascontiguousarray(g[i::nj]))) for i in range(nj))
    return Case("ipa-collapsed-generators", "h2_ipa_collapsed_generators_device", COLLAPSED, lambda seed: {}, lambda: {"out": 64 * nj}, call, expected,
                nothing_to_check)


OPEN_SEED = 8000 + IPA_SMALL_K


def _open_rng(seed, s_poly):
    """The rng of the argument: the first draw is s_poly (the call's input, or the host vector of the seed), the later ones are those of
    call_sequences.seeded_rng"""
    inner = cs.seeded_rng(IPA_SF, OPEN_SEED + 10)

    def rng(count):
        vals = inner(count)
        return s_poly if count == 1 << IPA_SMALL_K else vals
    return rng


def _open_inputs(seed):
    """REAL is the argument call_sequences.opening_proof_wanted restates"""
    px, _, _ = cs._opening_inputs(IPA_CURVE, IPA_SMALL_K, OPEN_SEED)
    s = co.random_field(IPA_SF, OPEN_SEED + 11, 1 << IPA_SMALL_K)
    if seed != REAL:
        px, s = rf(IPA_SF, 0x7850, seed, 1 << IPA_SMALL_K), rf(IPA_SF, 0x7851, seed, 1 << IPA_SMALL_K)
    return px, s


@functools.lru_cache(maxsize=None)
def _opening_points(k):
    """g, w, u of call_sequences.opening_params(IPA_CURVE, k, OPEN_SEED), without the Params (which needs a device)"""
    assert OPEN_SEED not in cs.IDENTITY_COLUMNS
    return co.generate_bases(IPA_CURVE, OPEN_SEED, 1 << k), co.generate_bases(IPA_CURVE, 60, 1)[0], co.generate_bases(IPA_CURVE, 61, 1)[0]


def _open_wanted(px, s_poly):
    g, w, u = _opening_points(IPA_SMALL_K)
    _, blind, x = cs._opening_inputs(IPA_CURVE, IPA_SMALL_K, OPEN_SEED)
    ot = oipa.Transcript(IPA_CURVE)
    oipa.create_proof(IPA_CURVE, IPA_SMALL_K, g, w, u, _open_rng(0, s_poly.copy()), ot, px, blind.value, x)
    return bytes(ot.out)


def open_proof_length():
    return 32 * (1 + 2 * IPA_SMALL_K + 2)


def _open_case(name, entry, resident_s):
    def call(ins, outs, sp):
        import halo2_amd as h  # noqa: F401
        from halo2_amd.opening import create_proof
        from halo2_amd.transcript import Blake2bWrite
        import torch
        params = cs.opening_params(IPA_CURVE, IPA_SMALL_K, OPEN_SEED)[0]
        _, blind, x = cs._opening_inputs(IPA_CURVE, IPA_SMALL_K, OPEN_SEED)
        tr = Blake2bWrite(IPA_CURVE)
        with on_stream(sp):
            p_poly = ins["p_poly"].view(torch.int64).view(-1, 4)
            s_poly = ins["s_poly"].view(torch.int64).view(-1, 4) if resident_s else _open_inputs(REAL)[1]
            create_proof(params, _open_rng(0, s_poly), tr, p_poly, blind, x)
        return tr.finalize()

    def inputs(seed):
        px, s = _open_inputs(seed)
        return {"p_poly": px, "s_poly": s} if resident_s else {"p_poly": px}

    def expected(seed):
        px, s = _open_inputs(seed)
        return _open_wanted(px, s if resident_s else _open_inputs(REAL)[1])
    return Case(name, entry, IPA_SMALL_K, inputs, lambda: {}, call, expected, fields_valid(IPA_SF, *(["p_poly", "s_poly"] if resident_s else ["p_poly"])),
                host_bytes=open_proof_length())


def _ipa_rounds_case():
    k = IPA_SMALL_K
    z = rf(IPA_SF, 0x7860, 0, 1)[0]
    rands = rf(IPA_SF, 0x7861, 0, 2 * k)

    def call(ins, outs, sp):
        import torch
        from halo2_amd.transcript import Blake2bWrite
        params = cs.opening_params(IPA_CURVE, k, OPEN_SEED)[0]
        tr = Blake2bWrite(IPA_CURVE)
        with on_stream(sp):
            c, f = params.opening_rounds(ins["p"].view(torch.int64).view(-1, 4), ins["b"].view(torch.int64).view(-1, 4), z, rands, tr, paired=False)
        return tr.finalize() + _b(c, f)

    def inputs(seed):
        return {"p": rf(IPA_SF, 0x7862, seed, 1 << k), "b": rf(IPA_SF, 0x7863, seed, 1 << k)}

    def expected(seed):
        """the round loop of oracle/ipa.py's create_proof (prover.rs:104-142) from a given p', b and z"""
        g, w, u = _opening_points(k)
        m = MODULUS[IPA_SF]
        one = lambda v: ints_of(v, IPA_SF)[0]
        a = inputs(seed)
        p_prime, b, g_prime, uw = a["p"].copy(), a["b"].copy(), np.ascontiguousarray(g).copy(), np.stack([u, w])
        ot, z_i, f = oipa.Transcript(IPA_CURVE), one(z), 0
        for j in range(k):
            half = 1 << (k - j - 1)
            l_j = co.best_multiexp(IPA_CURVE, p_prime[half:], g_prime[:half])
            r_j = co.best_multiexp(IPA_CURVE, p_prime[:half], g_prime[half:])
            value_l, value_r = one(co.inner_product(IPA_SF, p_prime[half:], b[:half])), one(co.inner_product(IPA_SF, p_prime[:half], b[half:]))
            l_rand, r_rand = rands[2 * j], rands[2 * j + 1]
            for acc, val, rnd in ((l_j, value_l, l_rand), (r_j, value_r, r_rand)):
                extra = co.best_multiexp(IPA_CURVE, np.stack([fe(IPA_SF, val * z_i), rnd]), uw)
                co.lib().orc_point_add(IPA_CURVE, co._p(acc), co._p(acc), co._p(extra))
            ot.write_point(co.jac_to_affine_ints(IPA_CURVE, l_j))
            ot.write_point(co.jac_to_affine_ints(IPA_CURVE, r_j))
            u_j = ot.squeeze_challenge()
            u_inv = pow(u_j, -1, m)
            p_prime, b = co.fold_scalars(IPA_SF, p_prime, fe(IPA_SF, u_inv)), co.fold_scalars(IPA_SF, b, fe(IPA_SF, u_j))
            g_prime = co.generator_collapse(IPA_CURVE, g_prime, fe(IPA_SF, u_j))
            f = (f + one(l_rand) * u_inv + one(r_rand) * u_j) % m
        return bytes(ot.out) + _b(p_prime[0], fe(IPA_SF, f))
    return Case("ipa-rounds", "h2_ipa_rounds_device", k, inputs, lambda: {}, call, expected, fields_valid(IPA_SF, "p", "b"), host_bytes=64 * k + 64)


# ---- f. selector compression, the evaluator, the lookup argument, the MockProver's checks -----------------------------------------------
SEL_N = ssc.K_TILE + 1
SEL_WORDS = (SEL_N + 31) // 32
SEL_COUNT = 5
SEL_COLUMNS = 2


def _bit_rows(keep):
    """(S, n_words) uint32 planes with bit r of selector s set where keep(s, r)"""
    bits = np.zeros((SEL_COUNT, SEL_WORDS), dtype=np.uint32)
    for s in range(SEL_COUNT):
        for r in range(SEL_N):
            if keep(s, r):
                bits[s, r >> 5] |= np.uint32(1 << (r & 31))
    return bits


def _rows_of(bits):
    return [{r for r in range(SEL_N) if (int(bits[s * SEL_WORDS + (r >> 5)]) >> (r & 31)) & 1} for s in range(SEL_COUNT)]


def _no_bits_past_n(bits):
    assert not any(int(w) >> (SEL_N & 31) for w in np.asarray(bits).reshape(SEL_COUNT, SEL_WORDS)[:, -1]), "bits past n must be zero"


def _selector_conflicts_case():
    def inputs(seed):
        """selector s may be enabled on the rows of two residues mod 7, so some pairs meet and some never do"""
        rnd = random.Random(0x7900 + seed)
        return {"bits": _bit_rows(lambda s, r: r % 7 in (s, (s + 1) % 7) and rnd.random() < 0.3).reshape(-1)}

    def call(ins, outs, sp):
        ok(_lib().h2_selector_conflicts_device(ins["bits"].data_ptr(), SEL_COUNT, SEL_WORDS, outs["out"].data_ptr(), _st(sp)))

    def expected(seed):
        rows = _rows_of(inputs(seed)["bits"])
        return bytes(1 if i != j and rows[i] & rows[j] else 0 for i in range(SEL_COUNT) for j in range(SEL_COUNT))
    return Case("selector-conflicts", "h2_selector_conflicts_device", (SEL_COUNT, SEL_N), inputs, lambda: {"out": SEL_COUNT * SEL_COUNT}, call, expected,
                lambda arrays: _no_bits_past_n(arrays["bits"]))


def _selector_combine_case():
    def inputs(seed):
        """selector s is enabled only on rows = s mod 5: no two selectors share a row under any mixture of two seeds"""
        rnd = random.Random(0x7910 + seed)
        return {"bits": _bit_rows(lambda s, r: r % SEL_COUNT == s and rnd.random() < 0.6).reshape(-1),
                "roots": np.array([1 + (s + seed) % 3 for s in range(SEL_COUNT)], dtype=np.uint32),
                "columns": np.array([((s // 2 if seed == THIRD else s + seed)) % SEL_COLUMNS for s in range(SEL_COUNT)], dtype=np.uint32)}

    def valid(arrays):
        _no_bits_past_n(arrays["bits"])
        rows = _rows_of(arrays["bits"])
        assert all(not rows[i] & rows[j] for i in range(SEL_COUNT) for j in range(i)), "two selectors share a row"
        assert all(int(c) < SEL_COLUMNS for c in arrays["columns"])

    def call(ins, outs, sp):
        ok(_lib().h2_selector_combine_device(FP, ins["bits"].data_ptr(), ins["roots"].data_ptr(), ins["columns"].data_ptr(), SEL_COUNT, SEL_N,
                                             outs["out"].data_ptr(), SEL_COLUMNS, _st(sp)))

    def expected(seed):
        a = inputs(seed)
        cols = [[0] * SEL_N for _ in range(SEL_COLUMNS)]
        for s, rows in enumerate(_rows_of(a["bits"])):
            for r in rows:
                cols[int(a["columns"][s])][r] = int(a["roots"][s])
        return _b(*[limbs(col, FP) for col in cols])
    return Case("selector-combine", "h2_selector_combine_device", (SEL_COUNT, SEL_N, SEL_COLUMNS), inputs, lambda: {"out": SEL_COLUMNS * SEL_N * 32},
                call, expected, valid)


EVAL_CASE = cs.EVAL_SHAPES[1]


def _evaluate_case():
    basis, log_len, words, consts, polys0, omega, values0 = cs._eval_case(EVAL_CASE)
    n, m, names = 1 << log_len, MODULUS[FP], [f"poly{i}" for i in range(len(polys0))]

    def polys(seed):
        if seed == REAL:
            return polys0
        rnd = random.Random(0x7920 + seed)
        return [[rnd.randrange(m) for _ in range(n)] for _ in polys0]

    def call(ins, outs, sp):
        prog = (C.c_uint32 * len(words))(*words)
        cst = np.ascontiguousarray(limbs(consts or [0], FP))
        ok(_lib().h2_evaluate_device(FP, basis, prog, len(words), _p(cst), len(consts), _vp(*[ins[nm] for nm in names]), len(names), log_len,
                                     _p(fe(FP, omega)), outs["out"].data_ptr(), _st(sp)))

    def expected(seed):
        import evaluator_model as em
        return _b(limbs(values0 if seed == REAL else em.interpret(words, consts, polys(seed), basis, n, m, omega)[0], FP))
    return Case("evaluate", "h2_evaluate_device", EVAL_CASE, lambda seed: {nm: limbs(p, FP) for nm, p in zip(names, polys(seed))},
                lambda: {"out": 32 * n}, call, expected, fields_valid(FP, *names), mode_c=True)


def _planes(flags):
    """one bit per row, row r = bit r % 64 of 64-bit word r / 64"""
    words = np.zeros((len(flags) + 63) // 64, dtype=np.uint64)
    for r, v in enumerate(flags):
        if v:
            words[r >> 6] |= np.uint64(1 << (r & 63))
    return words


def _check_expressions_case():
    import evaluator_cases as ec
    import evaluator_model as em
    programs, offsets, consts, polys0 = ec.mock_programs(FP)
    log_len, n, m = ec.MOCK_LOG_LEN, 1 << ec.MOCK_LOG_LEN, MODULUS[FP]
    names, n_programs = [f"poly{i}" for i in range(len(polys0))], len(offsets) - 1

    def polys(seed):
        if seed == REAL:
            return polys0
        rnd = random.Random(0x7930 + seed)
        return [[rnd.randrange(m) for _ in range(n)] for _ in polys0]

    def call(ins, outs, sp):
        cst = np.ascontiguousarray(limbs(consts, FP))
        values = outs["values"].data_ptr()
        ok(_lib().h2_check_expressions_device(FP, (C.c_uint32 * len(programs))(*programs), (C.c_size_t * len(offsets))(*offsets), n_programs, _p(cst),
                                              len(consts), _vp(*[ins[nm] for nm in names]), (C.c_uint8 * len(names))(*([0] * len(names))), len(names),
                                              log_len, n, outs["nonzero"].data_ptr(), outs["poison"].data_ptr(), outs["counts"].data_ptr(),
                                              _vp(*[values + 32 * n * p for p in range(n_programs)]), _st(sp)))

    def expected(seed):
        """no advice column, every row usable: no poison, the non-zero plane is `value != 0`"""
        runs = [em.interpret(programs[offsets[p]:offsets[p + 1]], consts, polys(seed), ec.LAGRANGE, n, m, None)[0] for p in range(n_programs)]
        counts = np.array([c for v in runs for c in (sum(1 for x in v if x), 0)], dtype=np.uint32)
        return _b(*[_planes(v) for v in runs], np.zeros(n_programs * (n // 64), dtype=np.uint64), counts, *[limbs(v, FP) for v in runs])
    return Case("check-expressions", "h2_check_expressions_device", log_len, lambda seed: {nm: limbs(p, FP) for nm, p in zip(names, polys(seed))},
                lambda: {"nonzero": n_programs * n // 8, "poison": n_programs * n // 8, "counts": 8 * n_programs, "values": n_programs * n * 32},
                call, expected, fields_valid(FP, *names))


LOOKUP_N = ssc.K_TILE + 1


def _sort_case():
    def inputs(seed):
        a = rf(FP, 0x7940, seed, LOOKUP_N)
        a[LOOKUP_N // 2] = a[0]                                   # a repeated value
        return {"a": a}
    return Case("sort", "h2_sort_device", LOOKUP_N, inputs, lambda: {"a": ("in", "a", 32 * LOOKUP_N)},
                lambda ins, outs, sp: ok(_lib().h2_sort_device(FP, ins["a"].data_ptr(), LOOKUP_N, MONT, _st(sp))),
                lambda seed: _b(limbs(sorted(ints_of(inputs(seed)["a"], FP)), FP)), fields_valid(FP, "a"), mode_c=True)


@functools.lru_cache(maxsize=None)
def _lookup_values():
    rnd = random.Random(0x7950)
    return [rnd.randrange(MODULUS[FP]) for _ in range((LOOKUP_N + 1) // 2)]


def _permute_inputs(seed):
    """Table rows 2 j hold value j under every seed, so every mixture of two tables still holds every value; the odd rows and the
    inputs are the seed's choice among the same values."""
    vals, rnd = _lookup_values(), random.Random(0x7951 + seed)
    table = [vals[i // 2] if i % 2 == 0 else rnd.choice(vals) for i in range(LOOKUP_N)]
    return [rnd.choice(vals) for _ in range(LOOKUP_N)], table


def _permute_case():
    def inputs(seed):
        inp, table = _permute_inputs(seed)
        return {"input": limbs(inp, FP), "table": limbs(table, FP)}

    def valid(arrays):
        below_modulus(arrays["input"], FP)
        below_modulus(arrays["table"], FP)
        assert olk.permute_expression_pair(ints_of(arrays["input"], FP), ints_of(arrays["table"], FP), LOOKUP_N) is not None, "ConstraintSystemFailure"

    def call(ins, outs, sp):
        ok(_lib().h2_permute_expression_pair_device(FP, ins["input"].data_ptr(), ins["table"].data_ptr(), LOOKUP_N, MONT,
                                                    outs["permuted_input"].data_ptr(), outs["permuted_table"].data_ptr(), _st(sp)))

    def expected(seed):
        a, s = olk.permute_expression_pair(*_permute_inputs(seed), LOOKUP_N)
        return _b(limbs(a, FP), limbs(s, FP))
    return Case("permute-expression-pair", "h2_permute_expression_pair_device", LOOKUP_N, inputs,
                lambda: {"permuted_input": 32 * LOOKUP_N, "permuted_table": 32 * LOOKUP_N}, call, expected, valid, mode_c=True)


CHECK_N, CHECK_USABLE, CHECK_W = ssc.K_TILE + 1, ssc.K_TILE - 6, 2


def _lookup_check_case():
    names = [f"{kind}{c}" for kind in ("input", "table") for c in range(CHECK_W)]

    def ints(seed):
        """tuples of small components (so that a tuple, not a component, decides); five input rows hold a tuple the table lacks"""
        rnd = random.Random(0x7960 + seed)
        table = [tuple(rnd.randrange(40) for _ in range(CHECK_W)) for _ in range(CHECK_N)]
        inp = [rnd.choice(table[:CHECK_USABLE]) for _ in range(CHECK_N)]
        for r in rnd.sample(range(CHECK_USABLE), 5):
            inp[r] = (41 + r, 0)
        return inp, table

    def inputs(seed):
        inp, table = ints(seed)
        cols = [[t[c] for t in inp] for c in range(CHECK_W)] + [[t[c] for t in table] for c in range(CHECK_W)]
        return {nm: limbs(col, FP) for nm, col in zip(names, cols)}

    def call(ins, outs, sp):
        ok(_lib().h2_lookup_check_device(FP, _vp(*[ins[f"input{c}"] for c in range(CHECK_W)]), None, _vp(*[ins[f"table{c}"] for c in range(CHECK_W)]), None,
                                         CHECK_W, CHECK_N, CHECK_USABLE, MONT, outs["fail"].data_ptr(), outs["count"].data_ptr(), _st(sp)))

    def expected(seed):
        inp, table = ints(seed)
        present = set(table[:CHECK_USABLE])
        fail = [r < CHECK_USABLE and inp[r] not in present for r in range(CHECK_N)]
        assert sum(fail) == 5
        return _b(_planes(fail), np.array([sum(fail)], dtype=np.uint32))
    return Case("lookup-check", "h2_lookup_check_device", (CHECK_W, CHECK_N, CHECK_USABLE), inputs, lambda: {"fail": 8 * ((CHECK_N + 63) // 64), "count": 4},
                call, expected, fields_valid(FP, *names))


PERM_LOG, PERM_COLUMNS = 9, 3


def _permutation_check_case():
    n = 1 << PERM_LOG
    names = [f"column{c}" for c in range(PERM_COLUMNS)]

    def ints(seed):
        """transpositions of cells: forty that hold equal values, three that do not; every other cell maps to itself"""
        rnd = random.Random(0x7970 + seed)
        cols = [[rnd.randrange(MODULUS[FP]) for _ in range(n)] for _ in range(PERM_COLUMNS)]
        mapping = list(range(PERM_COLUMNS * n))
        cells = rnd.sample(range(PERM_COLUMNS * n), 86)
        for i in range(43):
            a, b = cells[2 * i], cells[2 * i + 1]
            mapping[a], mapping[b] = b, a
            if i < 40:
                cols[b // n][b % n] = cols[a // n][a % n]
        return cols, mapping

    def inputs(seed):
        cols, mapping = ints(seed)
        out = {nm: limbs(col, FP) for nm, col in zip(names, cols)}
        out["mapping"] = np.array(mapping, dtype=np.int64)
        return out

    def valid(arrays):
        for nm in names:
            below_modulus(arrays[nm], FP)
        assert all(0 <= int(v) < PERM_COLUMNS * n for v in arrays["mapping"]), "a mapping entry outside the table"

    def call(ins, outs, sp):
        ok(_lib().h2_permutation_check_device(FP, _vp(*[ins[nm] for nm in names]), (C.c_uint8 * PERM_COLUMNS)(0, 0, 0), PERM_COLUMNS,
                                              ins["mapping"].data_ptr(), PERM_LOG, n, MONT, outs["fail"].data_ptr(), outs["counts"].data_ptr(), _st(sp)))

    def expected(seed):
        cols, mapping = ints(seed)
        flat = [v for col in cols for v in col]
        fail = [[flat[c * n + r] != flat[mapping[c * n + r]] for r in range(n)] for c in range(PERM_COLUMNS)]
        assert sum(map(sum, fail)) == 6
        return _b(*[_planes(f) for f in fail], np.array([sum(f) for f in fail], dtype=np.uint32))
    return Case("permutation-check", "h2_permutation_check_device", (PERM_COLUMNS, PERM_LOG), inputs,
                lambda: {"fail": PERM_COLUMNS * n // 8, "counts": 4 * PERM_COLUMNS}, call, expected, valid)


# ---- g. compressed points and hash-to-curve -----------------------------------------------------------------------------------------------
ENCODED = 257
H2C_MESSAGES, H2C_LEN, H2C_PREFIX = 65, 5, "Halo2-Parameters"


def _encoded_points(seed):
    g = co.generate_bases(PALLAS, 0x7A00 + 0x101 * seed, ENCODED)
    g[ENCODED // 2] = 0                                           # the identity: 32 zero bytes
    return g


def _encodings(points) -> bytes:
    return b"".join(o.point_to_bytes(co.affine_to_ints(PALLAS, pt), P) for pt in points)


def _compress_case():
    return Case("points-compress", "h2_points_compress_device", ENCODED, lambda seed: {"xy": _encoded_points(seed)}, lambda: {"bytes": 32 * ENCODED},
                lambda ins, outs, sp: ok(_lib().h2_points_compress_device(PALLAS, ins["xy"].data_ptr(), ENCODED, MONT, outs["bytes"].data_ptr(), _st(sp))),
                lambda seed: _encodings(_encoded_points(seed)), _points_valid(PALLAS, points=["xy"]))


def _decompress_case():
    def inputs(seed):
        return {"bytes": np.frombuffer(_encodings(_encoded_points(seed)), dtype=np.uint8).reshape(ENCODED, 32).copy()}

    def valid(arrays):
        for row in arrays["bytes"]:
            o.point_from_bytes(row.tobytes(), P)                  # raises where from_bytes yields none
    return Case("points-decompress", "h2_points_decompress_device", ENCODED, inputs, lambda: {"xy": 64 * ENCODED},
                lambda ins, outs, sp: ok(_lib().h2_points_decompress_device(PALLAS, ins["bytes"].data_ptr(), ENCODED, MONT, outs["xy"].data_ptr(), _st(sp))),
                lambda seed: _b(_encoded_points(seed)), valid)


def _hash_to_curve_case():
    def inputs(seed):
        rnd = random.Random(0x7A10 + seed)
        return {"msgs": np.array([[rnd.randrange(256) for _ in range(H2C_LEN)] for _ in range(H2C_MESSAGES)], dtype=np.uint8)}

    def expected(seed):
        hasher = oh.hash_to_curve("pallas", H2C_PREFIX)
        return _b(point_limbs([hasher(row.tobytes()) for row in inputs(seed)["msgs"]]))
    return Case("hash-to-curve", "h2_hash_to_curve_device", (H2C_MESSAGES, H2C_LEN), inputs, lambda: {"xy": 64 * H2C_MESSAGES},
                lambda ins, outs, sp: ok(_lib().h2_hash_to_curve_device(PALLAS, H2C_PREFIX.encode(), ins["msgs"].data_ptr(), H2C_LEN, H2C_MESSAGES, MONT,
                                                                        outs["xy"].data_ptr(), _st(sp))),
                expected, lambda arrays: None)


# ---- h. the gadgets: 65 lanes are two workgroups, and the traces' two-pass inversion in between ----------------------------------------------
LANES = cs.TRACE_COUNTS[1]


def _poseidon_cases():
    import poseidon_cases as pc
    states = lambda seed: pc.random_states(LANES, FP, 0x7B00 + seed)
    messages = lambda seed: [s + s[:1] for s in pc.random_states(LANES, FP, 0x7B10 + seed)]       # 4 elements: two permutations, no padding
    flat = lambda rows: limbs([v for row in rows for v in row], FP).reshape(len(rows), -1, 4)
    L = _lib
    return {
        "h2_poseidon_permute_device": Case(
            "poseidon-permute", "h2_poseidon_permute_device", LANES, lambda seed: {"states": flat(states(seed))}, lambda: {"out": 96 * LANES},
            lambda i, u, sp: ok(L().h2_poseidon_permute_device(FP, i["states"].data_ptr(), LANES, u["out"].data_ptr(), _st(sp))),
            lambda seed: _b(flat([pc.permute_ints(s, FP) for s in states(seed)])), fields_valid(FP, "states")),
        "h2_poseidon_hash_device": Case(
            "poseidon-hash", "h2_poseidon_hash_device", (LANES, 4), lambda seed: {"messages": flat(messages(seed))}, lambda: {"out": 32 * LANES},
            lambda i, u, sp: ok(L().h2_poseidon_hash_device(FP, i["messages"].data_ptr(), LANES, 4, u["out"].data_ptr(), _st(sp))),
            lambda seed: _b(limbs([pc.hash_ints(msg, FP) for msg in messages(seed)], FP)), fields_valid(FP, "messages")),
        "h2_poseidon_trace_device": Case(
            "poseidon-trace", "h2_poseidon_trace_device", LANES, lambda seed: {"states": flat(states(seed))}, lambda: {"columns": 4 * 37 * LANES * 32},
            lambda i, u, sp: ok(L().h2_poseidon_trace_device(FP, i["states"].data_ptr(), LANES, u["columns"].data_ptr(), _st(sp))),
            lambda seed: _b(pc.trace_limbs(states(seed), FP)), fields_valid(FP, "states")),
    }


HASH_WORDS = 52                                                   # the length of a MerkleCRH message
MERKLE_LAYER = 7


def sinsemilla_table(stream_ptr):
    """halo2_amd.sinsemilla's generator table as its wrappers fetch it: with the call's stream current"""
    from halo2_amd import sinsemilla
    with on_stream(stream_ptr):
        return sinsemilla.generator_table()


def _status(points):
    return bytes(1 if pt is None else 0 for pt in points)


def _sinsemilla_cases():
    import sinsemilla_cases as sc
    import sinsemilla_commit_cases as cc
    import ecc_cases as ec
    import ecc_fixed_cases as fx
    L = _lib
    q_merkle = lambda: sc.q_of(sc.MERKLE_DOMAIN)
    q_limbs = lambda q: np.ascontiguousarray(point_limbs([q]).reshape(8))
    out = {}

    def words(seed, length=HASH_WORDS):
        rnd = random.Random(0x7C00 + seed)
        return np.array([[rnd.randrange(1024) for _ in range(length)] for _ in range(LANES)], dtype=np.uint16)

    def ten_bits(*names):
        def valid(arrays):
            for nm in names:
                assert int(arrays[nm].max()) < 1024
        return valid

    def qs(seed):
        return cc.private_qs()[:LANES] if seed == REAL else ec.random_bases(LANES, seed=0x7C10 + seed)

    def both(*checks):
        def valid(arrays):
            for check in checks:
                check(arrays)
        return valid

    # -- the hash, from the domain's Q and from a point per message
    out["h2_sinsemilla_hash_device"] = Case(
        "sinsemilla-hash", "h2_sinsemilla_hash_device", (LANES, HASH_WORDS), lambda seed: {"words": words(seed)}, lambda: {"xy": 64 * LANES, "status": LANES},
        lambda i, u, sp: ok(L().h2_sinsemilla_hash_device(i["words"].data_ptr(), LANES, HASH_WORDS, _p(q_limbs(q_merkle())), sinsemilla_table(sp).data_ptr(),
                                                          u["xy"].data_ptr(), u["status"].data_ptr(), _st(sp))),
        lambda seed: (lambda pts: _b(point_limbs(pts)) + _status(pts))([sc.hash_to_point(q_merkle(), [int(w) for w in row]) for row in words(seed)]),
        ten_bits("words"), mode_c=True)
    out["h2_sinsemilla_hash_from_device"] = Case(
        "sinsemilla-hash-from", "h2_sinsemilla_hash_from_device", (LANES, HASH_WORDS), lambda seed: {"words": words(seed), "q": point_limbs(qs(seed))},
        lambda: {"xy": 64 * LANES, "status": LANES},
        lambda i, u, sp: ok(L().h2_sinsemilla_hash_from_device(i["words"].data_ptr(), LANES, HASH_WORDS, i["q"].data_ptr(), sinsemilla_table(sp).data_ptr(),
                                                               u["xy"].data_ptr(), u["status"].data_ptr(), _st(sp))),
        lambda seed: (lambda pts: _b(point_limbs(pts)) + _status(pts))([sc.hash_to_point(q, [int(w) for w in row]) for q, row in zip(qs(seed), words(seed))]),
        both(ten_bits("words"), _points_valid(PALLAS, points=["q"])), mode_c=True)

    # -- MerkleCRH of 65 pairs
    def pairs(seed):
        rnd = random.Random(0x7C20 + seed)
        return [(rnd.randrange(P), rnd.randrange(P)) for _ in range(LANES)]

    def merkle_wanted(seed):
        xs = [sc.merkle_crh(q_merkle(), MERKLE_LAYER, left, right) for left, right in pairs(seed)]
        return _b(limbs([x or 0 for x in xs], FP)) + _status(xs)
    out["h2_sinsemilla_merkle_layer_device"] = Case(
        "sinsemilla-merkle-layer", "h2_sinsemilla_merkle_layer_device", LANES, lambda seed: {"pairs": limbs([v for pr in pairs(seed) for v in pr], FP).reshape(-1, 8)},
        lambda: {"x": 32 * LANES, "status": LANES},
        lambda i, u, sp: ok(L().h2_sinsemilla_merkle_layer_device(MERKLE_LAYER, i["pairs"].data_ptr(), LANES, _p(q_limbs(q_merkle())),
                                                                  sinsemilla_table(sp).data_ptr(), u["x"].data_ptr(), u["status"].data_ptr(), _st(sp))),
        merkle_wanted, fields_valid(FP, "pairs"), mode_c=True)

    # -- the two witness traces
    nw = sc.STRUCTURES["merkle"]
    rows = sum(nw) + 1

    def pieces(seed):
        return [sc.random_pieces(nw, 0x7C30 + 100 * seed + i, high_zero=i % 3 == 1) for i in range(LANES)]

    def piece_limbs(msgs):
        return limbs([p for msg in msgs for p in msg], FP, montgomery=False).reshape(len(msgs), -1, 4)

    def pieces_valid(structure):
        def valid(arrays):
            for msg in arrays["pieces"]:
                assert all(v < 1 << (10 * w) for v, w in zip(ints_of(msg, FP, montgomery=False), structure)), "a piece is wider than its words"
        return valid
    num_words = lambda structure: (C.c_uint32 * len(structure))(*structure)
    out["h2_sinsemilla_trace_device"] = Case(
        "sinsemilla-trace", "h2_sinsemilla_trace_device", (LANES, tuple(nw)), lambda seed: {"pieces": piece_limbs(pieces(seed))},
        lambda: {"columns": 5 * rows * LANES * 32, "status": LANES},
        lambda i, u, sp: ok(L().h2_sinsemilla_trace_device(i["pieces"].data_ptr(), LANES, num_words(nw), len(nw), _p(q_limbs(q_merkle())),
                                                           sinsemilla_table(sp).data_ptr(), u["columns"].data_ptr(), u["status"].data_ptr(), _st(sp))),
        lambda seed: cs._columns([sc.trace(q_merkle(), msg, nw) for msg in pieces(seed)], 5) + bytes(LANES), pieces_valid(nw), mode_c=True)
    cw = cc.COMMIT_WORDS
    rows_from = sum(cw) + 2
    commit_pieces = lambda seed: cc.random_messages(cw, LANES, seed=0x7C + seed)
    out["h2_sinsemilla_trace_from_device"] = Case(
        "sinsemilla-trace-from", "h2_sinsemilla_trace_from_device", (LANES, tuple(cw)),
        lambda seed: {"pieces": piece_limbs(commit_pieces(seed)), "q": point_limbs(qs(seed))}, lambda: {"columns": 5 * rows_from * LANES * 32, "status": LANES},
        lambda i, u, sp: ok(L().h2_sinsemilla_trace_from_device(i["pieces"].data_ptr(), LANES, num_words(cw), len(cw), i["q"].data_ptr(),
                                                                sinsemilla_table(sp).data_ptr(), u["columns"].data_ptr(), u["status"].data_ptr(), _st(sp))),
        lambda seed: cs._columns([cc.trace_from(q, msg, cw) for q, msg in zip(qs(seed), commit_pieces(seed))], 5) + bytes(LANES),
        both(pieces_valid(cw), _points_valid(PALLAS, points=["q"])), mode_c=True)

    # -- the commitment: hash and blinding product in one launch
    commit_len = sum(cw)

    def scalars(seed):
        return (fx.EDGE_SCALARS + ec.random_scalars(LANES, seed=0x7C40 + seed))[:LANES] if seed == REAL else ec.random_scalars(LANES, seed=0x7C40 + seed)

    def commit_wanted(seed):
        q = cc.q_of(cc.PERSONALIZATION)
        pts = [cc.commit(q, [int(w) for w in row], r) for row, r in zip(words(seed, commit_len), scalars(seed))]
        return _b(point_limbs(pts)) + _status(pts)

    def commit_call(i, u, sp):
        ok(L().h2_sinsemilla_commit_device(i["words"].data_ptr(), LANES, commit_len, _p(q_limbs(cc.q_of(cc.PERSONALIZATION))), None,
                                           sinsemilla_table(sp).data_ptr(), commit_domain().fixed_base.points.data_ptr(), i["scalars"].data_ptr(),
                                           u["xy"].data_ptr(), u["status"].data_ptr(), _st(sp)))
    out["h2_sinsemilla_commit_device"] = Case(
        "sinsemilla-commit", "h2_sinsemilla_commit_device", (LANES, commit_len),
        lambda seed: {"words": words(seed, commit_len), "scalars": limbs(scalars(seed), FP, montgomery=False)}, lambda: {"xy": 64 * LANES, "status": LANES},
        commit_call, commit_wanted, both(ten_bits("words"), below_2_255("scalars")), mode_c=True)
    return out


def below_2_255(name):
    def valid(arrays):
        assert not (np.asarray(arrays[name], dtype=np.uint64).reshape(-1, 4)[:, 3] >> np.uint64(63)).any(), "a scalar has bit 255 set"
    return valid


@functools.lru_cache(maxsize=None)
def commit_domain():
    """CommitDomain("MerkleCRH") with R's window table on the device (a set-up object)"""
    import sinsemilla_commit_cases as cc
    from halo2_amd import sinsemilla
    dom = sinsemilla.CommitDomain(cc.PERSONALIZATION)
    dom.fixed_base                                               # noqa: B018 -- builds the table
    return dom


def _square_roots_at(offset, count):
    """post: `count` Montgomery elements from byte `offset` on are roots whose sign the library picks: compare their squares"""
    def post(name, raw):
        v = ints_of(np.frombuffer(raw[offset:offset + 32 * count], dtype=np.uint64), FP)
        return raw[:offset] + _b(limbs([x * x % P for x in v], FP)) + raw[offset + 32 * count:]
    return post


def _ecc_cases():
    import ecc_cases as ec
    import ecc_fixed_cases as fx
    import sinsemilla_commit_cases as cc
    L = _lib
    out = {}
    bases = lambda seed: ec.random_bases(LANES, seed=0x7D00 + seed)

    def scalars(seed):
        rnd = ec.random_scalars(LANES, seed=0x7D10 + seed)
        return (fx.EDGE_SCALARS + rnd)[:LANES] if seed == REAL else rnd
    canonical = lambda ks: limbs(ks, FP, montgomery=False)
    on_pallas = lambda *names: _points_valid(PALLAS, points=list(names))

    def both(*checks):
        def valid(arrays):
            for check in checks:
                check(arrays)
        return valid

    # -- variable base: the products, and the witness of the chip
    out["h2_ecc_mul_device"] = Case(
        "ecc-mul", "h2_ecc_mul_device", LANES, lambda seed: {"bases": point_limbs(bases(seed)), "scalars": canonical(scalars(seed))},
        lambda: {"xy": 64 * LANES, "status": LANES},
        lambda i, u, sp: ok(L().h2_ecc_mul_device(i["bases"].data_ptr(), i["scalars"].data_ptr(), LANES, u["xy"].data_ptr(), u["status"].data_ptr(), _st(sp))),
        lambda seed: _b(point_limbs([ec.ec_mul(k, b) for k, b in zip(scalars(seed), bases(seed))])) + bytes(LANES),
        both(on_pallas("bases"), below_2_255("scalars")))

    def alphas(seed):
        a = [v % P for v in ec.random_scalars(LANES, bits=254, seed=0x7D20 + seed)]
        a[0] = 0
        return a

    def mul_trace_wanted(seed):
        want = [ec.mul_trace(b, a) for b, a in zip(bases(seed), alphas(seed))]
        return cs._columns([w[0] for w in want], 10) + _b(limbs([v for w in want for v in w[1]], FP)) + bytes(LANES)
    out["h2_ecc_mul_trace_device"] = Case(
        "ecc-mul-trace", "h2_ecc_mul_trace_device", LANES, lambda seed: {"bases": point_limbs(bases(seed)), "alphas": limbs(alphas(seed), FP)},
        lambda: {"columns": 10 * 137 * LANES * 32, "aux": 16 * LANES * 32, "status": LANES},
        lambda i, u, sp: ok(L().h2_ecc_mul_trace_device(i["bases"].data_ptr(), i["alphas"].data_ptr(), LANES, u["columns"].data_ptr(), u["aux"].data_ptr(),
                                                        u["status"].data_ptr(), _st(sp))),
        mul_trace_wanted, both(on_pallas("bases"), fields_valid(FP, "alphas")))

    # -- fixed base: the tables (no device input), the products and the witness over the generator's tables
    nw = fx.NUM_WINDOWS

    def tables_wanted(seed):
        table, coeffs, zs, us = fx.generator_tables(nw)
        return _b(point_limbs([pt for row in table for pt in row]), limbs([c for row in coeffs for c in row], FP), np.array(zs, dtype=np.uint64),
                  limbs([u for row in us for u in row], FP))
    out["h2_ecc_fixed_tables_device"] = Case(
        "ecc-fixed-tables", "h2_ecc_fixed_tables_device", ("generator", nw), lambda seed: {},
        lambda: {"points": nw * 8 * 64, "lagrange": nw * 8 * 32, "z": nw * 8, "u": nw * 8 * 32},
        lambda i, u, sp: ok(L().h2_ecc_fixed_tables_device(_p(np.ascontiguousarray(point_limbs([fx.GENERATOR]).reshape(8))), nw, 0, u["points"].data_ptr(),
                                                           u["lagrange"].data_ptr(), u["z"].data_ptr(), u["u"].data_ptr(), _st(sp))),
        tables_wanted, nothing_to_check, post=lambda name, raw: _square_roots_at(0, nw * 8)(name, raw) if name == "u" else raw)
    out["h2_ecc_mul_fixed_device"] = Case(
        "ecc-mul-fixed", "h2_ecc_mul_fixed_device", LANES, lambda seed: {"scalars": canonical(scalars(seed))}, lambda: {"xy": 64 * LANES},
        lambda i, u, sp: ok(L().h2_ecc_mul_fixed_device(cs.generator_fixed_base().points.data_ptr(), nw, i["scalars"].data_ptr(), LANES, u["xy"].data_ptr(), _st(sp))),
        lambda seed: _b(point_limbs([ec.ec_mul(k, fx.GENERATOR) for k in scalars(seed)])), below_2_255("scalars"))

    def fixed_trace_wanted(seed):
        """over the host tables and the oracle's roots; the column u is compared as its squares (either root is a valid table)"""
        table, _, _, us = fx.generator_tables(nw)
        want = [fx.mul_fixed_trace(table, us, k) for k in scalars(seed)]
        return cs._columns([w[0] for w in want], 6) + _b(limbs([v for w in want for v in w[1]], FP))
    fixed_base = cs.generator_fixed_base
    out["h2_ecc_mul_fixed_trace_device"] = Case(
        "ecc-mul-fixed-trace", "h2_ecc_mul_fixed_trace_device", LANES, lambda seed: {"scalars": canonical(scalars(seed))},
        lambda: {"columns": 6 * nw * LANES * 32, "aux": 11 * LANES * 32},
        lambda i, u, sp: ok(L().h2_ecc_mul_fixed_trace_device(fixed_base().points.data_ptr(), fixed_base().us.data_ptr(), nw, i["scalars"].data_ptr(), LANES,
                                                              u["columns"].data_ptr(), u["aux"].data_ptr(), _st(sp))),
        fixed_trace_wanted, below_2_255("scalars"),
        post=lambda name, raw: _square_roots_at(5 * nw * LANES * 32, nw * LANES)(name, raw) if name == "columns" else raw)

    # -- complete additions, every branch
    def add_pairs(seed):
        if seed == REAL:
            return cc.add_pairs(LANES)
        pts = ec.random_bases(2 * LANES, seed=0x7D30 + seed)
        return [(pts[2 * i], pts[2 * i + 1]) for i in range(LANES)]
    out["h2_ecc_add_trace_device"] = Case(
        "ecc-add-trace", "h2_ecc_add_trace_device", LANES,
        lambda seed: {"p": point_limbs([a for a, _ in add_pairs(seed)]), "q": point_limbs([b for _, b in add_pairs(seed)])}, lambda: {"aux": 11 * LANES * 32},
        lambda i, u, sp: ok(L().h2_ecc_add_trace_device(i["p"].data_ptr(), i["q"].data_ptr(), LANES, u["aux"].data_ptr(), _st(sp))),
        lambda seed: _b(limbs([v for a, b in add_pairs(seed) for v in cc.add_row(a, b)], FP)), on_pallas("p", "q"))
    return out


RANGE_WORDS, SHORT_BITS = 10, 6


def _range_check_cases():
    def values(seed, bits):
        """most values fit, every fifth is wider (its status is 1, its rows are written all the same)"""
        rnd = random.Random(0x7E00 + seed + bits)
        return [rnd.getrandbits(bits + 7 if i % 5 == 4 else bits) for i in range(LANES)]
    wide = lambda seed: values(seed, 10 * RANGE_WORDS)
    short = lambda seed: values(seed, SHORT_BITS)
    canonical = lambda vs: limbs(vs, FP, montgomery=False)
    L = _lib

    def range_wanted(seed):
        vs = wide(seed)
        return (_b(limbs([v >> (10 * j) for v in vs for j in range(RANGE_WORDS + 1)], FP)) + bytes(1 if v >> (10 * RANGE_WORDS) else 0 for v in vs))

    def short_wanted(seed):
        vs, shift, inv = short(seed), 1 << (10 - SHORT_BITS), pow(1 << SHORT_BITS, -1, P)
        return _b(limbs([x for v in vs for x in (v, v * shift % P, inv)], FP)) + bytes(1 if v >> SHORT_BITS else 0 for v in vs)
    return {
        "h2_range_check_trace_device": Case(
            "range-check-trace", "h2_range_check_trace_device", (LANES, RANGE_WORDS), lambda seed: {"values": canonical(wide(seed))},
            lambda: {"rows": LANES * (RANGE_WORDS + 1) * 32, "status": LANES},
            lambda i, u, sp: ok(L().h2_range_check_trace_device(FP, i["values"].data_ptr(), LANES, RANGE_WORDS, u["rows"].data_ptr(), u["status"].data_ptr(), _st(sp))),
            range_wanted, fields_valid(FP, "values", montgomery=False)),
        "h2_short_range_check_trace_device": Case(
            "short-range-check-trace", "h2_short_range_check_trace_device", (LANES, SHORT_BITS), lambda seed: {"values": canonical(short(seed))},
            lambda: {"rows": LANES * 3 * 32, "status": LANES},
            lambda i, u, sp: ok(L().h2_short_range_check_trace_device(FP, i["values"].data_ptr(), LANES, SHORT_BITS, u["rows"].data_ptr(), u["status"].data_ptr(), _st(sp))),
            short_wanted, fields_valid(FP, "values", montgomery=False)),
    }


# ---- the table -----------------------------------------------------------------------------------------------------------------------------
def _build():
    cases = {
        "h2_msm_device": tuple(_msm_case(n) for n in MSM_SIZES),
        "h2_msm_batch_device": _msm_batch_case(),
        "h2_commit_device": _commit_case(),
        "h2_commit_range_device": _commit_range_case(),
        "h2_commit_pair_device": _commit_pair_case(),
        "h2_commit_batch_device": (_commit_batch_case("commit-batch-alternating", *ALTERNATING, cp.BATCH_COLUMNS, 2),
                                   _commit_batch_case("commit-batch-spread", *SPREAD, cp.BATCH_FORK, SPREAD[1])),
        "h2_points_sum_device": _points_sum_case(),
        "h2_ntt_device": _ntt_case("ntt", "h2_ntt_device", 0),
        "h2_ifft_device": _ntt_case("ifft", "h2_ifft_device", 1),
        "h2_ntt_batch_device": _ntt_batch_case("ntt-batch", "h2_ntt_batch_device", 0),
        "h2_ifft_batch_device": _ntt_batch_case("ifft-batch", "h2_ifft_batch_device", 1),
        "h2_coeff_to_extended_device": _coeff_to_extended_case(),
        "h2_extended_to_coeff_device": _extended_to_coeff_case(),
        "h2_divide_by_vanishing_poly_device": _divide_by_vanishing_case(),
        "h2_lagrange_basis_device": _lagrange_basis_case(),
        "h2_generator_collapse_device": _generator_collapse_case(),
        "h2_fold_scalars_device": _fold_scalars_case(),
        "h2_ipa_round_scalars_device": _round_scalars_case(),
        "h2_ipa_s_combine_device": _s_combine_case(),
        "h2_ipa_collapsed_generators_device": _collapsed_generators_case(),
        "h2_ipa_rounds_device": _ipa_rounds_case(),
        "h2_open_device": _open_case("open-device", "h2_open_device", True),
        "h2_open_device_host_s": _open_case("open-device-host-s", "h2_open_device_host_s", False),
        "h2_selector_conflicts_device": _selector_conflicts_case(),
        "h2_selector_combine_device": _selector_combine_case(),
        "h2_evaluate_device": _evaluate_case(),
        "h2_check_expressions_device": _check_expressions_case(),
        "h2_sort_device": _sort_case(),
        "h2_permute_expression_pair_device": _permute_case(),
        "h2_lookup_check_device": _lookup_check_case(),
        "h2_permutation_check_device": _permutation_check_case(),
        "h2_points_compress_device": _compress_case(),
        "h2_points_decompress_device": _decompress_case(),
        "h2_hash_to_curve_device": _hash_to_curve_case(),
        "h2_msm_last_path": Excluded("host bookkeeping, enqueues nothing"),
        "h2_commit_last_plan": Excluded("host bookkeeping, enqueues nothing"),
        "h2_msm_split_rccl_device": Excluded("needs an RCCL world of several processes"),
        "h2_commit_split_rccl_device": Excluded("needs an RCCL world of several processes"),
    }
    for family in (_poly_cases(), _poseidon_cases(), _sinsemilla_cases(), _ecc_cases(), _range_check_cases()):
        assert not set(family) & set(cases)
        cases.update(family)
    return cases


CASES = _build()


def cases_of(entry):
    value = CASES[entry]
    return () if isinstance(value, Excluded) else value if isinstance(value, tuple) else (value,)


ALL_CASES = [case for entry in sorted(CASES) for case in cases_of(entry)]
BY_NAME = {case.name: case for case in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)
MODE_C = [case for case in ALL_CASES if case.mode_c]
