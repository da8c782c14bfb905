"""Shared by test_field_edge_case_coverage.py, test_field_inv_host.py, test_gpu_field_edges.py and the two CPU model tests of the generated
multipliers: crafted operands for the field layer (csrc/field.cuh, field9.cuh, field_inv.cuh) and what plain big integers say each device
function must return.  Uniformly random 256-bit operands reach a zero low word, a sum equal to p or a borrow through eight limbs with
probability 2^-32 or less per lane; the lists here are built to stand on those places.  Pure Python, deterministic, both fields.

A case is a tuple of operands: an integer for an 8 x 32 word (`f`), a list of nine signed integers for a 9 x 29 limb vector (`n`).  MODES
gives the operand and result kinds of every mode of tests/native/field_edge_driver.hip; `runs(mode, field)` the lists, in two lane orders;
`judge(mode, field, case, out)` the verdict on one result.  Every operation is tested inside the operand contract its header states, and
the header line is quoted next to each family; what a header does not allow is not a case (see NOT_CASES)."""
import functools
import random

FIELDS = (0, 1)                                  # FP, FQ of field.cuh
FIELD_ARG = {0: "fp", 1: "fq"}
P = {0: 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001,
     1: 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001}
R = 1 << 256                                     # the Montgomery radix of the 8 x 32 layer
R9 = 1 << 261                                    # ... of the 9 x 29 layer
M29, M32 = (1 << 29) - 1, (1 << 32) - 1
LAZY_D = 1 << 130                                # lazy values lie in [0, 2p + d): the d test_field_mul_asm_model.py holds the multiplier to
WAVE = 64

# mode -> (operand kinds, result kinds): f = 8 x u32, n = 9 x i32, w = one u32
MODES = {
    "mul": ("ff", "f"), "sqr": ("f", "f"), "mul_c": ("ff", "f"), "to_mont": ("f", "f"), "from_mont": ("f", "f"), "redc": ("f", "f"),
    "add": ("ff", "f"), "sub": ("ff", "f"), "neg": ("f", "f"), "dbl": ("f", "f"), "reduce_once": ("f", "f"),
    "mul_lazy": ("ff", "f"), "add_lazy": ("ff", "f"), "sub_lazy": ("ff", "f"), "reduce_lazy": ("f", "f"), "is_zero_lazy": ("f", "w"),
    "inv": ("f", "f"), "modinv30": ("f", "f"),
    "unpack9": ("f", "n"), "pack9": ("n", "f"), "from_r256": ("f", "n"), "to_r256": ("n", "f"), "mul9": ("nn", "n"), "sqr9": ("n", "n"),
    "mul9_c": ("nn", "n"), "dot2": ("nnnn", "n"), "sqr_minus": ("nn", "n"), "norm9": ("n", "n"), "quadruple_norm9": ("n", "n"),
    "canonical9": ("n", "f"), "canonical_small9": ("n", "f"), "maybe_zero9": ("n", "w"), "is_zero9": ("n", "w"),
}
KIND_WORDS = {"f": 8, "n": 9, "w": 1}

# What the issue's wish list names but a header rules out, and why it is not in any list:
NOT_CASES = {
    "modinv30(p)": "field_inv.cuh: `x < p`",
    "mul / add / sub of operands >= p": "field.cuh: fe_add's `a + b < 2p`, fe_mul_sched's one conditional subtraction: canonical operands",
    "a + 2p with a >= 2^128 as a lazy value": "field.cuh: lazy values lie in [0, 2p + d), d ~ 2^130; field_check.hip keeps to a < 2^128 too",
    "fe9_norm with EVERY limb at +-(2^31 - 1)": "field9.cuh: the carry pass adds the carry to the next limb in int32: a limb at 2^31 - 1 that "
                                                  "receives a carry of 3 overflows.  The lists put limb 0 at +-(2^31 - 1) and every later limb "
                                                  "where limb + carry is the int32 extreme",
    "fe9_quadruple_norm with limbs beyond 2^29": "field9.cuh: `for a PRODUCT a (limbs 0..7 in [0, 2^29] ...)`",
    "fe9_is_zero_mod_p(+-16 p)": "field9.cuh: `|value| < 2^258`; 16 p is above it",
}


# ---- representations -------------------------------------------------------------------------------------------------------------
def words8(x):
    assert 0 <= x < R
    return [(x >> (32 * i)) & M32 for i in range(8)]


def limbs9(x):
    """the normalised 9 x 29 limbs of any integer: limbs 0..7 its base-2^29 digits, limb 8 the signed rest"""
    return [(x >> (29 * i)) & M29 for i in range(8)] + [x >> 232]


def value9(limbs):
    return sum(x << (29 * i) for i, x in enumerate(limbs))


_value = value9                                  # the name the CPU model tests use


# ---- the palette -----------------------------------------------------------------------------------------------------------------
def fixed_values(field):
    p = P[field]
    base = [0, 1, 2, 3, p - 1, p - 2, p - 3, (p - 1) // 2, (p + 1) // 2, R % p, R * R % p, R9 % p]
    out = []
    for v in base + [(p - v) % p for v in base]:
        if v not in out:
            out.append(v)
    return out


def power_values(field, ks):
    """2^k, 2^k - 1, 2^k + 1 and p - 2^k; k <= 254, and 2^254 + 1 < p in both fields"""
    p = P[field]
    out = []
    for k in ks:
        for v in ((1 << k), (1 << k) - 1, (1 << k) + 1, p - (1 << k)):
            assert 0 <= v < p
            out.append(v)
    return out


SEAM_KS = sorted({k + d for step in (29, 30, 32) for k in range(0, 255, step) for d in (-1, 0, 1) if 0 <= k + d <= 254})
SEAM_MULTIPLES = sorted({k for step in (29, 30, 32) for k in range(0, 255, step)})


def limb_values(field):
    """a one and all ones in each of the eight 32-bit and nine 29-bit limb positions, cut to what stays below p (the top limbs hold
    30 resp. 22 bits of a value below 2^254), and every bit below 254 set"""
    out = []
    for i in range(8):
        out += [1 << (32 * i), (M32 if i < 7 else (1 << 30) - 1) << (32 * i)]
    for i in range(9):
        out += [1 << (29 * i), (M29 if i < 8 else (1 << 22) - 1) << (29 * i)]
    out.append((1 << 254) - 1)
    assert all(v < P[field] for v in out)
    return out


def random_values(field, n=64, tag="palette"):
    rng = random.Random(f"field-edges {tag} {field}")
    return [rng.randrange(P[field]) for _ in range(n)]


def _unique(values):
    seen, out = set(), []
    for v in values:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


@functools.lru_cache(maxsize=None)
def inversion_values(field):
    """the whole palette: every k in 0 .. 254 (about 1 100 values): the list of `inv`, `modinv30` and the host program"""
    return _unique(fixed_values(field) + power_values(field, range(255)) + limb_values(field) + random_values(field))


@functools.lru_cache(maxsize=None)
def pair_palette(field):
    """about 120 values for the cross products: the fixed ones, 2^k for k on and next to a multiple of 29, 30 or 32, 2^k - 1 and
    p - 2^k on the multiples themselves, every bit below 254 set, and 16 random values"""
    p = P[field]
    vals = fixed_values(field) + [1 << k for k in SEAM_KS] + [(1 << k) - 1 for k in SEAM_MULTIPLES]
    vals += [p - (1 << k) for k in SEAM_MULTIPLES[1::3]] + [(1 << 254) - 1] + random_values(field, 16, "pairs")
    return _unique(vals)


@functools.lru_cache(maxsize=None)
def unary_values(field):
    """one-operand modes on canonical values: the palette with the seam powers in all four shapes"""
    return _unique(fixed_values(field) + power_values(field, SEAM_KS) + limb_values(field) + random_values(field))


# ---- the 8 x 32 layer: expectations ----------------------------------------------------------------------------------------------
def mont_mul(a, b, field):
    return a * b * pow(R, -1, P[field]) % P[field]


def redc_value(a, field):
    """field.cuh: `(a + (R - 1) p) / R < p + 1`, REDC of a 256-bit number, made canonical"""
    return a * pow(R, -1, P[field]) % P[field]


def mont_inv(a, field):
    """field.cuh fe_inv: `1 / a (Montgomery in, Montgomery out; 0 for 0)`: a = x R -> x^-1 R = a^-1 R^2"""
    p = P[field]
    return pow(a, -1, p) * R * R % p if a % p else 0


def plain_inv(x, field):
    """field_inv.cuh: `out = x^-1 mod p as integers (0 for x = 0), x < p`"""
    return pow(x, -1, P[field]) if x else 0


def sub_lazy_exact(a, b, field):
    """field.cuh fe_sub_lazy: `a - b + 2p when the difference is negative`, the subtrahend made smaller first while its bit 255 is set"""
    p = P[field]
    while b >> 255:
        b = b - p if b >= p else b
    d = a - b
    return d + 2 * p if d < 0 else d


def add_lazy_exact(a, b, field):
    """field.cuh fe_add_lazy: `the carry out of the top limb counts as ">= 2p"`"""
    s = a + b
    return s - 2 * P[field] if s >= 2 * P[field] else s


# ---- the 8 x 32 layer: lists -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def canonical_pairs(field):
    """crafted pairs of canonical values, for mul / mul_c / add / sub: a + b in {p - 1, p, p + 1, 2p - 2}, a - b in {0, +-1}, differences
    whose borrow (and sums whose carry) runs through all eight limbs, a carry or borrow across exactly one limb boundary, and the REDC
    operands times one (rows of fe_mul_c whose running low word is zero)"""
    p, rng = P[field], random.Random(f"field-edges pairs {field}")
    out = []
    for a in [1, 2, (p - 1) // 2, (p + 1) // 2, p - 2, p - 1] + [rng.randrange(1, p) for _ in range(6)]:
        out += [(a, p - 1 - a), (a, p - a), (a, (p + 1 - a) % p or 1)]
        out += [(a, a), (a, a - 1), (a - 1, a)]
    out += [(p - 1, p - 1), (0, 0), (0, 1), (1, 0), (0, p - 1), (p - 1, 0)]
    # a borrow through all eight limbs: 2^224 k - 1 subtracted from ... 0, and 0 - 1; a carry through all: all ones below 254 plus one
    out += [(1 << 224, 1), (0, 1), ((1 << 253), (1 << 253) - 1 + 2), ((1 << 254) - 1, 1), (1, (1 << 254) - 1), ((1 << 254) - 1, (1 << 254) - 1)]
    for i in range(1, 8):                            # one boundary each: word i - 1 into word i
        lo = M32 << (32 * (i - 1))
        out += [(lo, 1 << (32 * (i - 1))), (1 << (32 * i), 1 << (32 * (i - 1))), (lo, lo if i < 7 else 1)]
    for a in redc_values(field):
        if a < p:
            out += [(a, 1), (1, a)]
    assert all(0 <= a < p and 0 <= b < p for a, b in out)
    return _unique(out)


def _redc_backwards(t, steps, p):
    """the word a with REDC's running value equal to t after `steps` reduction steps: each step is t' = (t + m p) / 2^32 with m = -t_0,
    so t = t' 2^32 - m p for the one m that keeps t inside [0, p); None when some m would be zero or t' is no reachable running value"""
    for _ in range(steps):
        m = (t << 32) // p
        if not 0 < m <= M32:
            return None
        t = (t << 32) - m * p
        assert 0 <= t < p and t & M32 == (-m) & M32
    return t


@functools.lru_cache(maxsize=None)
def redc_values(field):
    """256-bit words for `redc` and `from_mont` (field.cuh: `REDC of a 256-bit number`): for each step s in 0 .. 7 four words whose running
    low word is zero at step s and at no earlier step (they are below p, so `mul_c` takes them too); 0; low word 1 (the largest quotient digit
    2^32 - 1) in every step position; p, 2p, 3p (the value before the last subtraction is exactly p), the word that reduces to p - 1,
    p +- 1, 2^256 - 1 and its neighbours, and random words above p"""
    p, rng = P[field], random.Random(f"field-edges redc {field}")
    out = [0]
    for s in range(8):
        found = 0
        while found < 4:
            a = _redc_backwards(rng.randrange(1, p >> 32) << 32, s, p)                                     # low word zero at step s
            if a is not None:
                out.append(a)
                found += 1
        t1 = _redc_backwards((rng.randrange(1, p >> 32) << 32) | 1, s, p)                       # low word one at step s
        if t1 is not None:
            out.append(t1)
    out += [1, p - 1, p, p + 1, 2 * p - 1, 2 * p, 2 * p + 1, 3 * p, 3 * p + 1, R - 1, R - 2, R - (1 << 32), p - R % p, 2 * p - R % p,
            (R % p), (1 << 255), (1 << 255) - 1, M32, M32 << 224]
    out += [rng.randrange(p, R) for _ in range(32)] + [rng.randrange(R) for _ in range(32)]
    assert all(0 <= a < R for a in out)
    return _unique(out)


@functools.lru_cache(maxsize=None)
def reduce_once_values(field):
    """field.cuh: `r = a - p if a >= p else a          (a < 2p)`"""
    p = P[field]
    out = [0, 1, p - 2, p - 1, p, p + 1, 2 * p - 2, 2 * p - 1, (1 << 254), (1 << 254) - 1, (1 << 255) - 1, 1 << 255]
    out += [p + v for v in unary_values(field)[:80]] + unary_values(field)[:80]
    # p + 2^(32 i): the subtraction's borrow stops at every limb; p - 1 + 2^(32 i) ...
    out += [p + (1 << (32 * i)) - 1 for i in range(8)] + [p - (1 << (32 * i)) for i in range(8)]
    assert all(0 <= a < 2 * p for a in out)
    return _unique(out)


def lazy_representatives(a, field):
    """a, a + p, and a + 2p only where a < 2^128: every one a legal lazy value, below 2p + d"""
    p = P[field]
    return [a, a + p] + ([a + 2 * p] if a < 1 << 128 else [])


@functools.lru_cache(maxsize=None)
def lazy_values(field):
    p = P[field]
    small = [0, 1, 2, (1 << 127), (1 << 128) - 1, (1 << 64) + 1]
    big = [p - 1, p - 2, (p - 1) // 2, (1 << 254) - 1, (1 << 254), R % p, (1 << 255) - p, (1 << 255) - p - 1, (1 << 255) - p + 1]
    out = [r for a in small + big + random_values(field, 8, "lazy") for r in lazy_representatives(a, field)]
    assert all(0 <= v < 2 * p + LAZY_D for v in out)
    return _unique(out)


@functools.lru_cache(maxsize=None)
def lazy_pairs(field):
    """for mul_lazy, add_lazy and sub_lazy: every pair of lazy_values, then sums equal to 2p - 1, 2p and 2p + 1, sums past 2^256 (the
    carry out of limb 7), subtrahends with bit 255 set (fe_sub_lazy's loop) next to ones just below 2^255, and differences equal to
    0, p and 2p with their neighbours"""
    p = P[field]
    vals = lazy_values(field)
    out = [(a, b) for a in vals for b in vals]
    out += [(p, p - 1), (p - 1, p), (p, p), (2 * p, 0), (0, 2 * p), (2 * p - 1, 0), (p + 5, p - 6), (p + 5, p - 5), (p + 5, p - 4), (2 * p, 1)]
    out += [(2 * p, 2 * p), (2 * p + 1, 2 * p - 1), (2 * p - 1, 2 * p - 1), (R - 2 * p, 2 * p), (R - 2 * p - 1, 2 * p), (2 * p + LAZY_D - 1, 2 * p + LAZY_D - 1)]
    out += [(a, b) for a in (0, 1, p, 2 * p - 1, 2 * p) for b in ((1 << 255) - 1, 1 << 255, (1 << 255) + 1, 2 * p - 1, 2 * p, 2 * p + 1, 2 * p + LAZY_D - 1)]
    for a in (0, 1, 5, (1 << 127)):
        out += [(a, a), (a + p, a), (a + 2 * p, a), (a, a + p), (a, a + 2 * p), (a + p, a + 2 * p), (a + 1, a), (a, a + 1), (a + p + 1, a), (a + p, a + 1),
                (a + 2 * p + 1, a), (a + 2 * p, a + 1)]
    assert all(0 <= a < 2 * p + LAZY_D and 0 <= b < 2 * p + LAZY_D for a, b in out)
    return _unique(out)


@functools.lru_cache(maxsize=None)
def is_zero_lazy_values(field):
    """field.cuh: `lazy value = 0 mod p ?`: 0, p and 2p against +-1 of each, every lazy value, and what fe_sub_lazy leaves of the pairs
    whose difference is 0, p or 2p or next to one"""
    p = P[field]
    out = [0, 1, p - 1, p, p + 1, 2 * p - 1, 2 * p, 2 * p + 1, 2 * p + LAZY_D - 1, p - (1 << 254), p + (1 << 200), 2 * p - (1 << 32), p + (1 << 224)]
    out += lazy_values(field) + [sub_lazy_exact(a, b, field) for a, b in lazy_pairs(field)[-48:]]
    return _unique(v for v in out if 0 <= v < 2 * p + LAZY_D)


@functools.lru_cache(maxsize=None)
def reduce_lazy_values(field):
    """field.cuh: `canonical representative of a lazy value (< 3p)`"""
    p = P[field]
    out = [0, p - 1, p, p + 1, 2 * p - 1, 2 * p, 2 * p + 1, 3 * p - 1] + lazy_values(field) + [v + 2 * p for v in unary_values(field)[:40] if v < p]
    assert all(0 <= v < 3 * p for v in out)
    return _unique(out)


# ---- the 9 x 29 layer: the operand generators of the CPU model tests -----------------------------------------------------------------
def _limbs_of(value, rng, spread):
    """A signed 9-limb representation of `value` (limbs 0..7 within +-2^spread around their canonical digits)."""
    out, carry = [], 0
    for i in range(8):
        digit = ((value >> (29 * i)) & M29) + carry
        wobble = rng.randrange(-(1 << spread) // (1 << 29), (1 << spread) // (1 << 29) + 1) if spread > 29 else 0
        out.append(digit - (wobble << 29))
        carry = wobble
    out.append((value >> 232) + carry)
    assert _value(out) == value
    return out


def _operand(rng, p, kind):
    if kind == "normalised":                   # what a product leaves: value in (-2^255, 2^255 + p), limbs 0..7 in [0, 2^29)
        return _limbs_of(rng.randrange(-(1 << 255), (1 << 255) + p), rng, 29)
    if kind == "difference":                   # normalised - normalised: limbs in (-2^29, 2^29), |value| < 2^257
        a, b = _operand(rng, p, "normalised"), _operand(rng, p, "normalised")
        return [x - y for x, y in zip(a, b)]
    if kind == "wide":                         # limbs up to 2^30 in magnitude, |value| < 2^258
        return _limbs_of(rng.randrange(-(1 << 258) + 1, 1 << 258), rng, 30)
    raise ValueError(kind)


def point_formula_trials(field):
    """The 60 trials of test_field9_asm_model.test_generated_multipliers_against_big_integers, in its order of draws: signed and
    un-normalised operands at the bounds the point formulas use (curve9.cuh), trial 7 with the limb value 2^29 only a product's limb 0
    takes.  Per trial: mul (a, b); sqr d; dot2 (d, c, f, e) -- difference x difference + (-normalised) x normalised; sqr_minus (d, s) with
    the subtrahend's limbs up to 3 * 2^29."""
    p = P[field]
    rng = random.Random(0x9E37 + field)
    trials = []
    for trial in range(60):
        kinds = ("normalised", "difference", "wide") if trial % 3 else ("normalised", "normalised", "normalised")
        a, b = _operand(rng, p, kinds[trial % 2]), _operand(rng, p, "normalised")
        if trial == 7:
            a[0] = 1 << 29                      # the limb value only a product's limb 0 takes
        d = _operand(rng, p, "difference")
        c, e = _operand(rng, p, "difference"), _operand(rng, p, "normalised")
        f = [-x for x in _operand(rng, p, "normalised")]
        s = [x + 2 * y for x, y in zip(_operand(rng, p, "normalised"), _operand(rng, p, "normalised"))]
        trials.append({"a": a, "b": b, "d": d, "c": c, "e": e, "f": f, "s": s})
    return trials


DOT2_EXTREME = [(1 << 29)] * 8 + [1 << 24]       # every limb of every operand at +-2^29: the column bound of fe9_dot2


def twiddle_limbs(v):
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def ntt_regime_trials(field):
    """The 80 trials of test_field9_asm_model.test_ntt_operand_regime_of_the_multiplier: RAW limbs in (-2^30, 3 x 2^29), limb 8 within
    +-2^29, times a normalised twiddle in [0, p); the first three at the corners of the limb range.  [(a, w)]"""
    p = P[field]
    rng = random.Random(0x4E5454 + field)
    lo, hi = -(1 << 30) + 1, 3 * (1 << 29) - 1
    trials = []
    for trial in range(80):
        a = [rng.randrange(lo, hi + 1) for _ in range(8)] + [rng.randrange(-(1 << 29), (1 << 29) + 1)]
        if trial == 0:
            a = [hi] * 8 + [1 << 29]                   # every limb at the top of the RAW range
        elif trial == 1:
            a = [lo] * 8 + [-(1 << 29)]                # ... at the bottom
        elif trial == 2:
            a = [hi if i % 2 else lo for i in range(8)] + [1 << 29]
        w = p - 1 - trial if trial < 4 else rng.randrange(0, p)
        trials.append((a, w))
    return trials


def mul_model_edges(field):
    """the edge operands of test_field_mul_asm_model.py (the generated 8 x 32 multiplier on the CPU interpreter)"""
    p = P[field]
    return [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (1 << 254), (1 << 254) - 1, (1 << 255) - 1 if (1 << 255) - 1 < p else p - 3]


def mul_model_pairs(field):
    """(canonical pairs, lazy pairs) of test_field_mul_asm_model.py, in its order of draws"""
    p = P[field]
    rng = random.Random(0x8832 + field)
    edge = mul_model_edges(field)
    pairs = [(x, y) for x in edge for y in edge] + [(rng.randrange(p), rng.randrange(p)) for _ in range(300)]
    d = LAZY_D
    lazy = [(rng.randrange(2 * p + d), rng.randrange(2 * p + d)) for _ in range(300)]
    return pairs, lazy


# ---- the 9 x 29 layer: lists -----------------------------------------------------------------------------------------------------
PRODUCT_BOUND = lambda p: (1 << 255) + p + 1     # field9.cuh: `the product is normalised and lies in (-2^255, 2^255 + p)`


@functools.lru_cache(maxsize=None)
def mul9_cases(field):
    """[(a, b, |value| bound)]: the point-formula operands (field9.cuh: `limbs of both operands ... 9 |a_i| |b_j| + 2^61 < 2^63`, `|value| <
    2^258`) and the NTT regime (ntt_pass.cuh's raw limbs by a normalised twiddle, a few p more)"""
    p = P[field]
    out = [(t["a"], t["b"], PRODUCT_BOUND(p)) for t in point_formula_trials(field)]
    out += [(a, twiddle_limbs(w), (1 << 255) + 4 * p) for a, w in ntt_regime_trials(field)]
    for v in (0, 1, p - 1, p, R9 % p, (1 << 255) + p - 1, -(1 << 255) + 1):
        for w in (0, 1, p - 1, R9 % p, R9 * R9 % p):
            out.append((limbs9(v), limbs9(w), PRODUCT_BOUND(p)))
    prod_like = [1 << 29] + [M29] * 7 + [(1 << 23) - 1]          # what a product may leave: limb 0 equal to 2^29
    out += [(prod_like, prod_like, PRODUCT_BOUND(p)), (prod_like, [-x for x in prod_like], PRODUCT_BOUND(p))]
    return out


@functools.lru_cache(maxsize=None)
def sqr9_cases(field):
    p = P[field]
    out = [(t["d"], PRODUCT_BOUND(p)) for t in point_formula_trials(field)]
    out += [(limbs9(v), PRODUCT_BOUND(p)) for v in (0, 1, -1, p - 1, p, R9 % p, (1 << 255) + p - 1, -(1 << 255) + 1)]
    out += [([1 << 29] + [M29] * 7 + [(1 << 23) - 1], PRODUCT_BOUND(p)), ([-(1 << 29) + 1] * 8 + [-(1 << 24)], PRODUCT_BOUND(p))]
    return out


@functools.lru_cache(maxsize=None)
def dot2_cases(field):
    """field9.cuh: `limbs of all four operands in [-2^29, 2^29], |a b + c d| < 2^516 for a normalised result`"""
    out = [(t["d"], t["c"], t["f"], t["e"], 1 << 256) for t in point_formula_trials(field)]
    neg = [-x for x in DOT2_EXTREME]
    out += [(DOT2_EXTREME, DOT2_EXTREME, neg, neg, 1 << 256), (DOT2_EXTREME, neg, DOT2_EXTREME, DOT2_EXTREME, 1 << 256),
            (limbs9(0), limbs9(0), limbs9(0), limbs9(0), 1 << 256), (limbs9(1), limbs9(1), limbs9(-1), limbs9(1), 1 << 256)]
    return out


@functools.lru_cache(maxsize=None)
def sqr_minus_cases(field):
    """field9.cuh: `a signed limb vector s (limbs below 2^31 in magnitude)`; the value is the square's minus s"""
    out = [(t["d"], t["s"], 1 << 258) for t in point_formula_trials(field)]
    out += [(limbs9(0), limbs9(0), 1 << 258), (limbs9(1), [3 * M29] * 8 + [3 << 22], 1 << 258), (limbs9(P[field] - 1), [-3 * M29] * 8 + [-(3 << 22)], 1 << 258)]
    return out


@functools.lru_cache(maxsize=None)
def unpack_values(field):
    """field9.cuh fe9_unpack: any 256-bit word.  2^(29 i) +- 1 and 2^(32 w) +- 1 (a one that straddles each seam), all ones, single
    fields of ones, alternating words"""
    out = [0, R - 1, P[field], P[field] - 1]
    for i in range(9):
        out += [(1 << (29 * i)) - 1, 1 << (29 * i), (1 << (29 * i)) + 1, (M29 << (29 * i)) & (R - 1), (R - 1) ^ ((M29 << (29 * i)) & (R - 1))]
    for w in range(8):
        out += [(1 << (32 * w)) - 1, 1 << (32 * w), (1 << (32 * w)) + 1, M32 << (32 * w), (R - 1) ^ (M32 << (32 * w))]
    out += [sum(M32 << (64 * i) for i in range(4)), sum(M32 << (64 * i + 32) for i in range(4)), sum(M29 << (58 * i) for i in range(5)) & (R - 1),
            sum(1 << (29 * i) for i in range(9)), sum(1 << (29 * i + 28) for i in range(9)) & (R - 1)]
    out += [v for v in random_values(field, 16, "unpack")] + [random.Random(f"field-edges unpack-wide {field} {i}").randrange(R) for i in range(16)]
    return _unique(v for v in out if 0 <= v < R)


@functools.lru_cache(maxsize=None)
def pack_cases(field):
    """field9.cuh fe9_pack: `normalised, non-negative, < 2^256`"""
    return [(limbs9(v),) for v in unpack_values(field)]


def layouts(value):
    """the five limb layouts of field_check.hip's filter section for one value: normalised, a 2^29 moved from limb 0 down, every low limb
    raised by 2^29, every second one lowered, and 2^30 on limb 0"""
    base = limbs9(value)
    out = [list(base) for _ in range(5)]
    out[1][0] -= 1 << 29
    out[1][1] += 1
    for i in range(8):
        out[2][i] += 1 << 29
        out[2][i + 1] -= 1
    for i in range(0, 8, 2):
        out[3][i] -= 1 << 29
        out[3][i + 1] += 1
    out[4][0] += 1 << 30
    out[4][1] -= 2
    assert all(value9(v) == value for v in out)
    return out


@functools.lru_cache(maxsize=None)
def canonical9_cases(field):
    """field9.cuh fe9_canonical: `any valid operand (|value| < 2^258)`: k p + d for |k| <= 15, d in {0, +-1}, five layouts each (k + 16 in
    1 .. 31 spells which of the five subtractions are taken; d = 0 stands exactly on a boundary, d = -1 one below), and the model tests'
    operands"""
    p = P[field]
    out = [(v,) for k in range(-15, 16) for d in (0, 1, -1) for v in layouts(k * p + d)]
    out += [(t[k],) for t in point_formula_trials(field)[:20] for k in ("a", "b", "d")]
    out += [(limbs9(v),) for v in ((1 << 258) - 1, -(1 << 258) + 1, R9 % p, 1 << 255, -(1 << 255))]
    return out


@functools.lru_cache(maxsize=None)
def canonical_small9_cases(field):
    """field9.cuh fe9_canonical_small: `a value known to lie in (-p, 2p)`: both ends, 0 and p with their neighbours, each normalised and
    in the four un-normalised layouts"""
    p = P[field]
    vals = [-p + 1, -p + 2, -1, 0, 1, 2, p - 2, p - 1, p, p + 1, 2 * p - 2, 2 * p - 1, (p - 1) // 2, -(p - 1) // 2, R % p, (1 << 254), -(1 << 254)]
    out = [(v,) for x in vals for v in layouts(x)]
    rng = random.Random(f"field-edges small9 {field}")
    out += [(limbs9(rng.randrange(-p + 1, 2 * p)),) for _ in range(32)]
    return out


@functools.lru_cache(maxsize=None)
def norm9_cases(field):
    """field9.cuh fe9_norm: `limbs 0..7 into [0, 2^29), limb 8 keeps the sign`, for limbs whose sum with the incoming carry fits an int32:
    limb 0 at +-(2^31 - 1) and every later limb at the int32 extreme once its carry has come in, a carry and a borrow that ripple
    through all limbs, and the layouts above"""
    top, bot = (1 << 31) - 1, -(1 << 31)
    out = [([top] + [top - 3] * 8,), ([-top] + [bot + 4] * 8,), ([top] + [bot, top] * 4,), ([-top] + [top, bot] * 4,)]
    out += [([1 << 29] + [M29] * 7 + [0],), ([-1] + [0] * 8,), ([M29 + 1] + [M29] * 7 + [-1],), ([-1] + [0] * 7 + [1],), ([0] * 9,), ([M29] * 9,),
            ([1 << 29] * 9,), ([-(1 << 29)] * 9,), ([3 * M29] * 9,), ([-3 * M29] * 9,)]
    p = P[field]
    out += [(v,) for x in (0, 1, -1, p, -p, 15 * p + 1, -15 * p - 1) for v in layouts(x)]
    out += [(t[k],) for t in point_formula_trials(field)[:20] for k in ("a", "d", "s")]
    for case in out:
        c = 0
        for x in case[0]:                                # inside the contract: no int32 addition overflows
            assert -(1 << 31) <= x < (1 << 31) and -(1 << 31) <= x + c < (1 << 31), case
            c = (x + c) >> 29
    return out


@functools.lru_cache(maxsize=None)
def quadruple_norm9_cases(field):
    """field9.cuh fe9_quadruple_norm: `for a PRODUCT a (limbs 0..7 in [0, 2^29], limb 0 may equal 2^29 ...; limb 8 is small and signed)`"""
    p = P[field]
    out = [([1 << 29] + [M29] * 7 + [1 << 23],), ([1 << 29] * 8 + [-(1 << 23)],), ([M29] * 8 + [(1 << 23) + 5],), ([0] * 9,), ([1] + [0] * 8,),
           ([1 << 29] + [0] * 8,), ([1 << 27] * 8 + [0],), ([(1 << 27) - 1] * 8 + [-1],), ([M29] * 8 + [-(1 << 23)],), ([0] * 8 + [-1],)]
    out += [(limbs9(v),) for v in (1, p - 1, p, (1 << 255) + p - 1, -(1 << 255) + 1, R9 % p)]
    rng = random.Random(f"field-edges quad9 {field}")
    out += [(limbs9(rng.randrange(-(1 << 255) + 1, (1 << 255) + p)),) for _ in range(32)]
    return out


@functools.lru_cache(maxsize=None)
def zero9_cases(field):
    """field9.cuh: `value = 0 mod p ?  a: limbs below 2^31, |value| < 2^258`: k p + d for |k| <= 15 and the near misses of
    field_check.hip's filter section, five layouts each"""
    p = P[field]
    return [(v,) for k in range(-15, 16) for d in (0, 1, -1, 16, -16, 17, -17, 1 << 28) for v in layouts(k * p + d)]


@functools.lru_cache(maxsize=None)
def to_r256_cases(field):
    """field9.cuh fe9_to_r256: fe9_mul of a valid operand by the canonical constant 2^256 mod p, then fe9_canonical_small"""
    p = P[field]
    out = [(t[k],) for t in point_formula_trials(field) for k in ("a", "b", "d")]
    out += [(limbs9(v),) for v in (0, 1, -1, p - 1, p, p + 1, R9 % p, 32 % p, (1 << 258) - 1, -(1 << 258) + 1)]
    out += [([1 << 29] + [M29] * 7 + [(1 << 23) - 1],)]
    return out


# ---- lane orders -----------------------------------------------------------------------------------------------------------------
def _orders(crafted, bulk=()):
    """interleaved: the bulk list, then the crafted cases, different cases in neighbouring lanes; grouped: each crafted case in a whole
    wave of 64 lanes, which makes fe_sub_lazy's loop and fe9_canonical's selects wave-uniform"""
    crafted = list(crafted)
    return {"interleaved": list(bulk) + crafted, "grouped": [c for c in crafted for _ in range(WAVE)]}


@functools.lru_cache(maxsize=None)
def runs(mode, field):
    """{"interleaved": cases, "grouped": cases} of one driver mode"""
    one = lambda values: [(v,) for v in values]
    if mode in ("mul", "mul_c", "add", "sub"):
        pal = pair_palette(field)
        bulk = [(a, b) for a in pal for b in pal]
        crafted = canonical_pairs(field) + (mul_model_pairs(field)[0] if mode in ("mul", "mul_c") else [])
        return _orders(crafted, bulk)
    if mode in ("sqr", "to_mont", "neg", "dbl"):
        return _orders(one(unary_values(field)))
    if mode in ("from_mont", "redc"):
        return _orders(one(redc_values(field)))
    if mode == "reduce_once":
        return _orders(one(reduce_once_values(field)))
    if mode == "mul_lazy":
        return _orders(lazy_pairs(field)[-160:], lazy_pairs(field)[:-160] + mul_model_pairs(field)[1])
    if mode in ("add_lazy", "sub_lazy"):
        return _orders(lazy_pairs(field)[-160:], lazy_pairs(field)[:-160])
    if mode == "reduce_lazy":
        return _orders(one(reduce_lazy_values(field)))
    if mode == "is_zero_lazy":
        return _orders(one(is_zero_lazy_values(field)))
    if mode in ("inv", "modinv30"):
        values = inversion_values(field)
        return _orders(one(values[:40] + values[-8:]), one(values[40:-8]))
    if mode in ("unpack9", "from_r256"):
        return _orders(one(unpack_values(field)))
    table = {"pack9": pack_cases, "to_r256": to_r256_cases, "norm9": norm9_cases, "quadruple_norm9": quadruple_norm9_cases,
             "canonical9": canonical9_cases, "canonical_small9": canonical_small9_cases, "maybe_zero9": zero9_cases, "is_zero9": zero9_cases}
    if mode in table:
        return _orders(table[mode](field))
    if mode in ("mul9", "mul9_c"):
        return _orders([c[:2] for c in mul9_cases(field)])
    if mode == "sqr9":
        return _orders([c[:1] for c in sqr9_cases(field)])
    if mode == "dot2":
        return _orders([c[:4] for c in dot2_cases(field)])
    if mode == "sqr_minus":
        return _orders([c[:2] for c in sqr_minus_cases(field)])
    raise KeyError(mode)


def _key(case):
    return tuple(tuple(x) if isinstance(x, list) else x for x in case)


@functools.lru_cache(maxsize=None)
def value_bounds(mode, field):
    """{case: |value| bound} of the product modes"""
    src = {"mul9": mul9_cases, "mul9_c": mul9_cases, "sqr9": sqr9_cases, "dot2": dot2_cases, "sqr_minus": sqr_minus_cases}[mode](field)
    return {_key(c[:-1]): c[-1] for c in src}


# ---- verdicts --------------------------------------------------------------------------------------------------------------------
def _product_verdict(out, want_mod_p, p, bound, generated):
    """field9.cuh: limbs 0..7 in [0, 2^29] -- limbs 1..7 below 2^29, limb 0 in [1, 2^29] for the generated statements (the pending +1
    lands there) -- the value congruent and inside its bound"""
    if not all(0 <= x < (1 << 29) for x in out[1:8]):
        return "limbs 1..7 outside [0, 2^29)"
    if not ((1 if generated else 0) <= out[0] <= (1 << 29)):
        return "limb 0 outside its range"
    v = value9(out)
    if (v - want_mod_p) % p:
        return "value not congruent"
    if not abs(v) < bound:
        return "value outside its bound"
    return None


def judge(mode, field, case, out):
    """None when `out` (an integer, or a list of nine signed limbs) is what the header promises for `case`; else a short reason"""
    p = P[field]
    eq = lambda want: None if out == want else f"want {want:#x}" if isinstance(want, int) else f"want {want}"
    if mode in ("mul", "mul_c"):
        return eq(mont_mul(case[0], case[1], field))
    if mode == "sqr":
        return eq(mont_mul(case[0], case[0], field))
    if mode == "to_mont":
        return eq(case[0] * R % p)
    if mode in ("from_mont", "redc"):
        return eq(redc_value(case[0], field))
    if mode == "add":
        return eq((case[0] + case[1]) % p)
    if mode == "sub":
        return eq((case[0] - case[1]) % p)
    if mode == "neg":
        return eq(-case[0] % p)
    if mode == "dbl":
        return eq(2 * case[0] % p)
    if mode == "reduce_once":
        return eq(case[0] - p if case[0] >= p else case[0])
    if mode == "mul_lazy":                           # field.cuh: products stay in [0, 2p + d)
        if (out - case[0] * case[1] * pow(R, -1, p)) % p:
            return "not congruent"
        return None if 0 <= out < 2 * p + LAZY_D else "outside [0, 2p + d)"
    if mode == "add_lazy":
        return eq(add_lazy_exact(case[0], case[1], field))
    if mode == "sub_lazy":
        if (out - (case[0] - case[1])) % p:
            return "not congruent"
        return eq(sub_lazy_exact(case[0], case[1], field))
    if mode == "reduce_lazy":
        return eq(case[0] % p)
    if mode == "is_zero_lazy":
        return eq(int(case[0] % p == 0))
    if mode == "inv":
        return eq(mont_inv(case[0], field))
    if mode == "modinv30":
        return eq(plain_inv(case[0], field))
    if mode == "unpack9":
        return eq([(case[0] >> (29 * i)) & M29 for i in range(9)])
    if mode == "pack9":
        return eq(value9(case[0]))
    if mode == "from_r256":                          # unpack(x) times 2^266 over 2^261
        return _product_verdict(out, 32 * case[0], p, PRODUCT_BOUND(p), True)
    if mode == "to_r256":
        return eq(value9(case[0]) * R * pow(R9, -1, p) % p)
    rinv = pow(R9, -1, p)
    if mode in ("mul9", "mul9_c"):
        return _product_verdict(out, value9(case[0]) * value9(case[1]) * rinv, p, value_bounds(mode, field)[_key(case)], mode == "mul9")
    if mode == "sqr9":
        return _product_verdict(out, value9(case[0]) ** 2 * rinv, p, value_bounds(mode, field)[_key(case)], True)
    if mode == "dot2":
        want = (value9(case[0]) * value9(case[1]) + value9(case[2]) * value9(case[3])) * rinv
        return _product_verdict(out, want, p, value_bounds(mode, field)[_key(case)], True)
    if mode == "sqr_minus":
        return _product_verdict(out, value9(case[0]) ** 2 * rinv - value9(case[1]), p, value_bounds(mode, field)[_key(case)], True)
    if mode == "norm9":
        if not all(0 <= x < (1 << 29) for x in out[:8]):
            return "limbs 0..7 outside [0, 2^29)"
        return None if value9(out) == value9(case[0]) else "value changed"
    if mode == "quadruple_norm9":
        if not all(0 <= x < (1 << 29) for x in out[:8]):
            return "limbs 0..7 outside [0, 2^29)"
        return None if value9(out) == 4 * value9(case[0]) else "value is not 4 a"
    if mode in ("canonical9", "canonical_small9"):
        return eq(value9(case[0]) % p)
    if mode == "maybe_zero9":
        # field9.cuh: `unless the low limb is within +-16 of a multiple of 2^29 the answer is no`; a multiple k p, |k| <= 16, must pass
        near = ((case[0][0] + 16) % (1 << 29)) <= 32
        if value9(case[0]) % p == 0 and not near:
            return "the case list is wrong"
        return eq(int(near))
    if mode == "is_zero9":
        return eq(int(value9(case[0]) % p == 0))
    raise KeyError(mode)


# ---- files -----------------------------------------------------------------------------------------------------------------------
def encode(mode, cases):
    """the driver's input file: per lane the operands' words, little-endian u32 / two's-complement i32"""
    buf = bytearray()
    for case in cases:
        assert len(case) == len(MODES[mode][0])
        for kind, x in zip(MODES[mode][0], case):
            if kind == "f":
                buf += int(x).to_bytes(32, "little")
            else:
                for limb in x:
                    buf += int(limb).to_bytes(4, "little", signed=True)
    return bytes(buf)


def decode(mode, raw, n):
    """the driver's output file -> one result per lane: an integer (f, w) or nine signed limbs (n)"""
    kind = MODES[mode][1]
    size = 4 * KIND_WORDS[kind]
    assert len(raw) == size * n, (mode, len(raw), n)
    if kind == "n":
        return [[int.from_bytes(raw[size * i + 4 * j:size * i + 4 * j + 4], "little", signed=True) for j in range(9)] for i in range(n)]
    return [int.from_bytes(raw[size * i:size * i + size], "little") for i in range(n)]
