"""The structured case list for the O(n) kernels under every proof -- the scans and reductions of halo2_amd/csrc/poly.hip and the bitonic
sort / permute_expression_pair of halo2_amd/csrc/lookup.hip -- with a host replica of their launch geometry.  Pure Python and numpy:
tests/test_scan_sort_case_coverage.py proves on the CPU that the list reaches every path of the replica and holds the replica's
constants to the sources; tests/test_gpu_scan_sort_cases.py runs the list on the device against the oracle, bit for bit."""
from __future__ import annotations

import random

import numpy as np

FP, FQ = 0, 1
P = 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001
Q = 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001
MODULUS = {FP: P, FQ: Q}
CANONICAL, MONTGOMERY = 0, 1

# ---- geometry: constants mirrored from the sources (held to them by the coverage test) -------------------------------------------------
K_PT = 256                   # poly_plan.h kPT: lanes per workgroup
K_PC = 8                     # poly_plan.h kPC: consecutive elements per lane
K_TILE = K_PT * K_PC         # poly_plan.h kTile
K_INV_GROUP = 8              # poly_plan.h kInvGroup: lanes per Fermat inversion
REDUCE_CAP = 1024            # poly_plan.h kReduceCap: most workgroups of a reduction
EVAL_CAP = 256               # poly_plan.h kEvalCap: most workgroups of the Horner evaluation
LK_TILE_LOG = 11             # lookup.hip kTileLog: keys per sort tile = 2^11
LK_SCAN_BLOCK = 1024         # lookup.hip kScanBlock
KEY_LIMBS = 8                # lookup_keys.cuh key256: u32 limbs, compared from limb 7 down


def ceil_log2(n: int) -> int:
    l = 0
    while (1 << l) < n:
        l += 1
    return l


def sort_schedule(n: int):
    """The launches of lookup.hip's sort_padded for n keys (padded to 2^ceil_log2(n)): ("tile", log_n, tail_kl), ("global2", kl, jl),
    ("global", kl, jl), in order."""
    log_n = ceil_log2(max(n, 1))
    out = [("tile", log_n, 0)]
    for kl in range(LK_TILE_LOG + 1, log_n + 1):
        jl = kl - 1
        while jl - 1 >= LK_TILE_LOG:
            out.append(("global2", kl, jl))
            jl -= 2
        if jl >= LK_TILE_LOG:
            out.append(("global", kl, jl))
        out.append(("tile", log_n, kl))
    return out


def permute_geometry(n: int):
    """(nb, chunks): workgroups of lk_scan_blocks and trips of lk_scan_totals' chunk loop."""
    nb = (n + LK_SCAN_BLOCK - 1) // LK_SCAN_BLOCK
    return nb, (nb + LK_SCAN_BLOCK - 1) // LK_SCAN_BLOCK


def scan_geometry(n: int):
    """(nblk, per, entries, phantom) of poly_kate_carry / poly_product_carry for an n-element scan: tiles, tiles per lane, real tiles in the
    last non-empty lane and the steps that lane walks past the last tile."""
    nblk = (n + K_TILE - 1) // K_TILE
    per = (nblk + K_PT - 1) // K_PT
    lane = (nblk - 1) // per
    entries = nblk - lane * per
    return nblk, per, entries, per - entries


def _trips(n: int, blocks: int):
    T = blocks * K_PT
    most = (n - 1) // T + 1
    least = n // T if n >= T else 1            # lanes t >= n do nothing at all
    return most, least


def reduce_geometry(n: int):
    """{"eval": (blocks, most, least, ragged), "inner": ...}: workgroups and the per-lane trip counts of poly_eval_partial's Horner loop
    (lane t takes (n - 1 - t) / T + 1 steps) and poly_inner_partial's strided loop; ragged = the working lanes differ."""
    out = {}
    base = min(REDUCE_CAP, (n + K_PT - 1) // K_PT)
    for name, blocks in (("eval", min(EVAL_CAP, base)), ("inner", base)):
        most, least = _trips(n, blocks)
        out[name] = (blocks, most, least, most != least)
    return out


# ---- values ----------------------------------------------------------------------------------------------------------------------------
def full_width(field: int) -> int:
    return 0x2f1e0d3c4b5a69788796a5b4c3d2e1f00f1e2d3c4b5a69788796a5b4c3d2e1f0       # below 2^254, so below both moduli; no limb is 0


def limb_pair(i: int):
    """(lo, hi), lo < hi < 2^254: equal in every u32 limb above i, different in limb i, and ordered the OTHER way by every limb below i --
    a comparison that skips limb i, or starts from the wrong end, orders them wrongly."""
    top = sum((0x1234567 + j) << (32 * j) for j in range(i + 1, KEY_LIMBS))
    lo = top | (0x10000000 + i) << (32 * i) | ((1 << (32 * i)) - 1)
    hi = top | (0x30000000 + i) << (32 * i)
    return lo, hi


def specials(field: int):
    p = MODULUS[field]
    return [0, 1, 2, p - 1, p - 2, full_width(field)]


def palette(field: int):
    """The specials, then every limb pair in both orders."""
    seq = specials(field)
    for i in range(KEY_LIMBS):
        lo, hi = limb_pair(i)
        seq += [lo, hi, hi, lo]
    return seq


def deciding_limbs(values):
    """The set of i such that two of the values have limb i as their highest differing u32 limb (all pairs of a small set, neighbours in
    sorted order of a large one)."""
    u = sorted(set(int(v) for v in values))
    pairs = [(a, b) for k, a in enumerate(u) for b in u[k + 1:]] if len(u) <= 64 else list(zip(u, u[1:]))
    return {((a ^ b).bit_length() - 1) // 32 for a, b in pairs}


SCALARS = ("zero", "one", "minus_one", "full")


def scalar_value(name: str, field: int) -> int:
    return {"zero": 0, "one": 1, "minus_one": MODULUS[field] - 1, "full": full_width(field)}[name]


# ---- sort cases ------------------------------------------------------------------------------------------------------------------------
SORT_PATTERNS = ("ascending", "descending", "constant", "organ_pipe", "two_valued_half", "two_valued_64th", "palette", "max_tail", "random")
SORT_LOGS = tuple(range(1, 15))              # 1..11 tile only; 12 lone global; 13 one global2; 14 global2 + global
SORT_LENGTHS = tuple(sorted({v for m in SORT_LOGS for v in ((1 << m) - 1, 1 << m, (1 << (m - 1)) + 1)} - {1}))
SORT_LARGE = (1 << 20) + 1                   # padded to 2^21: jl reaches 20, 2^20 - 1 padding keys behind 2^20 + 1 real ones


def sort_values(n: int, pattern: str, field: int):
    """n canonical integers of `pattern`."""
    p = MODULUS[field]
    rnd = random.Random(f"{n}/{pattern}/{field}")
    if pattern in ("ascending", "descending", "organ_pipe"):
        step = p // (n + 1)                                              # spread over the whole field: every limb takes part
        asc = [i * step + i for i in range(n)]
        if pattern == "ascending":
            return asc
        if pattern == "descending":
            return asc[::-1]
        return asc[0::2] + asc[1::2][::-1]
    if pattern == "constant":
        return [full_width(field)] * n
    if pattern.startswith("two_valued"):
        lo, hi = limb_pair(4)
        one_in = 2 if pattern.endswith("half") else 64
        return [hi if rnd.randrange(one_in) == 0 else lo for _ in range(n)]
    if pattern == "palette":
        pal = palette(field)
        return [pal[i % len(pal)] for i in range(n)]
    if pattern == "max_tail":                                            # p - 1 duplicated next to the all-ones padding
        tail = max(1, n // 8)
        return [rnd.randrange(p) for _ in range(n - tail)] + [p - 1] * tail
    assert pattern == "random"
    return [rnd.randrange(p) for _ in range(n)]


def sort_cases():
    """(n, pattern, form, field).  Both forms at every length; the order is the canonical value's either way, so the canonical runs use Fp and
    the Montgomery runs Fq -- except the patterns made of field-specific values (p - 1 and its neighbours), which run both fields in both."""
    out = []
    for n in SORT_LENGTHS:
        for pattern in SORT_PATTERNS:
            if pattern in ("palette", "max_tail"):
                out += [(n, pattern, form, field) for form in (CANONICAL, MONTGOMERY) for field in (FP, FQ)]
            else:
                out += [(n, pattern, CANONICAL, FP), (n, pattern, MONTGOMERY, FQ)]
    return out


def sort_large_limbs(n: int = SORT_LARGE, seed: int = 2021):
    """(keys, sorted keys) as (n, 4) canonical limbs with values below 2^63, built without Python integers: repeats included."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
    v[rng.integers(0, n, size=n // 16)] = v[0]
    keys = np.zeros((n, 4), dtype=np.uint64)
    keys[:, 0] = v
    want = np.zeros_like(keys)
    want[:, 0] = np.sort(v)
    return keys, want


# ---- permute_expression_pair cases -----------------------------------------------------------------------------------------------------
def permute_model(inputs, table):
    """The reference's sequential walk (plonk/lookup/prover.rs:567-623) restated with numpy on two equally long 1-D arrays of any ordered
    dtype (uint64, or object for Python integers): sort, first-occurrence flags, the sorted table minus one instance of every distinct
    input, the leftover handed to the repeated rows from the end.  Returns (A', S'), or None for ConstraintSystemFailure."""
    a, t = np.sort(np.asarray(inputs)), np.sort(np.asarray(table))
    n = len(a)
    first = np.ones(n, dtype=bool)
    first[1:] = a[1:] != a[:-1]
    distinct = a[first]
    pos = np.searchsorted(t, distinct, side="left")
    found = pos < n
    found[found] = t[pos[found]] == distinct[found]
    if not found.all():
        return None
    keep = np.ones(n, dtype=bool)
    keep[pos] = False
    leftover = t[keep]                                                   # ascending, as the BTreeMap iterates
    s = a.copy()
    s[np.flatnonzero(~first)] = leftover[::-1]                           # `pop()` takes the rows from the end
    return a, s


PERMUTE_SMALL = (1, 2, 1023, 1024, 1025, 2049)
PERMUTE_2_20 = 1 << 20                                   # nb = 1024: one full chunk of lk_scan_totals
PERMUTE_2_20_1 = (1 << 20) + 1                           # nb = 1025: a second chunk of one block
PERMUTE_2_20_3K = (1 << 20) + 3 * 1024 + 5               # second chunk of four blocks, the last one ragged
PERMUTE_SHAPES = ("distinct", "constant_input", "input_is_table", "constant_table", "leftover_absent", "runs", "palette")
PERMUTE_FAILURES = ("missing_below", "missing_above", "missing_last")


def _universe(n: int, field: int, big: bool):
    """n + 4 ascending distinct values; index 0 is below and index n + 3 above everything a table holds."""
    if big:
        i = np.arange(n + 4, dtype=np.uint64)
        return (i + np.uint64(1)) * np.uint64(((1 << 63) - 1) // (n + 5)) + i % np.uint64(7)
    step = MODULUS[field] // (n + 5)
    return np.array([(i + 1) * step + i % 7 for i in range(n + 4)], dtype=object)


def run_boundaries(n: int):
    """The multiples of the scan block that a three-row run of repeats is laid across (rows b - 1 .. b + 1 of the sorted input)."""
    return [b for b in (LK_SCAN_BLOCK, 1 << 20, (1 << 20) + 2 * LK_SCAN_BLOCK) if b + 2 <= n]


def permute_indices(n: int, shape: str, seed: int = 0):
    """(input, table) as int64 indices into _universe(n): the shape without the values."""
    rng = np.random.default_rng([n, PERMUTE_SHAPES.index(shape) if shape in PERMUTE_SHAPES else 16 + PERMUTE_FAILURES.index(shape), seed])
    every = np.arange(1, n + 1, dtype=np.int64)
    if shape == "distinct":                                              # n_rep = 0: nothing left over
        return rng.permutation(every), rng.permutation(every)
    if shape == "constant_input":                                        # n_rep = n - 1: the whole table but one row is left over
        return np.full(n, n // 2 + 1, dtype=np.int64), rng.permutation(every)
    if shape == "input_is_table":
        col = rng.integers(1, max(2, n // 3) + 1, size=n, dtype=np.int64)
        return col, col.copy()
    if shape == "constant_table":
        return np.full(n, 3, dtype=np.int64), np.full(n, 3, dtype=np.int64)
    if shape == "leftover_absent":                                       # one table row per distinct input; the rest are values no input has
        d = max(1, n // 2)
        col = rng.integers(1, d + 1, size=n, dtype=np.int64)
        have = np.unique(col)
        absent = rng.integers(d + 1, n + 2, size=n - len(have), dtype=np.int64) if n > len(have) else np.empty(0, dtype=np.int64)
        return col, rng.permutation(np.concatenate([have, absent]))
    if shape == "runs":                                                  # distinct rows but for runs of three across scan-block boundaries
        sorted_in = every.copy()
        for b in run_boundaries(n):
            sorted_in[b - 1:b + 2] = sorted_in[b - 1]
        have = np.unique(sorted_in)
        extra = rng.integers(1, n + 1, size=n - len(have), dtype=np.int64)
        return rng.permutation(sorted_in), rng.permutation(np.concatenate([have, extra]))
    # the failures: a well-formed multiset, then one input row is given a value the table lacks
    col = rng.integers(1, max(2, n // 3) + 1, size=n, dtype=np.int64)
    table = col.copy()
    if shape == "missing_below":                                         # lower_bound = 0, key differs
        col[int(rng.integers(0, n))] = 0
    elif shape == "missing_above":                                       # lower_bound = n
        col[int(rng.integers(0, n))] = n + 3
    else:                                                                # the largest input, alone in the last sorted row; the table goes higher
        assert shape == "missing_last"
        hole, row = int(col.max()) + 1, int(rng.integers(0, n))
        col[row] = hole
        table[row] = hole + 1                                            # the instance that row's old value no longer needs
    return col, table


def permute_columns(n: int, shape: str, field: int, big: bool):
    """(input, table) as 1-D value arrays: uint64 below 2^63 when `big`, else Python integers spread over the whole field."""
    if shape == "palette":                                               # equal / unequal and the order decided in every limb
        pal = np.array(sorted(set(palette(field))), dtype=object)
        rng = np.random.default_rng([n, 99])
        return pal[rng.integers(0, len(pal), size=n)], pal[rng.permutation(np.arange(n) % len(pal))]
    u = _universe(n, field, big)
    a, t = permute_indices(n, shape)
    return u[a], u[t]


def permute_cases():
    """(n, shape, big).  Small cases run both fields in both forms; `big` cases use values below 2^63, Fp, canonical form."""
    out = [(n, shape, False) for n in PERMUTE_SMALL for shape in ("distinct", "constant_input", "input_is_table", "constant_table", "leftover_absent")]
    out += [(2049, "runs", False), (1025, "palette", False), (2049, "palette", False)]
    out += [(PERMUTE_2_20, "input_is_table", True), (PERMUTE_2_20, "constant_input", True)]
    out += [(PERMUTE_2_20_1, "input_is_table", True), (PERMUTE_2_20_1, "constant_input", True), (PERMUTE_2_20_1, "distinct", True)]
    out += [(PERMUTE_2_20_3K, "runs", True), (PERMUTE_2_20_3K, "leftover_absent", True)]
    return out


def permute_failure_cases():
    out = [(n, shape, False) for n in (2, 1025) for shape in PERMUTE_FAILURES]
    out += [(1, "missing_below", False), (1, "missing_above", False), (PERMUTE_2_20_1, "missing_last", True)]
    return out


def limbs_of_u64(v) -> np.ndarray:
    """values below 2^64 as (n, 4) canonical limbs."""
    out = np.zeros((len(v), 4), dtype=np.uint64)
    out[:, 0] = v
    return out


# ---- poly cases ------------------------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 7, 8, 9, 255, 2047, 2048, 2049, 5000, 70001, (1 << 19) + 3)      # tests/test_gpu_poly.py
EVAL_T = EVAL_CAP * K_PT                     # 65536: stride of the Horner evaluation once its grid is capped
INNER_T = REDUCE_CAP * K_PT                  # 262144: stride of the inner product once its grid is capped
PER3 = (1 << 20) + K_TILE + 1                # nblk = 514, per = 3: the last lane holds one tile and walks two phantom steps
POLY_LENGTHS = SIZES + (EVAL_T, EVAL_T + 1, INNER_T, INNER_T + 1, 2 * INNER_T, PER3)   # 2 * INNER_T: the inner product's uniform trip count 2

PLACEMENTS = ("first", "last", "lane_first", "lane_last", "tile_first", "tile_last", "lane", "group", "tile", "all")
INVERT_LENGTHS = (1, 8, 9, 64, 65, 2047, 2048, 2049, 5000, 70001)
ASSIGNED_LENGTHS = (1, 8, 9, 64, 65, 2047, 2048, 2049, 5000)
GROUP = K_PC * K_INV_GROUP                   # 64 elements share one inversion


def placement(name: str, n: int):
    """The indices `name` overlays in a vector of n elements (lane / group / tile: whole and aligned, away from index 0 when the vector is
    long enough), or None when the vector is too short to hold it."""
    def block(size):
        start = size * min(3, n // size - 1) if size < K_TILE else K_TILE * min(1, n // K_TILE - 1)
        return np.arange(start, start + size) if n >= size else None
    if name == "first":
        return np.array([0])
    if name == "last":
        return np.array([n - 1])
    if name == "all":
        return np.arange(n)
    if name in ("lane", "lane_first", "lane_last"):
        idx = block(K_PC)
        return idx if idx is None or name == "lane" else idx[:1] if name == "lane_first" else idx[-1:]
    if name == "group":
        return block(GROUP)
    idx = block(K_TILE)
    return idx if idx is None or name == "tile" else idx[:1] if name == "tile_first" else idx[-1:]


def invert_cases():
    """(n, placement) of zeros in the vector handed to batch_invert."""
    return [(n, name) for n in INVERT_LENGTHS for name in PLACEMENTS if placement(name, n) is not None]


ASSIGNED_FILLS = ("zero", "one", "mix01")    # what the placement writes into the denominators; mix01: 0 or 1 at random, so nothing is inverted there


def assigned_cases():
    """(n, placement, fill) of the denominators handed to assigned_to_field; the 0/1 mix only where it empties a whole product."""
    out = [(n, name, fill) for n in ASSIGNED_LENGTHS for name in PLACEMENTS for fill in ("zero", "one") if placement(name, n) is not None]
    out += [(n, name, "mix01") for n in ASSIGNED_LENGTHS for name in ("lane", "group", "tile", "all") if placement(name, n) is not None]
    return out


def overlay_mask(n: int, name: str, fill: str):
    """(indices, 0/1 values) of an assigned_to_field overlay."""
    idx = placement(name, n)
    if fill == "mix01":
        return idx, np.random.default_rng([n, PLACEMENTS.index(name)]).integers(0, 2, size=len(idx))
    return idx, np.full(len(idx), 1 if fill == "one" else 0)


def eval_cases():
    """(n, x): eval_polynomial, powers and (x as the other vector's seed only) compute_inner_product."""
    return [(n, x) for n in POLY_LENGTHS for x in SCALARS]


KATE_KINDS = ("random", "multiple")          # `multiple`: a = (X - b) q, the remainder the division drops is zero


def kate_cases():
    """(n, b, kind)."""
    return [(n, b, kind) for n in POLY_LENGTHS if n >= 2 for b in SCALARS for kind in KATE_KINDS]


PRODUCT_LENGTHS = (1, 2, 2047, 2048, 2049, 5000, (1 << 19) + 3, PER3)
ZERO_FACTORS = ("none", "index0", "mid_tile", "tile_last")


def zero_factor_index(where: str, n: int):
    """Index of the zero among the n - 1 factors, or None."""
    idx = {"none": None, "index0": 0, "mid_tile": K_TILE // 2 + 3, "tile_last": K_TILE - 1}[where]
    return idx if idx is None or idx < n - 1 else None


def product_cases():
    """(n, init, zero factor)."""
    out = []
    for n in PRODUCT_LENGTHS:
        for init in SCALARS:
            out += [(n, init, where) for where in ZERO_FACTORS if where == "none" or zero_factor_index(where, n) is not None]
    return out


POISON_LENGTHS = (K_TILE, K_TILE + 1)        # grand_product handed n factors: m[n - 1] belongs to no z
