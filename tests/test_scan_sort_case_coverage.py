"""What the GPU sweep of tests/test_gpu_scan_sort_cases.py executes, proved on the CPU: the geometry replica of tests/scan_sort_cases.py computes
what halo2_amd/csrc/poly_plan.h computes (the header poly.hip launches by, compiled for the CPU) and has the constants of lookup.hip and
lookup_keys.cuh, and the case list reaches every path that replica distinguishes --
every launch kind of the sort, both trip counts of lk_scan_totals' chunk loop, per = 1, 2, 3 of the carry kernels with a ragged last lane,
the three trip-count regimes of the reductions, every zero placement, every extreme scalar and an order decided in every limb.  A retuned
tile moves the case list or fails here; a hole in the list fails with the name of the path it leaves out."""
import os
import random
import re
import subprocess

import numpy as np

import scan_sort_cases as sc
from oracle import lookup as olk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo2_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _const(src, pattern):
    m = re.search(pattern, src)
    assert m, f"not found in the source: {pattern}"
    return m.group(1)


def plan_lengths():
    """The lengths the compiled geometry is held to the replica at: every n up to three tiles, every length of the poly case lists, the
    strides at which a capped grid's lanes take a second step and the length at which the carry kernels' lanes take a second tile, each
    with its neighbours, and the longest vector the entry points accept."""
    lengths = set(range(1, 3 * sc.K_TILE + 1)) | set(sc.POLY_LENGTHS) | set(sc.PRODUCT_LENGTHS) | set(sc.INVERT_LENGTHS) | set(sc.POISON_LENGTHS)
    lengths |= {n + d for n in (sc.EVAL_T, sc.INNER_T, sc.K_PT * sc.K_TILE) for d in (-1, 0, 1)} | {1 << 30}
    return sorted(lengths)


def _poly_plan(exe, lengths_file, *flags):
    """Builds tests/native/poly_plan_check.cpp -- csrc/poly_plan.h, the text poly.hip compiles, on the CPU -- and returns what it prints."""
    made = subprocess.run(["g++", "-O2", "-std=c++17", *flags, os.path.join(ROOT, "tests", "native", "poly_plan_check.cpp"), "-o", exe],
                          capture_output=True, text=True)
    assert made.returncode == 0, made.stderr
    ran = subprocess.run([exe, lengths_file], capture_output=True, text=True, timeout=60)
    assert ran.returncode == 0, (ran.returncode, ran.stderr[-2000:])
    return ran.stdout


def test_the_replica_has_the_constants_of_the_sources():
    """poly.hip's geometry is the arithmetic of csrc/poly_plan.h, so the header is compiled and run, not read: its constants and, at every
    length of plan_lengths(), its grids, tile counts and carry spans equal the replica's.  Built twice, plain and with
    -fsanitize=address,undefined (a stand-alone program, nothing preloaded); both print the same."""
    lengths = plan_lengths()
    build = os.path.join(ROOT, "build")
    os.makedirs(build, exist_ok=True)
    lengths_file = os.path.join(build, "poly_plan_lengths.txt")
    with open(lengths_file, "w") as f:
        f.write("".join("%d\n" % n for n in lengths))
    out = _poly_plan(os.path.join(build, "poly_plan_check"), lengths_file)
    assert out == _poly_plan(os.path.join(build, "poly_plan_check_san"), lengths_file, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    head, *rows = out.splitlines()
    words = head.split()
    assert words[0] == "constants:"
    k = dict(zip(words[1::2], map(int, words[2::2])))
    assert (k["kPT"], k["kPC"], k["kTile"], k["kInvGroup"]) == (sc.K_PT, sc.K_PC, sc.K_TILE, sc.K_INV_GROUP) and sc.K_TILE == sc.K_PT * sc.K_PC
    assert (k["kReduceCap"], k["kEvalCap"]) == (sc.REDUCE_CAP, sc.EVAL_CAP)
    # a lane's row holds its kPC elements and one word of padding, the scan array one value per lane: what the launches ask LDS for
    assert k["kPitch"] > 8 * sc.K_PC and k["kSPitch"] >= 8 and k["kTileLds"] == 4 * sc.K_PT * k["kPitch"]
    assert k["kScanLds"] == k["kTileLds"] + 4 * sc.K_PT * k["kSPitch"] <= 160 * 1024
    assert len(rows) == len(lengths)
    for n, row in zip(lengths, rows):
        got = tuple(int(v) for v in row.split())
        geo = sc.reduce_geometry(n)
        assert got == (n, geo["inner"][0], geo["eval"][0]) + sc.scan_geometry(n), (n, got)

    lookup, keys = _src("lookup.hip"), _src("lookup_keys.cuh")
    assert int(_const(lookup, r"constexpr int kTileLog = (\d+);")) == sc.LK_TILE_LOG
    assert int(_const(lookup, r"constexpr u32 kScanBlock = (\d+);")) == sc.LK_SCAN_BLOCK
    assert _const(lookup, r"for \(u32 base = 0; base < nb; base \+= (\w+)\)") == "kScanBlock"
    assert int(_const(keys, r"struct key256 \{\s*u32 v\[(\d+)\];")) == sc.KEY_LIMBS
    assert int(_const(keys, r"for \(int i = (\d+); i >= 0; --i\) \{\s*if \(a\.v\[i\] != b\.v\[i\]\) return a\.v\[i\] < b\.v\[i\];")) == sc.KEY_LIMBS - 1


def test_the_geometry_rows_the_lengths_were_chosen_for():
    assert sc.sort_schedule(2048) == [("tile", 11, 0)]
    assert sc.sort_schedule(4096) == [("tile", 12, 0), ("global", 12, 11), ("tile", 12, 12)]
    assert sc.sort_schedule(8192)[3:] == [("global2", 13, 12), ("tile", 13, 13)]
    assert sc.sort_schedule(16384)[5:] == [("global2", 14, 13), ("global", 14, 11), ("tile", 14, 14)]
    assert sc.permute_geometry(1 << 20) == (1024, 1) and sc.permute_geometry((1 << 20) + 1) == (1025, 2)
    assert sc.scan_geometry(sc.PER3) == (514, 3, 1, 2)
    assert sc.scan_geometry(257 * sc.K_TILE) == (257, 2, 1, 1) and sc.scan_geometry(256 * sc.K_TILE) == (256, 1, 1, 0)
    assert sc.reduce_geometry(sc.EVAL_T)["eval"] == (256, 1, 1, False) and sc.reduce_geometry(sc.EVAL_T + 1)["eval"] == (256, 2, 1, True)
    assert sc.reduce_geometry(sc.INNER_T + 1)["inner"] == (1024, 2, 1, True) and sc.reduce_geometry(2 * sc.INNER_T)["inner"] == (1024, 2, 2, False)
    assert sc.reduce_geometry(300)["inner"] == (2, 1, 1, False)            # the lanes past n take no step at all: not a second trip count


# ---- sort ------------------------------------------------------------------------------------------------------------------------------
def _sort_launches():
    lengths = {n for n, *_ in sc.sort_cases()} | {sc.SORT_LARGE}
    return {launch for n in lengths for launch in sc.sort_schedule(n)}


def test_the_sort_cases_reach_every_launch_kind():
    """A merge size 2^kl above the tile has the strides kl-1 .. kTileLog as global passes: an even count goes in pairs (global2 only), an odd
    count leaves one lone `global` -- so a lone global exists only when kl - kTileLog is odd, a global2 only from kl - kTileLog = 2 on,
    and the tail tile launch follows either way."""
    launches = _sort_launches()
    tile_only = {n for n, *_ in sc.sort_cases() if len(sc.sort_schedule(n)) == 1}
    for log in range(1, sc.LK_TILE_LOG + 1):
        assert any(sc.ceil_log2(n) == log for n in tile_only), f"no tile-only sort of padded size 2^{log}"
        for n in ((1 << log) - 1, 1 << log, (1 << (log - 1)) + 1):          # no padding, one padding key, maximal padding
            assert n < 2 or n in tile_only, f"tile-only length {n} is missing"
    for parity in (0, 1):
        of = lambda kind: {l for l in launches if l[0] == kind and (l[2 if kind == "tile" else 1] - sc.LK_TILE_LOG) % 2 == parity and l[2]}
        assert of("tile"), f"no tail tile launch with kl - kTileLog of parity {parity}"
        assert of("global2"), f"no global2 launch with kl - kTileLog of parity {parity}"
        assert bool(of("global")) == (parity == 1), f"lone global launches with kl - kTileLog of parity {parity}: {sorted(of('global'))}"
    assert any(l[0] == "global2" and l[2] >= 20 for l in launches), "no launch with jl >= 20 (a stride of 2^20 keys)"
    for m in (12, 13, 14):
        for n in ((1 << m) - 1, 1 << m, (1 << (m - 1)) + 1):
            assert n in {c[0] for c in sc.sort_cases()}, n
    for pattern in sc.SORT_PATTERNS:
        for form in (sc.CANONICAL, sc.MONTGOMERY):
            assert {n for n, p_, f_, _ in sc.sort_cases() if p_ == pattern and f_ == form} == set(sc.SORT_LENGTHS), (pattern, form)


def test_the_sort_patterns_are_what_their_names_say():
    for field in (sc.FP, sc.FQ):
        p = sc.MODULUS[field]
        for n in (2, 5, 64, 2049):
            v = {pat: sc.sort_values(n, pat, field) for pat in sc.SORT_PATTERNS}
            assert all(len(x) == n and all(0 <= e < p for e in x) for x in v.values())
            assert v["ascending"] == sorted(set(v["ascending"])) and v["descending"] == v["ascending"][::-1]
            assert len(set(v["constant"])) == 1 and sorted(v["organ_pipe"]) == v["ascending"]
            peak = v["organ_pipe"].index(max(v["organ_pipe"]))
            assert v["organ_pipe"][:peak + 1] == sorted(v["organ_pipe"][:peak + 1]) and v["organ_pipe"][peak:] == sorted(v["organ_pipe"][peak:], reverse=True)
            assert set(v["two_valued_half"]) <= set(sc.limb_pair(4)) and v["max_tail"][-1] == p - 1
        assert len(set(sc.sort_values(2049, "two_valued_half", field))) == 2 and len(set(sc.sort_values(2049, "two_valued_64th", field))) == 2
        assert sc.sort_values(16, "max_tail", field)[-2:] == [p - 1, p - 1]
    keys, want = sc.sort_large_limbs(5000)
    assert keys[:, 0].max() < 1 << 63 and not keys[:, 1:].any() and sorted(keys[:, 0].tolist()) == want[:, 0].tolist()
    assert len(set(keys[:, 0].tolist())) < 5000                            # repeats


def test_the_palette_decides_the_order_in_every_limb():
    for field in (sc.FP, sc.FQ):
        p = sc.MODULUS[field]
        pal = sc.palette(field)
        assert all(0 <= v < p for v in pal) and {0, 1, 2, p - 1, p - 2, sc.full_width(field)} <= set(pal)
        for i in range(sc.KEY_LIMBS):
            lo, hi = sc.limb_pair(i)
            assert lo < hi and sc.deciding_limbs([lo, hi]) == {i}
            assert i == 0 or (lo & ((1 << (32 * i)) - 1)) > (hi & ((1 << (32 * i)) - 1))          # the lower limbs say the opposite
            assert lo in pal and hi in pal, f"the palette has no pair of values whose highest differing limb is {i}"
            k = pal.index(lo)
            assert pal[k:k + 4] == [lo, hi, hi, lo]                           # both orders
    every = set(range(sc.KEY_LIMBS))
    for what, got in (("sort", {i for n, pat, _, field in sc.sort_cases() if pat == "palette" and n >= 64 for i in sc.deciding_limbs(sc.sort_values(n, pat, field))}),
                      ("permute", {i for n, shape, big in sc.permute_cases() if not big for col in sc.permute_columns(n, shape, sc.FP, big)
                                   for i in sc.deciding_limbs(col)})):
        assert got == every, f"no {what} case holds two keys whose highest differing limb is {sorted(every - got)}"
    for i in range(sc.KEY_LIMBS):                                              # and not only through the spread-out patterns: the palette case alone does
        assert any(i in sc.deciding_limbs(sc.permute_columns(n, "palette", sc.FP, False)[0]) for n, shape, _ in sc.permute_cases() if shape == "palette"), i


# ---- permute_expression_pair -----------------------------------------------------------------------------------------------------------
def _n_rep(col):
    return len(col) - len(np.unique(col))


def test_the_permute_cases_reach_both_chunk_counts_and_both_extremes_of_n_rep():
    cases = sc.permute_cases()
    chunks = {sc.permute_geometry(n)[1] for n, _, _ in cases}
    assert chunks == {1, 2}, f"lk_scan_totals chunk counts reached: {sorted(chunks)}; the second pass of its loop needs more than 2^20 rows"
    rows = set(sc.PERMUTE_SMALL) | {sc.PERMUTE_2_20, sc.PERMUTE_2_20_1, sc.PERMUTE_2_20_3K}
    assert {n for n, _, _ in cases} == rows, f"row counts without a permute case: {sorted(rows - {n for n, _, _ in cases})}"
    assert sc.PERMUTE_2_20_1 in {n for n, _, _ in cases}, "no case with nb = 1025: the second chunk of lk_scan_totals never holds exactly one block"
    assert sc.permute_geometry(sc.PERMUTE_2_20) == (1024, 1) and sc.permute_geometry(sc.PERMUTE_2_20_1) == (1025, 2)
    assert sc.permute_geometry(sc.PERMUTE_2_20_3K)[0] == 1028 and sc.PERMUTE_2_20_3K % sc.LK_SCAN_BLOCK
    assert {shape for _, shape, _ in cases} == set(sc.PERMUTE_SHAPES)
    for chunk_count in (1, 2):                                                 # n_rep = 0 and n - 1, under either trip count
        reps = {(_n_rep(sc.permute_indices(n, shape)[0]), n) for n, shape, _ in cases if shape != "palette" and n > 2 and sc.permute_geometry(n)[1] == chunk_count}
        assert any(r == 0 for r, n in reps), f"no case with n_rep = 0 and {chunk_count} chunk(s)"
        assert any(r == n - 1 for r, n in reps), f"no case with n_rep = n - 1 and {chunk_count} chunk(s)"
    for n, shape, big in cases:                                                # a repeat total that the second chunk has to carry
        if sc.permute_geometry(n)[1] == 2 and shape == "input_is_table":
            a, _ = sc.permute_indices(n, shape)
            first = np.ones(n, dtype=bool)
            s = np.sort(a)
            first[1:] = s[1:] != s[:-1]
            assert (~first)[:1 << 20].sum() > 0 and (~first)[1 << 20:].sum() > 0
            break
    else:
        raise AssertionError("no two-chunk case with repeats on both sides of row 2^20")


def test_the_permute_shapes_are_what_their_names_say():
    for n, shape, big in sc.permute_cases():
        if shape == "palette":
            continue
        a, t = sc.permute_indices(n, shape)
        assert len(a) == len(t) == n and a.min() >= 1 and t.min() >= 1 and max(a.max(), t.max()) <= n + 2          # index n + 3 stays above every table
        assert set(np.unique(a)) <= set(np.unique(t)), (n, shape)
        if shape == "distinct":
            assert _n_rep(a) == 0 and _n_rep(t) == 0
        if shape == "constant_input":
            assert _n_rep(a) == n - 1 and _n_rep(t) == 0
        if shape == "input_is_table":
            assert np.array_equal(a, t) and (n < 8 or 0 < _n_rep(a) < n - 1)
        if shape == "constant_table":
            assert _n_rep(t) == n - 1
        if shape == "leftover_absent":                                         # the table holds each input value once
            values, counts = np.unique(t, return_counts=True)
            assert (counts[np.isin(values, a)] == 1).all() and (n < 8 or not np.isin(values, a).all())
        if shape == "runs":
            s = np.sort(a)
            bounds = sc.run_boundaries(n)
            assert bounds and _n_rep(a) == 2 * len(bounds)
            for b in bounds:                                                    # the run starts in one scan block and ends in the next
                assert b % sc.LK_SCAN_BLOCK == 0 and s[b - 1] == s[b] == s[b + 1] and s[b - 2] != s[b - 1] and (b + 2 >= n or s[b + 2] != s[b + 1])
    assert sc.run_boundaries(2049) == [1024] and sc.run_boundaries(sc.PERMUTE_2_20_3K) == [1024, 1 << 20, (1 << 20) + 2048]
    for big in (False, True):
        u = sc._universe(100, sc.FP, big)
        assert len(u) == 104 and all(u[i] < u[i + 1] for i in range(103)) and int(u[-1]) < (1 << 63 if big else sc.P)


def test_the_failure_cases_take_the_branch_they_name():
    got = set()
    for n, shape, big in sc.permute_failure_cases():
        a, t = sc.permute_indices(n, shape)
        missing = sorted(set(a.tolist()) - set(t.tolist()))
        assert len(missing) == 1 and (a == missing[0]).sum() == 1, (n, shape)
        ts = np.sort(t)
        p = int(np.searchsorted(ts, missing[0]))
        if shape == "missing_below":
            assert p == 0 and missing[0] < ts[0]
        elif shape == "missing_above":
            assert p == n
        else:
            assert 0 < p < n and missing[0] == a.max() and np.sort(a)[n - 1] == missing[0]
        assert sc.permute_model(*sc.permute_columns(n, shape, sc.FP, big)) is None
        got.add((shape, n > 1 << 20))
    assert {s for s, _ in got} == set(sc.PERMUTE_FAILURES) and ("missing_last", True) in got, "the last distinct input has to sit in a row past 2^20"


def _pairs(a, s):
    return [int(v) for v in a], [int(v) for v in s]


def test_permute_model_is_the_sequential_walk():
    checked = 0
    for n, shape, big in sc.permute_cases() + sc.permute_failure_cases():
        if n > 2049:
            continue
        for field in (sc.FP, sc.FQ):
            a, t = sc.permute_columns(n, shape, field, big)
            want = olk.permute_expression_pair([int(v) for v in a], [int(v) for v in t], n)
            got = sc.permute_model(a, t)
            assert (got is None) == (want is None) == (shape in sc.PERMUTE_FAILURES), (n, shape)
            assert got is None or _pairs(*got) == (want[0], want[1]), (n, shape)
            checked += 1
    assert checked >= 60
    rnd = random.Random(2049)
    failures = 0
    for trial in range(200):                                                   # seeded random multisets, in both dtypes the model is used with
        n = rnd.choice([1, 2, 3, 5, 17, 100, 333])
        span = rnd.choice([1, 2, 3, n, 4 * n])
        table = [rnd.randrange(span) for _ in range(n)]
        inputs = [rnd.choice(table) for _ in range(n)]
        if trial % 4 == 0:
            inputs[rnd.randrange(n)] = rnd.choice([span + 1, rnd.randrange(span)])
        want = olk.permute_expression_pair(inputs, table, n)
        failures += want is None
        for dtype, scale in ((np.uint64, 1), (object, sc.P // (8 * n + 8))):
            got = sc.permute_model(np.array([v * scale for v in inputs], dtype=dtype), np.array([v * scale for v in table], dtype=dtype))
            assert (got is None) == (want is None)
            assert got is None or _pairs(*got) == ([v * scale for v in want[0]], [v * scale for v in want[1]])
    assert 10 < failures < 100


# ---- poly ------------------------------------------------------------------------------------------------------------------------------
def test_the_poly_lengths_reach_every_carry_and_reduction_regime():
    for name, lengths in (("kate_division", {n for n, _, _ in sc.kate_cases()}), ("grand_product", {n for n, _, _ in sc.product_cases()})):
        geo = {n: sc.scan_geometry(n) for n in lengths}
        pers = {g[1] for g in geo.values()}
        assert {1, 2, 3} <= pers, f"{name}: the carry kernel never runs with per = {sorted({1, 2, 3} - pers)}"
        assert any(g[1] >= 3 and g[3] >= 2 for g in geo.values()), f"{name}: no ragged last lane with two or more phantom steps"
    assert set(sc.SIZES) <= set(sc.POLY_LENGTHS)
    lengths = {n for n, _ in sc.eval_cases()}
    for name in ("eval", "inner"):
        regimes = {("one" if most == 1 else "ragged" if ragged else "uniform") for _, most, _, ragged in (sc.reduce_geometry(n)[name] for n in lengths)}
        assert regimes == {"one", "uniform", "ragged"}, f"{name}: trip-count regimes never run: {sorted({'one', 'uniform', 'ragged'} - regimes)}"
    assert {sc.EVAL_T, sc.EVAL_T + 1, sc.INNER_T, sc.INNER_T + 1} <= lengths


def test_every_zero_placement_occurs():
    inv = {name for _, name in sc.invert_cases()}
    assert inv == set(sc.PLACEMENTS), f"batch_invert never sees zeros at: {sorted(set(sc.PLACEMENTS) - inv)}"
    for fill in ("zero", "one"):
        got = {name for _, name, f in sc.assigned_cases() if f == fill}
        assert got == set(sc.PLACEMENTS), f"assigned_to_field never sees a denominator of {fill} at: {sorted(set(sc.PLACEMENTS) - got)}"
    assert {name for _, name, f in sc.assigned_cases() if f == "mix01"} == {"lane", "group", "tile", "all"}
    # what the names mean, at a length with three tiles
    n = 5000
    at = {name: sc.placement(name, n) for name in sc.PLACEMENTS}
    assert at["first"].tolist() == [0] and at["last"].tolist() == [n - 1] and len(at["all"]) == n
    for name, size in (("lane", sc.K_PC), ("group", sc.GROUP), ("tile", sc.K_TILE)):
        assert len(at[name]) == size and at[name][0] % size == 0 and at[name][0] > 0 and (np.diff(at[name]) == 1).all()
    assert at["lane_first"] == at["lane"][0] and at["lane_last"] == at["lane"][-1] and at["lane_last"] % sc.K_PC == sc.K_PC - 1
    assert at["tile_first"] == at["tile"][0] and at["tile_last"] == at["tile"][-1] and at["tile_last"] % sc.K_TILE == sc.K_TILE - 1
    assert sc.placement("tile", sc.K_TILE - 1) is None and sc.placement("group", 63) is None and sc.placement("lane", 7) is None
    assert sc.GROUP == sc.K_PC * sc.K_INV_GROUP
    idx, vals = sc.overlay_mask(n, "tile", "mix01")
    assert len(idx) == sc.K_TILE and set(vals.tolist()) == {0, 1}


def test_every_extreme_scalar_occurs():
    for what, got in (("x of eval_polynomial / powers", {x for _, x in sc.eval_cases()}), ("b of kate_division", {b for _, b, _ in sc.kate_cases()}),
                      ("init of grand_product", {i for _, i, _ in sc.product_cases()})):
        assert {"zero", "one", "minus_one"} <= got, f"{what} never takes: {sorted({'zero', 'one', 'minus_one'} - got)}"
    for field in (sc.FP, sc.FQ):
        assert [sc.scalar_value(s, field) for s in sc.SCALARS] == [0, 1, sc.MODULUS[field] - 1, sc.full_width(field)]
    for n in sc.POLY_LENGTHS:                                                  # every length meets every scalar
        assert {x for m, x in sc.eval_cases() if m == n} == set(sc.SCALARS)
        assert n < 2 or {(b, k) for m, b, k in sc.kate_cases() if m == n} == {(b, k) for b in sc.SCALARS for k in sc.KATE_KINDS}
    zeros = {where for _, _, where in sc.product_cases()}
    assert zeros == set(sc.ZERO_FACTORS), f"grand_product never has its zero factor at: {sorted(set(sc.ZERO_FACTORS) - zeros)}"
    assert sc.zero_factor_index("tile_last", sc.K_TILE + 1) == sc.K_TILE - 1 and sc.zero_factor_index("tile_last", sc.K_TILE) is None
    assert sc.POISON_LENGTHS == (sc.K_TILE, sc.K_TILE + 1)


def test_the_size_of_the_sweep():
    sort_elems = sum(n for n, *_ in sc.sort_cases()) + sc.SORT_LARGE
    perm = sc.permute_cases() + sc.permute_failure_cases()
    perm_elems = sum(n * (1 if big else 4) for n, _, big in perm)
    poly = {"eval": sc.eval_cases(), "kate": sc.kate_cases(), "product": sc.product_cases(), "invert": sc.invert_cases(), "assigned": sc.assigned_cases()}
    poly_elems = sum(2 * c[0] for cases in poly.values() for c in cases)
    print(f"\nsort: {len(sc.sort_cases()) + 1} cases, {sort_elems} keys; permute: {len(perm)} cases, {perm_elems} rows; "
          + ", ".join(f"{k}: {len(v)}" for k, v in poly.items()) + f" cases, {poly_elems} elements over both fields")
    assert len(sc.sort_cases()) > 700 and len(perm) > 40
