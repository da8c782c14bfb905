"""The sweep of tests/commit_plans.py reaches every plan of the registered commit, proved on the CPU with the host replica: every summary the
replica can produce within commit_plans.BOUNDS (tables up to 2^20 points, widths 4 to 20, 1 to 9 batched columns, every entry point, every
column length at which a field changes) is projected onto its discrete fields, and the set of projections must be exactly what SWEEP
reaches plus what EXCLUDED names -- and EXCLUDED may only name shapes whose smallest table has more than 2^19 points.  The sizes the
issue behind this file quotes are asserted from the replica; the GPU test holds the replica to the device."""
import commit_plans as cp

L = cp.LANES_MI355X


def _proj(case):
    r = cp.expected(case, L)
    return None if isinstance(r, str) else cp.projection(r)


def test_the_sweep_and_the_exclusions_are_exactly_the_plans_there_are():
    enumerated = cp.enumerate_projections()
    swept = {_proj(c) for c in cp.SWEEP} - {None}
    excluded = {p for p, _, _ in cp.EXCLUDED}
    assert len(enumerated) > 400
    missing, unknown = set(enumerated) - (swept | excluded), (swept | excluded) - set(enumerated)
    assert not missing, f"plans no case of SWEEP reaches and EXCLUDED does not name: {sorted(map(str, missing))}"
    assert not unknown, f"SWEEP or EXCLUDED name plans the enumeration does not produce: {sorted(map(str, unknown))}"
    assert not swept & excluded


def test_only_plans_beyond_2_19_points_are_excluded():
    enumerated = cp.enumerate_projections()
    for p, points, reason in cp.EXCLUDED:
        assert points > 1 << 19 and str(points) in reason, (p, points)
        witness = enumerated[p]
        assert witness.points > 1 << 19
        # no table of the sweep's size reaches the shape: not the column's own length, not any size at which the geometry changes
        for smaller in {max(witness.n_used, 8)} | set(cp._tables_for(witness.bits, 1 << 19)):
            if smaller > 1 << 19:
                continue
            if witness.entry == "pair":
                assert _proj(witness._replace(points=smaller, n_used=smaller)) != p
            elif witness.n_used <= smaller <= 1 << 19:
                assert _proj(witness._replace(points=smaller)) != p, (witness, smaller)
    assert all(c.points <= cp.MAX_TABLE for c in cp.SWEEP)


def test_every_case_of_the_sweep_is_a_call_the_library_takes_or_refuses_by_design():
    # (a paired commit over 8191 points, which h2_commit_pair_supported declines, still runs: a 16-bit table of up to 2^16 + 4 points takes
    # the sub-digit form whatever its size)
    assert not [c for c in cp.SWEEP if isinstance(cp.expected(c, L), str)]
    assert cp.expected(cp.Case(8191, 0, "pair", 8191, 0, pair_shift=0), L)["caller"] == cp.PAIR_SUBDIGIT
    assert len(set(cp.SWEEP)) == len(cp.SWEEP)


def test_the_sizes_the_dispatch_is_documented_with():
    assert [cp.choose_c(n, True) for n in (384, 385, 6144, 6145)] == [8, 13, 13, 16]
    assert (cp.pair_supported(8191), cp.pair_supported(8192)) == (0, 1)
    assert cp.h2_commit_column_window_bits((1 << 18) - 1) == 16 and cp.h2_commit_column_window_bits(1 << 18) == 17
    # the side array at 20 bits: from 322639 table columns (322638 points and the blind's column) on, never at 17 bits up to 2^20 points
    assert cp.SIDE_EDGE == 322638
    assert cp.sort2_geometry(cp.SIDE_EDGE + 1, 20, True)[2] == 1 and cp.sort2_geometry(cp.SIDE_EDGE, 20, True)[2] == 0
    assert cp._first(lambda n: cp.sort2_geometry(n + 1, 19, True)[2] == 1, 1 << 19, 1 << 20) == 599186
    assert all(cp.sort2_geometry(n + 1, 17, True)[2] == 0 for n in cp._tables_for(17, 1 << 20))
    # the chunked pass 2: no table up to 2^19 points takes it; the smallest that does has 940416 points at 13 bits
    assert cp.CHUNKED == (940416, 13, 940416)
    # one-pass / two-pass at 8191 / 8192 digit columns from 13 bits on, always two-pass from 17 bits
    for c in range(4, 21):
        lo, hi = cp.plan(L, cp.SMALL, c, 8191, 0), cp.plan(L, cp.SMALL, c, 8192, 0)
        assert (lo["use_sort2"], hi["use_sort2"]) == ((1, 1) if c >= 17 else (0, 1) if c >= 13 else (0, 0)), c
        assert hi["fold9"] == int(c >= 8)
    # max_big and lane_div at 4-bit windows
    W = cp.windows(4)
    assert W == 64 and (3 << 20) // W == 49152
    assert [cp.plan(L, 49152, 4, n, 0)["max_big"] for n in (49151, 49152)] == [0, cp.MAX_BIG]
    assert [cp.plan(L, 49152, 4, n, 0)["lane_div"] for n in (16383, 16384)] == [8, 16]


def test_the_forms_the_issue_names_are_in_the_sweep():
    swept = [cp.expected(c, L) for c in cp.SWEEP]
    swept = [r for r in swept if not isinstance(r, str) and not r["empty"]]
    assert any(r["s2_side"] == 1 for r in swept)
    # the chunked pass 2: a single commit takes it from 940416 points only (EXCLUDED), a paired commit over narrow windows much earlier
    chunked = [r for r in swept if r["use_sort2"] and not r["s2_bins_form"]]
    assert chunked and all(r["pair"] and r["c"] <= 9 for r in chunked) and min(r["m"] for r in chunked) == 63561
    assert any(p[3] == 1 and p[5] == 0 and p[10] == 0 for p, _, _ in cp.EXCLUDED)      # (use_sort2, s2_bins_form, pair) of a projection
    for c in (4, 5, 6, 7, 18, 19):
        assert any(r["c"] == c and r["T"] > 256 for r in swept), c
    assert any(r["c"] == 16 and not r["use_sort2"] and r["m"] < 8192 and r["caller"] == cp.DIRECT for r in swept)      # one pass over 2^15 buckets
    assert {r["caller"] for r in swept} == {cp.DIRECT, cp.HOST_RANGE, cp.HOST_PIPELINED, cp.BATCH_COLUMNS, cp.BATCH_FORK, cp.PAIR_TWO_PASS, cp.PAIR_SUBDIGIT}
    assert any(r["caller"] == cp.BATCH_COLUMNS and r["caller_count"] == 2 and (r["cols_first"], r["cols_last"]) == (5, 4) for r in swept)
    assert any(r["caller"] == cp.HOST_PIPELINED and r["caller_count"] == 2 and r["wide_reduce"] and r["add_only"] and r["fold_only"] for r in swept)
