"""What tests/region_cases.py reaches, proved on the CPU: the event counts around a ballot word and a workgroup, pair sizes, selectors
shared and doubled, the wrapping rotations, foreign and repeated assignments, the long range among short ones, no range at all, the
instance lengths, the caps and both sizes -- and that the model's answer on each case is non-trivial where it should be.
tests/test_gpu_region_check.py is read with `ast`, never imported."""
import ast
import os

import pytest

import region_cases as rc
import region_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_TEST_FILE = os.path.join(ROOT, "tests", "test_gpu_region_check.py")
WAVE, WORKGROUP = 64, 256                                 # ra_check: a ballot word per wave, 256 lanes per workgroup


def _events(case, selector=0):
    return [row for _, _, enabled in case.regions for row in enabled.get(selector, [])]


def test_event_counts_cover_a_ballot_word_and_a_workgroup():
    counts = [len(_events(rc.BY_NAME[f"events-{c}"])) for c in rc.EVENT_COUNTS]
    assert counts == [0, 1, WAVE - 1, WAVE, WAVE + 1, WORKGROUP + 1] == list(rc.EVENT_COUNTS)
    for c in rc.EVENT_COUNTS:
        case = rc.BY_NAME[f"events-{c}"]
        per_pair, records = rc.expected(case)
        events = [e for _, e, _ in records]
        assert sum(per_pair) == len(records) and (c == 0) == (not records)
        if c:
            assert c - 1 in events                        # the last event fails: the last word's top bit in use is set
            assert 0 < len(records) < c or c == 1         # and some pass
        if c > WAVE:
            assert {e // WAVE for e in events} == set(range((c + WAVE - 1) // WAVE))          # a failure in every ballot word
    assert {e // WORKGROUP for _, e, _ in rc.expected(rc.BY_NAME["events-257"])[1]} == {0, 1}     # and in both workgroups


def test_pair_sizes_and_selector_sharing():
    sizes = {len(cells) for case in rc.CASES for _, _, cells in case.gates}
    assert {1, 9} <= sizes
    case = rc.BY_NAME["selectors-and-gates"]
    selectors = [s for _, s, _ in case.gates]
    assert any(len(s) == 2 for s in selectors)                                                # a gate with two selectors
    assert sum(1 for s in selectors if 0 in s) == 2                                           # a selector shared by two gates
    assert [] in selectors                                                                    # and a gate that is always on: no pair
    assert rc.pairs_of(case) == [(0, 0, 1), (0, 1, 0), (1, 0, 0), (3, 0, 2)]
    counts, records = rc.expected(case)
    assert all(counts) and len({p for p, _, _ in records}) == 4                               # every pair reports something
    # the events of selector 0 are region-major: rows 0, 1 of the first region, then row 4 of the second
    assert rc.arrays(case)[3][:3] == [0, 1, 4] and rc.arrays(case)[4][:3] == [0, 0, 1]


def test_rotations_wrap_at_both_ends():
    case = rc.BY_NAME["wrapping"]
    n = 1 << case.k
    assert n == 16 and _events(case) == [0, n - 1] and [rot for _, rot in case.gates[0][2]] == [-1, 1]
    assert (0 - 1) % n == n - 1 and (n - 1 + 1) % n == 0
    assert rc.expected(case)[1] == [(0, 0, 1), (0, 1, 0)]                                     # row 0 finds row 15, row 15 finds row 0
    errors = dict(rm.selector_errors(n, rc.model_regions(case), case.gates, []))
    assert errors[(0, 0, 0, 1)][-1] == 1 and errors[(0, 0, 1, 0)][-1] == 14                   # offsets from the region's first row, 0


def test_foreign_and_repeated_assignments():
    case = rc.BY_NAME["another-region"]
    assert rc.expected(case)[1] == [(0, 1, 0)]            # region 0's own event passes, region 1's on the same row fails, its own row passes
    case = rc.BY_NAME["assigned-twice"]
    ranges = case.regions[0][1]
    cells = [(column, row) for column, first, count in ranges for row in range(first, first + count)]
    assert len(cells) - len(set(cells)) == 2              # one cell three times
    assert rc.expected(case)[1] == [(0, 3, 0)]            # only row 5 is unassigned


def test_the_long_range_sits_among_a_thousand_short_ones():
    case = rc.BY_NAME["big-range"]
    counts = [count for _, first, count in case.regions[0][1]]
    at = counts.index(rc.BIG_RANGE)
    assert counts.count(1) == rc.SMALL_RANGES == 1000 and len(counts) == 1001 and at == 500 and rc.BIG_RANGE == 70000
    assert (sum(counts) + WORKGROUP - 1) // WORKGROUP > 256                                   # more workgroups than the chip has CUs
    assert 1 << case.k == 1 << 17 and rc.BIG_RANGE > (1 << 16)
    _, records = rc.expected(case)
    events = _events(case)
    failing = {e for _, e, c in records if c == 0}                                            # a0 in the event's row: the long range
    assert 0 < len(failing) < len(events)                                                     # rows before, inside and past the range
    assert 0 in failing and len(events) - 1 in failing and len(events) // 2 not in failing
    short = {e for _, e, c in records if c == 1}                                              # a1: the one-cell ranges, rows 0 .. 999
    assert 0 not in short and len(events) // 2 in short and short == {e for e, row in enumerate(events) if row >= rc.SMALL_RANGES}
    assert {c for _, _, c in records} == {0, 1, 2}


def test_no_ranges_and_instance_lengths():
    case = rc.BY_NAME["no-ranges"]
    assert rc.arrays(case)[1].shape == (0, 4) and rc.expected(case)[0] == [4]
    case = rc.BY_NAME["instance-lengths"]
    row = rc.INSTANCE_ROW
    assert case.instance_lens == [0, row, row + 1] and _events(case) == [row]
    assert rc.expected(case)[1] == [(0, 0, 0), (0, 0, 2), (0, 0, 4)]                          # lengths 0 and row fail, row + 1 passes; row + 1 is past it
    assert {code >> 31 for code, _ in rc.arrays(case)[7][0]} == {0, 1}


def test_caps_and_sizes():
    caps = {(cap if isinstance(cap, str) else min(cap, 1)) for case in rc.CASES for cap in case.caps}
    assert caps == {0, 1, rc.EXACT, rc.ONE_LESS}
    for case in rc.CASES:
        total = sum(rc.expected(case)[0])
        for cap in case.caps:
            if isinstance(cap, str):
                assert total >= 2 and 0 < rc.cap_of(case, rc.ONE_LESS) < rc.cap_of(case, rc.EXACT) == total, case.name
            elif cap:
                assert cap >= total, case.name            # the open runs see every record
    assert {1 << case.k for case in rc.CASES} >= {16, 1 << 17}


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c.name)
def test_the_arrays_are_what_the_entry_point_accepts(case):
    n_planes, ranges, lens, rows, owners, offsets, selectors, cells = rc.arrays(case)
    n = 1 << case.k
    assert all(p < n_planes and first + count <= n and r < len(case.regions) for p, first, count, r in ranges.tolist())
    assert len(rows) == len(owners) == offsets[-1] and offsets[0] == 0 and offsets == sorted(offsets) and len(offsets) == case.n_selectors + 1
    assert all(r < n for r in rows) and all(s < case.n_selectors for s in selectors) and len(selectors) == len(cells)
    for code, _ in (cell for pair in cells for cell in pair):
        assert (code & 0x7FFFFFFF) < (len(lens) if code >> 31 else n_planes)
    counts, records = rc.expected(case)
    assert len(counts) == len(selectors) and records == sorted(set(records))


def test_the_gpu_file_runs_every_case_and_is_marked_gpu():
    tree = ast.parse(open(GPU_TEST_FILE).read())
    marks = [node for node in tree.body if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "pytestmark" for t in node.targets)]
    assert len(marks) == 1 and ast.unparse(marks[0].value) == "pytest.mark.gpu"
    funcs = {node.name: node for node in tree.body if isinstance(node, ast.FunctionDef)}
    params = [ast.unparse(d) for d in funcs["test_every_case_against_the_model"].decorator_list]
    assert any("rc.CASES" in d and "parametrize" in d for d in params), params
