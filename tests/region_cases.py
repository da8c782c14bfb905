"""Synthetic cases of the regions' check (h2_cells_assigned_check), built directly as region records and gates -- no circuit.  A case is
written in the terms of tests/region_model.py; `arrays` flattens it into what the entry point takes and `expected` asks the model.
tests/test_region_case_coverage.py proves on the CPU what the list reaches; tests/test_gpu_region_check.py runs it.

Planes: fixed columns first, then advice.  One pair per (gate, selector of the gate), gates in order, a gate's selectors in the order it
queried them; a pair's cells are the gate's queried cells."""
from collections import namedtuple

import numpy as np

import region_model as rm

# regions: [(name, [((kind, index), first row, count)], {selector: [rows]})]; caps: the max_records to run with, an int or EXACT / ONE_LESS
Case = namedtuple("Case", "name k n_fixed n_advice n_selectors regions gates instance_lens caps")
EXACT, ONE_LESS = "exact", "one less"
A = lambda i: ("advice", i)
F = lambda i: ("fixed", i)
I = lambda i: ("instance", i)
EVENT_COUNTS = (0, 1, 63, 64, 65, 257)
BIG_RANGE, SMALL_RANGES = 70000, 1000


def _events_case(count):
    """One selector enabled on `count` consecutive rows from 3 on; the gate reads a0 in its row.  a0 is assigned except where the row
    is a multiple of 7 and on the last enabled row: failures in the first and in the last ballot word and in every workgroup."""
    rows = list(range(3, 3 + count))
    ranges = [(A(0), r, 1) for r in rows[:-1] if r % 7]
    return Case(f"events-{count}", 9, 0, 1, 1, [("r", ranges, {0: rows})], [("g", [0], [(A(0), 0)])], [], [1024])


def _nine_cells():
    cells = [(A(c), rot) for c in range(3) for rot in (-1, 0, 1)]
    ranges = [(A(0), 2, 5), (A(1), 3, 3), (A(2), 2, 2), (A(2), 5, 2)]
    return Case("nine-cells", 4, 0, 3, 1, [("r", ranges, {0: [3, 4, 5]})], [("nine", [0], cells)], [], [1024, 0, EXACT, ONE_LESS])


def _selectors_and_gates():
    """Gate 0 queries selectors 1 and 0 (in that order), gate 1 shares selector 0, gate 2 has no selector at all; two regions enable them."""
    regions = [("first", [(A(0), 0, 2), (F(0), 0, 1)], {0: [0, 1], 1: [1]}), ("second", [(A(0), 4, 1)], {0: [4], 2: [4]})]
    gates = [("two selectors", [1, 0], [(A(0), 0), (F(0), 0)]), ("shared", [0], [(A(1), 0)]), ("none", [], [(A(0), 0)]), ("third", [2], [(A(0), 1)])]
    return Case("selectors-and-gates", 4, 1, 2, 3, regions, gates, [], [1024, EXACT, ONE_LESS])


def _wrapping():
    """n = 16: the selector on row 0 and on row 15, the last event; the gate reads a0 above and below.  Row 15 is assigned (row 0 looks
    back at it), row 1 and row 14 are not, row 0 is (row 15 looks ahead at it)."""
    return Case("wrapping", 4, 0, 1, 1, [("r", [(A(0), 15, 1), (A(0), 0, 1)], {0: [0, 15]})], [("g", [0], [(A(0), -1), (A(0), 1)])], [], [1024])


def _another_region():
    """Region 1 enables the gate on row 3; the cell is assigned -- by region 0.  Region 0's own enabling on row 3 passes."""
    regions = [("owner", [(A(0), 3, 1)], {0: [3]}), ("borrower", [(A(0), 8, 1)], {0: [3, 8]})]
    return Case("another-region", 4, 0, 1, 1, regions, [("g", [0], [(A(0), 0)])], [], [1024])


def _assigned_twice():
    regions = [("r", [(A(0), 2, 3), (A(0), 3, 1), (A(0), 3, 1)], {0: [2, 3, 4, 5]})]
    return Case("assigned-twice", 4, 0, 1, 1, regions, [("g", [0], [(A(0), 0)])], [], [1024])


def _big_range():
    """n = 2^17: one range of 70 000 cells between 500 + 500 ranges of one cell: the binary search over the prefix sums with a long
    plateau, lanes of one range across 274 workgroups.  The selector sits on every 97th row from 400 to 71 400."""
    small = [(A(1), r, 1) for r in range(SMALL_RANGES)]
    ranges = small[:SMALL_RANGES // 2] + [(A(0), 1000, BIG_RANGE)] + small[SMALL_RANGES // 2:]
    rows = list(range(400, 71400, 97))
    return Case("big-range", 17, 0, 2, 1, [("r", ranges, {0: rows})], [("g", [0], [(A(0), 0), (A(1), 0), (A(0), -1)])], [], [4096])


def _no_ranges():
    return Case("no-ranges", 4, 1, 1, 1, [("r", [], {0: [2, 9]})], [("g", [0], [(A(0), 0), (F(0), 0)])], [], [1024, EXACT, ONE_LESS, 0])


INSTANCE_ROW = 5


def _instance_lengths():
    """The gate on row 5 reads three instance columns given 0, 5 and 6 values: the first two cells are padding, the third is assigned."""
    regions = [("r", [(A(0), INSTANCE_ROW, 1)], {0: [INSTANCE_ROW]})]
    gates = [("g", [0], [(I(0), 0), (A(0), 0), (I(1), 0), (I(2), 0), (I(2), 1)])]
    return Case("instance-lengths", 4, 0, 1, 1, regions, gates, [0, INSTANCE_ROW, INSTANCE_ROW + 1], [1024])


CASES = [_events_case(c) for c in EVENT_COUNTS] + [_nine_cells(), _selectors_and_gates(), _wrapping(), _another_region(), _assigned_twice(),
                                                    _big_range(), _no_ranges(), _instance_lengths()]
BY_NAME = {c.name: c for c in CASES}


def model_regions(case):
    return [rm.region_of(name, ranges, enabled) for name, ranges, enabled in case.regions]


def pairs_of(case):
    """[(gate index, selector position, selector)] in the entry point's pair order."""
    return [(g, pos, s) for g, (_, selectors, _) in enumerate(case.gates) for pos, s in enumerate(selectors)]


def expected(case):
    """(counts per pair, every failure as (pair, event, cell) in the order (pair, event, cell)) from the model."""
    pair_index = {(g, pos): p for p, (g, pos, _) in enumerate(pairs_of(case))}
    errors = rm.selector_errors(1 << case.k, model_regions(case), case.gates, case.instance_lens)
    records = sorted((pair_index[(g, pos)], e, c) for (g, pos, e, c), _ in errors)
    counts = [0] * len(pair_index)
    for p, _, _ in records:
        counts[p] += 1
    return counts, records


def cap_of(case, cap) -> int:
    total = sum(expected(case)[0])
    return total if cap == EXACT else total - 1 if cap == ONE_LESS else cap


def arrays(case):
    """The arguments of `dev.cells_assigned_check` after k: n_planes, ranges, instance_lens, event rows, event regions, selector offsets,
    pair selectors, pair cells."""
    plane = lambda column: column[1] + (case.n_fixed if column[0] == "advice" else 0)
    code = lambda column: 0x80000000 | column[1] if column[0] == "instance" else plane(column)
    ranges = [(plane(column), first, count, r) for r, (_, rs, _) in enumerate(case.regions) for column, first, count in rs]
    rows, owners, offsets = [], [], [0]
    for s in range(case.n_selectors):
        for r, (_, _, enabled) in enumerate(case.regions):
            rows += enabled.get(s, [])
            owners += [r] * len(enabled.get(s, []))
        offsets.append(len(rows))
    pairs = pairs_of(case)
    return (case.n_fixed + case.n_advice, np.array(ranges, dtype=np.uint32).reshape(-1, 4), case.instance_lens, rows, owners, offsets,
            [s for _, _, s in pairs], [[(code(column), rot) for column, rot in case.gates[g][2]] for g, _, _ in pairs])
