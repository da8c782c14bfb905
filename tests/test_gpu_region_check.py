"""h2_cells_assigned_check on the device against tests/region_model.py: every case of tests/region_cases.py with exact counts and equal
records under every cap, every refusal with its outputs untouched, the conflict count, and the workspaces across an h2_trim."""
import ctypes as C

import numpy as np
import pytest

import halo2_amd as h
import region_cases as rc
from halo2_amd import _lib
from halo2_amd.dev import cells_assigned_check

pytestmark = pytest.mark.gpu


def _run(case, cap):
    return cells_assigned_check(case.k, *rc.arrays(case), cap)


def _agrees(case, cap):
    counts, records = rc.expected(case)
    got_counts, got_records, conflicts = _run(case, cap)
    assert got_counts.tolist() == counts, case.name
    assert [tuple(r) for r in got_records.tolist()] == records[:cap], (case.name, cap)
    assert conflicts == 0


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c.name)
def test_every_case_against_the_model(case):
    for cap in case.caps:
        _agrees(case, rc.cap_of(case, cap))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
SENTINEL = 0xA5A5A5A5


def _call(**over):
    """A valid small call (n = 16, one plane, one range, one instance column, two events, one pair of two cells) with some arguments
    replaced; -> (return code, whether any output changed)."""
    u32 = lambda *v: np.array(v, dtype=np.uint32)
    a = dict(log_len=4, n_planes=1, ranges=u32(0, 2, 3, 0), n_ranges=1, instance_lens=np.array([1], dtype=np.uint64), n_instance=1,
             event_rows=u32(2, 9), event_regions=u32(0, 0), selector_offsets=np.array([0, 2], dtype=np.uintp), n_selectors=1,
             pair_selector=u32(0), pair_cell_offsets=np.array([0, 2], dtype=np.uintp), n_pairs=1, cells=u32(0, 0, 0x80000000, 0),
             counts=np.full(1, SENTINEL, dtype=np.uint64), records=np.full(3 * 8, SENTINEL, dtype=np.uint32), max_records=8,
             n_records=C.c_size_t(SENTINEL), n_conflicts=C.c_uint64(SENTINEL))
    a.update(over)
    ptr = lambda v, kind: None if v is None else v.ctypes.data_as(C.POINTER(kind))
    ref = lambda v: None if v is None else C.byref(v)
    rc_ = h.lib().h2_cells_assigned_check(
        a["log_len"], a["n_planes"], ptr(a["ranges"], C.c_uint32), a["n_ranges"], ptr(a["instance_lens"], C.c_uint64), a["n_instance"],
        ptr(a["event_rows"], C.c_uint32), ptr(a["event_regions"], C.c_uint32), ptr(a["selector_offsets"], C.c_size_t), a["n_selectors"],
        ptr(a["pair_selector"], C.c_uint32), ptr(a["pair_cell_offsets"], C.c_size_t), a["n_pairs"], ptr(a["cells"], C.c_uint32),
        ptr(a["counts"], C.c_uint64), ptr(a["records"], C.c_uint32), a["max_records"], ref(a["n_records"]), ref(a["n_conflicts"]))
    outputs = [v for v in (a["counts"], a["records"]) if v is not None] + [np.array([v.value]) for v in (a["n_records"], a["n_conflicts"]) if v is not None]
    return rc_, any((v != SENTINEL).any() for v in outputs), a


def test_the_valid_call_of_the_refusal_table_answers():
    code, changed, a = _call()
    assert code == _lib.H2_OK and changed
    # event 0 (row 2): the plane cell is assigned, the instance cell (row 2 >= 1 value) is not; event 1 (row 9): neither
    assert a["counts"].tolist() == [3] and a["n_records"].value == 3 and a["n_conflicts"].value == 0
    assert a["records"][:9].reshape(3, 3).tolist() == [[0, 0, 1], [0, 1, 0], [0, 1, 1]]


U32 = lambda *v: np.array(v, dtype=np.uint32)
REFUSED = {
    "null ranges": dict(ranges=None),
    "null instance lengths": dict(instance_lens=None),
    "null event rows": dict(event_rows=None),
    "null event regions": dict(event_regions=None),
    "null selector offsets": dict(selector_offsets=None),
    "null pair selectors": dict(pair_selector=None),
    "null pair cell offsets": dict(pair_cell_offsets=None),
    "null cells": dict(cells=None),
    "null counts": dict(counts=None),
    "null records": dict(records=None),
    "null n_records": dict(n_records=None),
    "null n_conflicts": dict(n_conflicts=None),
    "log_len 31": dict(log_len=31),
    "a range past the last row": dict(ranges=U32(0, 14, 3, 0)),
    "a plane that does not exist": dict(ranges=U32(1, 2, 3, 0)),
    "a queried plane that does not exist": dict(cells=U32(1, 0, 0x80000000, 0)),
    "a queried instance column that does not exist": dict(cells=U32(0, 0, 0x80000001, 0)),
    "an event row past the last row": dict(event_rows=U32(2, 16)),
    "selector offsets that decrease": dict(selector_offsets=np.array([0, 2, 1], dtype=np.uintp), n_selectors=2),
    "selector offsets that do not start at 0": dict(selector_offsets=np.array([1, 2], dtype=np.uintp)),
    "cell offsets that decrease": dict(pair_cell_offsets=np.array([0, 2, 1], dtype=np.uintp), n_pairs=2, pair_selector=U32(0, 0),
                                       counts=np.full(2, SENTINEL, dtype=np.uint64)),
    "a selector that does not exist": dict(pair_selector=U32(1)),
    # 4 ranges of 2^30 cells: 2^32 cells in all, refused before anything is allocated
    "2^32 range cells": dict(log_len=30, ranges=U32(*([0, 0, 1 << 30, 0] * 4)), n_ranges=4),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refusals_leave_the_outputs_untouched(what):
    code, changed, _ = _call(**REFUSED[what])
    assert code == _lib.H2_ERR_ARGS and not changed, what


def test_two_regions_claiming_one_cell_is_one_conflict():
    # rows 2 .. 4 are region 0's, rows 4 .. 5 region 1's: whoever comes second to row 4 is the conflict; region 0 repeating rows 2 .. 3 is none
    k, ranges = 4, np.array([(0, 2, 3, 0), (0, 4, 2, 1), (0, 2, 2, 0)], dtype=np.uint32)
    counts, records, conflicts = cells_assigned_check(k, 1, ranges, [], [3, 5], [0, 1], [0, 2], [0], [[(0, 0)]], 16)
    assert conflicts == 1
    assert counts.tolist() == [0] and len(records) == 0                                       # rows 3 and 5 are each their region's


def test_answers_survive_regrowth_and_trim():
    """A small and a large call back to back (the workspaces grow), h2_trim (they are released), then the same two again."""
    small, large = rc.BY_NAME["nine-cells"], rc.BY_NAME["big-range"]
    assert small.k != large.k
    for _ in range(2):
        _agrees(small, 1024)
        _agrees(large, 4096)
        _agrees(small, 1024)
        assert h.lib().h2_trim() == _lib.H2_OK
