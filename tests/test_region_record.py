"""What `circuit.synthesize(..., regions=True)` records (dev.rs:42-73, :314-461): one `RegionRecord` per region and table in enter
order, extents from assignments alone, selectors as absolute rows in enable order, cells as ranges; constants placed by the layouter
and table fills in no region; the same under `V1` at the planner's starts; nothing else changed by recording.  CPU only."""
import importlib.util
import os

import numpy as np

from halo2_amd import circuit as front
from halo2_amd.circuit import ADVICE, FIXED, Circuit, Column, Value
from halo2_amd.floor_planner import V1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP = 0
VECTOR = 300


def _example():
    spec = importlib.util.spec_from_file_location("unassigned_cell", os.path.join(ROOT, "examples", "unassigned_cell.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class RecordCircuit(Circuit):
    """Five brackets: a two-cell region, a region with one vector of 300 cells and a selector on every other row, a region with a cell
    constrained to a constant, a table, and a last region.  `floor_planner` is set by the subclasses."""
    K = 10

    def without_witnesses(self):
        return type(self)()

    @staticmethod
    def configure(meta):
        a, b = meta.advice_column(), meta.advice_column()
        constants = meta.fixed_column()
        meta.enable_constant(constants)
        meta.enable_equality(a)
        s = meta.selector()
        table = meta.lookup_table_column()
        meta.create_gate("g", lambda q: [q.query_selector(s) * (q.query_advice(a, 0) - q.query_advice(b, 0))])
        meta.lookup(lambda q: [(q.query_advice(b, 0), table)])
        return dict(a=a, b=b, s=s, table=table, constants=constants)

    def synthesize(self, cfg, layouter):
        a, b, s = cfg["a"], cfg["b"], cfg["s"]

        def small(region):
            region.assign_advice(b, 1, lambda: Value.known(2))
            region.assign_advice(a, 0, lambda: Value.known(1))
        layouter.assign_region("small", small)

        def vector(region):
            region.assign_advice_column(a, 0, np.zeros((VECTOR, 4), dtype=np.uint64))
            region.enable_selector_rows(s, np.arange(0, VECTOR, 2)[::-1])
            region.assign_advice(b, VECTOR - 1, lambda: Value.known(0))
        layouter.assign_region(lambda: "vector", vector)
        layouter.assign_region("constant", lambda region: region.assign_advice_from_constant(a, 0, 7))
        layouter.assign_table("the table", lambda t: [t.assign_cell(cfg["table"], i, lambda i=i: Value.known(i)) for i in range(4)])

        def last(region):
            s.enable(region, 0)
            region.assign_advice(a, 0, lambda: Value.known(3))
            region.assign_advice(b, 0, lambda: Value.known(3))
            region.assign_advice(b, 0, lambda: Value.known(3))
        layouter.assign_region("last", last)


class RecordCircuitV1(RecordCircuit):
    floor_planner = V1


A, B, CONSTANTS, TABLE = Column(ADVICE, 0), Column(ADVICE, 1), Column(FIXED, 0), Column(FIXED, 1)


def _plain(record):
    return (record.index, record.name, record.columns, record.rows, record.enabled_selectors, record.cells)


def test_the_record_of_unassigned_cell():
    mod = _example()
    _, assembly, _ = front.synthesize(mod.FaultyCircuit(), mod.K, FP, fixed=True, advice=True, instances=[], regions=True)
    assert [_plain(r) for r in assembly.regions] == [(0, "Faulty synthesis", {A}, (0, 0), {0: [1]}, [(A, 0, 1)])]
    _, fixed, _ = front.synthesize(mod.FaultyCircuit(forget_b=False), mod.K, FP, fixed=True, advice=True, instances=[], regions=True)
    assert [_plain(r) for r in fixed.regions] == [(0, "Faulty synthesis", {A, B}, (0, 1), {0: [1]}, [(A, 0, 1), (B, 1, 1)])]
    assert assembly.current_region is None


def test_single_pass_records():
    cs, assembly, layouter = front.synthesize(RecordCircuit(), RecordCircuit.K, FP, fixed=True, advice=True, instances=[], regions=True)
    assert layouter.regions == [0, 2, 2 + VECTOR, 3 + VECTOR]
    small, vector, constant, table, last = assembly.regions
    assert _plain(small) == (0, "small", {A, B}, (0, 1), {}, [(B, 1, 1), (A, 0, 1)])
    # a vector of 300 cells is ONE range; the selector's rows are absolute and in enable order; enabling extends nothing
    assert _plain(vector) == (1, "vector", {A, B}, (2, 1 + VECTOR), {0: list(range(2 + VECTOR - 2, 1, -2))}, [(A, 2, VECTOR), (B, 1 + VECTOR, 1)])
    assert len(vector.enabled_selectors[0]) == VECTOR // 2
    # the constant 7 goes into the constants column after exit_region: the region holds the advice cell alone, and no region the fixed one
    assert _plain(constant) == (2, "constant", {A}, (2 + VECTOR, 2 + VECTOR), {}, [(A, 2 + VECTOR, 1)])
    assert assembly.host_columns(assembly.fixed)[CONSTANTS.index][0] == 7
    assert not any(column == CONSTANTS for r in assembly.regions for column, _, _ in r.cells)
    # a table is a region under its name with its fixed cells; the fill below it (rows 4 .. usable) is not recorded
    assert _plain(table) == (3, "the table", {TABLE}, (0, 3), {}, [(TABLE, i, 1) for i in range(4)])
    # a cell assigned twice is listed twice
    assert _plain(last) == (4, "last", {A, B}, (3 + VECTOR, 3 + VECTOR), {0: [3 + VECTOR]}, [(A, 3 + VECTOR, 1), (B, 3 + VECTOR, 1), (B, 3 + VECTOR, 1)])
    assert repr(small).startswith("RegionRecord(0, 'small'")


def test_v1_gives_the_same_records_at_the_planners_starts():
    _, simple, simple_layouter = front.synthesize(RecordCircuit(), RecordCircuit.K, FP, fixed=True, advice=True, instances=[], regions=True)
    _, planned, plan = front.synthesize(RecordCircuitV1(), RecordCircuit.K, FP, fixed=True, advice=True, instances=[], regions=True)
    assert plan.regions != simple_layouter.regions and plan.regions[1] == 0                   # the vector has the largest advice area: first fit at row 0
    assert [(r.index, r.name) for r in planned.regions] == [(r.index, r.name) for r in simple.regions]      # the order of the assign_region calls
    starts = lambda layouter: layouter.regions[:3] + [0] + layouter.regions[3:]                # the table is a bracket, not one of the planner's regions
    for old, new, was, now in zip(simple.regions, planned.regions, starts(simple_layouter), starts(plan)):
        shift = now - was
        assert new.columns == old.columns and new.rows == (old.rows[0] + shift, old.rows[1] + shift)
        assert new.cells == [(column, first + shift, count) for column, first, count in old.cells]
        assert new.enabled_selectors == {s: [row + shift for row in rows] for s, rows in old.enabled_selectors.items()}
    assert not any(column == CONSTANTS for r in planned.regions for column, _, _ in r.cells)
    assert planned.host_columns(planned.fixed)[CONSTANTS.index].count(7) == 1


def test_nothing_is_recorded_or_changed_without_the_keyword():
    for circuit in (RecordCircuit, RecordCircuitV1):
        _, off, layouter_off = front.synthesize(circuit(), RecordCircuit.K, FP, fixed=True, advice=True, instances=[])
        _, on, layouter_on = front.synthesize(circuit(), RecordCircuit.K, FP, fixed=True, advice=True, instances=[], regions=True)
        assert off.regions is None and off.current_region is None and len(on.regions) == 5
        assert layouter_off.regions == layouter_on.regions
        assert off.host_columns(off.fixed) == on.host_columns(on.fixed) and off.host_columns(off.advice) == on.host_columns(on.advice)
        assert np.array_equal(off.selectors, on.selectors) and np.array_equal(off.permutation.mapping, on.permutation.mapping)
        off.enter_region("ignored")                                                           # both are no-ops unless recording
        off.exit_region()
        assert off.regions is None and off.current_region is None


def test_fill_from_row_inside_a_region_is_the_regions():
    """dev.rs:452-466 assigns the fill row by row through assign_fixed: inside a bracket the rows are the region's cells (the layouters
    fill after exit_region, so theirs are nobody's)."""
    _, assembly, _ = front.synthesize(RecordCircuit(), RecordCircuit.K, FP, fixed=True, advice=True, instances=[], regions=True)
    assembly.enter_region("by hand")
    assembly.fill_from_row(TABLE, 10, lambda: Value.known(0))
    assembly.exit_region()
    assert _plain(assembly.regions[-1]) == (5, "by hand", {TABLE}, (10, assembly.usable - 1), {}, [(TABLE, 10, assembly.usable - 10)])
