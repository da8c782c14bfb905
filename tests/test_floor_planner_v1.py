"""The V1 floor planner on the host: the model of the reference's strategy against a brute-force first fit, the shipped planner
against the model, layouts worked out by hand (the reference's own test among them), and both passes through `circuit.synthesize` -- where every cell,
selector bit, copy, table and constant lands.  Nothing here needs a device."""
import functools
import itertools

import numpy as np
import pytest

import halo2_amd as h
from halo2_amd import circuit as front
from halo2_amd import floor_planner as fp
from halo2_amd.circuit import ADVICE, FIXED, INSTANCE, Column, Selector

import floor_planner_cases as fc

FP = 0
A = fc.A


@functools.lru_cache(maxsize=None)
def _sequences():
    return fc.small_sequences()


@functools.lru_cache(maxsize=None)
def _model_on_sequences():
    return [fc.model_slot_in(shapes) for shapes in _sequences()]


def test_the_public_surface():
    assert h.V1 is fp.V1 and h.floor_planner is fp
    assert fp.SimpleFloorPlanner is front.SimpleFloorPlanner is h.SimpleFloorPlanner
    assert front.Circuit.floor_planner is fp.SimpleFloorPlanner


# ---- the model, then the planner against it --------------------------------------------------------------------------------------------------
def test_the_model_is_a_first_fit():
    """3000 seeded sequences of 1 to 14 regions, 1 to 5 columns, 1 to 9 rows: `slot_in` of the line-by-line port gives every region the
    lowest row at which all of its columns are free, as a search row by row does.  Most sequences place a region into a gap: a port
    that stops its scan at the first allocation beyond the window, and so loses the closing interval, fails here"""
    gaps = 0
    for shapes, (starts, _) in zip(_sequences(), _model_on_sequences()):
        assert starts == fc.brute_force_slot_in(shapes), shapes
        gaps += starts != fc.simple_starts(shapes)
    assert gaps > 1000


def test_the_planner_equals_the_model_on_the_small_sequences():
    for shapes, (starts, allocations) in zip(_sequences(), _model_on_sequences()):
        got = fp.slot_in(shapes)
        assert got[0] == starts and got[1] == allocations, shapes
        assert fp.slot_in_biggest_advice_first(shapes) == fc.model_slot_in_biggest_advice_first(shapes), shapes


def test_the_planner_equals_the_model_on_1500_regions():
    """1 to 4 advice columns out of 10, 1 to 40 rows: starts, allocations and the first unassigned row"""
    shapes = fc.random_regions(1500)
    want_starts, want_allocations = fc.model_slot_in_biggest_advice_first(shapes)
    starts, allocations = fp.slot_in_biggest_advice_first(shapes)
    assert starts == want_starts and allocations == want_allocations
    assert fp.first_unassigned_row(allocations) == fc.rows_used(starts, shapes) < fc.rows_used(fc.simple_starts(shapes), shapes)
    in_order = fp.slot_in(shapes)
    assert in_order == fc.model_slot_in(shapes)


# ---- fixed expectations -----------------------------------------------------------------------------------------------------------------------
def test_the_references_own_case():
    assert fp.slot_in(fc.REFERENCE_SHAPES)[0] == [0, 0, 15] == fc.model_slot_in(fc.REFERENCE_SHAPES)[0]


def test_equal_areas_place_the_higher_index_first():
    starts, allocations = fp.slot_in_biggest_advice_first(fc.TIE_SHAPES)
    assert starts == [8, 4, 0] == fc.model_slot_in_biggest_advice_first(fc.TIE_SHAPES)[0]
    assert allocations == {A[0]: [(0, 4), (4, 4), (8, 4)]}


def _gap_layouter(circuit, k=6, **kw):
    kw = dict(dict(fixed=True, advice=True, instances=[[fc.GapCircuit.INSTANCE]]), **kw)
    return front.synthesize(circuit, k, FP, **kw)


def test_the_gap_circuits_shapes():
    _, _, simple = _gap_layouter(fc.GapCircuit())
    _, _, v1 = _gap_layouter(fc.GapCircuitV1())
    assert simple.shapes == v1.shapes
    assert [(sorted(c.index for c in columns if isinstance(c, Column)), rows) for columns, rows in v1.shapes] == \
        [([0, 1], 15), ([2], 10), ([0, 2], 10), ([2], 5)]
    assert simple.regions == fc.GapCircuit.SIMPLE_STARTS == fc.simple_starts(simple.shapes) and fc.rows_used(simple.regions, simple.shapes) == 30
    assert v1.regions == fc.GapCircuit.V1_STARTS == fp.slot_in_biggest_advice_first(v1.shapes)[0] and fc.rows_used(v1.regions, v1.shapes) == 25
    assert isinstance(v1, fp.AssignmentPass) and v1.cs is not None


def test_a_region_without_columns_starts_at_zero():
    shapes = [([A[0]], 3), ([], 0), ([A[0]], 2), ([], 5)]
    assert fp.slot_in(shapes) == ([0, 0, 3, 0], {A[0]: [(0, 3), (3, 2)]}) == fc.model_slot_in(shapes)
    assert fp.slot_in([]) == ([], {}) and fp.first_unassigned_row({}) == 0
    with pytest.raises(ValueError):
        fp.slot_in([([A[0]], 0)])


# ---- column order and column kind ---------------------------------------------------------------------------------------------------------------
def test_column_order_and_kind():
    """A region's columns are visited Instance, Advice, Fixed, each by index, then the selectors by index.  What the order can and
    cannot change: the first fit is the lowest row at which EVERY column is free, so the start of a region is the same whichever
    column the search begins with -- the model is run over all 120 orders of a five-column region to show it -- and no case exists in
    which the order alone moves a start.  What does move a start is the KIND of a column: only advice columns count towards the
    area the regions are sorted by.  Below, a fixed column counted as advice would place the first region first."""
    mixed = [Selector(1), Column(FIXED, 0), Column(ADVICE, 1), Selector(0), Column(INSTANCE, 0), Column(ADVICE, 0), Column(FIXED, 1)]
    want = [Column(INSTANCE, 0), Column(ADVICE, 0), Column(ADVICE, 1), Column(FIXED, 0), Column(FIXED, 1), Selector(0), Selector(1)]
    assert sorted(mixed, key=fp.column_order) == want == sorted(mixed, key=fc.region_column_ord)
    five = [Selector(0), Column(FIXED, 0), Column(ADVICE, 1), Column(INSTANCE, 0), Column(ADVICE, 0)]
    before = [([five[0]], 2), ([five[1]], 5), ([five[2]], 3), ([five[1], five[3]], 4), ([five[4]], 1), ([five[0]], 3), (five, 3)]
    starts, allocations = fp.slot_in(before)
    assert starts == [0, 0, 0, 5, 0, 2, 9] and list(allocations)[:3] == [Selector(0), Column(FIXED, 0), Column(ADVICE, 1)]
    for order in itertools.permutations(five):
        got = fc.model_slot_in(before, column_key=lambda c, order=order: order.index(c) if c in order else -1)
        assert got[0] == starts and got[1] == allocations
    kinds = [([A[0], Column(FIXED, 0)], 6), ([A[0]], 7)]                         # areas 6 and 7: the second region goes first
    assert fp.advice_area(kinds[0]) == 6 and fp.advice_area(([Column(INSTANCE, 0), Selector(3)], 9)) == 0
    assert fp.slot_in_biggest_advice_first(kinds)[0] == [7, 0] == fc.model_slot_in_biggest_advice_first(kinds)[0]
    assert fp.slot_in(kinds)[0] == [0, 6]


# ---- through circuit.synthesize -------------------------------------------------------------------------------------------------------------------
def _column(assembly, cells, column):
    return cells[column.index].integers(assembly.n, FP)


def test_every_cell_of_the_gap_circuit_sits_at_its_regions_start():
    log = []
    cs, assembly, layouter = _gap_layouter(fc.GapCircuitV1(log=log))
    s = layouter.regions
    assert s == [0, 0, 15, 10]
    a0, a1, a2 = (_column(assembly, assembly.advice, Column(ADVICE, i)) for i in range(3))
    want0, want1, want2 = [0] * 64, [0] * 64, [0] * 64
    want0[s[0]:s[0] + 15] = range(1, 16)
    want1[s[0]:s[0] + 15] = [v * v for v in range(1, 16)]
    want2[s[1]:s[1] + 10] = range(100, 110)
    want0[s[2]:s[2] + 10] = range(5, 15)
    want2[s[2]:s[2] + 10] = range(10, 30, 2)
    want2[s[3]:s[3] + 5] = range(7, 12)
    assert (a0, a1, a2) == (want0, want1, want2)
    # no two regions share a cell: every advice cell was assigned once, and the columns hold all 15 + 15 + 10 + 10 + 10 + 5 of them
    assert sum(v != 0 for v in a0 + a1 + a2) == 65
    for (ci, ri), (cj, rj) in itertools.combinations(zip(layouter.shapes, s), 2):
        if set(ci[0]) & set(cj[0]):
            assert ri + ci[1] <= rj or rj + cj[1] <= ri
    # selector bits: pair on all 15 rows, count on all but the last row of its two regions, cross on all 10
    rows = lambda i: set(int(r) for r in np.flatnonzero(assembly.selectors[i]))
    assert rows(0) == set(range(s[0], s[0] + 15))
    assert rows(1) == set(range(s[1], s[1] + 9)) | set(range(s[3], s[3] + 4))
    assert rows(2) == set(range(s[2], s[2] + 10))
    # copies: a0 of the cross region's first row <-> the fifth pair row; the last cross a2 <-> instance row 0; the constant <-> a2
    n = assembly.n
    columns = cs.permutation_columns
    flat = lambda column, row: columns.index(column) * n + row
    mapping = assembly.permutation.mapping
    cycles = {frozenset((i, int(mapping[i]))) for i in range(len(mapping)) if int(mapping[i]) != i}
    constants = cs.constants[0]
    assert cycles == {frozenset((flat(Column(ADVICE, 0), s[2]), flat(Column(ADVICE, 0), s[0] + 4))),
                      frozenset((flat(Column(ADVICE, 2), s[2] + 9), flat(Column(INSTANCE, 0), 0))),
                      frozenset((flat(constants, 0), flat(Column(ADVICE, 2), s[3])))}
    assert _column(assembly, assembly.fixed, constants)[:3] == [7, 0, 0]
    # the passes: one copy without witnesses, and only the circuit WITH witnesses had a value closure called, once per advice cell
    # that is not a copy or a constant
    assert log.count(("without_witnesses",)) == 1
    assert [e for e in log if e[0] == "value"] == [("value", True)] * 63


def test_the_measurement_pass_of_keygen_calls_no_closure_either():
    log = []
    _gap_layouter(fc.GapCircuitV1(log=log).without_witnesses(), fixed=True, advice=False, instances=None)
    assert [e for e in log if e[0] == "value"] == []


def test_tables_are_assigned_once():
    calls = []
    cs, assembly, layouter = front.synthesize(fc.TableCircuit(calls), fc.TableCircuit.K, FP, fixed=True, advice=True, instances=[])
    assert calls == ["table"]
    assert layouter.regions == [5, 0] and len(layouter.table_columns) == 1
    assert _column(assembly, assembly.fixed, Column(FIXED, 0))[:10] == [0, 1, 2, 3, 4, 5, 6, 7, 0, 0]
    assert _column(assembly, assembly.advice, Column(ADVICE, 0))[:9] == [7, 6, 5, 4, 3, 0, 1, 2, 0]


class _ManyConstants(fc.Circuit):
    """two constants columns, the first used by a region on rows 1 and 2 of four: the free rows are (c0, 0), (c0, 3), then c1's"""
    floor_planner = fp.V1

    def without_witnesses(self):
        return _ManyConstants()

    @staticmethod
    def configure(meta):
        advice, c0, c1 = meta.advice_column(), meta.fixed_column(), meta.fixed_column()
        meta.enable_equality(advice)
        meta.enable_constant(c0)
        meta.enable_constant(c1)
        return advice, c0, c1

    def synthesize(self, config, layouter):
        advice, c0, c1 = config

        def used(region):
            region.assign_fixed(c0, 0, lambda: 50)
            region.assign_fixed(c0, 1, lambda: 51)
        layouter.assign_region("four constants", lambda region: [region.assign_advice_from_constant(advice, i, 10 + i) for i in range(4)])
        layouter.assign_region("two fixed cells", used)
        layouter.assign_region("a fifth constant", lambda region: region.assign_advice_from_constant(advice, 0, 20))


def test_constants_land_on_the_planned_rows_in_order():
    """regions: advice x 4 at 0; {c0} x 2 (no advice: placed last) at 0; advice x 1 at 4.  first_unassigned_row is 5, c0 is free on rows
    2, 3, 4 and c1 throughout: the five constants, in pass order, take (c0, 2), (c0, 3), (c0, 4), (c1, 0), (c1, 1)"""
    cs, assembly, layouter = front.synthesize(_ManyConstants(), 4, FP, fixed=True, advice=True, instances=[])
    assert layouter.regions == [0, 0, 4]
    assert [(c.row_offset, k) for k, c in layouter.constants] == [(0, 10), (1, 11), (2, 12), (3, 13), (0, 20)]
    assert _column(assembly, assembly.fixed, Column(FIXED, 0))[:6] == [50, 51, 10, 11, 12, 0]
    assert _column(assembly, assembly.fixed, Column(FIXED, 1))[:3] == [13, 20, 0]
    allocations = fp.slot_in_biggest_advice_first(layouter.shapes)[1]
    assert list(fp.constant_positions(allocations, cs.constants, 5))[:5] == \
        [(Column(FIXED, 0), 2), (Column(FIXED, 0), 3), (Column(FIXED, 0), 4), (Column(FIXED, 1), 0), (Column(FIXED, 1), 1)]
    n, columns, mapping = assembly.n, cs.permutation_columns, assembly.permutation.mapping
    flat = lambda column, row: columns.index(column) * n + row
    for fixed, advice_row in [((Column(FIXED, 0), 2), 0), ((Column(FIXED, 0), 4), 2), ((Column(FIXED, 1), 0), 3), ((Column(FIXED, 1), 1), 4)]:
        assert int(mapping[flat(*fixed)]) == flat(Column(ADVICE, 0), advice_row)


# ---- errors ---------------------------------------------------------------------------------------------------------------------------------------
def test_not_enough_columns_for_constants():
    with pytest.raises(front.NotEnoughColumnsForConstants):
        front.synthesize(fc.NoConstantsColumnCircuit(), 4, FP, fixed=True, advice=True, instances=[])
    with pytest.raises(front.NotEnoughColumnsForConstants):
        front.synthesize(fc.NoConstantsColumnCircuit(), 4, FP, fixed=True, advice=False)


def test_a_constants_column_filled_below_the_first_unassigned_row():
    _, assembly, layouter = front.synthesize(fc.FilledConstantsColumnCircuit(), 4, FP, fixed=True, advice=True, instances=[])
    assert layouter.regions == [0] and _column(assembly, assembly.fixed, Column(FIXED, 0))[:6] == [0, 1, 2, 3, 9, 0]
    with pytest.raises(front.NotEnoughColumnsForConstants):
        front.synthesize(fc.FilledConstantsColumnCircuitV1(), 4, FP, fixed=True, advice=True, instances=[])


def test_v1_fits_where_the_single_pass_runs_out_of_rows():
    cs = front.ConstraintSystem(fc.M)
    fc.GapCircuit.configure(cs)
    usable = (1 << fc.GapCircuit.K) - (cs.blinding_factors() + 1)
    assert 25 <= usable < 30
    with pytest.raises(front.NotEnoughRowsAvailable):
        _gap_layouter(fc.GapCircuit(), k=fc.GapCircuit.K)
    _, assembly, layouter = _gap_layouter(fc.GapCircuitV1(), k=fc.GapCircuit.K)
    assert assembly.usable == usable and fc.rows_used(layouter.regions, layouter.shapes) == 25


def test_a_second_pass_with_one_more_region():
    with pytest.raises(front.Synthesis):
        front.synthesize(fc.OneMoreRegionCircuit(), 4, FP, fixed=True, advice=True, instances=[])
    with pytest.raises(front.Synthesis):
        front.synthesize(fc.OneMoreRegionCircuit(), 4, FP, fixed=True, advice=False)
