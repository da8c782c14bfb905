"""The circuit front-end on the host (halo2_amd/circuit.py, halo2_amd/compress_selectors.py): configure, the single-pass floor
planner, the copy-constraint assembly, lowering, the pinned Debug print, selector compression's grouping, `Assigned`.  No device:
cells are evaluated on the host (`Assembly.host_columns`)."""
import importlib.util
import os
import random

import numpy as np
import pytest

from halo2_amd import circuit as front
from halo2_amd import compress_selectors, fields
from halo2_amd.circuit import (Assigned, Circuit, ConstraintSystem, Expression, NotEnoughColumnsForConstants, NotEnoughRowsAvailable,
                               TableError, Value, lower)
from halo2_amd.plonk import ConstraintSystem as Lowered
from oracle import pasta as o
from oracle import plonk_api as pa

from circuit_cases import FP, M, PLONK_API_A, PlonkApiCircuit, SelectorCircuit, SimpleExampleCircuit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _RandomCells:
    """A lowered expression's cells as fixed random field elements, the same for every expression asked."""

    def __init__(self, seed):
        self.rng, self.values = random.Random(seed), {}

    def _get(self, key):
        if key not in self.values:
            self.values[key] = self.rng.randrange(M)
        return self.values[key]

    def fixed(self, col, rot=0):
        return self._get(("fixed", col, rot))

    def advice(self, col, rot=0):
        return self._get(("advice", col, rot))

    def instance(self, col, rot=0):
        return self._get(("instance", col, rot))


def _same_expressions(got, want, seeds=(1, 2, 3)):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for seed in seeds:
            assert int(g(_RandomCells(seed))) % M == int(w(_RandomCells(seed))) % M


def _same_system(low, want):
    for name in ("num_fixed_columns", "num_advice_columns", "num_instance_columns", "advice_queries", "instance_queries", "fixed_queries",
                 "permutation_columns", "degree", "blinding_factors"):
        assert getattr(low, name) == getattr(want, name), name
    _same_expressions(low.gates, want.gates)
    assert len(low.lookups) == len(want.lookups)
    for (gi, gt), (wi, wt) in zip(low.lookups, want.lookups):
        _same_expressions(gi, wi)
        _same_expressions(gt, wt)


@pytest.fixture(scope="module")
def plonk_api():
    return front.synthesize(PlonkApiCircuit().without_witnesses(), pa.K, FP, fixed=True, advice=False)


def test_plonk_api_layout_equals_the_restated_keygen(plonk_api):
    cs, assembly, _ = plonk_api
    fixed, mapping = pa.keygen_columns(o.P)
    assert assembly.host_columns(assembly.fixed) == fixed
    assert assembly.permutation.pairs() == mapping                    # cell for cell: `copy` merges cycles in the reference's order
    assert cs.num_selectors == 0 and cs.blinding_factors() == 5 and cs.degree() == 4 and cs.minimum_rows() == 8
    _same_system(lower(cs), pa.constraint_system(Lowered))


def test_plonk_api_pinned_constraint_system_text(plonk_api, golden_dir):
    cs = plonk_api[0]
    compact = pa.compact_debug(open(os.path.join(golden_dir, "plonk_api_pinned_vk.txt")).read())
    start = compact.index("cs: PinnedConstraintSystem {") + len("cs: ")
    end = compact.index(", fixed_commitments: [")
    assert cs.pinned() == compact[start:end]
    # and the whole key's text and its transcript_repr, given the reference's own commitments
    from test_reference_goldens import PINNED

    class _Params:
        curve = 1
    domain = type("D", (), {"k": 5, "extended_k": 7, "omega": o.omega_for(o.P, 5)})
    text = front.pinned_verification_key(_Params, domain, cs, PINNED[:7], PINNED[7:])
    assert text == compact
    assert front.transcript_repr(text, o.P) == pa.transcript_repr(compact)


def test_plonk_api_too_few_rows():
    for k in (1, pa.K - 1):                                           # plonk_api.rs:411-429
        with pytest.raises(NotEnoughRowsAvailable) as e:
            front.synthesize(PlonkApiCircuit().without_witnesses(), k, FP, fixed=True, advice=False)
        assert e.value.current_k == k


def test_plonk_api_witness_equals_the_restated_witness():
    adv, _ = pa.witness(o.P)
    for rational in (False, True):
        _, assembly, _ = front.synthesize(PlonkApiCircuit(PLONK_API_A, rational=rational), pa.K, FP,
                                          fixed=False, advice=True, instances=[[2]])
        assert assembly.host_columns(assembly.advice) == adv
        assert any(c.rational for c in assembly.advice) == rational


def _simple_example():
    spec = importlib.util.spec_from_file_location("simple_example", os.path.join(ROOT, "examples", "simple_example.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _partition(mapping, n_columns, n):
    """The copy cycles as a set of frozensets of cells."""
    seen, cycles = set(), set()
    for c in range(n_columns):
        for r in range(n):
            if (c, r) in seen:
                continue
            cycle, cell = [], (c, r)
            while cell not in cycle:
                cycle.append(cell)
                cell = tuple(mapping[cell[0]][cell[1]])
            seen |= set(cycle)
            if len(cycle) > 1:
                cycles.add(frozenset(cycle))
    return cycles


def test_simple_example_equals_the_hand_lowered_example():
    k, n = 4, 16
    a, b, constant = 2, 3, 7
    want_advice, want_fixed, want_mapping, c = _simple_example().build(M, n, a, b, constant)
    cs, assembly, _ = front.synthesize(SimpleExampleCircuit(constant, a, b), k, FP, fixed=True, advice=True, instances=[[c]])
    assert assembly.host_columns(assembly.advice) == want_advice
    assert assembly.host_columns(assembly.fixed) == want_fixed[:1]
    assert [list(np.flatnonzero(s)) for s in assembly.selectors] == [[3, 5, 7]]
    assert _partition(assembly.permutation.pairs(), 4, n) == _partition(want_mapping, 4, n)
    combinations = cs.compress_selectors([[0]])
    assert combinations == [[(0, 1)]] and cs.num_fixed_columns == 2
    want = Lowered(num_fixed_columns=2, num_advice_columns=2, num_instance_columns=1,
                   gates=[lambda q: q.fixed(1) * (q.advice(0) * q.advice(1) - q.advice(0, 1))],
                   advice_queries=[(0, 0), (1, 0), (0, 1)], instance_queries=[(0, 0)], fixed_queries=[(0, 0), (1, 0)],
                   permutation_columns=[("instance", 0), ("fixed", 0), ("advice", 0), ("advice", 1)], degree=3, blinding_factors=5)
    _same_system(lower(cs), want)
    assert cs.polynomials()[0].debug() == ("Product(Fixed { query_index: 1, column_index: 1, rotation: Rotation(0) }, Sum(Product("
                                           "Advice { query_index: 0, column_index: 0, rotation: Rotation(0) }, Advice { query_index: 1, "
                                           "column_index: 1, rotation: Rotation(0) }), Negated(Advice { query_index: 2, column_index: 0, "
                                           "rotation: Rotation(1) })))")


# ---- selector compression: worked cases for `process`, degree bound 3 ---------------------------------------------------------------------
def _process(degrees, conflict_pairs, max_degree=3):
    s = len(degrees)
    conflicts = [[(i, j) in conflict_pairs or (j, i) in conflict_pairs for j in range(s)] for i in range(s)]
    allocated = []

    def allocate():
        allocated.append(Expression("Fixed", len(allocated), len(allocated), 0))
        return allocated[-1]
    descriptions = [compress_selectors.SelectorDescription(i, d) for i, d in enumerate(degrees)]
    combinations, assignments = compress_selectors.process(descriptions, conflicts, max_degree, allocate)
    return combinations, {a.selector: a for a in assignments}, assignments


def _q(c):
    return f"Fixed {{ query_index: {c}, column_index: {c}, rotation: Rotation(0) }}"


def _const(v):
    return "Constant(0x" + format(v, "064x") + ")"


def test_process_three_disjoint_selectors():
    combinations, by, _ = _process([2, 2, 2], set())
    assert combinations == [[(0, 1), (1, 2)], [(2, 1)]]               # the loop breaks at d + len == max_degree
    assert by[0].expression.debug() == f"Product({_q(0)}, Sum({_const(2)}, Negated({_q(0)})))"      # q (2 - q)
    assert by[1].expression.debug() == f"Product({_q(0)}, Sum({_const(1)}, Negated({_q(0)})))"      # q (1 - q)
    assert by[2].expression.debug() == _q(1)
    assert (by[0].combination_index, by[1].combination_index, by[2].combination_index) == (0, 0, 1)


def test_process_conflict_moves_the_partner():
    combinations, _, _ = _process([2, 2, 2], {(0, 1)})
    assert combinations == [[(0, 1), (2, 2)], [(1, 1)]]


def test_process_degree_zero_selectors_come_first():
    combinations, by, order = _process([2, 0, 2, 0], set())           # selector 1: complex, selector 3: in no gate
    assert combinations == [[(1, 1)], [(3, 1)], [(0, 1), (2, 2)]]
    assert [a.selector for a in order] == [1, 3, 0, 2]
    assert by[1].expression.debug() == _q(0) and by[3].expression.debug() == _q(1)


def test_process_full_degree_never_shares():
    combinations, by, _ = _process([3, 2, 2], set())
    assert combinations == [[(0, 1)], [(1, 1), (2, 2)]]
    assert by[0].expression.debug() == _q(0)


def test_process_properties_on_random_cases():
    """The two properties of the reference's own unit test (compress_selectors.rs:229-): every substituted expression is non-zero
    exactly on its selector's rows, and no gate's degree passes the bound."""
    rng = random.Random(0xC0FFEE)
    n = 64
    for _ in range(50):
        s = rng.randrange(1, 13)
        max_degree = rng.randrange(2, 7)
        degrees = [rng.randrange(0, max_degree + 1) for _ in range(s)]
        density = rng.choice([0.02, 0.1, 0.5])
        act = np.array([[rng.random() < density for _ in range(n)] for _ in range(s)], dtype=bool)
        pairs = {(i, j) for i in range(s) for j in range(i) if (act[i] & act[j]).any()}
        combinations, by, _ = _process(degrees, pairs, max_degree)
        assert sorted(sel for members in combinations for sel, _ in members) == list(range(s))
        columns = np.zeros((len(combinations), n), dtype=np.int64)
        for c, members in enumerate(combinations):
            for sel, root in members:
                assert not (columns[c][act[sel]]).any()               # disjoint within a column
                columns[c][act[sel]] = root
        for sel in range(s):
            e = by[sel].expression
            for r in range(n):
                value = e.evaluate(lambda c: c % M, None, lambda q: int(columns[q[1]][r]), None, None, lambda a: -a % M,
                                   lambda a, b: (a + b) % M, lambda a, b: a * b % M, lambda a, f: a * f % M)
                assert (value != 0) == bool(act[sel][r])
            if degrees[sel]:
                assert degrees[sel] - 1 + e.degree() <= max_degree


def test_selector_circuit_compression_through_the_constraint_system():
    cs, assembly, _ = front.synthesize(SelectorCircuit().without_witnesses(), SelectorCircuit.K, FP, fixed=True, advice=False)
    act = assembly.selectors
    conflicts = [[bool((act[i] & act[j]).any()) and i != j for j in range(6)] for i in range(6)]
    assert cs.selector_degrees() == [2, 3, 3, 2, 2, 0] and cs.degree() == 3
    combinations = cs.compress_selectors(conflicts)
    assert combinations == [[(5, 1)], [(0, 1), (4, 2)], [(1, 1)], [(2, 1)], [(3, 1)]]
    assert cs.num_fixed_columns == 5 and max(p.degree() for p in cs.polynomials()) == 3
    assert "Selector" not in cs.pinned()
    with pytest.raises(ValueError):
        lower(front.synthesize(SelectorCircuit().without_witnesses(), 6, FP, True, False)[0]).gates[0](_RandomCells(1))


# ---- Expression rules -----------------------------------------------------------------------------------------------------------------------
def test_expression_selector_rules_and_degree():
    cs = ConstraintSystem(M)
    a = cs.advice_column()
    s, t, cx = cs.selector(), cs.selector(), cs.complex_selector()
    made = {}

    def gate(q):
        made.update(a=q.query_advice(a, 0), s=q.query_selector(s), t=q.query_selector(t), cx=q.query_selector(cx))
        return [made["s"] * made["a"]]
    cs.create_gate("g", gate)
    ea, es, et, ecx = made["a"], made["s"], made["t"], made["cx"]
    for bad in (lambda: es + ea, lambda: ea - es, lambda: es * et, lambda: (es * ea) * (et * ea)):
        with pytest.raises(ValueError):
            bad()
    assert (ecx + ea).degree() == 1 and (ecx * es * ea).degree() == 3 and (ea * 5).degree() == 1 and Expression.constant(3).degree() == 0
    assert (es * ea).extract_simple_selector() == s and (ecx * ea).extract_simple_selector() is None
    with pytest.raises(ValueError):
        cs.lookup(lambda q: [(q.query_selector(s) * q.query_advice(a, 0), cs.lookup_table_column())])
    assert (ea * 5).debug(M) == ("Scaled(Advice { query_index: 0, column_index: 0, rotation: Rotation(0) }, 0x" + format(5, "064x") + ")")
    assert es.debug() == "Selector(Selector(0, true))" and ecx.debug() == "Selector(Selector(2, false))"
    assert (-ea).debug() == "Negated(Advice { query_index: 0, column_index: 0, rotation: Rotation(0) })"


# ---- Assigned (assigned.rs:368-) --------------------------------------------------------------------------------------------------------------
def test_assigned_inverse_of_zero_identities():
    T, R, Z = (lambda x: Assigned.trivial(x, M)), (lambda a, b: Assigned.rational(a, b, M)), Assigned.zero(M)
    inv0 = R(1, 0)
    for a in (T(2), R(1, 2)):                                         # add_{trivial,rational}_to_inv0_rational
        assert (a + inv0).evaluate() == a.evaluate() and (inv0 + a).evaluate() == a.evaluate()
        assert (a - inv0).evaluate() == a.evaluate() and (inv0 - a).evaluate() == (-a).evaluate()       # sub_*_from_inv0_rational
        assert (a * inv0).evaluate() == 0 and (inv0 * a).evaluate() == 0                                # mul_*_by_inv0_rational
    assert (inv0 + inv0).evaluate() == 0 and inv0.evaluate() == 0 and inv0.is_zero_vartime()
    assert T(0).invert().evaluate() == 0 and Z.invert().evaluate() == 0 and R(0, 5).invert().evaluate() == 0
    assert inv0.invert().evaluate() == 0 and inv0.square().evaluate() == 0 and inv0.double().evaluate() == 0
    # evaluate() of each form
    half = pow(2, -1, M)
    assert Z.evaluate() == 0 and T(7).evaluate() == 7 and R(1, 2).evaluate() == half and R(9, 1).evaluate() == 9
    assert T(2).invert().evaluate() == half and R(1, 2).invert().evaluate() == 2
    # against field arithmetic on random values
    rng = random.Random(7)
    for _ in range(200):
        vals = []
        for _ in range(2):
            kind = rng.randrange(4)
            num, den = rng.randrange(M), rng.choice([0, 1, rng.randrange(M)])
            vals.append([Z, T(num), R(num, den), R(0, den)][kind])
        x, y = vals
        ex, ey = x.evaluate(), y.evaluate()
        assert (x + y).evaluate() == (ex + ey) % M and (x - y).evaluate() == (ex - ey) % M and (x * y).evaluate() == ex * ey % M
        assert (-x).evaluate() == -ex % M and x.double().evaluate() == 2 * ex % M and x.square().evaluate() == ex * ex % M
        assert x.cube().evaluate() == pow(ex, 3, M) and x.invert().evaluate() == (pow(ex, -1, M) if ex else 0)


# ---- floor-planner errors -------------------------------------------------------------------------------------------------------------------
class _OneRegion(Circuit):
    def __init__(self, configure, synthesize):
        self.configure, self._synthesize = configure, synthesize

    def without_witnesses(self):
        return self

    def synthesize(self, config, layouter):
        self._synthesize(config, layouter)


def _run(configure, synthesize, k=4):
    return front.synthesize(_OneRegion(configure, synthesize), k, FP, fixed=True, advice=False)


def test_not_enough_rows():
    def rows(count):
        return lambda col, layouter: layouter.assign_region("r", lambda region: [region.assign_fixed(col, i, lambda: 1) for i in range(count)])
    _run(lambda meta: meta.fixed_column(), rows(10))                  # 16 rows, 6 of them unusable
    with pytest.raises(NotEnoughRowsAvailable):
        _run(lambda meta: meta.fixed_column(), rows(11))
    with pytest.raises(NotEnoughRowsAvailable):
        _run(lambda meta: meta.fixed_column(), rows(1), k=2)          # fewer than minimum_rows()


def test_table_errors():
    two = lambda meta: (meta.lookup_table_column(), meta.lookup_table_column())

    def twice(cols, layouter):
        fill = lambda t: [t.assign_cell(cols[0], i, lambda: 1) for i in range(3)]
        layouter.assign_table("first", fill)
        layouter.assign_table("second", fill)
    with pytest.raises(TableError) as e:
        _run(two, twice)
    assert e.value.kind == "UsedColumn"

    def uneven(cols, layouter):
        layouter.assign_table("t", lambda t: [t.assign_cell(cols[0], i, lambda: 1) for i in range(3)] + [t.assign_cell(cols[1], i, lambda: 2) for i in range(2)])
    with pytest.raises(TableError) as e:
        _run(two, uneven)
    assert e.value.kind == "UnevenColumnLengths"

    def gap(cols, layouter):
        layouter.assign_table("t", lambda t: [t.assign_cell(cols[0], i, lambda: 1) for i in (0, 2)])
    with pytest.raises(TableError) as e:
        _run(two, gap)
    assert e.value.kind == "ColumnNotAssigned"

    def overwrite(cols, layouter):
        layouter.assign_table("t", lambda t: [t.assign_cell(cols[0], 0, lambda: 1), t.assign_cell(cols[0], 0, lambda: 2)])
    with pytest.raises(TableError) as e:
        _run(two, overwrite)
    assert e.value.kind == "OverwriteDefault"
    # and the fill: the first value, over the usable rows past the table
    _, assembly, _ = _run(two, lambda cols, layouter: layouter.assign_table("t", lambda t: [t.assign_cell(cols[0], i, lambda i=i: 5 + i) for i in range(3)]))
    assert assembly.host_columns(assembly.fixed)[0] == [5, 6, 7] + [5] * 7 + [0] * 6


def test_constant_without_a_constants_column():
    def constant(col, layouter):
        layouter.assign_region("c", lambda region: region.assign_advice_from_constant(col, 0, 1))
    with pytest.raises(NotEnoughColumnsForConstants):                 # single_pass.rs:375-417
        _run(lambda meta: meta.advice_column(), constant)

    def with_column(meta):
        col, fixed = meta.advice_column(), meta.fixed_column()
        meta.enable_equality(col)
        meta.enable_constant(fixed)
        return col
    cs, assembly, _ = _run(with_column, lambda col, layouter: [constant(col, layouter), constant(col, layouter)])
    assert assembly.host_columns(assembly.fixed)[0][:3] == [1, 1, 0]  # constants go into the column one after the other
    assert _partition(assembly.permutation.pairs(), 2, 16) == {frozenset({(0, 0), (1, 0)}), frozenset({(0, 1), (1, 1)})}
    assert cs.pinned().endswith("constants: [Column { index: 0, column_type: Fixed }], minimum_degree: None }")


# ---- bulk assignment ------------------------------------------------------------------------------------------------------------------------
def test_bulk_assignment_lays_out_like_single_assignments():
    count, k = 9, 5
    values = [(i * i + 3) % M for i in range(count)]
    dens = [1, 0, 5, 1, 7, 1, 1, 2, 3]

    def configure(meta):
        a, b, f = meta.advice_column(), meta.advice_column(), meta.fixed_column()
        for col in (a, b, f):
            meta.enable_equality(col)
        return a, b, f

    def build(bulk):
        def synthesize(cols, layouter):
            a, b, f = cols
            layouter.assign_region("before", lambda region: region.assign_advice(a, 0, lambda: 1))

            def main(region):
                if bulk:
                    va = region.assign_advice_column(a, 2, (fields.to_limbs(values, FP, True), fields.to_limbs(dens, FP, True)))
                    vf = region.assign_fixed_column(f, 1, fields.to_limbs(values, FP, True))
                    cells_a, cells_f = [va.cell(i) for i in range(count)], [vf.cell(i) for i in range(count)]
                else:
                    cells_a = [region.assign_advice(a, 2 + i, lambda i=i: Assigned.rational(values[i], dens[i], M)).cell() for i in range(count)]
                    cells_f = [region.assign_fixed(f, 1 + i, lambda i=i: values[i]).cell() for i in range(count)]
                region.assign_advice(b, 0, lambda: 4)
                region.constrain_equal(cells_a[0], cells_f[0])
                region.constrain_equal(cells_a[count - 1], cells_f[3])
            layouter.assign_region("main", main)
            layouter.assign_region("after", lambda region: [region.assign_advice(a, 0, lambda: 2), region.assign_advice(b, 0, lambda: 3)])
        cs, assembly, layouter = front.synthesize(_OneRegion(configure, synthesize), k, FP, fixed=True, advice=True)
        return assembly, layouter
    (one, lay_one), (many, lay_many) = build(False), build(True)
    assert lay_one.regions == lay_many.regions == [0, 1, 12]
    assert lay_one.shapes == lay_many.shapes and lay_one.shapes[1][1] == 11
    assert lay_one.columns == lay_many.columns
    assert one.host_columns(one.advice) == many.host_columns(many.advice)
    assert one.host_columns(one.fixed) == many.host_columns(many.fixed)
    assert one.permutation.pairs() == many.permutation.pairs()
    want = [v * pow(d, -1, M) % M if d else 0 for v, d in zip(values, dens)]
    assert many.host_columns(many.advice)[0][3:12] == want
    with pytest.raises(NotEnoughRowsAvailable):                       # a vector that reaches into the unusable rows
        front.synthesize(_OneRegion(lambda meta: meta.advice_column(), lambda col, layouter: layouter.assign_region(
            "r", lambda region: region.assign_advice_column(col, 20, np.zeros((7, 4), dtype=np.uint64)))), k, FP, False, True)


# ---- the three entry points without a device ----------------------------------------------------------------------------------------------
def test_pack_selectors_bit_order():
    act = np.zeros((2, 70), dtype=bool)
    act[0, [0, 31, 32, 69]] = True
    act[1, 33] = True
    words = front.pack_selectors(act).view(np.uint32)
    assert words.shape == (2, 3) and words.dtype == np.uint32
    assert [int(w) for w in words[0]] == [0x80000001, 1, 1 << 5] and [int(w) for w in words[1]] == [0, 2, 0]


def test_entry_points_validate_and_fail_loudly_without_a_device():
    import halo2_amd as h
    from halo2_amd import _lib
    lib = h.lib()
    z = np.zeros((4, 4), np.uint64)
    p = lambda a: a.ctypes.data_as(_lib.u64p)
    assert lib.h2_assigned_to_field(7, p(z), p(z), p(z), 4, 1) == _lib.H2_ERR_ARGS                  # bad field
    assert lib.h2_assigned_to_field(0, p(z), p(z), p(z), 4, 9) == _lib.H2_ERR_ARGS                  # bad form
    assert lib.h2_assigned_to_field(0, None, p(z), p(z), 4, 1) == _lib.H2_ERR_ARGS                  # no numerators
    assert lib.h2_assigned_to_field_device(0, None, None, None, 4, 1, None) == _lib.H2_ERR_ARGS
    assert lib.h2_selector_conflicts_device(None, 5000, 1, None, None) == _lib.H2_ERR_ARGS          # more selectors than the matrix allows
    assert lib.h2_selector_conflicts_device(None, 2, 1, None, None) == _lib.H2_ERR_ARGS             # no output
    assert lib.h2_selector_combine_device(5, None, None, None, 0, 32, None, 0, None) == _lib.H2_ERR_ARGS
    assert lib.h2_selector_combine_device(0, None, None, None, 2, 32, None, 1, None) == _lib.H2_ERR_ARGS
    with pytest.raises(ValueError):
        h.assigned_to_field(z, np.zeros((5, 4), np.uint64), h.FP)
    if lib.h2_device_count() == 0:
        with pytest.raises(h.H2Error, match="no MI355X device|no HIP device"):
            h.assigned_to_field(z, z, h.FP)
        assert lib.h2_selector_conflicts_device(None, 0, 0, None, None) == _lib.H2_ERR_NODEV
        assert lib.h2_selector_combine_device(0, None, None, None, 0, 0, None, 0, None) == _lib.H2_ERR_NODEV
