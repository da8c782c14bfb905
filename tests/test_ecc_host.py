"""The ECC gadget on the host (no GPU): the restatement of tests/ecc_cases.py against `oracle.pasta.ec_mul`, and the chip's circuits
synthesized cell by cell and checked under tests/mock_prover_model.py -- every gate, lookup and copy constraint -- with the assigned
integers compared to the restatement."""
import pytest

import ecc_cases as ec
from ecc_cases import EDGE_SCALARS, P, ROWS, MulCircuit, PointOpsCircuit
from halo2_amd.circuit import Synthesis

K = 11
PER_CIRCUIT = 13                          # multiplications k = 11 holds beside the 1024-row table: 2 + 137 + 14 rows each
RANDOM = [a % P for a in ec.random_scalars(8, bits=254, seed=21)]


def _named(failures, names):
    return [(f[0],) + (names[f[1]] if f[0] == "ConstraintNotSatisfied" else (f[1],)) + (f[2],) for f in failures]


# ---- 1: the restatement ------------------------------------------------------------------------------------------------------------------------
def test_the_restatement_multiplies():
    """[alpha mod q]P for every edge scalar and 8 random ones; no denominator of the incomplete range vanishes; only alpha = 0 reaches
    the identity"""
    base = ec.random_bases(1)[0]
    for alpha in EDGE_SCALARS + RANDOM:
        cols, aux, result = ec.mul_trace(base, alpha)
        assert result == ec.ec_mul(alpha, base), alpha
        assert (result == (0, 0)) == (alpha == 0)
        assert aux[0] == (alpha + ((alpha + ec.T_Q) >> 254) * (1 << 130)) % P and aux[14] == aux[0] >> 130


# ---- 2: mul, cell by cell ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[0, 1])
def mul_run(request):
    scalars = (EDGE_SCALARS + RANDOM)[PER_CIRCUIT * request.param:PER_CIRCUIT * (request.param + 1)]
    bases = ec.random_bases(PER_CIRCUIT, seed=30 + request.param)
    circuit = MulCircuit(list(zip(bases, scalars)))
    failures, names, assembly, layouter, _ = ec.host_model(circuit, K)
    return circuit, failures, names, assembly, layouter


def test_mul_satisfies_every_constraint(mul_run):
    circuit, failures, names, _, _ = mul_run
    assert len(circuit.pairs) == PER_CIRCUIT and _named(failures, names) == []


def test_mul_cells_are_the_restatements(mul_run):
    circuit, _, _, assembly, layouter = mul_run
    advice = assembly.host_columns(assembly.advice)
    for (base, alpha), product in zip(circuit.pairs, circuit.products):
        cols, aux, result = ec.mul_trace(base, alpha)
        region = product.inner().x().cell().region_index
        start = layouter.regions[region]
        assert [advice[c][start:start + ROWS] for c in range(10)] == cols
        inner = product.inner()
        assert (inner.x().value().inner.evaluate(P), inner.y().value().inner.evaluate(P)) == result == ec.ec_mul(alpha, base)
        # the overflow check's regions follow: s, its range check (the running sums), the gate's three rows
        s_at, sums_at, gate_at = (layouter.regions[region + j] for j in (1, 2, 3))
        assert advice[6][s_at] == aux[0] and advice[9][sums_at:sums_at + 14] == aux[1:15] and advice[6][gate_at + 2] == aux[15]


@pytest.mark.parametrize("what, gate, constraint", [("z_hi", "q_mul_2 == 1 checks", "bool_check"), ("lambda", "complete addition", "1"),
                                                    ("eta", "overflow checks", "canonicity")])
def test_a_mutated_cell_is_named(what, gate, constraint):
    """alpha = 2^200 + 12345: k_254 = 0, z_130 and s >> 130 are not zero, so eta is constrained"""
    circuit = MulCircuit([(ec.random_bases(1)[0], (1 << 200) + 12345)], mutate=(0, what))
    failures, names, _, _, _ = ec.host_model(circuit, K)
    named = _named(failures, names)
    row = circuit.mutated_row - (1 if what == "eta" else 0)                   # the overflow gate sits one row above eta
    assert ("ConstraintNotSatisfied", gate, constraint, row) in named
    assert named and all(f[0] == "ConstraintNotSatisfied" and f[1] == gate and abs(f[3] - row) <= 1 for f in named), named
    if what == "z_hi":                                                        # the hi half's gate, not the lo half's of the same name
        assert {f[1] for f in failures} <= set(range(names.index((gate, "x_p_check")), names.index((gate, "x_p_check")) + 6))


# ---- 3: the point instructions -------------------------------------------------------------------------------------------------------------
def test_add_covers_every_branch():
    """P + Q, P + P, P + (-P), 0 + P, P + 0, 0 + 0 (add.rs tests::test_add), and incomplete addition of two distinct points"""
    p, q = ec.random_bases(2, seed=40)
    neg = (p[0], -p[1] % P)
    zero = (0, 0)
    ops = [("add", p, q, ec.o.ec_add(p, q, P)), ("add", p, p, ec.ec_mul(2, p)), ("add", p, neg, zero), ("add", zero, p, p), ("add", p, zero, p),
           ("add", zero, zero, zero), ("add_incomplete", p, q), ("witness", zero), ("witness", p), ("witness_non_id", q)]
    circuit = PointOpsCircuit(ops)
    failures, names, _, _, _ = ec.host_model(circuit, K)
    assert _named(failures, names) == []
    # a sum constrained equal to another point breaks the copies, nothing else
    failures, names, _, _, _ = ec.host_model(PointOpsCircuit([("add", p, q, p)]), K)
    assert failures and {f[0] for f in failures} == {"Permutation"}
    value = lambda r: (r.inner().x().value().inner.evaluate(P), r.inner().y().value().inner.evaluate(P))
    want = [ec.ec_mul(1, ec.o.ec_add(p, q, P)), ec.ec_mul(2, p), zero, p, p, zero, ec.incomplete_add(p, q), zero, p, q]
    assert [value(r) for r in circuit.results] == want


@pytest.mark.parametrize("ops", [[("add_incomplete", "p", "p")], [("add_incomplete", "p", "neg")], [("witness_non_id", (0, 0))]],
                         ids=["equal", "opposite", "identity"])
def test_incomplete_instructions_raise_where_the_reference_errors(ops):
    p = ec.random_bases(1, seed=41)[0]
    pts = {"p": p, "neg": (p[0], -p[1] % P)}
    ops = [tuple(pts.get(a, a) if isinstance(a, str) and a in pts else a for a in op) for op in ops]
    with pytest.raises(Synthesis):
        ec.front.synthesize(PointOpsCircuit(ops), K, ec.FP, fixed=True, advice=True, instances=[])


def test_witness_point_rejects_an_off_curve_pair():
    p = ec.random_bases(1, seed=42)[0]
    failures, names, _, _, _ = ec.host_model(PointOpsCircuit([("witness", (p[0], (p[1] + 1) % P))]), K)
    named = _named(failures, names)
    assert named and {f[1:3] for f in named} == {("witness point", "x == 0 v on_curve"), ("witness point", "y == 0 v on_curve")}
    failures, names, _, _, _ = ec.host_model(PointOpsCircuit([("witness_non_id", (p[0], (p[1] + 1) % P))]), K)
    assert [f[1:3] for f in _named(failures, names)] == [("witness non-identity point", "on_curve")]


# ---- 4: configure ----------------------------------------------------------------------------------------------------------------------------
def test_configure_follows_the_references_order():
    """chip.rs:280-292: the gates in creation order, the columns made equality-enabled in call order, and the selectors numbered as
    created: witness_point's two, add_incomplete, add, hi's three, lo's three, complete, overflow, then q_mul_lsb"""
    cs, _, _ = ec.front.synthesize(MulCircuit([]).without_witnesses(), K, ec.FP, fixed=True, advice=False)
    assert [g.name for g in cs.gates] == ["Short lookup bitshift"] + ec.GATE_NAMES
    # the range check enables equality on advices[9] first; then add_incomplete / add 0 - 3, hi 9 (already in) and 4, lo 6 and 8, the rest
    # already in; the instance-free test circuit has nothing else
    assert [(c.kind, c.index) for c in cs.permutation_columns if c.kind == "advice"] == [("advice", i) for i in (9, 0, 1, 2, 3, 4, 6, 8, 7)]
    config = ec.configure_ecc_chip(ec.front.ConstraintSystem(P))
    m = config.mul
    selectors = [config.witness_point.q_point, config.witness_point.q_point_non_id, config.add_incomplete.q_add_incomplete, config.add.q_add,
                 m.hi_config.q_mul_1, m.hi_config.q_mul_2, m.hi_config.q_mul_3, m.lo_config.q_mul_1, m.lo_config.q_mul_2, m.lo_config.q_mul_3,
                 m.complete_config.q_mul_decompose_var, m.overflow_config.q_mul_overflow, m.q_mul_lsb]
    assert [s.index for s in selectors] == list(range(3, 16))                 # after the range check's three
    add, hi, lo = config.add, m.hi_config, m.lo_config
    a = config.advices
    assert [add.x_p, add.y_p, add.x_qr, add.y_qr, add.lambda_, add.alpha, add.beta, add.gamma, add.delta] == a[:9]
    assert [hi.z, hi.double_and_add.x_a, hi.double_and_add.x_p, hi.y_p, hi.double_and_add.lambda_1, hi.double_and_add.lambda_2] == [a[i] for i in (9, 3, 0, 1, 4, 5)]
    assert [lo.z, lo.double_and_add.x_a, lo.double_and_add.x_p, lo.y_p, lo.double_and_add.lambda_1, lo.double_and_add.lambda_2] == [a[i] for i in (6, 7, 0, 1, 8, 2)]
    assert m.complete_config.z_complete == a[9] and m.overflow_config.advices == a[6:9]
