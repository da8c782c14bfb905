"""What the GPU sweep of tests/test_gpu_evaluator_shapes.py executes, proved on the CPU: every case of tests/evaluator_cases.py runs through
the integer interpreter of tests/evaluator_model.py, which records each executed (opcode, stack depth) and each rotation.  The union must
be the whole legal set -- computed here from the stack's size, not listed -- so thinning the case list fails here instead of quietly
shrinking what the device runs.  The interpreter itself is held to oracle/evaluator.py on every `Ast` case."""
import pytest

import evaluator_cases as ec
import evaluator_model as em
from evaluator_cases import ADD, BASES, COEFF, CONST, EXTENDED, LAGRANGE, LINEAR, MUL, MULADD, POLY, SCALE

DEEP = ec.MAX_DEPTH                       # nine slots: the register-resident top and eight spilled levels


def legal_ops(basis, pushes=ec.PUSHES):
    """{(opcode, values on the stack before it)}: a push needs a free slot, a binary node two operands, SCALE one; no MUL in the coefficient basis."""
    binaries = [op for op in ec.BINARIES if not (basis == COEFF and op == MUL)]
    return ({(op, d) for op in pushes for d in range(0, DEEP)} | {(op, d) for op in binaries for d in range(2, DEEP + 1)} |
            {(SCALE, d) for d in range(1, DEEP + 1)})


def ops_of(cases, field):
    out = set()
    for case in cases:
        out |= ec.materialize(case, field).trace.ops
    return out


@pytest.mark.parametrize("field", ec.FIELDS)
def test_the_model_agrees_with_the_oracle_on_every_ast_case(field):
    n_ast = 0
    for case in ec.CASES:
        mat = ec.materialize(case, field)
        assert mat.depth <= DEEP, case
        if case.is_ast:
            n_ast += 1
            assert mat.values == ec.oracle_values(mat), case
    assert n_ast >= 40


@pytest.mark.parametrize("field", ec.FIELDS)
@pytest.mark.parametrize("basis", BASES)
def test_every_opcode_runs_at_every_depth_it_can_have(field, basis):
    cases = [c for c in ec.CASES if c.basis == basis]
    assert ops_of(cases, field) == legal_ops(basis)
    # and the three deep-stack programs of a basis reach all of it on their own, at two workgroups and at eight.  (Three, not one: only a
    # program's first instruction runs on an empty stack, so POLY, CONST and LINEAR at depth 0 take a program each.)
    for log_len in (9, 11):
        deep = [c for c in cases if "stack" in c.tags and "mock" not in c.tags and c.log_len == log_len]
        assert len(deep) == 3 and ops_of(deep, field) == legal_ops(basis), (basis, log_len)
        for case in deep:
            mat = ec.materialize(case, field)
            assert mat.depth == DEEP
            assert len(set(mat.consts)) == len(mat.consts) and len({tuple(p) for p in mat.polys}) == len(mat.polys)      # all operands differ
            assert sorted(p for p, _ in ec.poly_reads(mat.words)) == list(range(len(mat.polys)))                                                # each leaf another polynomial


@pytest.mark.parametrize("field", ec.FIELDS)
def test_the_mock_prover_programs_reach_every_depth_and_every_poison_bit(field):
    mock = [c for c in ec.CASES if "mock" in c.tags]
    assert len(mock) == 3 and all(c.basis == LAGRANGE and c.log_len == ec.MOCK_LOG_LEN for c in mock)
    want = legal_ops(LAGRANGE, pushes=(POLY, CONST))                              # h2_check_expressions_device refuses LINEAR
    assert ops_of(mock, field) == want
    programs, offsets, consts, polys = ec.mock_programs(field)
    assert offsets[-1] == len(programs) and len(consts) == sum(len(ec.materialize(c, field).consts) for c in mock)
    plain, poisoned = ec.mock_model(field, False), ec.mock_model(field, True)
    ops, spilled, filled = set(), set(), set()
    for (values, trace), (pvalues, ptrace), case in zip(plain, poisoned, mock):
        ops |= ptrace.ops
        spilled |= ptrace.poison_spilled
        filled |= ptrace.poison_filled
        assert not trace.poison_spilled and em.POISON not in values
        # poison only removes values: the rest is the plain run
        assert all(p is em.POISON or p == v for p, v in zip(pvalues, values))
        n_poison = sum(p is em.POISON for p in pvalues)
        assert ec.MOCK_UNUSABLE <= n_poison < len(values) // 2, n_poison
    assert ops == want
    levels = set(range(em.SPILL_LEVELS))
    assert spilled == levels and filled == levels                                 # every bit of the kernel's `pbits` is set and read


@pytest.mark.parametrize("field", ec.FIELDS)
def test_the_rotations_and_lengths_the_sweep_promises(field):
    reached, lengths = {}, set()
    for case in ec.CASES:
        mat = ec.materialize(case, field)
        lengths.add((case.basis, case.log_len))
        for shift in mat.trace.shifts:
            assert abs(shift) <= mat.n                                            # what h2_evaluate_device accepts
            reached.setdefault((case.basis, case.log_len), set()).update(ec.shift_classes(shift, mat.n, case.step, case.basis))
    for basis in (LAGRANGE, EXTENDED):
        for log_len in ec.LOG_LENS[1:]:
            missing = ec.wanted_shift_classes(basis, log_len) - reached.get((basis, log_len), set())
            assert not missing, (basis, log_len, sorted(missing))
    assert {"+len", "-len"} <= reached[(LAGRANGE, 0)]
    assert lengths >= {(basis, log_len) for basis in BASES for log_len in (0,) + ec.LOG_LENS}
    # the extended lengths come from domains of every step: j = 3, 5, 9 are rotations of 2, 4, 8 elements, each at two workgroups or more
    steps = {(c.step, c.log_len) for c in ec.CASES if c.basis == EXTENDED and c.is_ast and "shifts" in c.tags}
    assert {s for s, _ in steps} == {2, 4, 8} and all(any(s == step and L >= 9 for s, L in steps) for step in (2, 4, 8))
    # one polynomial at several rotations inside one product
    for name in ("product-lagrange-L9", "product-extended-L9-j5"):
        words = ec.materialize(ec.BY_NAME[name], field).words
        reads = ec.poly_reads(words)
        assert len({shift for p, shift in reads if p == 0}) == 5 and len(reads) == 7
        assert sorted(op for op, _ in ec.instructions(words) if op != POLY) == [ADD] + [MUL] * 5


@pytest.mark.parametrize("field", ec.FIELDS)
def test_the_linear_and_value_cases_hold_what_they_are_listed_for(field):
    m = ec.fields.MODULUS[field]
    extremes = {0, 1, m - 1}
    for case in ec.CASES:
        mat = ec.materialize(case, field)
        if "linear" in case.tags and case.is_ast:
            zeta = mat.dom.g_coset if case.basis == EXTENDED else 1
            got = [mat.consts[arg] for op, arg in ec.instructions(mat.words) if op == LINEAR]
            assert got == [c * zeta % m for c in ec.LINEAR_CONSTS], case            # 0, 1, p - 1 and a random value, ZETA folded in
        if "values" in case.tags:
            assert [sorted(set(p)) for p in mat.polys[:4]] == [[0], [m - 1], [0, m - 1], [0, 1]]
            assert mat.polys[3][-1] == 1 and sum(mat.polys[3]) == 1
            for op in (CONST, SCALE, MULADD):
                assert extremes - {1 if op == MULADD else None} <= {mat.consts[arg] for o, arg in ec.instructions(mat.words) if o == op}, (case, op)
            assert {ADD, SCALE, MULADD} | ({MUL} - {MUL if case.basis == COEFF else None}) <= {op for op, _ in ec.instructions(mat.words)}
    linear = {(c.basis, c.log_len) for c in ec.CASES if "linear" in c.tags}
    assert linear >= {(basis, log_len) for basis in BASES for log_len in (0,) + ec.LOG_LENS}
    assert {(c.basis, c.j) for c in ec.CASES if "linear" in c.tags and c.basis == EXTENDED and c.is_ast} == {(EXTENDED, j) for j in (3, 5, 9)}
    # two true primitive roots at one length
    for basis in (LAGRANGE, EXTENDED):
        a, b = (ec.materialize(ec.BY_NAME[f"roots-{ec.BASIS_NAME[basis]}-L9-w{p}"], field) for p in (1, 3))
        assert a.omega != b.omega and b.omega == pow(a.omega, 3, m) and a.words == b.words and a.values != b.values
        for w in (a.omega, b.omega):
            assert pow(w, 256, m) == m - 1


@pytest.mark.parametrize("field", ec.FIELDS)
def test_the_late_constant_cases(field):
    for name, *_ in ec.LATE_CASES:
        late = ec.materialize_late(name, field)
        assert late.values == late.want, name                                      # the model with the slot filled = the oracle with y in the tree
        if "empty" in name:
            assert not late.slot_used and late.values[0] == late.values[1] == late.polys[0]
        else:
            assert late.slot_used and late.values[0] != late.values[1]


def test_the_launch_cases_and_the_refusals_are_what_they_claim():
    mat = ec.materialize(ec.BY_NAME["polys64-lagrange-L9"], ec.FIELDS[0])
    assert {p for p, _ in ec.poly_reads(mat.words)} == set(range(64))
    chain = ec.materialize(ec.BY_NAME["chain-lagrange-L9"], ec.FIELDS[0])
    assert 2000 < len(chain.words) < 5000 and chain.depth == 2
    a, b = (ec.materialize(ec.BY_NAME[name], ec.FIELDS[0]) for name in ec.BACK_TO_BACK)
    assert (a.case.basis, a.n, len(a.polys)) == (b.case.basis, b.n, len(b.polys)) and a.words != b.words
    names = [name for name, _ in ec.REFUSALS]
    assert len(set(names)) == len(names) and all(set(over) <= set(ec.REFUSAL_BASE) for _, over in ec.REFUSALS)
    # the base call of the refusals is itself a valid program: what each entry changes is what gets it refused
    words = ec.REFUSAL_BASE["words"]
    values, depth = em.interpret(words, [5], [[1] * 16, [2] * 16], LAGRANGE, 16, ec.fields.MODULUS[ec.FIELDS[0]], 1)
    assert values == [7] * 16 and depth == 2
