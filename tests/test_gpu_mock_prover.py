"""halo2_amd.dev.MockProver on the device against tests/mock_prover_model.py (the big-integer restatement of dev.rs:576-904):
failure lists compared for equality, exact counts, both fields."""
import ctypes as C
import random

import numpy as np
import pytest

import halo2_amd as h
import mock_prover_cases as cases
import mock_prover_model as model
import plonk_circuits as pc
from halo2_amd import fields
from halo2_amd.dev import ConstraintNotSatisfied, ConstraintPoisoned, Lookup, MockProver, Permutation
from oracle import plonk_api

pytestmark = pytest.mark.gpu

FIELDS = [h.FP, h.FQ]


def _device(case, field, **kw):
    k, cs, fixed, advice, instance, mapping = case
    return MockProver.run(k, cs, fixed, advice, instance, mapping, field, **kw)


def _agree(case, field, expect=None):
    """Device failures and exact counts equal the model's; returns the model's list."""
    m = fields.MODULUS[field]
    want = model.verify(*case, m)
    if expect is not None:
        assert want == expect
    prover = _device(case, field)
    got = model.as_tuples(prover.verify(max_failures=1 << 30))
    assert got == want, (got[:6], want[:6], len(got), len(want))
    assert prover.failure_counts == model.counts(want)
    if want:
        with pytest.raises(AssertionError, match="circuit was not satisfied"):
            prover.assert_satisfied()
    else:
        prover.assert_satisfied()
    return want


def _upload(col, field):
    import torch
    return torch.from_numpy(fields.to_limbs(col, field, True).view(np.int64)).cuda()


@pytest.mark.parametrize("field", FIELDS)
def test_reference_circuits(field):
    """The outcomes the reference tree holds (tests/test_mock_prover_model.py), on the device; k = 4 and k = 5 have fewer rows than a wave."""
    m = fields.MODULUS[field]
    assert _agree(cases.plonk_api_case(m), field) == []
    failure = _device(cases.doc_example_case(m), field).verify()
    assert failure == [ConstraintNotSatisfied(0, 0, (("fixed", 0, 0, 1), ("advice", 0, 0, 2), ("advice", 1, 0, 4), ("advice", 2, 0, 8)))]
    _agree(cases.doc_example_case(m), field)
    assert _device(cases.bad_lookup_case(m), field).verify() == [Lookup(0, 3)]
    _agree(cases.bad_lookup_case(m), field, [("Lookup", 0, 3)])


@pytest.mark.parametrize("field", FIELDS)
def test_poisoning_selector_of_the_reference_circuit(field):
    m = fields.MODULUS[field]
    k, cs, fixed, advice, instance, mapping = cases.plonk_api_case(m)
    n = 1 << k
    on = lambda row: [c if i != plonk_api.SF else [1 if r == row else 0 for r in range(n)] for i, c in enumerate(fixed)]
    assert _device((k, cs, on(0), advice, instance, mapping), field).verify() == [ConstraintPoisoned(0, 1, 0)]
    _agree((k, cs, on(0), advice, instance, mapping), field, [("ConstraintPoisoned", 0, 1, 0)])
    got = _agree((k, cs, on(3), advice, instance, mapping), field)
    assert len(got) == 1 and got[0][:3] == ("ConstraintNotSatisfied", 0, 3)
    assert _agree((k, cs, on(n - 7), advice, instance, mapping), field) == []             # Real(0) times the poisoned d
    # every row switched on: rows whose d or e is a blinding row are poisoned (and counted), the others simply fail
    every = [c if i != plonk_api.SF else [1] * n for i, c in enumerate(fixed)]
    got = _agree((k, cs, every, advice, instance, mapping), field)
    assert sum(1 for f in got if f[0] == "ConstraintPoisoned") == 1


@pytest.mark.parametrize("field", FIELDS)
def test_lookups_are_compared_as_exact_tuples(field):
    m = fields.MODULUS[field]
    assert _agree(cases.pair_lookup_case(m), field) == [("Lookup", 0, r) for r in range(58)]
    assert _agree(cases.rotated_lookup_case(m, False), field) == [("Lookup", 0, 25)]
    assert _agree(cases.rotated_lookup_case(m, True), field) == []
    wide = _agree(cases.wide_lookup_case(m), field)                                       # nine components: two packed keys
    assert 0 < len(wide) <= 12
    assert _agree(cases.wide_lookup_case(m, faults=0), field) == []
    assert len(_agree(cases.wide_lookup_case(m, k=7, width=16, seed=5, faults=20), field)) > 0    # three groups


@pytest.mark.parametrize("field", FIELDS)
def test_sums_and_products_that_vanish_only_after_reduction(field):
    """a + (m - a) and a * b - c wrap around the modulus: the zero test has to see the reduced value."""
    from halo2_amd.plonk import ConstraintSystem
    m = fields.MODULUS[field]
    rnd = random.Random(5)
    n = 16
    a = [rnd.randrange(1, m) for _ in range(n)]
    b = [m - v for v in a]
    c = [x * y % m for x, y in zip(a, b)]
    cs = ConstraintSystem(num_fixed_columns=0, num_advice_columns=3, num_instance_columns=0,
                          gates=[lambda q: q.advice(0) + q.advice(1), lambda q: q.advice(0) * q.advice(1) - q.advice(2),
                                 lambda q: 3 * q.advice(0) + q.advice(1) * 3, lambda q: 0 * q.advice(0, 1) + q.advice(2) * 0, lambda q: 7],
                          advice_queries=[(0, 0), (1, 0), (2, 0)], instance_queries=[], fixed_queries=[], degree=3, blinding_factors=5)
    got = _agree((4, cs, [], [a, b, c], [], []), field)
    # gates 0 - 2 are poisoned on the six blinding rows and hold elsewhere, gate 3 is Real(0) everywhere, gate 4 fails everywhere
    assert got[:3] == [("ConstraintPoisoned", g, 6, 10) for g in range(3)] and len(got) == 3 + 16
    c[4] = (c[4] + 1) % m
    assert [f[:3] if f[0] == "ConstraintNotSatisfied" else f for f in _agree((4, cs, [], [a, b, c], [], []), field)[:4]] == [
        ("ConstraintPoisoned", 0, 6, 10), ("ConstraintNotSatisfied", 1, 4), ("ConstraintPoisoned", 1, 6, 10), ("ConstraintPoisoned", 2, 6, 10)]


@pytest.mark.parametrize("variant", ["full", "two_lookups", "gates_only"])
def test_broken_gate_of_the_shared_test_circuit(variant):
    cs = pc.make_cs(variant)
    for field in FIELDS:
        m = fields.MODULUS[field]
        for broken in (False, True):
            fixed, advice, mapping, instance = pc.make_witness(random.Random(7), m, 64, 58, break_gate=broken)
            if variant == "gates_only":
                instance, mapping = [], []
            got = [f[:3] for f in _agree((6, cs, fixed, advice, instance, mapping), field)]
            want = [("ConstraintNotSatisfied", 0, 5)]
            if variant != "gates_only":
                want += [("Permutation", ("advice", 1), 6), ("Permutation", ("advice", 2), 5)]
            assert got == (want if broken else [])


@pytest.mark.parametrize("variant", ["full", "two_lookups", "gates_only"])
@pytest.mark.parametrize("k", [12, 16])
@pytest.mark.parametrize("field", FIELDS)
def test_seeded_faults(field, k, variant):
    """Satisfied, and 1, 2 and 100 faults of each kind (row 0 and the last usable row among them; blinding rows of every advice
    column changed as well, which nothing may report)."""
    m = fields.MODULUS[field]
    kk, cs, fixed, advice, instance, mapping = cases.variant_case(variant, m, k)
    fixed_dev = [_upload(c, field) for c in fixed]                                        # resident once; run() uses tensors in place
    flat = np.array([[c2 * (1 << k) + r2 for c2, r2 in col] for col in mapping], dtype=np.int64) if mapping else mapping
    assert _agree((kk, cs, fixed, advice, instance, mapping), field) == []
    for kind in ("gate", "copy", "lookup"):
        for count in (1, 2, 100):
            broken = cases.seeded_faults(m, k, kind, count)
            want = model.verify(kk, cs, fixed, broken, instance, mapping, m)
            prover = MockProver.run(kk, cs, fixed_dev, broken, instance, flat, field)
            got = model.as_tuples(prover.verify(max_failures=1 << 30))
            assert got == want, (kind, count, got[:4], want[:4], len(got), len(want))
            assert prover.failure_counts == model.counts(want)
            if variant != "gates_only" or kind == "gate":
                assert len(want) >= count                                                 # the faults are seen, and the changed blinding rows are not
            assert all(f[2] < (1 << k) - 6 for f in want if f[0] != "Permutation")


@pytest.mark.parametrize("field", FIELDS)
def test_cap_and_exact_counts(field):
    m = fields.MODULUS[field]
    k = 12
    for kind in ("gate", "copy", "lookup"):
        case = cases.variant_case("two_lookups", m, k, cases.seeded_faults(m, k, kind, 100))
        want = model.verify(*case, m)
        assert len(want) >= 100
        prover = _device(case, field)
        assert model.as_tuples(prover.verify(max_failures=3)) == model.capped(want, 3)
        assert prover.failure_counts == model.counts(want)
        assert model.as_tuples(prover.verify(max_failures=3)) == model.capped(want, 3)    # deterministic
        assert prover.verify(max_failures=0) == [] and prover.failure_counts == model.counts(want)
        assert model.as_tuples(prover.verify()) == model.capped(want, 1024)


@pytest.mark.parametrize("field", FIELDS)
def test_tensors_and_integer_lists_give_the_same_answer(field):
    import torch
    m = fields.MODULUS[field]
    k = 8
    kk, cs, fixed, advice, instance, mapping = cases.variant_case("two_lookups", m, k, cases.seeded_faults(m, k, "copy", 2))
    from_lists = _device((kk, cs, fixed, advice, instance, mapping), field).verify()
    flat = np.array([[c2 * (1 << k) + r2 for c2, r2 in col] for col in mapping], dtype=np.int64)
    up = lambda cols: [_upload(c, field) for c in cols]
    for mp in (flat, torch.from_numpy(flat).cuda()):
        prover = MockProver.run(kk, cs, up(fixed), up(advice), instance, mp, field)
        assert prover.verify() == from_lists and from_lists
    short = [c[:200] for c in advice]                                                     # rows never assigned are zero
    want = model.verify(kk, cs, fixed, short, instance, mapping, m)
    assert model.as_tuples(_device((kk, cs, fixed, short, instance, mapping), field).verify(1 << 30)) == want
    with pytest.raises(ValueError, match="mapping"):
        MockProver.run(kk, cs, fixed, advice, instance, flat[:2], field)


@pytest.mark.parametrize("field", FIELDS)
def test_muladd_and_stored_values_through_the_c_abi(field):
    """H2_EV_MULADD b is SCALE b of the accumulator, then ADD; the storing mode writes the value (0 where poisoned) beside the planes."""
    import torch
    m = fields.MODULUS[field]
    n, usable = 16, 10
    rnd = random.Random(9)
    a, b = [rnd.randrange(m) for _ in range(n)], [rnd.randrange(m) for _ in range(n)]
    b[3] = (-a[3] * 5) % m
    polys = [_upload(a, field), _upload(b, field)]
    prog = [1 | 0 << 8, 0, 1 | 1 << 8, 0, 7 | 0 << 8,          # a * consts[0] + b          a is advice: poisoned on rows >= usable
            1 | 0 << 8, 0, 1 | 1 << 8, 0, 7 | 1 << 8]          # a * consts[1] + b          consts[1] = 0: Real(0) + b everywhere
    consts = fields.to_limbs([5, 0], field, True)
    nz = torch.empty((2, 1), dtype=torch.int64, device="cuda")
    po = torch.empty((2, 1), dtype=torch.int64, device="cuda")
    counts = torch.empty(4, dtype=torch.int32, device="cuda")
    values = torch.empty((2, n, 4), dtype=torch.int64, device="cuda")
    vp = C.c_void_p
    rc = h.lib().h2_check_expressions_device(field, (C.c_uint32 * len(prog))(*prog), (C.c_size_t * 3)(0, 5, 10), 2, consts.ctypes.data_as(h._lib.u64p), 2,
                                             (vp * 2)(*[p.data_ptr() for p in polys]), (C.c_uint8 * 2)(1, 0), 2, 4, usable, nz.data_ptr(),
                                             po.data_ptr(), counts.data_ptr(), (vp * 2)(values[0].data_ptr(), values[1].data_ptr()), None)
    assert rc == 0
    torch.cuda.synchronize()
    bits = lambda t, p: [(int(t[p, 0].item()) >> r) & 1 for r in range(n)]
    want0 = [(a[r] * 5 + b[r]) % m for r in range(n)]
    assert bits(po, 0) == [0] * usable + [1] * (n - usable) and bits(po, 1) == [0] * n
    assert bits(nz, 0) == [1 if r < usable and want0[r] else 0 for r in range(n)] and bits(nz, 0)[3] == 0
    assert bits(nz, 1) == [1 if b[r] else 0 for r in range(n)]
    assert counts.cpu().tolist() == [sum(bits(nz, 0)), n - usable, sum(bits(nz, 1)), 0]
    got = [fields.from_limbs(values[p].cpu().numpy().view(np.uint64), field, True) for p in range(2)]
    assert got[0] == want0[:usable] + [0] * (n - usable) and got[1] == b


def test_k20_satisfied_and_planted_faults():
    """k = 20 once: a satisfied witness reports nothing, the same witness with a handful of planted faults reports exactly those.
    The expectation is by construction (cases.planted_faults); the construction itself is checked against the model at k = 12."""
    field, variant = h.FQ, "full"
    m = fields.MODULUS[field]
    rows = dict(gate_rows=[0, 1, 1000], copy_rows=[3, 999], lookup_rows=[4, 2001])
    advice12, expected12 = cases.planted_faults(variant, m, 12, **rows)
    case12 = cases.variant_case(variant, m, 12, advice12)
    assert model.verify(*case12, m) == expected12
    assert model.as_tuples(_device(case12, field).verify()) == expected12
    k = 20
    n = 1 << k
    usable = n - 6
    big = dict(gate_rows=[0, 1, 1000, usable - 1], copy_rows=[3, 999, 600000], lookup_rows=[4, 2001, 1000000])
    kk, cs, fixed, advice, instance, mapping = cases.variant_case(variant, m, k)
    flat = np.array([[c2 * n + r2 for c2, r2 in col] for col in mapping], dtype=np.int64)
    fixed_dev = [_upload(c, field) for c in fixed]
    prover = MockProver.run(kk, cs, fixed_dev, [_upload(c, field) for c in advice], instance, flat, field)
    assert prover.verify() == [] and prover.failure_counts == dict.fromkeys(model.counts([]), 0)
    prover.assert_satisfied()
    broken, expected = cases.planted_faults(variant, m, k, **big)
    prover = MockProver.run(kk, cs, fixed_dev, [_upload(c, field) for c in broken], instance, flat, field)
    assert model.as_tuples(prover.verify()) == expected and len(expected) == 4 + 3 + 6 + 6
    assert prover.failure_counts == model.counts(expected)
