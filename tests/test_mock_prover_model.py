"""tests/mock_prover_model.py (the restatement of dev.rs:76-156, 576-904 the device checker is compared against) pinned to outcomes
the reference tree itself holds: its own test circuit is satisfied (tests/plonk_api.rs:438-442), its documentation example fails
with exactly one ConstraintNotSatisfied and the cell values 2, 4, 8 (dev.rs:246-261), its `bad_lookup` test with exactly one
Lookup failure (dev.rs:1129-1139), and the Value algebra of dev.rs:104-156 case by case.  No GPU."""
import random

import pytest

import mock_prover_cases as cases
import mock_prover_model as model
import plonk_circuits as pc
from mock_prover_model import Value
from oracle import pasta as o
from oracle import plonk_api

MODULI = [o.P, o.Q]


def test_value_algebra_case_by_case():
    m = o.P
    real, poison = lambda x: Value(x % m, m), Value(None, m)
    assert -real(3) == real(m - 3) and (-poison).poison                                       # dev.rs:104-113
    assert real(3) + real(m - 1) == real(2)                                                   # :115-124
    assert (real(3) + poison).poison and (poison + real(0)).poison and (poison + poison).poison
    assert real(3) * real(5) == real(15)                                                      # :126-142
    assert real(0) * poison == real(0) and poison * real(0) == real(0)
    assert (real(1) * poison).poison and (poison * real(7)).poison and (poison * poison).poison
    assert poison * 0 == real(0) and (poison * 2).poison and real(4) * 3 == real(12)          # Mul<F>, :144-156
    assert 0 * poison == real(0) and (3 + poison).poison and (1 - poison).poison and 1 - real(3) == real(m - 2)
    assert (real(3) - poison).poison and real(3) - real(5) == real(m - 2)
    assert poison == Value(None, m) and poison != real(0) and real(0) != poison               # derived Eq, :87
    assert len({poison, Value(None, m), real(0), real(0)}) == 2


@pytest.mark.parametrize("m", MODULI)
def test_reference_test_circuit_is_satisfied(m):
    assert model.verify(*cases.plonk_api_case(m), m) == []


@pytest.mark.parametrize("m", MODULI)
def test_reference_test_circuit_with_the_poisoning_selector(m):
    """The d * e term of plonk_api's gate 0 (d at rotation +1, e at rotation -1) behind the fixed column sf."""
    k, cs, fixed, advice, instance, mapping = cases.plonk_api_case(m)
    n = 1 << k
    usable = n - 6
    on = lambda row: [c if i != plonk_api.SF else [1 if r == row else 0 for r in range(n)] for i, c in enumerate(fixed)]
    # sf is a permutation column of its own (identity mapping), so switching it on changes no copy constraint
    got = model.verify(k, cs, on(0), advice, instance, mapping, m)
    assert got == [("ConstraintPoisoned", 0, 1, 0)]                                           # row 0 reads e at row n - 1
    got = model.verify(k, cs, on(3), advice, instance, mapping, m)
    assert len(got) == 1 and got[0][:3] == ("ConstraintNotSatisfied", 0, 3)
    assert [c[:3] for c in got[0][3]] == [("advice", 1, 0), ("fixed", 2, 0), ("advice", 2, 0), ("fixed", 3, 0), ("fixed", 1, 0),
                                          ("advice", 3, 0), ("fixed", 4, 0), ("fixed", 0, 0), ("advice", 4, 1), ("advice", 0, -1)]
    assert model.verify(k, cs, on(usable - 1), advice, instance, mapping, m) == []            # the poisoned d meets e = Real(0)


@pytest.mark.parametrize("m", MODULI)
def test_documentation_example(m):
    got = model.verify(*cases.doc_example_case(m), m)
    assert got == [("ConstraintNotSatisfied", 0, 0, (("fixed", 0, 0, 1), ("advice", 0, 0, 2), ("advice", 1, 0, 4), ("advice", 2, 0, 8)))]


@pytest.mark.parametrize("m", MODULI)
def test_bad_lookup(m):
    assert model.verify(*cases.bad_lookup_case(m), m) == [("Lookup", 0, 3)]


@pytest.mark.parametrize("m", MODULI)
def test_pair_lookup_fails_on_every_usable_row(m):
    got = model.verify(*cases.pair_lookup_case(m), m)
    assert got == [("Lookup", 0, r) for r in range(58)]


@pytest.mark.parametrize("m", MODULI)
def test_lookup_input_poisoned_by_a_rotation(m):
    usable = 32 - 6
    assert model.verify(*cases.rotated_lookup_case(m, False), m) == [("Lookup", 0, usable - 1)]
    assert model.verify(*cases.rotated_lookup_case(m, True), m) == []


@pytest.mark.parametrize("variant", ["full", "two_lookups", "gates_only"])
def test_broken_gate_of_the_shared_test_circuit(variant):
    n, usable = 64, 58
    cs = pc.make_cs(variant)
    for broken in (False, True):
        fixed, advice, mapping, instance = pc.make_witness(random.Random(7), o.P, n, usable, break_gate=broken)
        if variant == "gates_only":
            instance, mapping = [], []
        got = [f[:3] for f in model.verify(6, cs, fixed, advice, instance, mapping, o.P)]
        want = [("ConstraintNotSatisfied", 0, 5)]
        if variant != "gates_only":
            want += [("Permutation", ("advice", 1), 6), ("Permutation", ("advice", 2), 5)]
        assert got == (want if broken else [])


@pytest.mark.parametrize("variant", ["full", "two_lookups", "gates_only"])
def test_planted_faults_are_what_the_model_finds(variant):
    """The by-construction expectation the k = 20 device test relies on, against the model."""
    m, k = o.Q, 8
    advice, expected = cases.planted_faults(variant, m, k, gate_rows=[0, 4, 249], copy_rows=[3, 123], lookup_rows=[1, 60, 100])
    kk, cs, fixed, advice, instance, mapping = cases.variant_case(variant, m, k, advice)
    assert model.verify(kk, cs, fixed, advice, instance, mapping, m) == expected
    assert len(expected) == (3 if variant == "gates_only" else 3 + 3 * len(cs.lookups) + 4 + 6)


def test_cap_keeps_the_first_of_each_kind():
    fs = [("ConstraintNotSatisfied", 0, r, ()) for r in range(5)] + [("Lookup", 0, 1), ("Lookup", 0, 2), ("Permutation", ("advice", 0), 9)]
    assert model.capped(fs, 2) == fs[:2] + fs[5:7] + fs[7:]
    assert model.counts(fs) == {"ConstraintNotSatisfied": 5, "ConstraintPoisoned": 0, "Lookup": 2, "Permutation": 1}
