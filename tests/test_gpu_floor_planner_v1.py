"""The V1 floor planner in front of the device: the circuits of floor_planner_cases.py through MockProver, keygen, create_proof and
verify_proof, the keys of the two planners compared, and a circuit of bulk gadgets whose measurement pass must launch nothing."""
import pytest

import halo2_amd as h
from halo2_amd import circuit as front
from halo2_amd import dev, fields, poseidon
from halo2_amd import verifier as hv
from halo2_amd.transcript import Blake2bWrite
from oracle import c_oracle as co

import floor_planner_cases as fc

pytestmark = pytest.mark.gpu
FP = 0
VESTA = h.VESTA
INSTANCES = [[fc.GapCircuit.INSTANCE]]


def _rng(seed):
    sf = co.field_of_curve(VESTA, "scalar")
    ctr = [seed]

    def rng(count):
        ctr[0] += 1
        return co.random_field(sf, ctr[0], count)
    return rng


@pytest.fixture(scope="module")
def params():
    made = {}

    def of(k):
        if k not in made:
            made[k] = h.Params.new(VESTA, k)
        return made[k]
    yield of
    for p in made.values():
        p.close()


def _prove_and_verify(params, circuit, instances, seed):
    pk = h.keygen_pk(params, circuit)
    tr = Blake2bWrite(VESTA)
    h.create_proof(params, pk, [circuit], [instances], _rng(seed), tr)
    proof = tr.finalize()
    bad = bytearray(proof)
    bad[len(bad) // 2] ^= 1
    return hv.verify_proof(params, pk.vk, instances, proof), hv.verify_proof(params, pk.vk, instances, bytes(bad))


# ---- GapCircuit -----------------------------------------------------------------------------------------------------------------------------------
def test_the_gap_circuit_is_satisfied_at_k_5():
    """25 rows under V1 where the single pass needs 30 and k = 5 has fewer"""
    assert dev.MockProver.run_circuit(fc.GapCircuit.K, fc.GapCircuitV1(), INSTANCES, FP).verify() == []
    with pytest.raises(front.NotEnoughRowsAvailable):
        dev.MockProver.run_circuit(fc.GapCircuit.K, fc.GapCircuit(), INSTANCES, FP)
    wrong = dev.MockProver.run_circuit(fc.GapCircuit.K, fc.GapCircuitV1(), [[fc.GapCircuit.INSTANCE + 1]], FP).verify()
    assert [(type(f).__name__, f.row) for f in wrong if tuple(f.column) == ("instance", 0)] == [("Permutation", 0)]


def test_an_overwritten_cell_fails_at_its_v1_row():
    """the last cell of the last region, 7 .. 11 on a2: offset 4 overwritten breaks `count` (gate 1) on the row before it, which V1 put
    at 10 + 3 (the single pass: 25 + 3)"""
    region, offset = 3, 4
    failures = dev.MockProver.run_circuit(fc.GapCircuit.K, fc.GapCircuitV1(bad=(region, "a2", offset)), INSTANCES, FP).verify()
    assert [(type(f).__name__, f.gate_index, f.row) for f in failures] == \
        [("ConstraintNotSatisfied", 1, fc.GapCircuit.V1_STARTS[region] + offset - 1)]
    assert ("advice", 2, 1, 12345) in failures[0].cell_values


def test_the_gap_circuit_proves_and_verifies_at_k_5(params):
    assert _prove_and_verify(params(fc.GapCircuit.K), fc.GapCircuitV1(), INSTANCES, 51) == (True, False)


def test_the_planners_keys_differ_where_the_layouts_do(params):
    simple, v1 = h.keygen_vk(params(6), fc.GapCircuit()), h.keygen_vk(params(6), fc.GapCircuitV1())
    assert simple.pinned() != v1.pinned() and simple.vk_repr != v1.vk_repr
    assert simple.circuit_cs.pinned() == v1.circuit_cs.pinned()                 # the same constraint system: the layout alone differs


# ---- the descending-area circuit --------------------------------------------------------------------------------------------------------------------
def test_descending_areas_give_both_planners_the_same_key(params):
    sides = []
    for circuit in (fc.DescendingCircuit(), fc.DescendingCircuitV1()):
        _, _, layouter = front.synthesize(circuit, fc.DescendingCircuit.K, FP, fixed=True, advice=True, instances=[])
        vk = h.keygen_vk(params(fc.DescendingCircuit.K), circuit)
        sides.append((layouter.regions, vk.pinned(), list(vk.fixed_commitments), list(vk.permutation_commitments)))
    assert sides[0] == sides[1] and sides[0][0] == fc.DescendingCircuit.STARTS
    assert dev.MockProver.run_circuit(fc.DescendingCircuit.K, fc.DescendingCircuitV1(), [], FP).verify() == []


# ---- a circuit of gadgets -----------------------------------------------------------------------------------------------------------------------------
def _gadget_circuit(kind):
    left = fields.to_limbs([11, 12], FP, True)
    right = fields.to_limbs([21, 22], FP, True)
    return kind(left, right)


def test_the_gadget_circuit_under_v1(params, monkeypatch):
    k = fc.GadgetCircuit.K
    dev.MockProver.run_circuit(k, _gadget_circuit(fc.GadgetCircuitV1), [], FP).assert_satisfied()
    calls = []
    trace = poseidon.trace
    monkeypatch.setattr(poseidon, "trace", lambda *a, **kw: calls.append(1) or trace(*a, **kw))
    launched, used = [], []
    for kind in (fc.GadgetCircuit, fc.GadgetCircuitV1):
        del calls[:]
        _, _, layouter = front.synthesize(_gadget_circuit(kind), k, FP, fixed=False, advice=True, instances=[])
        launched.append(len(calls))
        used.append(fc.rows_used(layouter.regions, layouter.shapes))
    assert launched == [1, 1]                                                 # the measurement pass launched nothing
    assert used[1] <= used[0]
    monkeypatch.undo()
    assert _prove_and_verify(params(k), _gadget_circuit(fc.GadgetCircuitV1), [], 52) == (True, False)
