"""Pow5Chip<F, WIDTH, RATE> with a Spec: mirrors of the reference benchmark's HashCircuit (halo2_gadgets/benches/poseidon.rs) at
(3, 2, L = 2), (9, 8, L = 8) and (12, 11, L = 11), K = 7, through MockProver, keygen, create_proof and verify_proof; the bulk
assignments `permute_many` / `hash_many` against the cell-by-cell mirror at width 9; and the example.  Expected digests are the
Python-integer model's (tests/poseidon_model.py; reference values exist for width 3 only, see tests/test_poseidon_spec_host.py)."""
import importlib.util
import os

import numpy as np
import pytest

import halo2_amd as h
import poseidon_cases as pc
import poseidon_model as pm
import poseidon_spec_cases as psc
from halo2_amd import circuit as front
from halo2_amd import dev, fields
from halo2_amd import verifier as hv
from halo2_amd.poseidon_spec import Spec
from halo2_amd.transcript import Blake2bWrite
from oracle import c_oracle as co
from poseidon_spec_cases import FP, WideHashCircuit, WideMirrorCircuit, WidePermuteManyCircuit

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
VESTA = h.VESTA
K = 7
WIDE = (9, 8, 8, 56)
BENCH = [((3, 2, 8, 56), 2), (WIDE, 8), ((12, 11, 8, 56), 11)]                  # benches/poseidon.rs:207-211: L = RATE


def _up(limbs):
    return torch.from_numpy(np.ascontiguousarray(limbs).view(np.int64)).to(fields.current_device())


def _rng(seed):
    sf = co.field_of_curve(VESTA, "scalar")
    ctr = [seed]

    def rng(count):
        ctr[0] += 1
        return co.random_field(sf, ctr[0], count)
    return rng


def _kinds(failures):
    return {type(f).__name__ for f in failures}


def _output_row(circuit, k):
    """the absolute row of the digest's cell, from a synthesis without a witness"""
    blank = circuit.without_witnesses()
    _, _, layouter = front.synthesize(blank, k, FP, fixed=True, advice=False)
    cell = blank.output_cell
    return cell.column, layouter.regions[cell.region_index] + cell.row_offset


@pytest.mark.parametrize("key,length", BENCH, ids=str)
def test_bench_hash_circuit_mock_proves_proves_and_verifies(key, length):
    model = pm.model(FP, *key)
    message = pm.random_states(1, length, FP, 0x700 + length)[0]
    digest = model.hash(message)
    circuit = WideHashCircuit(key, length, message)
    dev.MockProver.run_circuit(K, circuit, [[digest]], FP).assert_satisfied()
    # a public output off by one: the copy of the digest to the instance column fails, on the output cell and on the instance cell
    failures = dev.MockProver.run_circuit(K, circuit, [[(digest + 1) % pm.P]], FP).verify()
    column, row = _output_row(circuit, K)
    assert failures and _kinds(failures) == {"Permutation"}
    assert {((f.column[0], f.column[1]), f.row) for f in failures} == {((column.kind, column.index), row), (("instance", 0), 0)}
    params = h.Params.new(VESTA, K)
    pk = h.keygen_pk(params, circuit)
    tr = Blake2bWrite(VESTA)
    h.create_proof(params, pk, [circuit], [[[digest]]], _rng(7), tr)
    proof = tr.finalize()
    assert hv.verify_proof(params, pk.vk, [[digest]], proof)
    assert not hv.verify_proof(params, pk.vk, [[(digest + 1) % pm.P]], proof)
    params.close()


def test_two_permutations_and_seven_padding_words():
    model = pm.model(FP, *WIDE)
    message = pm.random_states(1, 9, FP, 0x709)[0]                             # L = 9 at rate 8
    digest = model.hash(message)
    circuit = WideHashCircuit(WIDE, 9, message)
    dev.MockProver.run_circuit(K, circuit, [[digest]], FP).assert_satisfied()
    _, assembly, layouter = front.synthesize(circuit.without_witnesses(), K, FP, fixed=True, advice=False)
    assert [rows for _, rows in layouter.shapes].count(37) == 2                 # two permutations
    assert int(assembly.selectors[2].sum()) == 2                                # two pad-and-add rows
    assert _kinds(dev.MockProver.run_circuit(K, circuit, [[(digest + 1) % pm.P]], FP).verify()) == {"Permutation"}


# ---- permute_many / hash_many ---------------------------------------------------------------------------------------------------------------
COUNT, K_MANY = 3, 7                                                            # 3 x 37 rows


def _bumped(trace, column, row):
    t = trace.copy()
    t[column, row] = fields.to_limbs([(fields.from_limbs(t[column, row], FP, True)[0] + 1) % pm.P], FP, True)[0]
    return _up(t)


def _gate_failures(prover, cs_of):
    failures = prover.verify()
    assert failures and _kinds(failures) == {"ConstraintNotSatisfied"}
    return {(pc.gate_of_polynomial(cs_of, f.gate_index)[0], f.row) for f in failures}


def test_permute_many_takes_its_witness_from_spec_trace_and_names_a_broken_cell():
    model = pm.model(FP, *WIDE)
    states = pm.random_states(COUNT, 9, FP, 0x710)
    limbs = _up(model.states_limbs(states))
    circuit = WidePermuteManyCircuit(WIDE, COUNT, limbs)
    dev.MockProver.run_circuit(K_MANY, circuit, [], FP).assert_satisfied()
    assert circuit.result.count == COUNT and psc.ints_of(circuit.result.outputs, FP) == [w for s in states for w in model.permute(s)]
    assert circuit.result.output_cell(2, 8) == front.Cell(0, 3 * 37 - 1, front.Column("advice", 8))
    cs, _, _ = front.synthesize(WidePermuteManyCircuit(WIDE, COUNT), K_MANY, FP, fixed=True, advice=False)
    trace = model.trace_limbs(states)
    dev.MockProver.run_circuit(K_MANY, WidePermuteManyCircuit(WIDE, COUNT, limbs, trace=_up(trace)), [], FP).assert_satisfied()
    # partial_sbox (column 9) of permutation 2, row 17
    prover = dev.MockProver.run_circuit(K_MANY, WidePermuteManyCircuit(WIDE, COUNT, limbs, trace=_bumped(trace, 9, 2 * 37 + 17)), [], FP)
    assert _gate_failures(prover, cs) == {("partial rounds", 2 * 37 + 17)}
    # state word 7 on row 2 of permutation 0: the output of the round of row 1, the input of the round of row 2
    prover = dev.MockProver.run_circuit(K_MANY, WidePermuteManyCircuit(WIDE, COUNT, limbs, trace=_bumped(trace, 7, 2)), [], FP)
    assert _gate_failures(prover, cs) == {("full round", 1), ("full round", 2)}
    with pytest.raises(front.Synthesis):
        dev.MockProver.run_circuit(K_MANY, WidePermuteManyCircuit(WIDE, COUNT), [], FP)
    with pytest.raises(ValueError):
        dev.MockProver.run_circuit(K_MANY, WidePermuteManyCircuit(WIDE, COUNT, limbs, trace=_up(trace[:4])), [], FP)


def _synthesized(circuit, k):
    cs, assembly, layouter = front.synthesize(circuit, k, FP, fixed=True, advice=True, instances=[])
    advice = [psc.ints_of(c, FP) for c in assembly.columns_to_field(assembly.advice)]
    fixed = [psc.ints_of(c, FP) for c in front.fixed_columns_of(assembly, cs)]
    return cs, assembly, layouter, advice, fixed


def test_bulk_permutations_equal_the_mirror_at_width_nine():
    k = 7
    inputs = pm.random_states(3, 9, FP, 0x720)
    a = _synthesized(WideMirrorCircuit(WIDE, inputs, bulk=False), k)
    b = _synthesized(WideMirrorCircuit(WIDE, inputs, bulk=True), k)
    assert a[2].regions[1] == b[2].regions[1] == 3                             # the permutations start under the inputs
    assert np.array_equal(a[1].selectors, b[1].selectors) and a[1].selectors[0].sum() == 3 * 8 and a[1].selectors[1].sum() == 3 * 28
    assert a[3] == b[3] and a[4] == b[4] and len(a[3]) == 10
    assert np.array_equal(a[1].permutation.flat(), b[1].permutation.flat()) and a[0].pinned() == b[0].pinned()
    model = pm.model(FP, *WIDE)
    assert [a[3][j][3 + 37 * i + 36] for i in range(3) for j in range(9)] == [w for s in inputs for w in model.permute(s)]


def test_hash_many_equals_the_cell_by_cell_hash_at_width_nine():
    k = 8
    model = pm.model(FP, *WIDE)
    messages = [s[:8] for s in pm.random_states(3, 9, FP, 0x730)]
    mirror, bulk = WideMirrorCircuit(WIDE, messages, bulk=False, hashing=True), WideMirrorCircuit(WIDE, messages, bulk=True, hashing=True)
    a, b = _synthesized(mirror, k), _synthesized(bulk, k)
    digests = [model.hash(msg) for msg in messages]
    assert psc.ints_of(bulk.many.digests, FP) == digests
    # the cell-by-cell hash lays an initial-state and an add-input region before every permutation; the 37 rows of the permutation
    # itself are the rows hash_many lays for that message, in all ten advice columns
    permutes = [start for start, (_, rows) in zip(a[2].regions, a[2].shapes) if rows == 37]
    assert len(permutes) == 3 and b[2].regions[1] == 3
    for i, start in enumerate(permutes):
        for column in range(10):
            assert a[3][column][start:start + 37] == b[3][column][3 + 37 * i:3 + 37 * (i + 1)], (i, column)
        assert a[3][0][start + 36] == digests[i]
        cell = mirror.outputs[i]
        assert a[2].regions[cell.region_index] + cell.row_offset == start + 36 and bulk.many.output_cell(i).row_offset == 37 * i + 36
    dev.MockProver.run_circuit(k, bulk, [], FP).assert_satisfied()
    dev.MockProver.run_circuit(k, mirror, [], FP).assert_satisfied()


# ---- the example -----------------------------------------------------------------------------------------------------------------------------
def test_wide_example_proves_verifies_and_rejects_a_wrong_digest():
    spec = importlib.util.spec_from_file_location("poseidon_wide", os.path.join(psc.ROOT, "examples", "poseidon_wide.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.main([]) is True
    message = pm.random_states(1, 8, FP, 0x740)[0]
    assert mod.public_digest(message) == pm.model(FP, *WIDE).hash(message) == Spec(FP, *WIDE).hash_ints(message)
