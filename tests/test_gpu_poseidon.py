"""Poseidon on the device: the three kernels of halo2_amd/csrc/poseidon.hip against `oracle.pasta.poseidon_permute`, Python integers
and the fixtures; the Pow5 chip's ported reference circuits, the bulk assignment `permute_many` against the cell-by-cell mirror, and
the Merkle example, through MockProver, keygen, create_proof and verify_proof."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import halo2_amd as h
from halo2_amd import dev, fields, poseidon
from halo2_amd import circuit as front
from halo2_amd import verifier as hv
from halo2_amd.transcript import Blake2bWrite
from oracle import c_oracle as co

import poseidon_cases as pc
from poseidon_cases import FP, FQ, HASH_KAT, KAT, MOD, NAME, ROWS, HashCircuit, MirrorCircuit, PermuteCircuit, PermuteManyCircuit

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VESTA = h.VESTA                                                                   # its scalar field is Fp, the field of the circuits


def _up(limbs):
    import torch
    return torch.from_numpy(np.ascontiguousarray(limbs).view(np.int64)).to(fields.current_device())


def _ints(t, field):
    a = t.cpu().numpy() if hasattr(t, "cpu") else t
    return fields.from_limbs(np.ascontiguousarray(a).view(np.uint64).reshape(-1, 4), field, True)


def _rng(seed):
    sf = co.field_of_curve(VESTA, "scalar")
    ctr = [seed]

    def rng(count):
        ctr[0] += 1
        return co.random_field(sf, ctr[0], count)
    return rng


# ---- permute -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pool(field):
    """257 states and their permutations: the 11 fixture vectors, the all-zero state, the state of all p - 1, random ones."""
    m = MOD[field]
    states = [[int(x, 16) for x in v["initial_state"]] for v in KAT[NAME[field]]["permute"]] + [[0, 0, 0], [m - 1] * 3]
    states += pc.random_states(257 - len(states), field, 7 + field)
    return states, [pc.permute_ints(s, field) for s in states]


@pytest.mark.parametrize("field", [FP, FQ])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_permute_against_the_oracle(field, n):
    states, want = _pool(field)
    first = 12 if n == 1 else 0                                                   # one state alone: all p - 1
    d_states = _up(pc.states_limbs(states[first:first + n], field))
    before = d_states.clone()
    out = poseidon.permute(d_states, field)
    assert out.shape == (n, 3, 4) and _ints(out, field) == [w for s in want[first:first + n] for w in s]
    assert (d_states == before).all()                                            # out of place leaves the input alone
    assert poseidon.permute(d_states, field, out=d_states) is d_states and (d_states == out).all()      # in place
    if n == 65:                                                                   # numpy in, numpy out
        got = poseidon.permute(pc.states_limbs(states[:n], field), field)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint64 and _ints(got, field) == [w for s in want[:n] for w in s]


def test_fixture_vectors_come_out_of_permute():
    for field in (FP, FQ):
        vectors = KAT[NAME[field]]["permute"]
        got = _ints(poseidon.permute(_up(pc.states_limbs([[int(x, 16) for x in v["initial_state"]] for v in vectors], field)), field), field)
        assert got == [int(x, 16) for v in vectors for x in v["final_state"]]
    assert poseidon.permute(_up(np.zeros((0, 3, 4), dtype=np.uint64)), FP).shape == (0, 3, 4)
    with pytest.raises(ValueError):
        poseidon.permute(np.zeros((2, 2, 4), dtype=np.uint64), FP)


# ---- hash, merkle_root -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [FP, FQ])
@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("length", [1, 2, 3, 4, 5])
def test_hash_against_the_restated_sponge(field, n, length):
    words = [w for s in pc.random_states((n * length + 2) // 3, field, 100 * length + n + field) for w in s][:n * length]
    words[0], words[-1] = MOD[field] - 1, 0
    messages = [words[i * length:(i + 1) * length] for i in range(n)]
    got = poseidon.hash(_up(fields.to_limbs(words, field, True).reshape(n, length, 4)), field)
    assert got.shape == (n, 4) and _ints(got, field) == [pc.hash_ints(msg, field) for msg in messages]


@pytest.mark.parametrize("field", [FP, FQ])
def test_reference_hash_vectors_bit_for_bit(field):
    vectors = HASH_KAT[NAME[field]]["hash"]
    inputs = fields.to_limbs([int(x, 16) for v in vectors for x in v["input"]], field, True).reshape(len(vectors), 2, 4)
    want = fields.to_limbs([int(v["output"], 16) for v in vectors], field, True)
    assert np.array_equal(poseidon.hash(inputs, field), want)                     # the host-array form
    assert np.array_equal(poseidon.hash(_up(inputs), field).cpu().numpy().view(np.uint64), want)
    with pytest.raises(ValueError):
        poseidon.hash(np.zeros((3, 0, 4), dtype=np.uint64), field)


@pytest.mark.parametrize("field", [FP, FQ])
@pytest.mark.parametrize("n_leaves", [8, 64])
def test_merkle_root(field, n_leaves):
    leaves = [s[0] for s in pc.random_states(n_leaves, field, 300 + n_leaves)]
    root = poseidon.merkle_root(_up(fields.to_limbs(leaves, field, True)), field)
    assert root.shape == (4,) and root.is_cuda and _ints(root, field) == [pc.merkle_root_ints(leaves, field)]
    with pytest.raises(ValueError):
        poseidon.merkle_root(np.zeros((6, 4), dtype=np.uint64), field)


# ---- trace ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [FP, FQ])
@pytest.mark.parametrize("count", [1, 3, 65])
def test_trace_every_cell(field, count):
    states, _ = _pool(field)
    states = states[12:12 + count]                                                # all p - 1 first
    want = pc.trace_limbs(states, field)
    got = poseidon.trace(_up(pc.states_limbs(states, field)), field)
    assert got.shape == (4, ROWS * count, 4)
    got = got.cpu().numpy().view(np.uint64)
    for column in range(4):
        assert np.array_equal(got[column], want[column]), f"column {column}"
    sbox = np.array([v != 0 for v in _ints(got[3], field)]).reshape(count, ROWS)
    assert not sbox[:, :4].any() and not sbox[:, 32:].any() and sbox[:, 4:32].all()


# ---- the ported reference circuits --------------------------------------------------------------------------------------------------------------
def _kinds(failures):
    return {type(f).__name__ for f in failures}


def test_ported_permute_circuit():
    dev.MockProver.run_circuit(6, PermuteCircuit(), [], FP).assert_satisfied()
    wrong = pc.permute_ints([0, 1, 2], FP)
    wrong[2] = (wrong[2] + 1) % MOD[FP]
    assert _kinds(dev.MockProver.run_circuit(6, PermuteCircuit(wrong), [], FP).verify()) == {"Permutation"}


def test_ported_hash_circuit():
    message = [s[0] for s in pc.random_states(2, FP, 41)]
    digest = pc.hash_ints(message, FP)
    dev.MockProver.run_circuit(6, HashCircuit(2, message, digest), [], FP).assert_satisfied()
    assert _kinds(dev.MockProver.run_circuit(6, HashCircuit(2, message, (digest + 1) % MOD[FP]), [], FP).verify()) == {"Permutation"}


def test_ported_longer_hash_circuit_proves_and_verifies():
    from oracle import pasta as o
    from oracle import plonk as op
    from oracle import plonk_api as pa
    k = 7
    message = [s[0] for s in pc.random_states(3, FP, 43)]
    digest = pc.hash_ints(message, FP)
    circuit = HashCircuit(3, message, digest)
    dev.MockProver.run_circuit(k, circuit, [], FP).assert_satisfied()
    failures = dev.MockProver.run_circuit(k, HashCircuit(3, message, (digest + 1) % MOD[FP]), [], FP).verify()
    assert failures and _kinds(failures) == {"Permutation"}                      # the digest + 1 has no proof: the copy of the output fails
    params = h.Params.new(VESTA, k)
    pk = h.keygen_pk(params, circuit)
    assert "Selector" not in pk.pinned() and pk.cs.degree == 6                    # compression never raises the degree
    tr = Blake2bWrite(VESTA)
    h.create_proof(params, pk, [circuit], [[]], _rng(7), tr)
    proof = tr.finalize()
    assert hv.verify_proof(params, pk.vk, [], proof)
    bad = bytearray(proof)
    bad[len(bad) // 2] ^= 1
    assert not hv.verify_proof(params, pk.vk, [], bytes(bad))
    # the restated verifier takes the same key
    g, _, w, u = pa.params_new("vesta", k, with_lagrange=False)
    ovk = {"cs": pk.cs, "vk_repr": pk.vk_repr, "domain": o.EvaluationDomain(pk.cs.degree, k, o.P),
           "fixed_commitments": pk.vk.fixed_commitments, "permutation_commitments": pk.vk.permutation_commitments}
    assert op.verify_proof_many(VESTA, k, co.points_to_mont(VESTA, g), co.points_to_mont(VESTA, [w])[0], co.points_to_mont(VESTA, [u])[0],
                                ovk, [[]], proof)
    params.close()


def test_reference_hash_vectors_in_circuit():
    for v in HASH_KAT["fp"]["hash"]:
        message, output = [int(x, 16) for x in v["input"]], int(v["output"], 16)
        dev.MockProver.run_circuit(6, HashCircuit(2, message, output), [], FP).assert_satisfied()


# ---- permute_many ----------------------------------------------------------------------------------------------------------------------------
COUNT, K_MANY = 65, 12


@functools.lru_cache(maxsize=None)
def _many():
    states, want = _pool(FP)
    return states[:COUNT], want[:COUNT], pc.trace_limbs(states[:COUNT], FP)


def _gate_failures(prover, cs_of):
    """{(gate name, row)} of the failures, all of which must be ConstraintNotSatisfied"""
    failures = prover.verify()
    assert failures and _kinds(failures) == {"ConstraintNotSatisfied"}
    return {(pc.gate_of_polynomial(cs_of, f.gate_index)[0], f.row) for f in failures}


def _bumped(trace, column, row):
    """the restated trace with one cell off by one, on the device"""
    t = trace.copy()
    t[column, row] = fields.to_limbs([(fields.from_limbs(t[column, row], FP, True)[0] + 1) % MOD[FP]], FP, True)[0]
    return _up(t)


def test_permute_many_mock_proves_and_names_a_broken_cell():
    states, want, trace = _many()
    limbs = _up(pc.states_limbs(states, FP))
    circuit = PermuteManyCircuit(COUNT, limbs)
    dev.MockProver.run_circuit(K_MANY, circuit, [], FP).assert_satisfied()
    assert circuit.result.count == COUNT and _ints(circuit.result.outputs, FP) == [w for s in want for w in s]
    assert circuit.result.input_cell(64, 2) == front.Cell(0, 64 * ROWS, front.Column("advice", 2))
    assert circuit.result.output_cell(1, 0) == front.Cell(0, 2 * ROWS - 1, front.Column("advice", 0))
    cs, _, _ = front.synthesize(PermuteManyCircuit(COUNT), K_MANY, FP, fixed=True, advice=False)      # the gates' names; no witness, no launch
    # the restated witness handed in as it is: satisfied too
    dev.MockProver.run_circuit(K_MANY, PermuteManyCircuit(COUNT, limbs, trace=_up(trace)), [], FP).assert_satisfied()
    # partial_sbox of permutation 64, row 17
    prover = dev.MockProver.run_circuit(K_MANY, PermuteManyCircuit(COUNT, limbs, trace=_bumped(trace, 3, 64 * ROWS + 17)), [], FP)
    assert _gate_failures(prover, cs) == {("partial rounds", 64 * ROWS + 17)}
    # state word 1 on row 2 of permutation 0: the output of the round of row 1, the input of the round of row 2
    prover = dev.MockProver.run_circuit(K_MANY, PermuteManyCircuit(COUNT, limbs, trace=_bumped(trace, 1, 2)), [], FP)
    assert _gate_failures(prover, cs) == {("full round", 1), ("full round", 2)}


def test_permute_many_without_a_witness():
    with pytest.raises(front.Synthesis):
        dev.MockProver.run_circuit(8, PermuteManyCircuit(3), [], FP)
    with pytest.raises(front.NotEnoughRowsAvailable):
        front.synthesize(PermuteManyCircuit(7), 8, FP, fixed=True, advice=False)  # 259 rows


def test_bulk_layout_equals_the_mirror():
    k = 8
    inputs = pc.random_states(5, FP, 77)
    sides = []
    for bulk in (False, True):
        cs, assembly, layouter = front.synthesize(MirrorCircuit(inputs, bulk), k, FP, fixed=True, advice=True, instances=[])
        selectors = assembly.selectors.copy()
        fixed = [_ints(c, FP) for c in front.fixed_columns_of(assembly, cs)]
        advice = [_ints(c, FP) for c in assembly.columns_to_field(assembly.advice)]
        sides.append((selectors, fixed, advice, assembly.permutation.flat().copy(), cs.pinned(), layouter.regions[1]))
    a, b = sides
    assert a[5] == b[5] == 5                                                      # the permutations start under the inputs
    assert np.array_equal(a[0], b[0]) and a[0][0].sum() == 40 and a[0][1].sum() == 140
    assert a[1] == b[1] and len(a[1]) > 6                                         # six constant columns and the compressed selectors
    assert a[2] == b[2]
    assert np.array_equal(a[3], b[3]) and a[4] == b[4]
    want = [w for s in inputs for w in pc.permute_ints(s, FP)]
    assert [a[2][j][5 + ROWS * i + ROWS - 1] for i in range(5) for j in range(3)] == want
    params = h.Params.new(VESTA, k)
    texts = [h.keygen_vk(params, MirrorCircuit(inputs, bulk)).pinned() for bulk in (False, True)]
    params.close()
    assert texts[0] == texts[1] and "fixed_commitments" in texts[0]


# ---- the example -----------------------------------------------------------------------------------------------------------------------------
def test_merkle_example_proves_verifies_and_rejects_a_wrong_root():
    spec = importlib.util.spec_from_file_location("poseidon_merkle", os.path.join(ROOT, "examples", "poseidon_merkle.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    k, n_leaves = 12, 64
    leaves = [s[0] for s in pc.random_states(n_leaves, FP, 900)]
    root = pc.merkle_root_ints(leaves, FP)
    circuit = mod.MerkleCircuit(n_leaves, _up(fields.to_limbs(leaves, FP, True)))
    assert mod.public_root(circuit.leaves, FP) == root
    blank = circuit.without_witnesses()
    assert blank.leaves is None                                                   # keygen runs with every witness None
    _, assembly, layouter = front.synthesize(blank, k, FP, fixed=True, advice=False)
    assert sum(rows for _, rows in layouter.shapes) == 63 * ROWS and assembly.selectors[0].sum() == 63 * 8
    dev.MockProver.run_circuit(k, circuit, [[root]], FP).assert_satisfied()
    assert _kinds(dev.MockProver.run_circuit(k, circuit, [[root + 1]], FP).verify()) == {"Permutation"}
    params = h.Params.new(VESTA, k)
    pk, proof, _, _ = mod.prove(params, circuit)
    assert hv.verify_proof(params, pk.vk, [[root]], proof)
    assert not hv.verify_proof(params, pk.vk, [[root + 1]], proof)
    params.close()
