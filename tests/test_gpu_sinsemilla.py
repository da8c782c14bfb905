"""Sinsemilla on the device: the kernels of halo2_amd/csrc/sinsemilla.hip against the restatement of tests/sinsemilla_cases.py
(a fold with affine incomplete addition over `oracle.pasta` and `oracle.hash_to_curve`)."""
import numpy as np
import pytest

from halo2_amd import fields, sinsemilla
from halo2_amd._lib import lib
from halo2_amd.arithmetic import _p

import sinsemilla_cases as sc
from sinsemilla_cases import P, STRUCTURES

pytestmark = pytest.mark.gpu
FP = 0
ERR_ARGS = 1


def _up(a, dtype=np.int64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).to(fields.current_device())


def _ints(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else t
    return fields.from_limbs(np.ascontiguousarray(a).view(np.uint64).reshape(-1, 4), FP, True)


def _points(t):
    v = _ints(t)
    return [(v[i], v[i + 1]) for i in range(0, len(v), 2)]


def test_the_device_builds_the_specifications_table_and_q():
    """the 1024 generators and Q("z.cash:Orchard-MerkleCRH") the product derives with h2_hash_to_curve_device are the restated map's"""
    assert sinsemilla.generator_table_ints() == sc.table()
    assert sinsemilla.HashDomain(sc.MERKLE_DOMAIN).Q == sc.q_of(sc.MERKLE_DOMAIN)
    assert sinsemilla.generator_table() is sinsemilla.generator_table()                       # built once


@pytest.mark.parametrize("words", [0, 1, 2, 52, 253])
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_hash_against_the_restatement(n, words):
    """bit-exact x and y; partial waves and more than one workgroup; random words, all 0 and all 1023; no message is excused"""
    q, msgs, want = sc.message_pool()
    first = 2 if n == 1 else 0
    w = np.array([m[:words] for m in msgs[first:first + n]], dtype=np.uint16).reshape(n, words)
    dom = sinsemilla.HashDomain(q)
    pts, status = dom.hash_to_point(_up(w, np.int16), with_status=True)
    assert status.shape == (n,) and not status.any()
    assert _points(pts) == [want[first + i][words] for i in range(n)]
    if n == 65:                                                                               # numpy in, numpy out; hash = the x
        got = dom.hash(w)
        assert isinstance(got, np.ndarray) and _ints(got) == [want[i][words][0] for i in range(n)]


def test_hash_rejects_more_than_c_words():
    import torch
    dev = fields.current_device()
    w = torch.zeros((1, 254), dtype=torch.int16, device=dev)
    out = torch.zeros((1, 8), dtype=torch.int64, device=dev)
    status = torch.zeros((1,), dtype=torch.uint8, device=dev)
    q = np.ascontiguousarray(fields.to_limbs(list(sc.q_of(sc.MERKLE_DOMAIN)), FP).reshape(8))
    rc = lib().h2_sinsemilla_hash_device(w.data_ptr(), 1, 254, _p(q),
                                         sinsemilla.generator_table().data_ptr(), out.data_ptr(), status.data_ptr(), None)
    assert rc == ERR_ARGS and not out.any()
    with pytest.raises(ValueError):
        sinsemilla.HashDomain(sc.q_of(sc.MERKLE_DOMAIN)).hash_to_point(np.zeros((1, 254), dtype=np.uint16))


@pytest.mark.parametrize("case", range(4), ids=["doubling", "identity", "second-addition", "round-3-of-5"])
def test_exceptional_additions_are_bottom(case):
    """Q is free, so each exception of incomplete addition can be met on purpose: status 1 on exactly that lane and a zero point, 0 and
    the restated points on the random neighbours of the same launch; the restatement has no value for the same message"""
    name, q, m = sc.exceptional_cases()[case]
    assert sc.hash_to_point(q, m) is None
    rng = np.random.default_rng(case)
    w = rng.integers(0, 1024, size=(70, 5)).astype(np.uint16)
    w[:, 0] = np.where(w[:, 0] == m[0], (m[0] + 1) % 1024, w[:, 0])
    w[37] = m
    want = [sc.hash_to_point(q, [int(x) for x in row]) for row in w]
    assert [i for i, pt in enumerate(want) if pt is None] == [37], name
    dom = sinsemilla.HashDomain(q)
    pts, status = dom.hash_to_point(_up(w, np.int16), with_status=True)
    assert status.cpu().tolist() == [1 if i == 37 else 0 for i in range(70)]
    want[37] = (0, 0)
    assert _points(pts) == want
    with pytest.raises(sinsemilla.Bottom):
        dom.hash_to_point(w)


# ---- trace ------------------------------------------------------------------------------------------------------------------------------
def _trace_messages(structure, count):
    nw = STRUCTURES[structure]
    return nw, [sc.random_pieces(nw, 100 * len(nw) + i, high_zero=i % 3 == 1) for i in range(count)]


@pytest.mark.parametrize("count", [1, 65])
@pytest.mark.parametrize("structure", ["one", "merkle", "full"])
def test_trace_against_the_restated_witness(structure, count):
    """all five columns at every row; every third message has a piece whose high words are zero"""
    nw, msgs = _trace_messages(structure, count)
    if count == 1:
        msgs = [sc.random_pieces(nw, 9, high_zero=True)]
    q = sc.q_of(sc.MERKLE_DOMAIN)
    rows = sum(nw) + 1
    pieces = fields.to_limbs([p for m in msgs for p in m], FP, montgomery=False).reshape(count, len(nw), 4)
    cols, status = sinsemilla.trace(_up(pieces), nw, q, with_status=True)
    assert cols.shape == (5, rows * count, 4) and not status.any()
    got = [_ints(cols[c]) for c in range(5)]
    for i, m in enumerate(msgs):
        want = sc.trace(q, m, nw)
        for c in range(5):
            assert got[c][i * rows:(i + 1) * rows] == want[c], (i, c)
        assert (want[0][-1], want[3][-1]) == sc.hash_to_point(q, sc.words_of(m, nw))          # the last row is the hash
    # and the integers the host chip assigns cell by cell (tests/test_sinsemilla_host.py ties them to the restatement too)
    circuit = sc.HashCircuit(nw, msgs[:2], q, table=sc.table())
    _, assembly, layouter = sc.front.synthesize(circuit, 11, FP, fixed=False, advice=True, instances=[])
    advice = assembly.host_columns(assembly.advice)
    for i, point in enumerate(circuit.points):
        start = layouter.regions[point.x().cell().region_index]
        assert [advice[c][start:start + rows] for c in range(5)] == [got[c][i * rows:(i + 1) * rows] for c in range(5)]
    if count == 65 and structure == "merkle":                                                 # numpy in, numpy out
        host = sinsemilla.trace(pieces, nw, q)
        assert isinstance(host, np.ndarray) and (host.view(np.int64) == cols.cpu().numpy()).all()


def test_trace_reports_bottom_per_message():
    name, q, m = sc.exceptional_cases()[3]
    msgs = [[sum(w << (10 * j) for j, w in enumerate(m))], [12345], [999]]
    pieces = fields.to_limbs([p for mm in msgs for p in mm], FP, montgomery=False).reshape(3, 1, 4)
    cols, status = sinsemilla.trace(_up(pieces), [5], q, with_status=True)
    assert status.cpu().tolist() == [1, 0, 0]
    got = [_ints(cols[c]) for c in range(5)]
    for i in (1, 2):
        assert [got[c][6 * i:6 * i + 6] for c in range(5)] == sc.trace(q, msgs[i], [5])
    with pytest.raises(sinsemilla.Bottom):
        sinsemilla.trace(pieces, [5], q)


def test_trace_across_a_chunk_of_scratch():
    """the trace goes through its scratch in chunks of 2^20 // rows messages: one message more than a chunk of the structure `one`
    (2 rows), 65 messages over and over, so the rows on both sides of the boundary must be those of a call of their own"""
    import torch
    nw = STRUCTURES["one"]
    rows = sum(nw) + 1
    per_chunk = (1 << 20) // rows
    count = per_chunk + 1
    _, msgs = _trace_messages("one", 65)
    q = sc.q_of(sc.MERKLE_DOMAIN)
    p65 = _up(fields.to_limbs([p for m in msgs for p in m], FP, montgomery=False).reshape(65, 1, 4))
    reps = (count + 64) // 65
    cols, status = sinsemilla.trace(p65.repeat(reps, 1, 1)[:count].contiguous(), nw, q, with_status=True)
    want = sinsemilla.trace(p65, nw, q)
    assert not status.any()
    for i in (0, per_chunk - 2, per_chunk - 1, per_chunk, count - 1):
        j = i % 65
        assert torch.equal(cols[:, rows * i:rows * (i + 1)], want[:, rows * j:rows * (j + 1)]), i
    # in full, 65 messages at a time: a comparison against the broadcast `want` keeps the test's memory at the columns themselves
    whole, got, want = count // 65, cols.view(5, count, rows, 4), want.view(5, 65, rows, 4)
    assert bool((got[:, :65 * whole].view(5, whole, 65, rows, 4) == want[:, None]).all())
    assert torch.equal(got[:, 65 * whole:], want[:, :count - 65 * whole])


def test_trace_rejects_bad_structures():
    q = sc.q_of(sc.MERKLE_DOMAIN)
    for nw in ([26], [0], [25] * 10 + [4], []):
        with pytest.raises(ValueError):
            sinsemilla.trace(np.zeros((1, len(nw), 4), dtype=np.uint64), nw, q)


# ---- MerkleCRH --------------------------------------------------------------------------------------------------------------------------
def _leaves(n):
    import random
    rng = random.Random(n)
    return [rng.randrange(P) for _ in range(n - 2)] + [0, P - 1]


@pytest.mark.parametrize("layer", [0, 31])
def test_merkle_crh_against_the_fold(layer):
    q = sc.q_of(sc.MERKLE_DOMAIN)
    vals = _leaves(66)
    left, right = vals[:33], vals[33:]
    got = sinsemilla.merkle_crh(layer, _up(fields.to_limbs(left, FP)), _up(fields.to_limbs(right, FP)))
    assert _ints(got) == [sc.merkle_crh(q, layer, l, r) for l, r in zip(left, right)]
    # the same through the word interface
    w = np.array([sc.merkle_words(layer, l, r) for l, r in zip(left, right)], dtype=np.uint16)
    assert _ints(sinsemilla.HashDomain(sc.MERKLE_DOMAIN).hash(w)) == _ints(got)


@pytest.mark.parametrize("n", [2, 64])
def test_merkle_root_against_the_fold(n):
    leaves = _leaves(n)
    got = sinsemilla.merkle_root(fields.to_limbs(leaves, FP))
    assert isinstance(got, np.ndarray) and _ints(got) == [sc.merkle_root(sc.q_of(sc.MERKLE_DOMAIN), leaves)]


def test_merkle_root_rejects_three_leaves():
    with pytest.raises(ValueError):
        sinsemilla.merkle_root(fields.to_limbs(_leaves(3), FP))


# ---- the gadgets: the reference's keys and proofs, a fresh proof, the bulk path ------------------------------------------------------------
import halo2_amd as h                                                         # noqa: E402
from halo2_amd import circuit as front                                        # noqa: E402
from halo2_amd import dev                                                     # noqa: E402
from halo2_amd import verifier as hv                                          # noqa: E402
from halo2_amd.transcript import Blake2bWrite                                 # noqa: E402
from oracle import c_oracle as co                                             # noqa: E402
from oracle import plonk_api                                                  # noqa: E402

VESTA = h.VESTA                                                               # its scalar field is Fp, the field of the circuits


@pytest.fixture(scope="module")
def params11():
    params = h.Params.new(VESTA, 11)
    yield params
    params.close()


def _rng(seed):
    sf = co.field_of_curve(VESTA, "scalar")
    ctr = [seed]

    def rng(count):
        ctr[0] += 1
        return co.random_field(sf, ctr[0], count)
    return rng


def _golden(name):
    return open(sc.os.path.join(sc.GOLDEN, name), "rb").read()


@pytest.mark.parametrize("circuit, vk_name, proof_name, size", [
    (lambda: sc.MerkleCircuit(), "vk_merkle_chip.rdata.gz", "proof_merkle_chip.bin", 4160),
    (lambda: sc.LookupCircuit(6), "vk_lookup_range_check.rdata", "proof_lookup_range_check.bin", 1888)], ids=["merkle_chip", "lookup_range_check"])
def test_the_references_key_and_proof(params11, circuit, vk_name, proof_name, size):
    """keygen reproduces the reference's pinned key text bit for bit -- through the fixed-column commitments that is the whole generator
    table, Q, every gate and lookup and the floor plan -- and the verifier accepts the proof the reference stored"""
    text = sc.fixture_text(vk_name)
    vk = h.keygen_vk(params11, circuit())
    assert vk.pinned() == plonk_api.compact_debug(text)
    assert vk.vk_repr == plonk_api.transcript_repr(text)
    proof = _golden(proof_name)
    assert len(proof) == size
    assert hv.verify_proof_many(params11, vk, [[]], proof)
    bad = bytearray(proof)
    bad[size // 2] ^= 1
    assert not hv.verify_proof_many(params11, vk, [[]], bytes(bad))


def _kinds(failures):
    return {type(f).__name__ for f in failures}


def test_a_fresh_merkle_proof(params11):
    leaf, pos, path = sc.merkle_witness()
    circuit = sc.MerkleCircuit(leaf, pos, path)
    dev.MockProver.run_circuit(11, circuit, [], FP).assert_satisfied()
    assert circuit.root.value().inner.evaluate(P) == sc.merkle_path_root(sc.q_of(sc.TEST_DOMAIN), leaf, pos, path)
    pk = h.keygen_pk(params11, circuit)
    tr = Blake2bWrite(VESTA)
    h.create_proof(params11, pk, [circuit], [[]], _rng(11), tr)
    proof = tr.finalize()
    assert len(proof) == 4160 and hv.verify_proof(params11, pk.vk, [], proof)
    # a wrong sibling: the MockProver names the decomposition gate or the copies into it
    prover = dev.MockProver.run_circuit(11, sc.TamperedMerkleCircuit(leaf, pos, path), [], FP)
    failures = prover.verify()
    assert failures and _kinds(failures) <= {"ConstraintNotSatisfied", "Permutation"}
    cs, _, _ = front.synthesize(sc.MerkleCircuit().without_witnesses(), 11, FP, fixed=True, advice=False)
    gates = [g.name for g in cs.gates for _ in g.polys]
    assert {gates[f.gate_index] for f in failures if type(f).__name__ == "ConstraintNotSatisfied"} <= {"Decomposition check"}


def test_bulk_hashes_equal_the_mirror(params11):
    """65 hashes of the MerkleCRH structure through hash_to_point_many against 65 calls of hash_to_point: the same cells"""
    nw = STRUCTURES["merkle"]
    q = sc.q_of(sc.MERKLE_DOMAIN)
    msgs = [sc.random_pieces(nw, 700 + i, high_zero=i % 5 == 2) for i in range(65)]
    k = 12                                                                    # 65 * 53 rows under 65 * 3 rows of pieces
    sides = []
    for bulk in (False, True):
        circuit = sc.HashCircuit(nw, msgs, q, bulk=bulk)
        cs, assembly, layouter = front.synthesize(circuit, k, FP, fixed=True, advice=True, instances=[])
        selectors = assembly.selectors.copy()
        fixed = [_ints(c) for c in front.fixed_columns_of(assembly, cs)]
        advice = [_ints(c) for c in assembly.columns_to_field(assembly.advice)]
        sides.append((selectors, fixed, advice, assembly.permutation.flat().copy(), cs.pinned(), circuit))
    a, b = sides
    assert np.array_equal(a[0], b[0]) and a[0].sum() > 65 * 52
    assert a[1] == b[1] and a[2] == b[2]
    assert np.array_equal(a[3], b[3]) and a[4] == b[4]
    want = [sc.hash_to_point(q, sc.words_of(m, nw)) for m in msgs]
    assert [(p.x().value().inner.evaluate(P), p.y().value().inner.evaluate(P)) for p in a[5].points] == want
    assert _points(b[5].many.outputs) == want
    circuit = sc.HashCircuit(nw, msgs, q, bulk=True)
    dev.MockProver.run_circuit(k, circuit, [], FP).assert_satisfied()
    params = h.Params.new(VESTA, k)
    try:
        texts = [h.keygen_vk(params, sc.HashCircuit(nw, msgs, q, bulk=bulk)).pinned() for bulk in (False, True)]
        assert texts[0] == texts[1] and "fixed_commitments" in texts[0]
        pk = h.keygen_pk(params, circuit)
        tr = Blake2bWrite(VESTA)
        h.create_proof(params, pk, [circuit], [[]], _rng(12), tr)
        assert hv.verify_proof(params, pk.vk, [], tr.finalize())
    finally:
        params.close()


def test_the_example_proves_one_path():
    """examples/sinsemilla_merkle.py end to end: its circuit is the one the tests above run; its root is the fold's, through one
    merkle_crh launch per layer outside the circuit"""
    mod = sc._example("sinsemilla_merkle")
    leaf, pos, path = sc.merkle_witness()
    assert mod.root_outside_the_circuit(leaf, pos, path) == sc.merkle_path_root(sc.q_of(sc.TEST_DOMAIN), leaf, pos, path)
    assert mod.main(["--pos", "0x5A5AA5A5"])
