"""Sinsemilla commitments, hashing from a private point and the batched complete addition on the device: the kernels of
halo2_amd/csrc/sinsemilla_commit.hip against the restatement of tests/sinsemilla_commit_cases.py.  Every comparison is bit for bit."""
import functools

import numpy as np
import pytest

from halo2_amd import ecc, fields, sinsemilla
from halo2_amd._lib import lib
from halo2_amd.arithmetic import _p

import ecc_cases as ec
import sinsemilla_cases as sc
import sinsemilla_commit_cases as cc
from sinsemilla_cases import STRUCTURES

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


def _point_limbs(pts):
    return fields.to_limbs([c for pt in pts for c in pt], FP).reshape(len(pts), 8)


def _scalar_limbs(scalars):
    return fields.to_limbs(scalars, FP, montgomery=False).reshape(len(scalars), 4)


@functools.lru_cache(maxsize=None)
def domain():
    return sinsemilla.CommitDomain(cc.PERSONALIZATION)


def _lanes(n):
    """the first n messages of the pool; a lone lane takes a random one"""
    first = 2 if n == 1 else 0
    return list(range(first, first + n))


def _words(lanes, words):
    _, msgs, _ = sc.message_pool()
    return np.array([msgs[i][:words] for i in lanes], dtype=np.uint16).reshape(len(lanes), words)


def test_the_domain_is_the_reference_crates():
    dom = domain()
    assert dom.M.Q == cc.q_of(cc.PERSONALIZATION) == sc.q_of(sc.TEST_DOMAIN)
    assert dom.R == cc.r_of(cc.PERSONALIZATION)
    assert dom.fixed_base is dom.fixed_base and dom.fixed_base.num_windows == 85 and dom.fixed_base.generator() == dom.R


# ---- hashing from one Q per message ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("words", [0, 1, 52, 253])
@pytest.mark.parametrize("n", [1, 65, 257])
def test_hash_from_a_q_per_message(n, words):
    """a lone lane, a partial wave, more than one workgroup; Q_i alternates among two domains' Q and random points; no message is excused"""
    lanes = _lanes(n)
    qs, want = cc.private_qs(), cc.private_pool()
    dom = sinsemilla.HashDomain(sc.MERKLE_DOMAIN)
    pts, status = dom.hash_to_point(_up(_words(lanes, words), np.int16), with_status=True, Q=_up(_point_limbs([qs[i] for i in lanes])))
    assert status.shape == (n,) and not status.any()
    assert _points(pts) == [want[i][words] for i in lanes]
    if n == 65:                                                                               # numpy in, numpy out
        host = dom.hash_to_point(_words(lanes, words), Q=_point_limbs([qs[i] for i in lanes]))
        assert isinstance(host, np.ndarray) and _points(host) == _points(pts)


def test_hash_from_exceptional_qs_is_bottom_on_those_lanes_alone():
    """the four exceptions of incomplete addition as per-message Q on lanes 1, 64, 65 and 200, the identity as Q on lane 100"""
    rng = np.random.default_rng(5)
    w = rng.integers(0, 1024, size=(257, 5)).astype(np.uint16)
    qs = list(cc.private_qs())
    at = dict(zip((1, 64, 65, 200), sc.exceptional_cases()))
    for lane, (_, q, m) in at.items():
        qs[lane], w[lane] = q, m
    qs[100] = (0, 0)
    want = [None if i == 100 else sc.hash_to_point(qs[i], [int(x) for x in w[i]]) for i in range(257)]
    bottom = sorted(list(at) + [100])
    assert [i for i, pt in enumerate(want) if pt is None] == bottom
    dom = sinsemilla.HashDomain(sc.MERKLE_DOMAIN)
    pts, status = dom.hash_to_point(_up(w, np.int16), with_status=True, Q=_up(_point_limbs(qs)))
    assert status.cpu().tolist() == [1 if i in bottom else 0 for i in range(257)]
    assert _points(pts) == [cc.point(pt) for pt in want]
    with pytest.raises(sinsemilla.Bottom):
        dom.hash_to_point(w, Q=_point_limbs(qs))


# ---- commit --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("private", [False, True], ids=["shared-q", "q-per-message"])
@pytest.mark.parametrize("words", [0, 1, 50, 253])
@pytest.mark.parametrize("n", [1, 65, 257])
def test_commit_against_the_restatement(n, words, private):
    """the edge scalars of the fixed-base product lead (0, 1, q - 1, 2^255 - 1, the two last-doubling strings), random ones follow"""
    lanes = _lanes(n)
    scalars, blinds = cc.scalar_pool()
    hashes = cc.private_pool() if private else cc.shared_pool()
    want = [cc.group_add(hashes[i][words], cc.point(blinds[j])) for j, i in enumerate(lanes)]
    q = _up(_point_limbs([cc.private_qs()[i] for i in lanes])) if private else None
    r = _up(_scalar_limbs(scalars[:n]))
    pts, status = domain().commit(_up(_words(lanes, words), np.int16), r, with_status=True, Q=q)
    assert status.shape == (n,) and not status.any()
    assert _points(pts) == want
    short = domain().short_commit(_up(_words(lanes, words), np.int16), r, Q=q)
    assert short.shape == (n, 4) and _ints(short) == [pt[0] for pt in want]
    # the composition the fused kernel stands in for
    m = domain().M.hash_to_point(_up(_words(lanes, words), np.int16), Q=q)
    assert _points(ecc.add(m, ecc.mul_fixed(domain().fixed_base, r))) == want
    if n == 65 and words == 50:                                                               # numpy in, numpy out
        host = domain().commit(_words(lanes, words), _scalar_limbs(scalars[:n]), Q=None if q is None else q.cpu().numpy().view(np.uint64))
        assert isinstance(host, np.ndarray) and _points(host) == want


def test_commit_doubles_cancels_and_reports_only_the_hash():
    """beside random neighbours: a Q crafted so that the hash IS [r]R (the sum is the double), one so that it is -[r]R (the identity,
    status 0), and one whose chain meets an exceptional addition (status 1)"""
    n, doubling, identity, bottom = 70, 3, 64, 65
    rng = np.random.default_rng(8)
    w = rng.integers(0, 1024, size=(n, 5)).astype(np.uint16)
    qs = list(cc.private_qs()[:n])
    scalars = list(cc.scalar_pool()[0][:n])
    crafted = cc.crafted_cases()
    for lane, kind in ((doubling, "doubling"), (identity, "identity")):
        qs[lane], w[lane], scalars[lane] = crafted[kind], cc.CRAFT_WORDS, cc.CRAFT_R
    _, qs[bottom], w[bottom] = sc.exceptional_cases()[3]
    want = [cc.commit(qs[i], [int(x) for x in w[i]], scalars[i]) for i in range(n)]
    t = cc.blind(cc.CRAFT_R)
    assert want[doubling] == cc.group_add(t, t) and want[identity] == (0, 0) and [i for i in range(n) if want[i] is None] == [bottom]
    pts, status = domain().commit(_up(w, np.int16), _up(_scalar_limbs(scalars)), with_status=True, Q=_up(_point_limbs(qs)))
    assert status.cpu().tolist() == [1 if i == bottom else 0 for i in range(n)]
    assert _points(pts) == [cc.point(pt) for pt in want]
    with pytest.raises(sinsemilla.Bottom):
        domain().commit(w, _scalar_limbs(scalars), Q=_point_limbs(qs))
    # r = 0 leaves the hash
    zero = domain().commit(w[:2], _scalar_limbs([0, 0]), Q=_point_limbs(qs[:2]))
    assert _points(zero) == [sc.hash_to_point(qs[i], [int(x) for x in w[i]]) for i in range(2)]


def test_commit_wants_exactly_one_q_and_at_most_c_words():
    import torch
    dev = fields.current_device()
    dom = domain()
    w = torch.zeros((1, 254), dtype=torch.int16, device=dev)
    out = torch.zeros((1, 8), dtype=torch.int64, device=dev)
    status = torch.zeros((1,), dtype=torch.uint8, device=dev)
    r = torch.zeros((1, 4), dtype=torch.int64, device=dev)
    q = np.ascontiguousarray(fields.to_limbs(list(dom.M.Q), FP).reshape(8))
    d_q = _up(q.reshape(1, 8))
    table, points = sinsemilla.generator_table().data_ptr(), dom.fixed_base.points.data_ptr()

    def call(words, q_xy, d_q_xy):
        return lib().h2_sinsemilla_commit_device(w.data_ptr(), 1, words, q_xy, d_q_xy, table, points, r.data_ptr(), out.data_ptr(),
                                                 status.data_ptr(), None)
    assert call(5, _p(q), d_q.data_ptr()) == ERR_ARGS and call(5, None, None) == ERR_ARGS and call(254, _p(q), None) == ERR_ARGS
    assert lib().h2_sinsemilla_hash_from_device(w.data_ptr(), 1, 254, d_q.data_ptr(), table, out.data_ptr(), status.data_ptr(), None) == ERR_ARGS
    assert not out.any()
    assert call(5, _p(q), None) == 0 and call(5, None, d_q.data_ptr()) == 0
    with pytest.raises(ValueError):
        dom.commit(np.zeros((1, 254), dtype=np.uint16), np.zeros((1, 4), dtype=np.uint64))


# ---- the batched complete addition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 6, 257])
def test_add_and_its_witness_on_every_branch(n):
    """P + Q, P + P, P + (-P), P + 0, 0 + Q, 0 + 0 in turn: all 11 elements of every row against add.rs restated with inv0"""
    pairs = cc.add_pairs(n)
    p, q = _up(_point_limbs([a for a, _ in pairs])), _up(_point_limbs([b for _, b in pairs]))
    aux = ecc.add_trace(p, q)
    assert aux.shape == (n, ecc.FIXED_AUX, 4)
    want = [cc.add_row(a, b) for a, b in pairs]
    assert _ints(aux) == [v for row in want for v in row]
    assert _points(ecc.add(p, q)) == [tuple(row[9:]) for row in want]
    if n == 6:
        assert [tuple(row[9:]) for row in want] == [cc.group_add(*pair) for pair in pairs]
        host = ecc.add(_point_limbs([a for a, _ in pairs]), _point_limbs([b for _, b in pairs]))
        assert isinstance(host, np.ndarray) and _points(host) == [tuple(row[9:]) for row in want]


# ---- the trace from a Q per message -----------------------------------------------------------------------------------------------------------
TRACE_STRUCTURES = {"one": STRUCTURES["one"], "merkle": STRUCTURES["merkle"], "commit": cc.COMMIT_WORDS}


@pytest.mark.parametrize("count", [1, 3, 65])
@pytest.mark.parametrize("structure", ["one", "merkle", "commit"])
def test_trace_from_against_the_restated_witness(structure, count):
    """every element of the five columns, the row of y_Q included, each message from its own Q"""
    nw = TRACE_STRUCTURES[structure]
    msgs = cc.random_messages(nw, count, seed=len(nw))
    qs = cc.private_qs()[:count]
    rows = sum(nw) + 2
    pieces = fields.to_limbs([p for m in msgs for p in m], FP, montgomery=False).reshape(count, len(nw), 4)
    cols, status = sinsemilla.trace_from(_up(pieces), nw, _up(_point_limbs(qs)), with_status=True)
    assert cols.shape == (5, rows * count, 4) and not status.any()
    got = [_ints(cols[c]) for c in range(5)]
    for i, m in enumerate(msgs):
        want = cc.trace_from(qs[i], m, nw)
        for c in range(5):
            assert got[c][i * rows:(i + 1) * rows] == want[c], (i, c)
    if count == 3:                                                                            # one (x, y) pair for all; numpy in, numpy out
        host = sinsemilla.trace_from(pieces, nw, qs[1])
        assert isinstance(host, np.ndarray)
        got = [_ints(host[c]) for c in range(5)]
        for i, m in enumerate(msgs):
            assert [got[c][i * rows:(i + 1) * rows] for c in range(5)] == cc.trace_from(qs[1], m, nw)


def test_trace_from_reports_bottom_per_message():
    _, q, m = sc.exceptional_cases()[3]
    msgs = [[12345], [sum(w << (10 * j) for j, w in enumerate(m))], [999]]
    qs = [cc.private_qs()[2], q, cc.private_qs()[0]]
    pieces = fields.to_limbs([p for mm in msgs for p in mm], FP, montgomery=False).reshape(3, 1, 4)
    cols, status = sinsemilla.trace_from(_up(pieces), [5], _up(_point_limbs(qs)), with_status=True)
    assert status.cpu().tolist() == [0, 1, 0]
    got = [_ints(cols[c]) for c in range(5)]
    for i in (0, 2):
        assert [got[c][7 * i:7 * i + 7] for c in range(5)] == cc.trace_from(qs[i], msgs[i], [5])
    with pytest.raises(sinsemilla.Bottom):
        sinsemilla.trace_from(pieces, [5], _point_limbs(qs))


def test_trace_from_across_a_chunk_of_scratch():
    """the trace goes through its scratch in chunks of 2^20 // rows messages: one message more than a chunk of the structure `one`
    (3 rows), 65 messages over and over, so the rows on both sides of the boundary must be those of a call of their own"""
    import torch
    nw = STRUCTURES["one"]
    rows = sum(nw) + 2
    per_chunk = (1 << 20) // rows
    count = per_chunk + 1
    msgs = cc.random_messages(nw, 65, seed=7)
    p65 = _up(fields.to_limbs([p for m in msgs for p in m], FP, montgomery=False).reshape(65, 1, 4))
    q65 = _up(_point_limbs(cc.private_qs()[:65]))
    reps = (count + 64) // 65
    cols, status = sinsemilla.trace_from(p65.repeat(reps, 1, 1)[:count].contiguous(), nw, q65.repeat(reps, 1)[:count].contiguous(), with_status=True)
    want = sinsemilla.trace_from(p65, nw, q65)
    assert not status.any()
    for i in (0, per_chunk - 2, per_chunk - 1, per_chunk, count - 1):
        j = i % 65
        assert torch.equal(cols[:, rows * i:rows * (i + 1)], want[:, rows * j:rows * (j + 1)]), i
    assert torch.equal(cols.view(5, count, rows, 4), want.view(5, 65, rows, 4).repeat(1, reps, 1, 1)[:, :count])


# ---- the gadgets: the reference's key and proof, private init, the bulk path ---------------------------------------------------------------------
import halo2_amd as h                                                         # noqa: E402
from halo2_amd import circuit as front                                        # noqa: E402
from halo2_amd import dev                                                     # noqa: E402
from halo2_amd import verifier as hv                                          # noqa: E402
from halo2_amd.gadgets import sinsemilla as g                                 # noqa: E402
from halo2_amd.transcript import Blake2bWrite                                 # noqa: E402
from oracle import c_oracle as co                                             # noqa: E402
from oracle import plonk_api                                                  # noqa: E402

VESTA = h.VESTA
P = sc.P
VK_NAME, PROOF_NAME, PROOF_SIZE = "vk_sinsemilla_chip.rdata.gz", "proof_sinsemilla_chip.bin", 4576


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


@functools.lru_cache(maxsize=None)
def device_domain():
    """Q and R's tables as the device built them"""
    return g.CommitDomains.of(domain())


def test_the_device_tables_of_r_are_the_host_tables():
    t, host = device_domain().R, cc.host_r_tables()
    assert (t.generator, t.window_table, t.lagrange_coeffs, t.z) == (host.generator, host.window_table, host.lagrange_coeffs, host.z)
    assert device_domain().Q == cc.q_of(cc.PERSONALIZATION)


def test_the_references_key_and_proof(params11):
    """keygen of the `MySinsemillaCircuit` mirror over the DEVICE's generator table and tables of R reproduces the reference's pinned key
    text bit for bit -- the Sinsemilla chip, the fixed-base chip and the complete addition laid out together as the reference lays them
    -- and the verifier accepts the proof the reference stored"""
    text = sc.fixture_text(VK_NAME)
    vk = h.keygen_vk(params11, cc.MySinsemillaCircuit(device_domain()).without_witnesses())
    assert vk.pinned() == plonk_api.compact_debug(text)
    assert vk.vk_repr == plonk_api.transcript_repr(text)
    proof = open(sc.os.path.join(sc.GOLDEN, PROOF_NAME), "rb").read()
    assert len(proof) == PROOF_SIZE
    assert hv.verify_proof_many(params11, vk, [[]], proof)
    bad = bytearray(proof)
    bad[PROOF_SIZE // 2] ^= 1
    assert not hv.verify_proof_many(params11, vk, [[]], bytes(bad))


def test_the_references_circuit_with_a_seeded_witness(params11):
    """the device MockProver is satisfied, and a fresh proof has the stored proof's size and verifies under the key the reference pins"""
    circuit = cc.MySinsemillaCircuit(device_domain(), seed=7)
    dev.MockProver.run_circuit(11, circuit, [], FP).assert_satisfied()
    pk = h.keygen_pk(params11, circuit)
    assert pk.vk_repr == plonk_api.transcript_repr(sc.fixture_text(VK_NAME))
    tr = Blake2bWrite(VESTA)
    h.create_proof(params11, pk, [circuit], [[]], _rng(21), tr)
    proof = tr.finalize()
    assert len(proof) == PROOF_SIZE and hv.verify_proof(params11, pk.vk, [], proof)


def test_hashing_from_a_private_point(params11):
    """the same circuit on chips configured with allow_init_from_private_point, plus a hash from a witnessed Q: satisfied, proved and
    verified; a y_Q changed on row 0 of that hash is reported by the gate that reads it, one row below; without the flag the call raises"""
    circuit = cc.MySinsemillaCircuit(device_domain(), seed=7, private=True)
    dev.MockProver.run_circuit(11, circuit, [], FP).assert_satisfied()
    pk = h.keygen_pk(params11, circuit)
    assert pk.vk_repr != plonk_api.transcript_repr(sc.fixture_text(VK_NAME))
    tr = Blake2bWrite(VESTA)
    h.create_proof(params11, pk, [circuit], [[]], _rng(22), tr)
    assert hv.verify_proof(params11, pk.vk, [], tr.finalize())
    mutated = cc.MySinsemillaCircuit(device_domain(), seed=7, private=True, mutate=True)
    failures = dev.MockProver.run_circuit(11, mutated, [], FP).verify()
    cs, _, _ = front.synthesize(mutated.without_witnesses(), 11, FP, fixed=True, advice=False)
    names = [(gate.name, n) for gate in cs.gates for n in gate.constraint_names]
    gates = [f for f in failures if type(f).__name__ == "ConstraintNotSatisfied"]
    assert [names[f.gate_index] + (f.row,) for f in gates] == [("Initial y_Q", "init_y_q_check", mutated.mutated_row + 1)]
    assert {type(f).__name__ for f in failures} == {"ConstraintNotSatisfied", "Permutation"}  # and the copy of Q's y
    with pytest.raises(g.IllegalHashFromPrivatePoint):
        front.synthesize(cc.MySinsemillaCircuit(device_domain(), seed=7, private=True, flag=False), 11, FP, fixed=True, advice=True, instances=[])


@pytest.mark.parametrize("private", [False, True], ids=["public-q", "private-q"])
def test_bulk_hashes_on_a_flagged_chip_equal_the_calls(private):
    """`hash_to_point_many` on a chip with allow_init_from_private_point, from a public Q under its extra row and from one witnessed Q
    per hash, through `trace_from`: every selector, fixed and advice cell and every copy of 5 calls of `hash_to_point` or of
    `hash_to_point_with_private_init`"""
    nw = STRUCTURES["merkle"]
    msgs = cc.random_messages(nw, 5, seed=4)
    start = list(cc.private_qs()[:5]) if private else cc.q_of(cc.PERSONALIZATION)
    sides = []
    for bulk in (False, True):
        circuit = cc.FlaggedHashCircuit(nw, msgs, start, bulk=bulk)
        cs, assembly, _ = front.synthesize(circuit, 11, FP, fixed=True, advice=True, instances=[])
        fixed = [_ints(c) for c in assembly.columns_to_field(assembly.fixed)]
        advice = [_ints(c) for c in assembly.columns_to_field(assembly.advice)]
        sides.append((assembly.selectors.copy(), fixed, advice, assembly.permutation.flat().copy(), cs.pinned(), circuit))
    a, b = sides
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and np.array_equal(a[3], b[3]) and a[4] == b[4]
    want = [sc.hash_to_point(start[i] if private else start, sc.words_of(m, nw)) for i, m in enumerate(msgs)]
    assert [(p.x().value().inner.evaluate(P), p.y().value().inner.evaluate(P)) for p in a[5].points] == want
    assert _points(b[5].many.outputs) == want and b[5].many.first == 1 and b[5].many.rows == 54
    dev.MockProver.run_circuit(11, cc.FlaggedHashCircuit(nw, msgs, start, bulk=True), [], FP).assert_satisfied()


def _commit_inputs(count):
    scalars = cc.scalar_pool()[0]
    scalars = scalars[5:6] if count == 1 else scalars[:count]                  # count = 1: the unreduced doubling string
    rng = cc.random.Random(90 + count)
    return [rng.getrandbits(500) for _ in range(count)], list(scalars)


@pytest.mark.parametrize("count", [1, 3])
def test_commit_many_lays_the_rows_of_commit(count):
    """the advice columns, the fixed columns of the tables and of the hash, and the selectors of the three bulk regions (and of the
    fixed-base products' closing additions) are the regions of `count` calls of `commit` one after the other"""
    messages, scalars = _commit_inputs(count)
    sides = []
    for many in (False, True):
        circuit = cc.CommitCircuit(messages, scalars, device_domain(), many=many)
        _, assembly, layouter = front.synthesize(circuit, 11, FP, fixed=True, advice=True, instances=[])
        advice = [_ints(c) for c in assembly.columns_to_field(assembly.advice)]
        fixed = [_ints(c) for c in assembly.columns_to_field(assembly.fixed)]
        sides.append((circuit, advice, fixed, assembly.selectors, layouter))
    (one, a, fa, sa, la), (bulk, b, fb, sb, lb) = sides
    ecc_config, _, chip = bulk.config
    tables = [c.index for c in ecc_config.mul_fixed.lagrange_coeffs] + [ecc_config.mul_fixed.fixed_z.index, chip.q_sinsemilla2.index]
    many = bulk.bulk
    hash_rows = many.hashes.rows
    assert hash_rows == 51 and many.hashes.first == 0
    for i, (point, _) in enumerate(one.results):
        last = point.inner().x().cell().region_index                          # "M + [r] R"; before it "M", and the product's two regions
        spans = [(la.regions[last - 3], lb.regions[many.blinds.region_index] + 85 * i, 85, range(0, 6)),
                 (la.regions[last - 2], lb.regions[many.blinds.add_region_index] + 2 * i, 2, range(0, 9)),
                 (la.regions[last - 1], lb.regions[many.hashes.region_index] + hash_rows * i, hash_rows, range(5, 10)),
                 (la.regions[last], lb.regions[many.add_region_index] + 2 * i, 2, range(0, 9))]
        for at, start, rows, columns in spans:
            for c in columns:
                assert b[c][start:start + rows] == a[c][at:at + rows], (i, c, at)
            for c in tables:
                assert fb[c][start:start + rows] == fa[c][at:at + rows], (i, c, at)
            assert (sb[:, start:start + rows] == sa[:, at:at + rows]).all(), (i, at)
    want = [cc.commit(cc.q_of(cc.PERSONALIZATION), sc.words_of([m], [50]), k) for m, k in zip(messages, scalars)]
    assert _points(many.outputs) == want
    assert [(pt.inner().x().value().inner.evaluate(P), pt.inner().y().value().inner.evaluate(P)) for pt, _ in one.results] == want
    assert many.result_y(count - 1).row_offset == 2 * count - 1 and many.hashes.z(0, 1, 24).row_offset == 49


def test_commit_many_keygen_and_65_commitments():
    """keygen lays out the same shape without a witness; the device MockProver is satisfied at 65 commitments, the edge scalars in front"""
    messages, scalars = _commit_inputs(3)
    params = h.Params.new(VESTA, 11)
    try:
        with_witness = h.keygen_vk(params, cc.CommitCircuit(messages, scalars, device_domain(), many=True))
        assert h.keygen_vk(params, cc.CommitCircuit(messages, scalars, device_domain(), many=True).without_witnesses()).vk_repr == with_witness.vk_repr
        assert h.keygen_vk(params, cc.CommitCircuit(messages, scalars, cc.host_domain(), many=True).without_witnesses()).vk_repr == with_witness.vk_repr
    finally:
        params.close()
    messages, scalars = _commit_inputs(65)
    circuit = cc.CommitCircuit(messages, scalars, device_domain(), many=True)
    dev.MockProver.run_circuit(14, circuit, [], FP).assert_satisfied()
    want = [cc.group_add(cc.shared_words_hash(m), cc.point(b)) for m, b in zip(messages, cc.scalar_pool()[1][:65])]
    assert _points(circuit.bulk.outputs) == want


def test_the_example_proves_two_commitments():
    """examples/sinsemilla_commit.py end to end"""
    assert sc._example("sinsemilla_commit").main(["--count", "2"]) is True
