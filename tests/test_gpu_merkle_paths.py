"""The bulk Merkle paths on the device: h2_sinsemilla_merkle_paths_device and h2_sinsemilla_merkle_trace_device bit for bit against the
integer model of tests/merkle_path_cases.py over its case list, bottom, every refusal, stream order, and `MerklePaths.calculate_roots`
against as many `MerklePath.calculate_root` calls: MockProver with regions, the multiset of every advice column, selector rows and
copies, four tampered witnesses that must fail at the right constraint, and a proof with public roots."""
import ctypes as C

import numpy as np
import pytest
import torch

import halo2_amd as h
from halo2_amd import _lib, dev, fields, sinsemilla
from halo2_amd import circuit as front
from halo2_amd import verifier as hv
from halo2_amd.transcript import Blake2bWrite
from oracle import c_oracle as co

import merkle_path_cases as mp
import sinsemilla_cases as sc
import stream_cases as stc

pytestmark = pytest.mark.gpu
FP = 0
P = sc.P
MARKER = 0xA5


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def _descriptor(depth, q, stream=0):
    q_limbs = np.ascontiguousarray(stc.point_limbs([q]).reshape(8))
    d = _lib.MerklePaths(depth, q_limbs.ctypes.data_as(_lib.u64p), sinsemilla.generator_table().data_ptr(), stream)
    d._keep = q_limbs
    return d


def _walk(case, q):
    """the C ABI on the default stream -> (nodes bytes, status bytes); the outputs are poisoned first"""
    leaves, positions, siblings = (_t(a) for a in case.arrays())
    nodes = torch.full((32 * case.n * (case.depth + 1),), MARKER, dtype=torch.uint8, device="cuda:0")
    status = torch.full((case.n * case.depth,), MARKER, dtype=torch.uint8, device="cuda:0")
    d = _descriptor(case.depth, q)
    rc = h.lib().h2_sinsemilla_merkle_paths_device(C.byref(d), leaves.data_ptr(), siblings.data_ptr(), positions.data_ptr(), case.n,
                                                   nodes.data_ptr(), status.data_ptr())
    assert rc == 0, h.lib().h2_last_error()
    torch.cuda.synchronize()
    return nodes, status


def _wanted_walk(case, q=None):
    nodes, status = case.walk(q)
    return mp.limbs([v for path in nodes for v in path]).tobytes(), bytes(v for path in status for v in path)


# ---- the walk -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mp.cases(), ids=repr)
def test_the_walk_is_the_models_on_every_node_and_status_byte(case):
    nodes, status = _walk(case, mp.q_merkle())
    want_nodes, want_status = _wanted_walk(case)
    assert status.cpu().numpy().tobytes() == want_status
    assert nodes.cpu().numpy().tobytes() == want_nodes


def test_bottom_through_the_c_abi():
    """Q = S(2): layer 2 of every path starts with a doubling.  Status 1 there and nowhere else, node 3 = 0, layer 3 hashed from 0."""
    case, q = mp.bottom_case()
    model_nodes, model_status = case.walk(q)
    assert model_status == [[0, 0, 1, 0]] * 3 and all(n[3] == 0 and n[4] != 0 for n in model_nodes)      # the CPU first
    nodes, status = _walk(case, q)
    assert status.cpu().numpy().reshape(3, 4).tolist() == [[0, 0, 1, 0]] * 3
    got = nodes.cpu().numpy().view(np.uint64).reshape(3, 5, 4)
    assert not got[:, 3].any()
    want_nodes, _ = _wanted_walk(case, q)
    assert got.tobytes() == want_nodes                                        # layers 0, 1 and 3 against the model


def test_bottom_through_python():
    case, q = mp.bottom_case()
    leaves, positions, siblings = case.arrays()
    domain = sinsemilla.HashDomain(q)
    with pytest.raises(sinsemilla.Bottom):
        sinsemilla.merkle_paths(leaves, positions, siblings, domain)
    nodes, status = sinsemilla.merkle_paths(leaves, positions, siblings, domain, with_status=True)
    want_nodes, want_status = _wanted_walk(case, q)
    assert isinstance(nodes, np.ndarray) and nodes.shape == (3, 5, 4) and status.shape == (3, 4)
    assert nodes.tobytes() == want_nodes and status.tobytes() == want_status
    # device tensors in, device tensors out; the domain's own Q has a value everywhere
    dev_in = [torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32)).to("cuda:0") for a in (leaves, positions, siblings)]
    out = sinsemilla.merkle_paths(*dev_in)
    assert torch.is_tensor(out) and out.is_cuda and out.cpu().numpy().tobytes() == _wanted_walk(case)[0]
    with pytest.raises(ValueError):
        sinsemilla.merkle_paths(leaves, dev_in[1], siblings)


# ---- the trace ----------------------------------------------------------------------------------------------------------------------------------
def _trace(case, lo, hi):
    nodes_model, _ = case.walk()
    _, positions, siblings = (_t(a) for a in case.arrays())
    nodes = _t(mp.limbs([v for path in nodes_model for v in path]))
    count = case.n * (hi - lo)
    out = torch.full((23 * 32 * count + 64,), MARKER, dtype=torch.uint8, device="cuda:0")
    d = _lib.MerklePaths(case.depth, None, None, 0)
    rc = h.lib().h2_sinsemilla_merkle_trace_device(C.byref(d), nodes.data_ptr(), siblings.data_ptr(), positions.data_ptr(), case.n, lo, hi, out.data_ptr())
    assert rc == 0, h.lib().h2_last_error()
    torch.cuda.synchronize()
    raw = out.cpu().numpy().tobytes()
    assert raw[-64:] == bytes([MARKER]) * 64                                  # nothing past the 23 * count elements
    return raw[:-64]


@pytest.mark.parametrize("case", mp.cases(), ids=repr)
def test_the_trace_is_the_models_and_every_element_is_written(case):
    nodes, _ = case.walk()
    got, want = _trace(case, 0, case.depth), mp.trace_bytes(nodes, case.positions, case.siblings, 0, case.depth)
    bad = [i // 32 for i in range(0, len(want), 32) if got[i:i + 32] != want[i:i + 32]]
    assert not bad, f"{len(bad)} of {len(want) // 32} elements differ, first {bad[:6]}"


def test_the_trace_of_a_proper_sub_range():
    case = mp.case("257x4")
    nodes, _ = case.walk()
    assert _trace(case, 1, 3) == mp.trace_bytes(nodes, case.positions, case.siblings, 1, 3)


def test_the_trace_through_python_feeds_the_hash_trace():
    """merkle_path_trace's canonical pieces through `sinsemilla.trace` are the 53 rows of each layer's hash: the digest is the next node"""
    case = mp.case("3x32")
    leaves, positions, siblings = case.arrays()
    nodes = sinsemilla.merkle_paths(leaves, positions, siblings)
    tr = sinsemilla.merkle_path_trace(nodes, positions, siblings, 30, 32)
    assert tr.count == 6 and tr.swap_rows.shape == (5, 6, 4) and tr.pieces.shape == (18, 4) and tr.decompose.shape == (5, 12, 4)
    assert tr.canonical.shape == (6, 3, 4) and tr.b_1.shape == tr.b_2.shape == (6, 4)
    assert tr.out.tobytes() == mp.trace_bytes(case.walk()[0], case.positions, case.siblings, 30, 32)
    columns = sinsemilla.trace(tr.canonical, sinsemilla.MERKLE_PIECE_WORDS, mp.q_merkle())
    digests = columns[0].reshape(6, 53, 4)[:, 52]
    assert digests.tobytes() == np.ascontiguousarray(nodes[:, 31:33].reshape(6, 4)).tobytes()
    with pytest.raises(ValueError):
        sinsemilla.merkle_path_trace(nodes, positions, siblings, 3, 3)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_and_the_empty_call():
    lib = h.lib()
    assert lib.h2_init(0) == 0
    scratch = torch.full((1 << 16,), MARKER, dtype=torch.uint8, device="cuda:0")
    at = scratch.data_ptr()
    rows = mp.refusals(at, at + 4096, at + 8192, at + 12288, at + 16384)
    assert len(rows) >= 24
    for row in rows:
        assert mp.refuse(lib, row) == _lib.H2_ERR_ARGS, row[:2]
    d = _descriptor(4, mp.q_merkle())
    assert lib.h2_sinsemilla_merkle_paths_device(C.byref(d), None, None, None, 0, None, None) == 0
    assert lib.h2_sinsemilla_merkle_trace_device(C.byref(d), None, None, None, 0, 0, 4, None) == 0
    assert lib.h2_sinsemilla_merkle_paths_device(C.byref(d), at, at, at, 0, at, at) == 0
    assert lib.h2_sinsemilla_merkle_trace_device(C.byref(d), at, at, at, 0, 1, 3, at) == 0
    torch.cuda.synchronize()
    assert bool((scratch == MARKER).all())


# ---- stream order -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig():
    """The harness of tests/test_gpu_stream_order.py for the two cases of tests/merkle_path_cases.py: a delay of four warm call times on
    `s`, and a stream `w` shown to overtake it."""
    import test_gpu_stream_order as so
    assert h.lib().h2_init(0) == 0, h.lib().h2_last_error()
    r = so.Rig()
    r.so = so
    r.null = torch.cuda.default_stream()
    r.pool = [torch.cuda.Stream() for _ in range(so.POOL_STREAMS)]
    r.cases = mp.stream_cases()
    r.warm_ms = {name: so._warm(case) for name, case in r.cases.items()}
    r.delay = so.Delay(r.pool[0])
    r.delay.size(max(20.0, so.DELAY_FACTOR * max(r.warm_ms.values())))
    r.s = r.w = None
    for s in r.pool:
        for w in [r.null] + [p for p in r.pool if p is not s]:
            if so._overtakes(r.delay, s, w):
                r.s, r.w = s, w
                break
        if r.s is not None:
            break
    if r.s is None:
        pytest.fail("no pair of streams overtakes: a misplaced launch cannot be told from an ordered one on this device")
    assert r.delay.measured_ms >= 2 * max(r.warm_ms.values()), (r.delay.ms, r.delay.measured_ms, r.warm_ms)
    return r


@pytest.mark.parametrize("entry", [mp.WALK, mp.TRACE])
def test_stream_order_late_producer_early_overwrite(entry, rig):
    """The inputs are produced late by work queued on the descriptor's stream, a non-default one, and overwritten on that stream right
    after the call; the result is the oracle's."""
    so, case = rig.so, rig.cases[entry]
    assert rig.s.cuda_stream != 0
    want = so._wanted(case, so.sc.REAL)
    clones, host, _ = so._ordered_run(case, rig.s, rig.s, rig.delay)
    rig.s.synchronize()
    got = so._collect(case, clones, host)
    torch.cuda.synchronize()
    assert got == want, f"{case} on a held-back stream: {so._first_difference(got, want)}"


# ---- the gadget ---------------------------------------------------------------------------------------------------------------------------------
def _ints(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else t
    return fields.from_limbs(np.ascontiguousarray(a).view(np.uint64).reshape(-1, 4), FP, True)


def _copies(assembly):
    _, sizes = np.unique(assembly.permutation.aux, return_counts=True)
    return sorted(int(s) for s in sizes if s > 1)


def _model_roots():
    return [nodes[-1] for nodes in mp.gadget_case().walk(sc.q_of(sc.TEST_DOMAIN))[0]]


@pytest.mark.parametrize("chips", [1, 2])
@pytest.mark.parametrize("tagged", [False, True], ids=["plain", "4_5b"])
def test_calculate_roots_is_the_loop_of_calculate_root(chips, tagged):
    circuit = mp.paths_circuit(chips=chips, tagged=tagged)
    dev.MockProver.run_circuit(mp.GADGET_K, circuit, [], FP, regions=True).assert_satisfied()
    assert [root.value().inner.evaluate(P) for root in circuit.roots] == _model_roots()
    sides = []
    for bulk in (True, False):
        c = mp.paths_circuit(chips=chips, tagged=tagged, bulk=bulk)
        _, assembly, layouter = front.synthesize(c, mp.GADGET_K, FP, fixed=True, advice=True, instances=[], regions=True)
        advice = [sorted(_ints(col)) for col in assembly.columns_to_field(assembly.advice)]
        sides.append((advice, assembly.selectors.sum(axis=1).tolist(), _copies(assembly), ([r.name for r in assembly.regions], list(layouter.regions)),
                      [root.value().inner.evaluate(P) for root in c.roots]))
    many, loop = sides
    for column, (a, b) in enumerate(zip(many[0], loop[0])):
        assert a == b, f"advice column {column}"
    assert many[1] == loop[1] and sum(many[1]) > 12 * 52 and many[2] == loop[2] and many[4] == loop[4]
    # the keygen shape lays out the regions of the witnessed one
    _, keygen, planned = front.synthesize(mp.paths_circuit(chips=chips, tagged=tagged).without_witnesses(), mp.GADGET_K, FP, fixed=True, advice=False,
                                          regions=True)
    assert ([r.name for r in keygen.regions], list(planned.regions)) == many[3] and many[3][0].count("hash_to_point many") == chips
    assert keygen.selectors.sum(axis=1).tolist() == many[1] and _copies(keygen) == many[2]


def _failures(tamper, **kw):
    return dev.MockProver.run_circuit(mp.GADGET_K, mp.tampered_paths_circuit(tamper, **kw), [], FP, regions=True).verify()


def _mont(v):
    return torch.from_numpy(mp.limbs([v]).view(np.int64)).to("cuda:0")[0]


def _plain(v):
    return torch.from_numpy(mp.limbs([v], montgomery=False).view(np.int64)).to("cuda:0")[0]


def _item_cells(t):
    """the model's cells of item t of the one-chip circuit: path t // 4, layer t % 4"""
    k = mp.gadget_case()
    path, l = divmod(t, mp.GADGET_DEPTH)                                      # noqa: E741
    nodes = k.walk(sc.q_of(sc.TEST_DOMAIN))[0]
    return mp.layer_cells(l, nodes[path][l], k.siblings[path][l], k.positions[path])


def test_a_flipped_swap_fails_the_swap_gate():
    t = 5

    def tamper(trace, lo, hi):
        trace.swap_rows[4][t] = _mont(1 - _item_cells(t)["swap"])
    failures = _failures(tamper, chips=1)
    assert failures and {type(f).__name__ for f in failures} == {"ConstraintNotSatisfied"}
    assert {f.constraint[3] for f in failures} <= {"a check", "b check", "swap is bool"} and {f.constraint[3] for f in failures} & {"a check", "b check"}
    assert {(f.location.region[1], f.location.offset) for f in failures} == {("swap many", t)}


def test_b_1_moved_into_b_2_fails_the_decomposition():
    t = next(t for t in range(12) if _item_cells(t)["b_1"] and (_item_cells(t)["b_1"] + _item_cells(t)["b_2"]) % 32 != _item_cells(t)["b_2"])
    cells = _item_cells(t)
    moved = (cells["b_1"] + cells["b_2"]) % 32

    def tamper(trace, lo, hi):
        trace.b_1[t], trace.b_2[t] = _plain(0), _plain(moved)
        trace.decompose[2][2 * t + 1], trace.decompose[3][2 * t + 1] = _mont(0), _mont(moved)
    failures = _failures(tamper, chips=1)
    assert failures and {type(f).__name__ for f in failures} == {"ConstraintNotSatisfied"}
    assert {f.constraint[1] for f in failures} == {"Decomposition check"}
    names = {f.constraint[3] for f in failures}
    assert {"b1_b2_check", "left_check"} <= names <= {"b1_b2_check", "left_check", "right_check"}
    assert {(f.location.region[1], f.location.offset) for f in failures} == {("Check piece decomposition many", 2 * t)}


def test_a_replaced_node_breaks_the_copy_into_the_next_swap_row():
    """layer 3 of path 1 swaps another node than the digest of layer 2 (and its swapped copy with it, so the swap gate holds)"""
    t = 1 * mp.GADGET_DEPTH + 3
    cells = _item_cells(t)
    other = (cells["a"] + 1) % P

    def tamper(trace, lo, hi):
        trace.swap_rows[0][t] = _mont(other)
        trace.swap_rows[3 if cells["swap"] else 2][t] = _mont(other)
    circuit = mp.tampered_paths_circuit(tamper, chips=1)
    prover = dev.MockProver.run_circuit(mp.GADGET_K, circuit, [], FP, regions=True)
    failures = prover.verify()
    assert failures and {type(f).__name__ for f in failures} == {"Permutation"}
    swap_region = next(r for r in prover.regions if r.name == "swap many")
    a_column = ("advice", 5)                                                  # the first chip's first column: advices[5]
    assert (a_column, swap_region.rows[0] + t) in {(tuple(f.column), f.row) for f in failures}
    assert any(f.location.region[1] == "swap many" and f.location.offset == t for f in failures)


@pytest.mark.parametrize("tagged", [False, True], ids=["plain", "4_5b"])
def test_b_1_of_32_fails_the_short_lookup(tagged):
    t = 7

    def tamper(trace, lo, hi):
        trace.b_1[t] = _plain(32)
        trace.decompose[2][2 * t + 1] = _mont(32)
    failures = _failures(tamper, chips=1, tagged=tagged)
    lookups = [f for f in failures if type(f).__name__ == "Lookup"]
    # plain: 32 itself is a row of the 10-bit table, its shift 32 * 2^5 = 1024 on the second of the three rows is not;
    # 4_5b: (32, tag 5) is no row of the tagged table, and the check is that one row
    assert lookups and {f.lookup_index for f in lookups} == {0}
    assert {(f.location.region[1], f.location.offset) for f in lookups} == {("Range check 5 bits many", t if tagged else 3 * t + 1)}
    others = [f for f in failures if type(f).__name__ != "Lookup"]
    assert all(type(f).__name__ == "ConstraintNotSatisfied" and f.constraint[1] == "Decomposition check" for f in others)


# ---- a proof ------------------------------------------------------------------------------------------------------------------------------------
def _rng(seed):
    sf = co.field_of_curve(h.VESTA, "scalar")
    ctr = [seed]

    def rng(count):
        ctr[0] += 1
        return co.random_field(sf, ctr[0], count)
    return rng


def test_a_proof_with_public_roots():
    roots = _model_roots()
    circuit = mp.paths_circuit(chips=2, public=True)
    dev.MockProver.run_circuit(mp.GADGET_K, circuit, [roots], FP, regions=True).assert_satisfied()
    params = h.Params.new(h.VESTA, mp.GADGET_K)
    try:
        vk = h.keygen_vk(params, circuit)
        pk = h.keygen_pk(params, circuit)
        assert pk.vk.pinned() == vk.pinned()
        transcript = Blake2bWrite(h.VESTA)
        h.create_proof(params, pk, [circuit], [[roots]], _rng(47), transcript)
        proof = transcript.finalize()
        assert hv.verify_proof(params, pk.vk, [roots], proof)
        wrong = list(roots)
        wrong[1] = (wrong[1] + 1) % P
        assert not hv.verify_proof(params, pk.vk, [wrong], proof)
    finally:
        params.close()


def test_the_example_runs(capsys):
    """examples/sinsemilla_merkle_many.py end to end at 4 paths of 8 layers (k = 11): planned, mock-proved, proved, verified, and
    rejected against one wrong root; the plan for its default size is the k = 15 it announces"""
    mod = sc._example("sinsemilla_merkle_many")
    assert mod.main(["--paths", "4", "--depth", "8"])
    out = capsys.readouterr().out
    assert "k = 11" in out and "MockProver satisfied" in out and "accepted; one wrong root: rejected" in out
    assert mod.planned_rows(16, 32) == 17408 and mod.smallest_k(17408) == 15 and mod.smallest_k(mod.planned_rows(16, 32, tagged=True)) == 14
