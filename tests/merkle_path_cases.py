"""Shared by test_merkle_path_host.py and test_gpu_merkle_paths.py (a helper: nothing here is collected): the integer model of a
Merkle path walk and of the cells MerkleChip.hash_layer and CondSwapChip.swap assign outside the hash region, built on
tests/sinsemilla_cases.py (merkle_crh, merkle_words, trace), the case list both files run, every call the two entry points must
refuse, their stream-order cases, and the circuits of `MerklePaths`."""
import ctypes as C
import functools
import random

import numpy as np

import sinsemilla_cases as sc
from halo2_amd import _lib

P = sc.P
FP = 0
PIECE_WORDS = [25, 2, 25]
MAX_ITEMS = 1 << 30                                       # n * depth, the limit include/halo2_mi355x.h states
EDGES = [0, 1, 31, 32, (1 << 240) - 1, 1 << 240, (1 << 250) - 1, 1 << 250, 1 << 254, P - 1]


def q_merkle():
    return sc.q_of(sc.MERKLE_DOMAIN)


# ---- the model --------------------------------------------------------------------------------------------------------------------------------
def swapped(node, sibling, pos, l):                                           # noqa: E741
    return (sibling, node) if pos >> l & 1 else (node, sibling)


def path_nodes(q, leaf, pos, path):
    """sinsemilla_cases.merkle_path_root keeping every node: -> (nodes 0 .. depth, status 0 .. depth - 1); a layer without a value
    has status 1 and node 0, and the walk goes on from 0"""
    nodes, status = [leaf], []
    for l, sibling in enumerate(path):                                        # noqa: E741
        left, right = swapped(nodes[-1], sibling, pos, l)
        x = sc.merkle_crh(q, l, left, right)
        status.append(1 if x is None else 0)
        nodes.append(x or 0)
    return nodes, status


def layer_cells(l, node, sibling, pos):                                       # noqa: E741
    """what the gadget assigns for layer l of a path outside the hash region, as integers"""
    left, right = swapped(node, sibling, pos, l)
    bits = lambda v, lo, hi: (v >> lo) & ((1 << (hi - lo)) - 1)
    b_0, b_1, b_2 = bits(left, 240, 250), bits(left, 250, 255), bits(right, 0, 5)
    a = l | bits(left, 0, 240) << 10
    b = b_0 | b_1 << 10 | b_2 << 15
    c = bits(right, 5, 255)
    return {"a": node, "b": sibling, "a_swapped": left, "b_swapped": right, "swap": pos >> l & 1, "pieces": [a, b, c], "b_1": b_1, "b_2": b_2,
            "z1_a": a >> 10, "z1_b": b >> 10, "l": l, "left": left, "right": right}


def trace_vectors(nodes, positions, siblings, lo, hi):
    """The 23 * count elements of h2_sinsemilla_merkle_trace_device in its order, as (integers, whether Montgomery) per vector group.
    nodes[i]: the depth + 1 nodes of path i.  -> [(ints, montgomery)]"""
    items = [layer_cells(l, nodes[i][l], siblings[i][l], positions[i]) for i in range(len(nodes)) for l in range(lo, hi)]
    swap_rows = [[it[k] for it in items] for k in ("a", "b", "a_swapped", "b_swapped", "swap")]
    pieces = [p for it in items for p in it["pieces"]]
    pair = lambda first, second: [v for it in items for v in (first(it), it[second])]
    decompose = [pair(lambda it: it["pieces"][0], "z1_a"), pair(lambda it: it["pieces"][1], "z1_b"), pair(lambda it: it["pieces"][2], "b_1"),
                 pair(lambda it: it["left"], "b_2"), pair(lambda it: it["right"], "l")]
    return [(sum(swap_rows, []), True), (pieces, True), (sum(decompose, []), True), (pieces, False),
            ([it["b_1"] for it in items] + [it["b_2"] for it in items], False)]


def limbs(ints, montgomery=True):
    import stream_cases as stc
    return stc.limbs(ints, FP, montgomery)


def trace_bytes(nodes, positions, siblings, lo, hi) -> bytes:
    return b"".join(limbs(ints, mont).tobytes() for ints, mont in trace_vectors(nodes, positions, siblings, lo, hi))


# ---- the case list ------------------------------------------------------------------------------------------------------------------------
class PathCase:
    def __init__(self, name, leaves, positions, siblings):
        self.name, self.leaves, self.positions, self.siblings = name, leaves, positions, siblings
        self.n, self.depth = len(leaves), len(siblings[0])

    def __repr__(self):
        return self.name

    @functools.lru_cache(maxsize=None)
    def walk(self, q=None):
        """-> (nodes per path, status per path) from the Merkle domain's Q, or from `q`"""
        walks = [path_nodes(q or q_merkle(), leaf, pos, path) for leaf, pos, path in zip(self.leaves, self.positions, self.siblings)]
        return [w[0] for w in walks], [w[1] for w in walks]

    def arrays(self):
        """-> leaves (n, 4), positions (n,) uint32, siblings (n, depth, 4): Montgomery limbs"""
        return (limbs(self.leaves), np.array(self.positions, dtype=np.uint32),
                limbs([s for path in self.siblings for s in path]).reshape(self.n, self.depth, 4))


def _random_case(name, n, depth, seed, positions=None):
    rng = random.Random(seed)
    leaves = [rng.randrange(P) for _ in range(n)]
    siblings = [[rng.randrange(P) for _ in range(depth)] for _ in range(n)]
    positions = positions or [rng.getrandbits(32) for _ in range(n)]
    return PathCase(name, leaves, positions, siblings)


def _edge_case():
    """depth 1, one path per (left, right) of EDGES x EDGES; odd paths reach the pair through a swap"""
    leaves, positions, siblings = [], [], []
    for i, (left, right) in enumerate((a, b) for a in EDGES for b in EDGES):
        swap = i & 1
        leaves.append(right if swap else left)
        siblings.append([left if swap else right])
        positions.append(swap)
    return PathCase("edges", leaves, positions, siblings)


@functools.lru_cache(maxsize=None)
def cases():
    leaf, pos, path = sc.merkle_witness()
    return [
        _random_case("one-lane-depth-1", 1, 1, 41),
        _random_case("257x4", 257, 4, 42),                                    # past a workgroup of 256; the largest
        PathCase("3x32", [leaf, (leaf * 7) % P, 5], [pos, pos ^ 0xFFFFFFFF, 1 << 31], [path, path[::-1], [(s + 1) % P for s in path]]),
        _edge_case(),
    ]


def case(name):
    return next(c for c in cases() if c.name == name)


BOTTOM_LAYER = 2


def bottom_case():
    """3 paths x depth 4 walked from Q = S(2): layer 2 starts with Acc = S(2) + S(2), a doubling"""
    return _random_case("bottom", 3, 4, 43), sc.table()[BOTTOM_LAYER]


# ---- the refusals ---------------------------------------------------------------------------------------------------------------------------
def descriptor(depth=4, q=None, table=0x3000, stream=0):
    q = np.zeros(8, dtype=np.uint64) if q is None else q
    d = _lib.MerklePaths(depth, None if q is False else q.ctypes.data_as(_lib.u64p), table, stream)
    d._keep = q
    return d


WALK, TRACE = "h2_sinsemilla_merkle_paths_device", "h2_sinsemilla_merkle_trace_device"


def refusals(a=0x1000, b=0x2000, c=0x4000, d=0x5000, e=0x6000):
    """[(what, entry point, descriptor or None, the arguments after it)]: every one is H2_ERR_ARGS before anything touches the device.
    The pointers are never read, so without a device any nonzero value does."""
    walk, trace = (a, b, c, 1, d, e), (a, b, c, 1, 0, 4, d)
    rows = []
    for entry, tail in ((WALK, walk), (TRACE, trace)):
        rows += [("a null descriptor", entry, None, tail), ("depth 0", entry, descriptor(depth=0), tail), ("depth 33", entry, descriptor(depth=33), tail),
                 ("n over the limit", entry, descriptor(), tail[:3] + (MAX_ITEMS // 4 + 1,) + tail[4:]),
                 ("n over the limit at depth 32", entry, descriptor(depth=32), tail[:3] + (MAX_ITEMS // 32 + 1,) + tail[4:])]
        pointers = (0, 1, 2, 4, 5) if entry == WALK else (0, 1, 2, 6)
        rows += [(f"null argument {at}", entry, descriptor(), tail[:at] + (None,) + tail[at + 1:]) for at in pointers]
    rows += [("a null Q", WALK, descriptor(q=False), walk), ("a null table", WALK, descriptor(table=None), walk),
             ("an empty layer range", TRACE, descriptor(), trace[:4] + (2, 2) + trace[6:]),
             ("a reversed layer range", TRACE, descriptor(), trace[:4] + (3, 1) + trace[6:]),
             ("a layer range past the depth", TRACE, descriptor(), trace[:4] + (0, 5) + trace[6:])]
    return rows


def refuse(lib, row):
    _, entry, spec, tail = row
    return getattr(lib, entry)(None if spec is None else C.byref(spec), *tail)


# ---- stream order -----------------------------------------------------------------------------------------------------------------------------
STREAM_LANES, STREAM_DEPTH = 65, 2                        # two waves; the second layer reads what the first wrote


@functools.lru_cache(maxsize=None)
def _stream_case(seed):
    return _random_case(f"stream-{seed}", STREAM_LANES, STREAM_DEPTH, 0x3E00 + seed)


def stream_cases():
    import stream_cases as stc
    n, depth = STREAM_LANES, STREAM_DEPTH
    q_limbs = lambda: np.ascontiguousarray(stc.point_limbs([q_merkle()]).reshape(8))

    def walk_inputs(seed):
        leaves, positions, siblings = _stream_case(seed).arrays()
        return {"leaves": leaves, "positions": positions, "siblings": siblings}

    def trace_inputs(seed):
        ins = walk_inputs(seed)
        del ins["leaves"]
        ins["nodes"] = limbs([v for path in _stream_case(seed).walk()[0] for v in path]).reshape(n, depth + 1, 4)
        return ins

    def walk_wanted(seed):
        nodes, status = _stream_case(seed).walk()
        return stc._b(limbs([v for path in nodes for v in path])) + bytes(v for path in status for v in path)

    def trace_wanted(seed):
        k = _stream_case(seed)
        return trace_bytes(k.walk()[0], k.positions, k.siblings, 0, depth)

    def walk_call(i, u, sp):
        q = q_limbs()
        d = _lib.MerklePaths(depth, q.ctypes.data_as(_lib.u64p), stc.sinsemilla_table(sp).data_ptr(), sp)
        stc.ok(stc._lib().h2_sinsemilla_merkle_paths_device(C.byref(d), i["leaves"].data_ptr(), i["siblings"].data_ptr(), i["positions"].data_ptr(), n,
                                                           u["nodes"].data_ptr(), u["status"].data_ptr()))

    def trace_call(i, u, sp):
        d = _lib.MerklePaths(depth, None, None, sp)
        stc.ok(stc._lib().h2_sinsemilla_merkle_trace_device(C.byref(d), i["nodes"].data_ptr(), i["siblings"].data_ptr(), i["positions"].data_ptr(), n,
                                                           0, depth, u["out"].data_ptr()))

    def positions_differ(arrays):
        stc.fields_valid(FP, *[name for name in arrays if name != "positions"])(arrays)
        assert arrays["positions"].dtype == np.uint32
    return {
        WALK: stc.Case("merkle-paths", WALK, (n, depth), walk_inputs, lambda: {"nodes": 32 * n * (depth + 1), "status": n * depth}, walk_call,
                       walk_wanted, positions_differ),
        TRACE: stc.Case("merkle-path-trace", TRACE, (n, depth), trace_inputs, lambda: {"out": 23 * 32 * n * depth}, trace_call, trace_wanted,
                        positions_differ),
    }


# ---- the circuits -------------------------------------------------------------------------------------------------------------------------------
GADGET_PATHS, GADGET_DEPTH, GADGET_K = 3, 4, 11           # the 1024-row generator table needs k = 11


@functools.lru_cache(maxsize=None)
def gadget_case():
    """3 paths x depth 4 whose positions take both values at every layer; some b_1 is nonzero"""
    k = _random_case("gadget", GADGET_PATHS, GADGET_DEPTH, 44, positions=[0b0101, 0b1010, 0b0110])
    assert any(layer_cells(l, n[l], s[l], p)["b_1"] for n, s, p in zip(k.walk(sc.q_of(sc.TEST_DOMAIN))[0], k.siblings, k.positions)
               for l in range(GADGET_DEPTH))                                  # noqa: E741
    return k


def paths_circuit_class():
    return sc._example("sinsemilla_merkle_many").MerklePathsCircuit


def paths_circuit(witness=True, **kw):
    """the circuit of examples/sinsemilla_merkle_many.py over gadget_case() and the reference's test domain, on the device's table"""
    k = gadget_case()
    args = (k.leaves, k.positions, k.siblings) if witness else ()
    return paths_circuit_class()(k.n, k.depth, *args, q=sc.q_of(sc.TEST_DOMAIN), **kw)


def tampered_paths_circuit(tamper, **kw):
    """paths_circuit whose `sinsemilla.merkle_path_trace` results pass through tamper(trace, layer_lo, layer_hi) before the gadget
    reads them: the views of a MerklePathTrace share one buffer, so a write through any of them is what the regions are filled from"""
    from halo2_amd.gadgets import sinsemilla as g

    class Tampered(paths_circuit_class()):
        def synthesize(self, config, layouter):
            original = g.primitive.merkle_path_trace

            def traced(nodes, positions, siblings, lo, hi, domain=None):
                trace = original(nodes, positions, siblings, lo, hi, domain)
                tamper(trace, lo, hi)
                return trace
            g.primitive.merkle_path_trace = traced
            try:
                super().synthesize(config, layouter)
            finally:
                g.primitive.merkle_path_trace = original
    k = gadget_case()
    return Tampered(k.n, k.depth, k.leaves, k.positions, k.siblings, q=sc.q_of(sc.TEST_DOMAIN), **kw)
