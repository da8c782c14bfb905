"""The bulk Merkle paths on the host: the integer model of tests/merkle_path_cases.py against the reference's fold, what its case list
reaches, the descriptor in the header and in ctypes, every refusal of the two entry points (they come before any device work), and the
circuit of `MerklePaths` without a witness: the reference's pinned constraint system and, region for region, selector for selector and
copy for copy, the keygen shape of as many `MerklePath.calculate_root` calls.  Nothing here needs a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import merkle_path_cases as mp
import sinsemilla_cases as sc
from halo2_amd import _lib
from halo2_amd import circuit as front

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "halo2_mi355x.h")
MerklePathsCircuit = sc._example("sinsemilla_merkle_many").MerklePathsCircuit


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
def test_the_model_walks_the_references_witness_to_its_root():
    leaf, pos, path = sc.merkle_witness()
    q = sc.q_of(sc.TEST_DOMAIN)
    nodes, status = mp.path_nodes(q, leaf, pos, path)
    assert len(nodes) == sc.MERKLE_DEPTH + 1 == 33 and nodes[0] == leaf and status == [0] * 32
    assert nodes[-1] == sc.merkle_path_root(q, leaf, pos, path)
    for l in (0, 15, 31):                                                     # noqa: E741 -- a node is the hash of the swapped pair below it
        left, right = mp.swapped(nodes[l], path[l], pos, l)
        assert nodes[l + 1] == sc.merkle_crh(q, l, left, right)


@pytest.mark.parametrize("case", mp.cases(), ids=repr)
def test_the_pieces_are_the_message_of_the_layer(case):
    """a || b || c in 25, 2 and 25 words is l || left || right, the words the hash consumes; the other cells follow from the pieces"""
    nodes, _ = case.walk()
    for path in range(case.n):
        for l in range(case.depth):                                           # noqa: E741
            cells = mp.layer_cells(l, nodes[path][l], case.siblings[path][l], case.positions[path])
            left, right = cells["left"], cells["right"]
            assert {left, right} == {nodes[path][l], case.siblings[path][l]} and cells["a_swapped"] == left and cells["b_swapped"] == right
            assert (left == case.siblings[path][l]) == bool(cells["swap"]) or left == right
            assert sc.words_of(cells["pieces"], mp.PIECE_WORDS) == sc.merkle_words(l, left, right)
            a, b, c = cells["pieces"]
            assert a < 1 << 250 and b < 1 << 20 and c < 1 << 250 and cells["b_1"] < 32 and cells["b_2"] < 32
            # the gate "Decomposition check" (merkle/chip.rs), with integers
            assert a - (cells["z1_a"] << 10) == l and cells["z1_b"] == cells["b_1"] + (cells["b_2"] << 5)
            assert cells["z1_a"] + ((b - (cells["z1_b"] << 10)) + (cells["b_1"] << 10) << 240) == left
            assert cells["b_2"] + (c << 5) == right


def test_the_trace_vectors_have_the_headers_layout():
    case = mp.case("257x4")
    nodes, _ = case.walk()
    groups = mp.trace_vectors(nodes, case.positions, case.siblings, 1, 3)
    count = case.n * 2
    assert [len(ints) for ints, _ in groups] == [5 * count, 3 * count, 10 * count, 3 * count, 2 * count]
    assert sum(len(ints) for ints, _ in groups) == 23 * count and [mont for _, mont in groups] == [True, True, True, False, False]
    assert len(mp.trace_bytes(nodes, case.positions, case.siblings, 1, 3)) == 23 * 32 * count
    # item t = path * layers + (l - layer_lo): the second item is layer 2 of path 0
    assert groups[0][0][1] == nodes[0][2] and groups[0][0][count + 1] == case.siblings[0][2]


def test_the_case_list_reaches_what_it_should():
    cases = mp.cases()
    assert {1, 32} <= {c.depth for c in cases} and {1, 257} <= {c.n for c in cases}
    assert max(c.n * c.depth for c in cases) == 257 * 4 and any(c.depth == 32 and c.n == 3 for c in cases)
    assert any(all({p >> l & 1 for p in c.positions} == {0, 1} for l in range(c.depth)) and c.depth == 32 for c in cases)
    lefts, rights, swaps = set(), set(), set()
    for c in cases:
        nodes, _ = c.walk()
        for path in range(c.n):
            for l in range(c.depth):                                          # noqa: E741
                left, right = mp.swapped(nodes[path][l], c.siblings[path][l], c.positions[path], l)
                if left in mp.EDGES and right in mp.EDGES:
                    lefts.add(left), rights.add(right), swaps.add((left, c.positions[path] >> l & 1))
    assert lefts == rights == set(mp.EDGES) and len(mp.EDGES) == 10
    assert mp.EDGES == [0, 1, 31, 32, (1 << 240) - 1, 1 << 240, (1 << 250) - 1, 1 << 250, 1 << 254, sc.P - 1]
    assert {s for _, s in swaps} == {0, 1}
    # every cut sees all ones below it and a lone one above it
    cut = lambda v, lo, hi: (v >> lo) & ((1 << (hi - lo)) - 1)
    assert {cut(v, 0, 240) for v in lefts} >= {(1 << 240) - 1, 0} and {cut(v, 240, 250) for v in lefts} >= {1023, 1, 0}
    assert {cut(v, 250, 255) for v in lefts} >= {1, 16, 0} and {cut(v, 0, 5) for v in rights} >= {31, 0, 1} and {cut(v, 5, 255) for v in rights} >= {1, 0}


def test_the_bottom_case_is_bottom_at_layer_two_and_nowhere_else():
    case, q = mp.bottom_case()
    assert q == sc.table()[2] and (case.n, case.depth) == (3, 4)
    nodes, status = case.walk(q)
    assert status == [[0, 0, 1, 0]] * 3
    for path in range(3):
        assert nodes[path][3] == 0 and nodes[path][4] != 0
        left, right = mp.swapped(0, case.siblings[path][3], case.positions[path], 3)
        assert nodes[path][4] == sc.merkle_crh(q, 3, left, right)             # the walk goes on from 0
    assert all(s == [0] * 4 for s in case.walk()[1])                          # from the domain's own Q the same inputs have a value


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------------
def test_the_descriptor_is_the_same_in_the_header_and_in_ctypes():
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct h2_merkle_paths \{(.*?)\} h2_merkle_paths_t;", header, flags=re.S).group(1)
    assert re.findall(r"([a-z_]+)\s*;", body) == [name for name, _ in _lib.MerklePaths._fields_] == ["depth", "q_xy", "d_table", "stream"]
    assert C.sizeof(_lib.MerklePaths) == 32
    protos = dict(re.findall(r"\bint\s+(h2_sinsemilla_merkle_(?:paths|trace)_device)\s*\(([^()]*)\)\s*;", header))
    assert set(protos) == {mp.WALK, mp.TRACE}
    for name, params in protos.items():
        assert re.match(r"\s*const\s+h2_merkle_paths_t\s*\*\s*paths\b", params) and "stream" not in params
        assert len(_lib.SIGNATURES[name][0]) == params.count(",") + 1


@pytest.mark.parametrize("row", mp.refusals(), ids=lambda row: f"{row[1][14:-7]}: {row[0]}")
def test_refusals_come_before_the_device(row):
    import halo2_amd as h
    assert mp.refuse(h.lib(), row) == _lib.H2_ERR_ARGS


def test_the_unit_owns_no_device_memory():
    text = open(os.path.join(ROOT, "halo2_amd", "csrc", "merkle_path.hip")).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert "StreamContexts" not in code and "DevBuf" not in code and "hipMalloc" not in code and "g_" not in code


# ---- the circuit without a witness --------------------------------------------------------------------------------------------------------------
def _circuit(**kw):
    return MerklePathsCircuit(3, 4, q=sc.q_of(sc.TEST_DOMAIN), table=sc.table(), **kw)


def test_the_constraint_system_is_the_references():
    cs = sc.host_keygen_cs(_circuit(), 11)
    assert cs.pinned() == sc.fixture_cs(sc.fixture_text("vk_merkle_chip.rdata.gz"))


def _keygen(circuit):
    _, assembly, _ = front.synthesize(circuit.without_witnesses(), 11, mp.FP, fixed=True, advice=False, regions=True)
    return assembly


def copies(assembly):
    """the sizes of the permutation's cycles of more than one cell: sum(size - 1) is the number of effective equality constraints"""
    _, sizes = np.unique(assembly.permutation.aux, return_counts=True)
    return sorted(int(s) for s in sizes if s > 1)


@pytest.mark.parametrize("chips", [1, 2])
@pytest.mark.parametrize("tagged", [False, True], ids=["plain", "4_5b"])
def test_the_keygen_shape_is_that_of_as_many_single_paths(chips, tagged):
    many, single = _keygen(_circuit(chips=chips, tagged=tagged)), _keygen(_circuit(chips=chips, tagged=tagged, bulk=False))
    assert many.selectors.sum(axis=1).tolist() == single.selectors.sum(axis=1).tolist()
    assert copies(many) == copies(single) and sum(s - 1 for s in copies(many)) > 12 * 14
    names = [r.name for r in many.regions]
    per_chip = ["swap many", "witness message pieces many", "Range check 5 bits many", "Range check 5 bits many", "hash_to_point many",
                "Check piece decomposition many"]
    assert names == ["generator_table"] + ["load private"] * 3 + per_chip * chips
    # the fixed columns hold the same multiset: q_sinsemilla2's pattern, y_Q, and the constants the cells are constrained to
    for a, b in zip(many.host_columns(many.fixed), single.host_columns(single.fixed)):
        assert sorted(a) == sorted(b)
