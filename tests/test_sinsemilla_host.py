"""The Sinsemilla, Merkle and lookup-range-check gadgets on the host: the constraint systems against the reference's pinned keys
(tests/golden/vk_merkle_chip.rdata.gz, vk_lookup_range_check.rdata), and the synthesized circuits evaluated with Python integers --
gates, lookups and copy constraints -- with the generator table of `oracle.hash_to_curve` injected.  No GPU."""
import pytest

import sinsemilla_cases as sc
from sinsemilla_cases import P, STRUCTURES, HashCircuit, LookupCircuit, MerkleCircuit, RangeCircuit


def _merkle(leaf=None, pos=None, path=None):
    return MerkleCircuit(leaf, pos, path, q=sc.q_of(sc.TEST_DOMAIN), table=sc.table())


# ---- 1: the constraint systems are the reference's ----------------------------------------------------------------------------------------
def test_merkle_constraint_system_is_the_references():
    """every gate, lookup, query, permutation column and constant, and the six columns the eleven selectors compress into"""
    cs = sc.host_keygen_cs(_merkle(), 11)
    assert (cs.num_fixed_columns, cs.num_advice_columns, cs.num_instance_columns, cs.num_selectors) == (14, 10, 0, 11)
    assert cs.pinned() == sc.fixture_cs(sc.fixture_text("vk_merkle_chip.rdata.gz"))


def test_lookup_range_check_constraint_system_is_the_references():
    cs = sc.host_keygen_cs(LookupCircuit(6), 11)
    assert (cs.num_fixed_columns, cs.num_advice_columns, cs.num_instance_columns, cs.num_selectors) == (5, 1, 0, 3)
    assert cs.pinned() == sc.fixture_cs(sc.fixture_text("vk_lookup_range_check.rdata"))


# ---- 2: the Merkle circuit, synthesized ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def merkle_run():
    leaf, pos, path = sc.merkle_witness()
    circuit = _merkle(leaf, pos, path)
    failures, assembly, layouter = sc.host_failures(circuit, 11)
    return circuit, failures


def test_merkle_circuit_computes_the_fold_and_satisfies_every_constraint(merkle_run):
    circuit, failures = merkle_run
    leaf, pos, path = sc.merkle_witness()
    assert {pos >> l & 1 for l in range(32)} == {0, 1}                        # both orders of (node, sibling) occur
    assert circuit.root.value().inner.evaluate(P) == sc.merkle_path_root(sc.q_of(sc.TEST_DOMAIN), leaf, pos, path)
    assert failures == []


def test_a_wrong_sibling_breaks_the_decomposition_or_a_copy():
    """the chip witnesses the pieces of the true sibling; one that differs from what the swap handed over cannot satisfy both the
    decomposition gate and the copies"""
    leaf, pos, path = sc.merkle_witness()

    failures, _, _ = sc.host_failures(sc.TamperedMerkleCircuit(leaf, pos, path, q=sc.q_of(sc.TEST_DOMAIN), table=sc.table()), 11)
    assert failures and all(f[0] == "copy" or f[1] == "Decomposition check" for f in failures), failures[:5]
    # and a path element that is simply different gives a different root with every constraint satisfied
    other = list(path)
    other[7] ^= 1
    circuit = _merkle(leaf, pos, other)
    failures, _, _ = sc.host_failures(circuit, 11)
    assert failures == [] and circuit.root.value().inner.evaluate(P) != sc.merkle_path_root(sc.q_of(sc.TEST_DOMAIN), leaf, pos, path)


# ---- 3: the lookup range check -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_words", [1, 6, 25])
def test_witness_check_accepts_n_words_and_rejects_one_bit_more(num_words):
    bits = 10 * num_words
    assert sc.host_failures(RangeCircuit([("witness", (1 << bits) - 1, num_words, True), ("witness", 1 << bits, num_words, False)]), 11)[0] == []
    failures = sc.host_failures(RangeCircuit([("witness", 1 << bits, num_words, True)]), 11)[0]      # 10 n + 1 bits, strict
    assert failures and all(f[0] == "copy" for f in failures)               # z_n = 1 is tied to the constant 0


def test_the_reference_lookup_circuit_is_satisfied():
    assert sc.host_failures(LookupCircuit(6), 11)[0] == []


def test_short_check_of_six_bits():
    assert sc.host_failures(RangeCircuit([("short", 0b111111, 6), ("short", 0, 6)]), 11)[0] == []
    failures = sc.host_failures(RangeCircuit([("short", 0b1000000, 6)]), 11)[0]                      # 7 bits
    assert failures and all(f[0] == "lookup" for f in failures)             # 2^6 * 2^4 is not in the table


# ---- 4: the chip's cells against the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("structure", ["one", "merkle", "full"])
def test_hash_to_point_cells_against_the_restatement(structure):
    nw = STRUCTURES[structure]
    q = sc.q_of(sc.MERKLE_DOMAIN)
    msgs = [sc.random_pieces(nw, 40, high_zero=False), sc.random_pieces(nw, 41, high_zero=True)]
    circuit = HashCircuit(nw, msgs, q, table=sc.table())
    failures, assembly, layouter = sc.host_failures(circuit, 11)
    assert failures == []
    config_columns = [0, 1, 2, 3, 4]                                          # x_a, x_p, bits, lambda_1, lambda_2 of configure_hash_chip
    advice = assembly.host_columns(assembly.advice)
    rows = sum(nw) + 1
    for i, m in enumerate(msgs):
        want = sc.trace(q, m, nw)
        start = layouter.regions[circuit.points[i].x().cell().region_index]
        assert [advice[c][start:start + rows] for c in config_columns] == want
        point = circuit.points[i]
        assert (point.x().value().inner.evaluate(P), point.y().value().inner.evaluate(P)) == sc.hash_to_point(q, sc.words_of(m, nw))
