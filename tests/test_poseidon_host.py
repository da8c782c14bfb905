"""Poseidon without a device: the generated constants (halo2_amd/poseidon_spec.py) against the pinned fixture, the committed table the
kernels read against a regeneration, the reference's hash vectors against the permutation restated in oracle/pasta.py, the structure
of the Pow5 chip (halo2_amd/gadgets/poseidon.py), the three reference test circuits evaluated with Python integers, and the argument
checks of the three C entry points."""
import importlib.util
import os

import numpy as np
import pytest

from halo2_amd import circuit as front
from halo2_amd import poseidon_spec as spec
from halo2_amd.gadgets import poseidon as gadget

import poseidon_cases as pc
from poseidon_cases import FP, FQ, HASH_KAT, KAT, MOD, NAME, HashCircuit, PermuteCircuit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ROWS = [0, 1, 2, 3, 32, 33, 34, 35]
PARTIAL_ROWS = list(range(4, 32))


# ---- the specification ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [FP, FQ])
def test_generated_constants_equal_the_fixture(field):
    assert spec.MODULUS[field] == MOD[field]
    rcs, mds, _ = spec.constants(field)
    want_rcs, want_mds = pc.kat_constants(field)
    assert len(rcs) == 64 and all(len(r) == 3 for r in rcs)
    assert rcs == want_rcs and mds == want_mds


@pytest.mark.parametrize("field", [FP, FQ])
def test_inverse_mds(field):
    m = MOD[field]
    _, mds, inv = spec.constants(field)
    for a, b in ((mds, inv), (inv, mds)):
        assert [[sum(a[i][k] * b[k][j] for k in range(3)) % m for j in range(3)] for i in range(3)] == [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    assert all(0 <= x < m for row in inv for x in row)


@pytest.mark.parametrize("field", [FP, FQ])
def test_host_permutation_equals_the_fixture_vectors(field):
    for v in KAT[NAME[field]]["permute"]:
        state = [int(x, 16) for x in v["initial_state"]]
        want = [int(x, 16) for x in v["final_state"]]
        assert spec.permute(state, field) == want and pc.permute_ints(state, field) == want
        assert [col[-1] for col in pc.trace_ints(state, field)[:3]] == want        # the trace restatement ends on the same state


def test_committed_table_equals_a_regeneration():
    path = os.path.join(ROOT, "halo2_amd", "csrc", "gen_poseidon_consts.py")
    loaded = importlib.util.spec_from_file_location("gen_poseidon_consts", path)
    gen = importlib.util.module_from_spec(loaded)
    loaded.loader.exec_module(gen)                                                # writes nothing: the file is written under __main__ only
    text = open(os.path.join(ROOT, "halo2_amd", "csrc", "poseidon_consts.inc")).read()
    assert text == gen.render()
    # and the table's first and last round constant, decoded, are the fixture's
    for field in (FP, FQ):
        m = MOD[field]
        rcs, _ = pc.kat_constants(field)
        for value in (rcs[0][0], rcs[63][2]):
            mont = value * (1 << 256) % m
            assert "{" + ", ".join("0x%08xu" % ((mont >> (32 * i)) & 0xFFFFFFFF) for i in range(8)) + "}" in text


@pytest.mark.parametrize("field", [FP, FQ])
def test_reference_hash_vectors_are_word_0_of_one_permutation(field):
    vectors = HASH_KAT[NAME[field]]["hash"]
    assert len(vectors) == 11
    for v in vectors:
        left, right = (int(x, 16) for x in v["input"])
        assert left < MOD[field] and right < MOD[field]
        assert pc.permute_ints([left, right, 2 << 64], field)[0] == int(v["output"], 16)
        assert pc.hash_ints([left, right], field) == int(v["output"], 16)
    assert spec.capacity(2) == 1 << 65


# ---- the chip ------------------------------------------------------------------------------------------------------------------------------
def test_chip_structure():
    cs, assembly, layouter = front.synthesize(PermuteCircuit().without_witnesses(), 6, FP, fixed=True, advice=False)
    assert [(g.name, len(g.polys)) for g in cs.gates] == [("full round", 3), ("partial rounds", 4), ("pad-and-add", 3)]
    assert [p.degree() for p in cs.gates[0].polys] == [6, 6, 6]
    assert [p.degree() for p in cs.gates[1].polys] == [6, 6, 2, 2]
    assert [p.degree() for p in cs.gates[2].polys] == [2, 2, 2]
    assert cs.degree() == 6                                                       # x^5 and the selector
    assert (cs.num_advice_columns, cs.num_fixed_columns, cs.num_selectors) == (4, 6, 3)
    assert [(c.kind, c.index) for c in cs.permutation_columns] == [("advice", 0), ("advice", 1), ("advice", 2), ("fixed", 3), ("fixed", 4), ("fixed", 5)]
    # regions: the initial state (1 row), the permutation (37 rows), the expected state (1 row)
    assert layouter.regions == [0, 1, 38] and [rows for _, rows in layouter.shapes] == [1, 37, 1]
    start = layouter.regions[1]
    s_full, s_partial, s_pad = assembly.selectors
    assert np.flatnonzero(s_full).tolist() == [start + r for r in FULL_ROWS]
    assert np.flatnonzero(s_partial).tolist() == [start + r for r in PARTIAL_ROWS]
    assert not s_pad.any()
    assert gadget.FULL_OFFSETS == FULL_ROWS and gadget.PARTIAL_OFFSETS == PARTIAL_ROWS
    # the fixed cells: rc_a holds the constant of the round that starts on the row, rc_b the second round of a partial pair
    rcs, _ = pc.kat_constants(FP)
    fixed = assembly.host_columns(assembly.fixed)
    first_round = [0, 1, 2, 3] + [4 + 2 * i for i in range(28)] + [60, 61, 62, 63]
    for j in range(3):
        assert fixed[j][start:start + 37] == [rcs[r][j] for r in first_round] + [0]
        assert fixed[3 + j][start:start + 37] == [0] * 4 + [rcs[5 + 2 * i][j] for i in range(28)] + [0] * 5


def test_hash_circuit_layout():
    cs, assembly, layouter = front.synthesize(HashCircuit(2), 6, FP, fixed=True, advice=False)
    # load message, initial state, add input (3 rows, selector on its row 1), permute, constrain output
    assert [rows for _, rows in layouter.shapes] == [1, 1, 3, 37, 1]
    add = layouter.regions[2]
    assert np.flatnonzero(assembly.selectors[2]).tolist() == [add + 1]
    assert cs.constants == [front.Column("fixed", 3)]
    # ConstantLength<3>: two absorptions, the second padded with a zero from rc_b[1]
    _, assembly3, layouter3 = front.synthesize(HashCircuit(3), 7, FP, fixed=True, advice=False)
    assert [rows for _, rows in layouter3.shapes] == [1, 1, 3, 37, 3, 37, 1]
    assert len(np.flatnonzero(assembly3.selectors[2])) == 2
    with pytest.raises(front.NotEnoughRowsAvailable):
        front.synthesize(HashCircuit(3), 6, FP, fixed=True, advice=False)


def test_region_selector_rows_is_many_enable_selector_calls():
    class Both(front.Circuit):
        def __init__(self, bulk):
            self.bulk = bulk

        def without_witnesses(self):
            return self

        def configure(self, meta):
            return meta.selector(), meta.advice_column()

        def synthesize(self, config, layouter):
            s, a = config
            layouter.assign_region("pad", lambda region: region.assign_advice(a, 2, 1))

            def assign(region):
                region.assign_advice(a, 0, 1)
                if self.bulk:
                    region.enable_selector_rows(s, np.array([5, 0, 9]))
                else:
                    for r in (5, 0, 9):
                        s.enable(region, r)
            layouter.assign_region("r", assign)
    got = front.synthesize(Both(True), 5, FP, fixed=True, advice=False)
    want = front.synthesize(Both(False), 5, FP, fixed=True, advice=False)
    assert np.array_equal(got[1].selectors, want[1].selectors) and np.flatnonzero(got[1].selectors[0]).tolist() == [3, 8, 12]
    assert got[2].shapes == want[2].shapes and got[2].regions == want[2].regions

    class TooFar(Both):
        def synthesize(self, config, layouter):
            layouter.assign_region("r", lambda region: region.enable_selector_rows(config[0], [0, 30]))
    with pytest.raises(front.NotEnoughRowsAvailable):
        front.synthesize(TooFar(True), 5, FP, fixed=True, advice=False)


# ---- the ported circuits, with Python integers -------------------------------------------------------------------------------------------------
def test_ported_permute_circuit_on_the_host():
    assert pc.host_failures(PermuteCircuit(), 6) == []
    wrong = pc.permute_ints([0, 1, 2], FP)
    wrong[1] = (wrong[1] + 1) % MOD[FP]
    assert {f[0] for f in pc.host_failures(PermuteCircuit(wrong), 6)} == {"copy"}


@pytest.mark.parametrize("length,k", [(2, 6), (3, 7)])
def test_ported_hash_circuits_on_the_host(length, k):
    message = [w[0] for w in pc.random_states(length, FP, 50 + length)]
    digest = pc.hash_ints(message, FP)
    assert pc.host_failures(HashCircuit(length, message, digest), k) == []
    assert {f[0] for f in pc.host_failures(HashCircuit(length, message, (digest + 1) % MOD[FP]), k)} == {"copy"}


def test_unknown_witness_is_a_synthesis_error():
    with pytest.raises(front.Synthesis):
        front.synthesize(HashCircuit(2), 6, FP, fixed=False, advice=True)


# ---- the C entry points -------------------------------------------------------------------------------------------------------------------------
def test_entry_points_validate_and_fail_loudly_without_a_device():
    import halo2_amd as h
    from halo2_amd import _lib
    lib = h.lib()
    p = 0x1000                                                                   # never dereferenced: the checks come first
    assert lib.h2_poseidon_permute_device(7, p, 1, p, None) == _lib.H2_ERR_ARGS                    # bad field
    assert lib.h2_poseidon_permute_device(0, None, 1, p, None) == _lib.H2_ERR_ARGS                 # no states
    assert lib.h2_poseidon_permute_device(0, p, 1, None, None) == _lib.H2_ERR_ARGS                 # no output
    assert lib.h2_poseidon_permute_device(0, p, (1 << 30) + 1, p, None) == _lib.H2_ERR_ARGS        # too many
    assert lib.h2_poseidon_hash_device(-1, p, 1, 2, p, None) == _lib.H2_ERR_ARGS
    assert lib.h2_poseidon_hash_device(1, None, 1, 2, p, None) == _lib.H2_ERR_ARGS
    assert lib.h2_poseidon_hash_device(1, p, 1, 2, None, None) == _lib.H2_ERR_ARGS
    assert lib.h2_poseidon_hash_device(1, p, 1, 0, p, None) == _lib.H2_ERR_ARGS                    # len = 0
    assert lib.h2_poseidon_hash_device(1, None, 0, 0, None, None) == _lib.H2_ERR_ARGS              # len = 0 even for no messages
    assert lib.h2_poseidon_hash_device(1, p, 1, 1 << 32, p, None) == _lib.H2_ERR_ARGS              # len >= 2^32
    assert lib.h2_poseidon_hash_device(1, p, 1 << 20, 1 << 21, p, None) == _lib.H2_ERR_ARGS        # n * len > 2^40
    assert lib.h2_poseidon_trace_device(2, p, 1, p, None) == _lib.H2_ERR_ARGS
    assert lib.h2_poseidon_trace_device(0, None, 1, p, None) == _lib.H2_ERR_ARGS
    assert lib.h2_poseidon_trace_device(0, p, 1, None, None) == _lib.H2_ERR_ARGS
    if lib.h2_device_count() == 0:
        assert lib.h2_poseidon_permute_device(0, None, 0, None, None) == _lib.H2_ERR_NODEV
        assert lib.h2_poseidon_hash_device(0, None, 0, 1, None, None) == _lib.H2_ERR_NODEV
        assert lib.h2_poseidon_trace_device(1, None, 0, None, None) == _lib.H2_ERR_NODEV
        assert lib.h2_poseidon_permute_device(0, p, 1, p, None) == _lib.H2_ERR_NODEV               # valid arguments, no device: no launch
