"""LookupRangeCheck4_5BConfig, mux and the bulk range checks on the host: the constraint systems of the mirrored circuits against the
keys the reference stored (tests/golden/vk_*_4_5b*, vk_short_range_check_case*), the reference's MockProver cases under
tests/mock_prover_model.py, and the bulk layout against the loop of single calls on a synthesis without a witness.  No GPU."""
import numpy as np
import pytest

import ecc_cases as ec
import ecc_fixed_cases as fx
import range_check_cases as rc
import sinsemilla_cases as sc
import sinsemilla_commit_cases as cc
from halo2_amd import circuit as front
from range_check_cases import P

K11 = 11


# ---- 1: the constraint systems of the stored keys --------------------------------------------------------------------------------------------
def _stored():
    return rc.stored_circuits(lambda: (fx.host_tables(fx.NUM_WINDOWS), fx.host_tables(fx.NUM_WINDOWS_SHORT)), cc.host_domain, table=sc.table())


@pytest.mark.parametrize("name", rc.STORED_NAMES)
def test_constraint_system_is_the_references(name):
    """every gate, lookup (both pairs of the 4_5b lookup, their trees in the reference's order), query, permutation column and constant,
    and the columns the selectors compress into"""
    make, vk_name, _ = _stored()[name]
    cs = sc.host_keygen_cs(make(), K11)
    assert cs.pinned() == sc.fixture_cs(sc.fixture_text(vk_name))


def test_the_plain_keys_still_match():
    assert sc.host_keygen_cs(rc.LookupCircuit(6, "plain"), K11).pinned() == sc.fixture_cs(sc.fixture_text("vk_lookup_range_check.rdata"))
    assert sc.host_keygen_cs(sc.LookupCircuit(6), K11).pinned() == sc.fixture_cs(sc.fixture_text("vk_lookup_range_check.rdata"))


def test_the_table_of_the_4_5b_config():
    """1072 rows: 0 .. 1023 tagged 0, 0 .. 15 tagged 4, 0 .. 31 tagged 5; then the default (0, 0) to the end"""
    _, assembly, _ = front.synthesize(rc.LookupCircuit(6, "4_5b"), K11, ec.FP, fixed=True, advice=False)
    fixed = assembly.host_columns(assembly.fixed)
    want = [(i, 0) for i in range(1024)] + [(i, 4) for i in range(16)] + [(i, 5) for i in range(32)]
    rows = list(zip(fixed[0], fixed[2]))
    assert rows[:1072] == want and set(rows[1072:assembly.usable]) == {(0, 0)}


# ---- 2: the reference's MockProver cases ---------------------------------------------------------------------------------------------------
def _short(element, num_bits, lookup):
    failures, _, _, layouter, _ = ec.host_model(rc.ShortRangeCheckCircuit(element, num_bits, lookup), K11)
    assert layouter.shapes[0][1] == (1 if lookup == "4_5b" and num_bits in (4, 5) else 3)
    return rc.region_offsets(layouter, failures)


@pytest.mark.parametrize("lookup", ["plain", "4_5b"])
@pytest.mark.parametrize("element, num_bits, offsets", rc.SHORT_CASES, ids=["zero-bits", "k-bits", "63", "64", "1024", "crafted"])
def test_short_range_check_cases(lookup, element, num_bits, offsets):
    """lookup_range_check.rs:1076-1223: lookup 0, region 1 "Range check 6 bits", exactly the listed offsets"""
    assert _short(element, num_bits, lookup) == [(0, 1, o) for o in offsets]


@pytest.mark.parametrize("element, num_bits, offsets", rc.SHORT_CASES_4_5B, ids=["15", "32", "16", "31"])
def test_short_range_check_cases_of_the_tagged_lookup(element, num_bits, offsets):
    """lookup_range_check.rs:1225-1247 and their neighbours: one row, looked up as (value, tag)"""
    assert _short(element, num_bits, "4_5b") == [(0, 1, o) for o in offsets]


def test_the_reference_lookup_circuit_is_satisfied_on_4_5b():
    assert ec.host_model(rc.LookupCircuit(6, "4_5b"), K11)[0] == []


def test_a_5_bit_value_passes_the_plain_three_rows_too():
    assert _short(31, 5, "plain") == [] and _short(32, 5, "plain") == [(0, 1, 1)]


# ---- 3: cond swap and mux ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("swap", [True, False])
def test_cond_swap(swap):
    a, b = 0x1234567, P - 5
    circuit = rc.CondSwapCircuit(a, b, swap)
    assert ec.host_model(circuit, 3)[0] == []
    got = tuple(c.value().inner.evaluate(P) for c in circuit.pair)
    assert got == ((b, a) if swap else (a, b))


def _points():
    left, right = ec.random_bases(2, seed=77)
    return left, right


@pytest.mark.parametrize("lookup", ["plain", "4_5b"])
@pytest.mark.parametrize("choice", [0, 1])
def test_mux(lookup, choice):
    left, right = _points()
    chosen = right if choice else left
    assert ec.host_model(rc.MuxCircuit(left, right, choice, lookup), 5, [list(chosen)])[0] == []
    failures = ec.host_model(rc.MuxCircuit(left, right, choice, lookup), 5, [list(left if choice else right)])[0]
    assert failures and {f[0] for f in failures} == {"Permutation"}


def test_mux_of_a_choice_that_is_no_bit():
    left, right = _points()
    failures, names, _, _, _ = ec.host_model(rc.MuxCircuit(left, right, 2, "plain"), 5, [list(right)])
    gates = [names[f[1]] for f in failures if f[0] == "ConstraintNotSatisfied"]
    # each of the four mux regions fails "swap is bool"; a' = 2 b - a is not the point the chip assigned either
    assert sum(n[1] == "swap is bool" for n in gates) == 4 and {n[0] for n in gates} == {"a' = b ⋅ swap + a ⋅ (1-swap)"}


def test_merkle_chip_forwards_mux_and_private_init():
    from halo2_amd.gadgets.sinsemilla import MerkleChip
    assert MerkleChip.mux is not None and MerkleChip.hash_to_point_with_private_init is not None
    calls = []

    class Inner:
        def mux(self, *a):
            calls.append(("mux", a))
            return "m"

        def hash_to_point_with_private_init(self, *a):
            calls.append(("hash", a))
            return "h"
    chip = MerkleChip.__new__(MerkleChip)
    chip._cond_swap = chip._sinsemilla = Inner()
    assert chip.mux("l", 1, 2, 3) == "m" and chip.hash_to_point_with_private_init("l", "q", "msg") == "h"
    assert calls == [("mux", ("l", 1, 2, 3)), ("hash", ("l", "q", "msg"))]


# ---- 4: the bulk layout ------------------------------------------------------------------------------------------------------------------------------
def _keygen_side(circuit, k):
    cs, assembly, layouter = front.synthesize(circuit.without_witnesses(), k, ec.FP, fixed=True, advice=False)
    fixed = assembly.host_columns(assembly.fixed)
    return assembly.selectors.copy(), fixed, assembly.permutation.flat().copy(), cs.pinned(), layouter


@pytest.mark.parametrize("copy", [False, True], ids=["witness", "copy"])
@pytest.mark.parametrize("lookup", ["plain", "4_5b"])
def test_bulk_layout_equals_the_loop(lookup, copy):
    """range_check_many and short_range_check_many against the loop of single calls, without a witness: the same selectors, fixed cells
    (the constants among them, in the same order) and copies, on the same rows"""
    checks = rc.bulk_checks(count=5)
    a = _keygen_side(rc.BulkCircuit(checks, lookup, many=False, copy=copy), K11)
    b = _keygen_side(rc.BulkCircuit(checks, lookup, many=True, copy=copy), K11)
    assert np.array_equal(a[0], b[0]) and a[0].sum() > 0
    assert a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3] == b[3]
    # one region per check instead of one per element, over the same rows
    first = 5 * 5 if copy else 0
    assert len(b[4].regions) == first + 5 and len(a[4].regions) == first + 25
    short_rows = 1 if lookup == "4_5b" else 3
    bulk = b[4].shapes[5::6] if copy else b[4].shapes                         # copy: five cells are loaded in front of every check
    assert [s[1] for s in bulk] == [5 * 14, 5 * 26, 5 * short_rows, 5 * short_rows, 5 * 3]


def test_bulk_cells_are_the_loops_cells_row_for_row():
    checks = rc.bulk_checks(count=3)
    sides = []
    for many in (False, True):
        circuit = rc.BulkCircuit(checks, "4_5b", many=many, witness=False)
        _, _, layouter = front.synthesize(circuit, K11, ec.FP, fixed=True, advice=False)
        rows = lambda cell: (cell.column, layouter.regions[cell.region_index] + cell.row_offset)      # noqa: E731
        sides.append([[[rows(z) for z in zs] for zs in c] if isinstance(c[0], list) else [rows(z) for z in c] for c in circuit.cells])
    assert sides[0] == sides[1]
