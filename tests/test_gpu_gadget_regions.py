"""The gadget circuits the repository already mock-proves, with `regions=True`: every cell a chip's gates read where the chip enables
them is assigned by the region that enables them (no CellNotAssigned, no InstanceCellNotAssigned), under both floor planners and on
the bulk (`*_many`) paths, whose whole columns are one recorded range each; and the circuits stay satisfied.  The circuits and their
witnesses come from the existing case modules and device tests."""
import pytest

from halo2_amd import dev, fields

import ecc_cases as ec
import ecc_fixed_cases as fx
import floor_planner_cases as fc
import poseidon_cases as pc
import range_check_cases as rcc
import sinsemilla_cases as sc
import sinsemilla_commit_cases as cc

pytestmark = pytest.mark.gpu
FP = 0


def _clean(k, circuit, instances=()):
    prover = dev.MockProver.run_circuit(k, circuit, list(instances), FP, regions=True)
    failures = prover.verify()
    assert failures == [], [str(f) for f in failures[:5]]
    counts = prover.failure_counts
    assert counts["CellNotAssigned"] == 0 and counts["InstanceCellNotAssigned"] == 0 and sum(counts.values()) == 0
    assert prover.regions and any(r.enabled_selectors for r in prover.regions)
    return prover


def test_poseidon_hash_and_permute_many():
    import test_gpu_poseidon as tp
    message = [s[0] for s in pc.random_states(2, FP, 41)]
    _clean(6, pc.HashCircuit(2, message, pc.hash_ints(message, FP)))
    states = pc.random_states(3, FP, 9)
    prover = _clean(8, pc.PermuteManyCircuit(3, tp._up(pc.states_limbs(states, FP))))
    assert any(count == 3 * pc.ROWS for r in prover.regions for _, _, count in r.cells)                   # a whole column is one range


def test_sinsemilla_merkle_path():
    leaf, pos, path = sc.merkle_witness()
    _clean(11, sc.MerkleCircuit(leaf, pos, path))


def test_sinsemilla_commit_domain():
    import test_gpu_sinsemilla_commit as tc
    _clean(11, cc.MySinsemillaCircuit(tc.device_domain(), seed=7))


def test_ecc_mul_and_mul_many():
    import test_gpu_ecc as te
    _clean(11, ec.MulCircuit(te._pairs(2)))
    _clean(11, ec.MulManyCircuit(te._pairs(2)))


def test_ecc_mul_fixed():
    import test_gpu_ecc_fixed_circuit as tf
    _clean(11, fx.MulFixedCircuit(tf._scalars(2), tf.device_tables()))
    _clean(11, fx.MulFixedCircuit(tf._scalars(2), tf.device_tables(), many=True))


@pytest.mark.parametrize("lookup", ["plain", "4_5b"])
@pytest.mark.parametrize("many", [False, True], ids=["scalar", "bulk"])
def test_lookup_range_checks(lookup, many):
    _clean(11, rcc.BulkCircuit(rcc.bulk_checks(count=3), lookup, many=many))


def test_the_gadget_circuit_under_v1():
    left, right = fields.to_limbs([11, 12], FP, True), fields.to_limbs([21, 22], FP, True)
    _clean(fc.GadgetCircuit.K, fc.GadgetCircuitV1(left, right))
    _clean(fc.GadgetCircuit.K, fc.GadgetCircuit(left, right))
