"""`plonk::create_proof` and both verifiers on every constraint-system shape of tests/plonk_shape_cases.py: rotations up to +-4 on advice, fixed
and instance columns, 5 / 6 / 7 blinding factors, permutations of 0 to 4 columns of every kind in 1 to 4 sets, 0 / 1 / 3 lookups, degrees 3 to 9,
1 to 3 circuits, both curves.  The device prover's bytes must EQUAL the sequential restatement's (oracle/plonk.py) for the same randomness -- a wrong
rotation scale, set boundary or point-set order still gives a transcript that looks like a proof -- the device-computed verifying key must equal the
oracle's, and the device verifier's verdict must equal the oracle verifier's on the proof, on every broken witness and on a one-bit flip in every
section of the proof.  tests/test_plonk_shape_case_coverage.py shows, without a GPU, that the oracle alone meets all of that.
Runs only on a real MI355X (`-m gpu`)."""
import pytest

import halo2_amd as h
from halo2_amd import verifier as hv
from halo2_amd._lib import ConstraintSystemFailure
from halo2_amd.plonk import create_proof_many, keygen_pk
from halo2_amd.transcript import Blake2bWrite
from oracle import c_oracle as co
from oracle import ipa
from oracle import plonk as oplonk

import plonk_shape_cases as cases

pytestmark = pytest.mark.gpu


def _rng(sf, seed):
    ctr = [seed]

    def rng(count):
        ctr[0] += 1
        return co.random_field(sf, ctr[0], count)
    return rng


def _first_difference(shape, ours: bytes, theirs: bytes) -> str:
    if len(ours) != len(theirs):
        return "%d bytes, the restated prover wrote %d" % (len(ours), len(theirs))
    at = next(i for i, (a, b) in enumerate(zip(ours, theirs)) if a != b)
    name, lo, _ = next(sec for sec in cases.sections(shape) if sec[1] <= at < sec[2])
    return "first difference at byte %d: element %d of the %s" % (at, (at - lo) // 32, name)


@pytest.mark.parametrize("shape", cases.SHAPES, ids=[s.name for s in cases.SHAPES])
def test_device_prover_and_verifier_equal_the_restatement(shape):
    s = shape
    curve, k, cs = s.curve, s.k, s.cs
    sf = co.field_of_curve(curve, "scalar")
    vk_repr = cases.VK_REPR % cases.modulus(curve)
    g = co.generate_bases(curve, cases.GENERATOR_SEED + k, s.n)
    w, u = co.generate_bases(curve, 60, 1)[0], co.generate_bases(curve, 61, 1)[0]
    params = h.Params.from_generators(curve, k, g, None, w, u)
    pk = keygen_pk(params, cs, s.fixed, s.mapping, vk_repr)

    def device_proof(circuits):
        tr = Blake2bWrite(curve)
        create_proof_many(params, pk, circuits, _rng(sf, cases.RNG_SEED), tr)
        return tr.finalize()

    def oracle_proof(circuits):
        ot = ipa.Transcript(curve)
        oplonk.create_proof_many(curve, k, g, w, u, cs, s.fixed, s.mapping, vk_repr, circuits, _rng(sf, cases.RNG_SEED), ot)
        return bytes(ot.out)

    # the verifying key, and the proof's bytes
    vk = oplonk.keygen_vk(curve, k, g, w, cs, s.fixed, s.mapping, vk_repr)
    dvk = hv.keygen_vk(params, pk)
    assert dvk.fixed_commitments == vk["fixed_commitments"]
    assert dvk.permutation_commitments == vk["permutation_commitments"]
    instances = [inst for _, inst in s.circuits]
    device = lambda inst, proof: hv.verify_proof_many(params, dvk, inst, proof)
    oracle = lambda inst, proof: oplonk.verify_proof_many(curve, k, g, w, u, vk, inst, proof)
    expected = oracle_proof(s.circuits)
    proof = device_proof(s.circuits)
    assert proof == expected, _first_difference(s, proof, expected)
    assert cases.sections(s)[-1][2] == len(proof)
    assert oracle(instances, proof) is True and device(instances, proof) is True

    # broken witnesses: a transcript both verifiers reject, or -- an input that is not in the table -- no transcript at all
    for variant in s.broken:
        circuits = cases.broken_circuits(s, variant)
        if variant == "lookup":
            with pytest.raises(ConstraintSystemFailure):
                device_proof(circuits)
            again = device_proof(s.circuits)                        # ... which leaves nothing behind on this Params
            assert again == expected, _first_difference(s, again, expected)
            continue
        bad = device_proof(circuits)
        bad_instances = [inst for _, inst in circuits]
        assert bad == oracle_proof(circuits), variant
        assert oracle(bad_instances, bad) is False and device(bad_instances, bad) is False, variant
        if variant == "public":                                    # the good proof is no proof of the wrong input, nor the bad one of the right input
            assert oracle(bad_instances, proof) is False and device(bad_instances, proof) is False
            assert oracle(instances, bad) is False and device(instances, bad) is False

    # one bit in every section
    for name, offset, mask in cases.section_flips(s):
        flipped = bytearray(proof)
        flipped[offset] ^= mask
        verdict = device(instances, bytes(flipped))
        assert verdict is False, name
        assert verdict == oracle(instances, bytes(flipped)), name
    assert device(instances, proof[:-1]) is False and device(instances, proof + b"\0") is False

    if len(s.circuits) > 1:
        swapped = [instances[1], instances[0]] + instances[2:]
        assert swapped != instances
        assert oracle(swapped, proof) is False and device(swapped, proof) is False
        assert oracle(instances[:-1], proof) is False and device(instances[:-1], proof) is False
    params.close()
