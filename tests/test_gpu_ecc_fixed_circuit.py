"""The fixed-base gadget on the device: `EccChip.mul_fixed_many` against the cell-by-cell `mul_fixed` over tables built by
`ecc.FixedBase`, the device MockProver, a proof of 65 multiplications, the example, the trace across a chunk of its scratch, and the
mirror of the reference's `MyEccCircuit` against the reference's pinned key and stored proof."""
import functools

import numpy as np
import pytest

import halo2_amd as h
from halo2_amd import circuit as front
from halo2_amd import dev, ecc, fields
from halo2_amd import verifier as hv
from halo2_amd.gadgets.ecc import FixedBaseTables
from halo2_amd.transcript import Blake2bWrite
from oracle import c_oracle as co

import ecc_cases as ec
import ecc_fixed_cases as fx
from ecc_fixed_cases import GENERATOR, NUM_WINDOWS, P, MulFixedCircuit

pytestmark = pytest.mark.gpu
FP = 0
VESTA = h.VESTA


def _ints(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else t
    return fields.from_limbs(np.ascontiguousarray(a).view(np.uint64).reshape(-1, 4), FP, True)


def _rng(seed):
    sf = co.field_of_curve(VESTA, "scalar")
    ctr = [seed]

    def rng(count):
        ctr[0] += 1
        return co.random_field(sf, ctr[0], count)
    return rng


@functools.lru_cache(maxsize=None)
def device_tables():
    return FixedBaseTables.of(ecc.FixedBase(fields.to_limbs(list(GENERATOR), FP).reshape(8)))


def _scalars(count):
    return (fx.EDGE_SCALARS + ec.random_scalars(65, seed=41))[:count]


def test_the_device_tables_are_the_host_tables():
    """z against the lists, the rest against the restatement, so that the circuits below stand on checked tables"""
    t, host = device_tables(), fx.host_tables()
    assert (t.generator, t.window_table, t.lagrange_coeffs, t.z) == (host.generator, host.window_table, host.lagrange_coeffs, host.z)
    assert all(u * u % P == (pt[1] + z) % P for row, z, us in zip(t.window_table, t.z, t.u) for pt, u in zip(row, us))


@pytest.mark.parametrize("count", [1, 3])
def test_mul_fixed_many_lays_the_rows_of_mul_fixed(count):
    """the ten advice columns, the fixed columns of the tables and the selectors of the bulk region are the regions of `count` calls of the host
    `mul_fixed` one after the other; the bulk additions hold the rows of the calls' complete additions; the copies bind the same cells"""
    scalars = _scalars(6)[-count:] if count == 1 else _scalars(count)          # count = 1: the unreduced doubling string
    tables = device_tables()
    sides = []
    for many in (False, True):
        circuit = MulFixedCircuit(scalars, tables, many=many)
        _, assembly, layouter = front.synthesize(circuit, 11, FP, fixed=True, advice=True, instances=[])
        advice = [_ints(c) for c in assembly.columns_to_field(assembly.advice)]
        fixed = [_ints(c) for c in assembly.columns_to_field(assembly.fixed)]
        sides.append((circuit, advice, fixed, assembly.selectors, layouter))
    (one, a, fa, sa, la), (bulk, b, fb, sb, lb) = sides
    nw = NUM_WINDOWS
    start, add_start = lb.regions[bulk.bulk.region_index], lb.regions[bulk.bulk.add_region_index]
    for i, (product, scalar) in enumerate(one.products):
        at = la.regions[scalar.windows[0].cell().region_index]
        add_at = la.regions[product.inner().x().cell().region_index]
        for c in range(10):
            assert b[c][start + nw * i:start + nw * (i + 1)] == a[c][at:at + nw], (i, c)
            assert b[c][add_start + 2 * i:add_start + 2 * i + 2] == a[c][add_at:add_at + 2], (i, c)
        for c in range(1, len(fa)):                                           # fixed column 0 is the range check's table
            assert fb[c][start + nw * i:start + nw * (i + 1)] == fa[c][at:at + nw], (i, c)
        assert (sb[:, start + nw * i:start + nw * (i + 1)] == sa[:, at:at + nw]).all()
        assert (sb[:, add_start + 2 * i:add_start + 2 * i + 2] == sa[:, add_at:add_at + 2]).all()
    want = [ec.ec_mul(k, GENERATOR) for k in scalars]
    got = _ints(bulk.bulk.outputs)
    assert [(got[2 * i], got[2 * i + 1]) for i in range(count)] == want
    assert bulk.bulk.window(count - 1, 84).row_offset == nw * count - 1 and bulk.bulk.result_y(0).row_offset == 1


def test_keygen_lays_out_the_same_shape_without_a_witness():
    scalars = _scalars(3)
    params = h.Params.new(VESTA, 11)
    try:
        with_witness = h.keygen_vk(params, MulFixedCircuit(scalars, device_tables(), many=True))
        assert h.keygen_vk(params, MulFixedCircuit(scalars, device_tables(), many=True).without_witnesses()).vk_repr == with_witness.vk_repr
        assert h.keygen_vk(params, MulFixedCircuit(scalars, fx.host_tables(), many=True).without_witnesses()).vk_repr == with_witness.vk_repr
    finally:
        params.close()


def test_mock_prover_accepts_both_paths():
    """the bulk path at k = 13 with 65 multiplications, the edge scalars in front; the per-call path at k = 11"""
    dev.MockProver.run_circuit(13, MulFixedCircuit(_scalars(65), device_tables(), many=True), [], FP).assert_satisfied()
    dev.MockProver.run_circuit(11, MulFixedCircuit(_scalars(6), device_tables()), [], FP).assert_satisfied()


def test_mock_prover_names_a_mutated_u():
    circuit = MulFixedCircuit([(1 << 255) - 1], device_tables(), mutate=(0, "u"))
    failures = dev.MockProver.run_circuit(11, circuit, [], FP).verify()
    cs, _, _ = front.synthesize(circuit.without_witnesses(), 11, FP, fixed=True, advice=False)
    names = [(g.name, n) for g in cs.gates for n in g.constraint_names]
    assert failures and [names[f.gate_index] + (f.row,) for f in failures] == [("Full-width fixed-base scalar mul", "check y",
                                                                                 circuit.mutated_row)]


def _example():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "ecc_fixed_mul.py")
    spec = importlib.util.spec_from_file_location("ecc_fixed_mul", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_a_proof_of_65_multiplications():
    """keygen, create_proof and verify_proof at k = 13 with the products as public inputs; one changed input is rejected"""
    scalars = _scalars(65)
    want = [c for k in scalars for c in ec.ec_mul(k, GENERATOR)]
    circuit = _example().EccFixedMulCircuit(scalars, device_tables())
    params = h.Params.new(VESTA, 13)
    try:
        pk = h.keygen_pk(params, circuit)
        tr = Blake2bWrite(VESTA)
        h.create_proof(params, pk, [circuit], [[want]], _rng(15), tr)
        proof = tr.finalize()
        assert hv.verify_proof(params, pk.vk, [want], proof)
        wrong = list(want)
        wrong[7] = (wrong[7] + 1) % P
        assert not hv.verify_proof(params, pk.vk, [wrong], proof)
    finally:
        params.close()


def test_the_example_proves_two_value_commitments():
    """examples/ecc_fixed_mul.py end to end (2 commitments [v]V + [r]R), its two bases' tables built on the way"""
    assert _example().main(["--count", "2"]) is True


def test_the_short_form_over_device_tables():
    """`mul_fixed_short` and `mul_sign` over the generator's 22-window tables from the device, under the device MockProver; the
    products are `ecc.mul_fixed_short`'s"""
    base = ecc.FixedBase(fields.to_limbs(list(GENERATOR), FP).reshape(8), fx.NUM_WINDOWS_SHORT)
    pairs = [(m, s) for m in (0, 1, (1 << 64) - 1) for s in (1, P - 1)]
    pt = ec.random_bases(1, seed=50)[0]
    circuit = fx.ShortCircuit(pairs, FixedBaseTables.of(base), [(pt, P - 1), ((0, 0), 1)])
    dev.MockProver.run_circuit(11, circuit, [], FP).assert_satisfied()
    got = [(p.inner().x().value().inner.evaluate(P), p.inner().y().value().inner.evaluate(P)) for p in circuit.products]
    outside = _ints(ecc.mul_fixed_short(base, fields.to_limbs([m for m, _ in pairs], FP, montgomery=False),
                                        [1 if s == 1 else -1 for _, s in pairs]))
    assert got == [(outside[2 * i], outside[2 * i + 1]) for i in range(len(pairs))] == [ec.ec_mul(m if s == 1 else -m, GENERATOR)
                                                                                        for m, s in pairs]


def test_trace_across_a_chunk_of_scratch():
    """the trace goes through its scratch in chunks of 2^23 / 83 = 101 067 multiplications: 70 more than one chunk, 65 scalars over and
    over, so the rows on both sides of the boundary must be the rows of the same scalars in a call of their own"""
    import torch
    base = device_tables().device
    k65 = torch.from_numpy(fields.to_limbs(_scalars(65), FP, montgomery=False).view(np.int64)).to(fields.current_device())
    per_chunk = (1 << 23) // 83
    count = per_chunk + 70
    reps = (count + 64) // 65
    cols, aux = ecc.mul_fixed_trace(base, k65.repeat(reps, 1)[:count].contiguous())
    want_cols, want_aux = ecc.mul_fixed_trace(base, k65)
    nw = NUM_WINDOWS
    for i in (0, per_chunk - 1, per_chunk, per_chunk + 1, count - 1):
        j = i % 65
        assert torch.equal(cols[:, nw * i:nw * (i + 1)], want_cols[:, nw * j:nw * (j + 1)]), i
        assert torch.equal(aux[i], want_aux[j]), i
    assert torch.equal(aux, want_aux.repeat(reps, 1, 1)[:count])


# ---- the reference's test circuit: its stored key and proof, and a proof of our own ----------------------------------------------------------
import sinsemilla_cases as sc                                                 # noqa: E402
from oracle import plonk_api                                                  # noqa: E402


@functools.lru_cache(maxsize=None)
def short_tables():
    return FixedBaseTables.of(ecc.FixedBase(fields.to_limbs(list(GENERATOR), FP).reshape(8), fx.NUM_WINDOWS_SHORT))


def test_the_references_key_and_proof():
    """keygen of the `MyEccCircuit` mirror over the DEVICE's tables reproduces the reference's pinned key text bit for bit -- through
    the fixed-column commitments that is every Lagrange coefficient and every z the search found, through the permutation commitments
    every copy -- and the verifier accepts the proof the reference stored"""
    text = sc.fixture_text("vk_ecc_chip.rdata.gz")
    params = h.Params.new(VESTA, 11)
    try:
        vk = h.keygen_vk(params, fx.MyEccCircuit(device_tables(), short_tables()).without_witnesses())
        assert vk.pinned() == plonk_api.compact_debug(text)
        assert vk.vk_repr == plonk_api.transcript_repr(text)
        proof = open(sc.os.path.join(sc.GOLDEN, "proof_ecc_chip.bin"), "rb").read()
        assert len(proof) == 3872
        assert hv.verify_proof_many(params, vk, [[]], proof)
        bad = bytearray(proof)
        bad[len(proof) // 2] ^= 1
        assert not hv.verify_proof_many(params, vk, [[]], bytes(bad))
    finally:
        params.close()


def test_the_references_circuit_with_a_seeded_witness():
    """the same circuit with witnesses from a seeded generator: the device MockProver is satisfied, and a proof of it verifies under
    the key the reference pins"""
    circuit = fx.MyEccCircuit(device_tables(), short_tables(), seed=7)
    dev.MockProver.run_circuit(11, circuit, [], FP).assert_satisfied()
    params = h.Params.new(VESTA, 11)
    try:
        pk = h.keygen_pk(params, circuit)
        assert pk.vk_repr == plonk_api.transcript_repr(sc.fixture_text("vk_ecc_chip.rdata.gz"))
        tr = Blake2bWrite(VESTA)
        h.create_proof(params, pk, [circuit], [[]], _rng(16), tr)
        proof = tr.finalize()
        assert len(proof) == 3872 and hv.verify_proof(params, pk.vk, [], proof)
    finally:
        params.close()
