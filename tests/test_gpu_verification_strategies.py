"""The verifier's strategies on the device: the batched challenge-product kernel (h2_ipa_s_combine*) against big-integer arithmetic,
`Guard::compute_g` / `use_g` and the AccumulationVerifier of the reference's own test (tests/plonk_api.rs:513-545), and
`BatchVerifier` (plonk/verifier/batch.rs; tests/plonk_api.rs:561-582) on the stored reference proof and on batches of fresh
proofs, every verdict checked against the oracle's restated verifier.  Runs only on a real MI355X (`-m gpu`)."""
import os
import random

import numpy as np
import pytest

import halo2_amd as h
from halo2_amd import batch as hb
from halo2_amd import fields
from halo2_amd import verifier as hv
from halo2_amd.plonk import ConstraintSystem, create_proof, create_proof_many, keygen_pk
from halo2_amd.transcript import Blake2bWrite
from oracle import c_oracle as co
from oracle import pasta as o
from oracle import plonk as oplonk
from oracle import plonk_api as pa
from plonk_circuits import make_cs, make_witness

pytestmark = pytest.mark.gpu
VESTA = h.VESTA


def _rng(sf, seed):
    ctr = [seed]

    def rng(count):
        ctr[0] += 1
        return co.random_field(sf, ctr[0], count)
    return rng


# ---- 1. the kernel against big integers ----------------------------------------------------------------------------------------
def _s_at(u, c, j, k, m):
    v = c
    for i in range(k):
        if (j >> i) & 1:
            v = v * u[k - 1 - i] % m
    return v


def _combined_full(us, cs_, k, m):
    total = [0] * (1 << k)
    for u, c in zip(us, cs_):
        s = [c % m]
        for u_j in reversed(u):                                       # compute_s, poly/commitment/verifier.rs:156-172
            s += [v * u_j % m for v in s]
        total = [(a + b) % m for a, b in zip(total, s)]
    return total


def _inputs(field, k, batch, seed):
    m = fields.MODULUS[field]
    rnd = random.Random(seed)
    us = [[rnd.randrange(m) for _ in range(k)] for _ in range(batch)]
    cs_ = [rnd.randrange(m) for _ in range(batch)]
    edges = [1, m - 1, 0]                                             # challenges 1, q - 1 and 0
    for b in range(batch):
        if b % 3 == 1:
            us[b][rnd.randrange(k)] = edges[b % len(edges)]
        if b % 4 == 2:
            us[b] = [edges[(b + i) % 2] for i in range(k)]            # all 1 / q - 1
    if batch > 1:
        cs_[0] = 0                                                    # a zero coefficient
    if batch > 3:
        us[3][0] = 0
    return us, cs_


def _run_kernel(field, k, us, cs_, form, init):
    import torch
    mont = form == h.FORM_MONTGOMERY
    ch = fields.to_limbs([v for u in us for v in u], field, mont)
    co_ = fields.to_limbs(cs_, field, mont)
    dev = fields.current_device()
    out = torch.from_numpy(fields.to_limbs(init, field, mont).view(np.int64)).to(dev) if init else \
        torch.full((1 << k, 4), -1, dtype=torch.int64, device=dev)    # garbage: accumulate = 0 must overwrite every row
    h.ipa_s_combine(k, ch, co_, field, out, form=form, accumulate=bool(init))
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64), ch, co_


FULL = [(1, 1), (1, 300), (2, 5), (2, 64), (7, 2), (7, 64), (7, 300), (12, 1), (12, 5), (12, 64), (16, 2), (16, 5)]


@pytest.mark.parametrize("k,batch", FULL)
@pytest.mark.parametrize("form", [h.FORM_MONTGOMERY, h.FORM_CANONICAL])
@pytest.mark.parametrize("field", [h.FP, h.FQ])
def test_s_combine_full_vector(field, form, k, batch):
    """Every output of the kernel, overwrite and accumulate, equals sum_b c_b * compute_s(u_b, 1) in Python integers."""
    m = fields.MODULUS[field]
    us, cs_ = _inputs(field, k, batch, 1000 * k + batch + field)
    want = _combined_full(us, cs_, k, m)
    mont = form == h.FORM_MONTGOMERY
    got, ch, co_ = _run_kernel(field, k, us, cs_, form, None)
    assert np.array_equal(got, fields.to_limbs(want, field, mont))
    rnd = random.Random(k + batch)
    init = [rnd.randrange(m) for _ in range(1 << k)]
    got_acc, _, _ = _run_kernel(field, k, us, cs_, form, init)
    assert np.array_equal(got_acc, fields.to_limbs([(a + b) % m for a, b in zip(init, want)], field, mont))
    if k <= 12 and batch <= 64:                                       # the host-pointer form: the same bytes
        host = np.zeros((1 << k, 4), dtype=np.uint64)
        h.ipa_s_combine(k, ch, co_, field, host, form=form)
        assert np.array_equal(host, got)
        h.ipa_s_combine(k, ch, co_, field, host, form=form, accumulate=True)
        assert np.array_equal(host, fields.to_limbs([2 * v % m for v in want], field, mont))


@pytest.mark.parametrize("field,form", [(h.FP, h.FORM_MONTGOMERY), (h.FQ, h.FORM_CANONICAL)])
def test_s_combine_k20(field, form):
    """k = 20: the full vector at batch 1 and 2; at batch 64, 4096+ spot indices (0, 2^k - 1, every power of two, random)."""
    k, m = 20, fields.MODULUS[field]
    mont = form == h.FORM_MONTGOMERY
    for batch in (1, 2):
        us, cs_ = _inputs(field, k, batch, 77 + batch)
        got, _, _ = _run_kernel(field, k, us, cs_, form, None)
        assert np.array_equal(got, fields.to_limbs(_combined_full(us, cs_, k, m), field, mont))
    us, cs_ = _inputs(field, k, 64, 99)
    got, ch, co_ = _run_kernel(field, k, us, cs_, form, None)
    rnd = random.Random(5)
    idx = sorted({0, (1 << k) - 1} | {1 << i for i in range(k)} | {rnd.randrange(1 << k) for _ in range(4200)})
    assert len(idx) >= 4096
    want = [sum(_s_at(u, c, j, k, m) for u, c in zip(us, cs_)) % m for j in idx]
    assert np.array_equal(got[idx], fields.to_limbs(want, field, mont))
    host = np.zeros((1 << k, 4), dtype=np.uint64)
    h.ipa_s_combine(k, ch, co_, field, host, form=form)
    assert np.array_equal(host, got)


def test_s_combine_batch_300_at_k16_spot():
    """Batch 300 (ten LDS chunks) at k = 16: spot indices against the definition."""
    field, k = h.FQ, 16
    m = fields.MODULUS[field]
    us, cs_ = _inputs(field, k, 300, 4242)
    got, _, _ = _run_kernel(field, k, us, cs_, h.FORM_MONTGOMERY, None)
    rnd = random.Random(6)
    idx = sorted({0, (1 << k) - 1} | {1 << i for i in range(k)} | {rnd.randrange(1 << k) for _ in range(300)})
    want = [sum(_s_at(u, c, j, k, m) for u, c in zip(us, cs_)) % m for j in idx]
    assert np.array_equal(got[idx], fields.to_limbs(want, field, True))


# ---- 2. the reference's own strategy tests on its stored proof ------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference_setup():
    from test_reference_goldens import GOLDEN
    g, _, w, u = pa.params_new("vesta", 5, with_lagrange=False)
    gm, wm, um = co.points_to_mont(VESTA, g), co.points_to_mont(VESTA, [w])[0], co.points_to_mont(VESTA, [u])[0]
    params = h.Params.from_generators(VESTA, 5, gm, None, wm, um)
    cs = pa.constraint_system(ConstraintSystem)
    fixed, mapping = pa.keygen_columns(o.P)
    vk_repr = pa.transcript_repr(open(os.path.join(GOLDEN, "plonk_api_pinned_vk.txt")).read())
    pk = keygen_pk(params, cs, fixed, mapping, vk_repr)
    dvk = hv.keygen_vk(params, pk)
    proof = open(os.path.join(GOLDEN, "plonk_api_proof.bin"), "rb").read()
    yield {"params": params, "pk": pk, "vk": dvk, "proof": proof, "g": g}
    params.close()


def test_reference_strategies_on_the_stored_proof(reference_setup):
    params, dvk, proof = reference_setup["params"], reference_setup["vk"], reference_setup["proof"]
    instances = [[[2]], [[2]]]
    acc = hv.AccumulationVerifier(params)
    assert hv.verify_proof_with_strategy(params, dvk, acc, instances, proof) is True
    assert isinstance(acc.accumulator, hv.Accumulator) and len(acc.accumulator.u) == 5 and acc.accumulator.g is not None
    assert hv.verify_proof_with_strategy(params, dvk, hv.SingleVerifier(params), instances, proof) is True
    assert hv.verify_proof_with_strategy(params, dvk, hv.AccumulationVerifier(params), [[[2]], [[3]]], proof) is False
    bv = hb.BatchVerifier()
    bv.add_proof(instances, proof)
    bv.add_proof(instances, proof)
    assert bv.finalize(params, dvk)
    bad_inst = hb.BatchVerifier()
    bad_inst.add_proof(instances, proof)
    bad_inst.add_proof([[[2]], [[3]]], proof)
    assert not bad_inst.finalize(params, dvk)
    for pos in (0, 1000, 2500, len(proof) - 1):
        bad = bytearray(proof)
        bad[pos] ^= 1
        bv = hb.BatchVerifier()
        bv.add_proof(instances, proof)
        bv.add_proof(instances, bytes(bad))
        assert not bv.finalize(params, dvk), pos
    # a fresh two-instance proof of the same circuit from the device prover joins the batch
    sf = co.field_of_curve(VESTA, "scalar")
    adv, inst = pa.witness(o.P)
    tr = Blake2bWrite(VESTA)
    create_proof_many(params, reference_setup["pk"], [(adv, inst), ([list(c) for c in adv], inst)], _rng(sf, 31337), tr)
    bv = hb.BatchVerifier()
    bv.add_proof(instances, proof)
    bv.add_proof(instances, tr.finalize())
    assert bv.finalize(params, dvk)


# ---- 3. compute_g is G'_0 -------------------------------------------------------------------------------------------------------
def _guard(params, vk, instances, proof):
    return hv._verify_guard(params, vk, instances, proof, hv.MSM(params))


def _check_compute_g(params, vk, instances, proof, g_mont):
    curve, k = params.curve, params.k
    sf = fields.CURVE_FIELDS[curve][1]
    m = fields.MODULUS[sf]
    guard = _guard(params, vk, instances, proof)
    G = guard.compute_g()
    s = _combined_full([guard.u], [1], k, m)
    want = co.jac_to_affine_ints(curve, co.best_multiexp(curve, co.to_mont(sf, co.ints_to_limbs(s)), g_mont))
    assert G == want
    if k <= 5:
        assert co.jac_to_affine_ints(curve, co.msm_naive(curve, co.to_mont(sf, co.ints_to_limbs(s)), g_mont)) == G
    msm, accumulator = guard.use_g(G)
    assert accumulator.g == G and accumulator.u == guard.u
    assert msm.eval()                                                 # the proof's MSM with [neg_c] G'_0 is the identity
    bm = fields.MODULUS[fields.CURVE_FIELDS[curve][0]]
    off = o.ec_add(G, (bm - 1, 2), bm)                                # G + the generator (-1, 2)
    msm2, _ = _guard(params, vk, instances, proof).use_g(off)
    assert not msm2.eval()


def test_compute_g_k5_reference_proof(reference_setup):
    _check_compute_g(reference_setup["params"], reference_setup["vk"], [[[2]], [[2]]], reference_setup["proof"],
                     co.points_to_mont(VESTA, reference_setup["g"]))


# ---- 4. batches of fresh proofs --------------------------------------------------------------------------------------------------
def _variant(base_advice, m, usable, seed):
    """Another satisfying witness for the same fixed columns and copy constraints as plonk_circuits.make_witness's: the distinct
    `a` values permuted among themselves (the lookup table and the equal-`a` cycles hold), fresh `b`, `c` recomputed."""
    a0, _, _ = base_advice
    rnd = random.Random(seed)
    vals = sorted(set(a0[:usable]))
    perm = dict(zip(vals, rnd.sample(vals, len(vals))))
    n = len(a0)
    a, b, c = [0] * n, [0] * n, [0] * n
    for r in range(usable):
        a[r] = perm[a0[r]]
        b[r] = c[r - 1] if r and r % 3 == 0 else rnd.randrange(m)
        c[r] = a[r] * b[r] % m if r % 2 else (a[r] + b[r]) % m
    return [a, b, c], [[a[0]]]


@pytest.fixture(scope="module", params=[7, 11])
def fresh(request):
    k = request.param
    curve = VESTA
    sf = fields.CURVE_FIELDS[curve][1]
    m = fields.MODULUS[sf]
    n = 1 << k
    cs = make_cs()
    usable = n - (cs.blinding_factors + 1)
    fixed, advice, mapping, _ = make_witness(random.Random(k), m, n, usable)
    g = co.generate_bases(curve, 970 + k, n)
    w, u = co.generate_bases(curve, 60, 1)[0], co.generate_bases(curve, 61, 1)[0]
    params = h.Params.from_generators(curve, k, g, None, w, u)
    vk_repr = 0x1234567890ABCDEF ** 3 % m
    pk = keygen_pk(params, cs, fixed, mapping, vk_repr)
    dvk = hv.keygen_vk(params, pk)
    ovk = oplonk.keygen_vk(curve, k, g, w, cs, fixed, mapping, vk_repr)
    items = []
    for i in range(8):
        adv, inst = _variant(advice, m, usable, 100 * k + i)
        tr = Blake2bWrite(curve)
        create_proof(params, pk, adv, inst, _rng(sf, 7000 + 50 * i), tr)
        items.append((inst, tr.finalize()))
    assert len({inst[0][0] for inst, _ in items}) > 1
    cache = {}

    def oracle_ok(inst, proof):
        key = (repr(inst), proof)
        if key not in cache:
            cache[key] = oplonk.verify_proof_many(curve, k, g, w, u, ovk, [inst], proof)
        return cache[key]
    yield {"k": k, "params": params, "vk": dvk, "items": items, "oracle": oracle_ok, "g": g, "m": m}
    params.close()


def _finalize(fx, items, rng=None):
    bv = hb.BatchVerifier()
    for inst, proof in items:
        bv.add_proof([inst], proof)
    got = bv.finalize(fx["params"], fx["vk"], rng=rng)
    assert got == all(fx["oracle"](inst, proof) for inst, proof in items)
    return got


def test_batch_of_fresh_proofs(fresh):
    items, m = fresh["items"], fresh["m"]
    assert _finalize(fresh, items)
    assert _finalize(fresh, items, rng=_rng(fields.CURVE_FIELDS[VESTA][1], 555))
    faults = []
    inst, proof = items[3]
    faults.append([(x if i != 3 else ([[(inst[0][0] + 1) % m]], proof)) for i, x in enumerate(items)])      # a wrong instance
    flipped = bytearray(proof)
    flipped[-33] ^= 1                                                                                      # inside the scalar c
    faults.append([(x if i != 3 else (inst, bytes(flipped))) for i, x in enumerate(items)])
    faults.append([(x if i != 3 else (inst, proof[:-1])) for i, x in enumerate(items)])                    # truncated
    swapped = list(items)
    i, j = next((i, j) for i in range(8) for j in range(i + 1, 8) if items[i][0] != items[j][0])
    (ia, pa_), (ib, pb) = items[i], items[j]
    swapped[i], swapped[j] = (ib, pa_), (ia, pb)                                                          # instances swapped
    faults.append(swapped)
    for bad in faults:
        assert not _finalize(fresh, bad)
    if fresh["k"] == 11:
        inst0, proof0 = items[0]
        _check_compute_g(fresh["params"], fresh["vk"], [inst0], proof0, fresh["g"])


# ---- 5. the weights matter -------------------------------------------------------------------------------------------------------
def test_weights_separate_cancelling_claims(reference_setup):
    params = reference_setup["params"]
    k = params.k
    sf = fields.CURVE_FIELDS[VESTA][1]
    m = fields.MODULUS[sf]
    bm = fields.MODULUS[fields.CURVE_FIELDS[VESTA][0]]
    P = reference_setup["g"][3]
    ones = [1] * k
    pos = hb.Claim({P[0]: [1, P[1]]}, None, None, 0, 0, ones)
    neg = hb.Claim({P[0]: [1, (bm - P[1]) % bm]}, None, None, 0, 0, ones)
    assert hb.combine_claims(params, [pos, neg], [1, 1]).eval()
    assert not hb.combine_claims(params, [pos, neg], hb.draw_weights(2, sf)).eval()
    rnd = random.Random(3)
    u = [rnd.randrange(1, m) for _ in range(k)]
    a = rnd.randrange(1, m)
    s_pos = hb.Claim({}, None, None, 0, a, u)
    s_neg = hb.Claim({}, None, None, 0, m - a, u)
    assert hb.combine_claims(params, [s_pos, s_neg], [1, 1]).eval()
    w = hb.draw_weights(2, sf, _rng(sf, 9))
    assert w == hb.draw_weights(2, sf, _rng(sf, 9)) and all(0 < x < m for x in w)
    assert not hb.combine_claims(params, [s_pos, s_neg], w).eval()
    calls = []

    def zero_first(count):                                            # a zero draw is drawn again
        calls.append(count)
        return np.zeros((count, 4), dtype=np.uint64) if len(calls) == 1 else co.random_field(sf, 1, count)
    again = hb.draw_weights(2, sf, zero_first)
    assert calls == [2, 2] and len(again) == 2 and all(0 < x < m for x in again)


# ---- 6. memory --------------------------------------------------------------------------------------------------------------------
def test_batch_memory_stays_bounded():
    """k = 16, B = 48 one-instance-column proofs: the peak device memory finalize adds stays <= 16 n-vectors (one n-vector per
    proof would be >= 48)."""
    import torch
    k, curve = 16, VESTA
    sf = fields.CURVE_FIELDS[curve][1]
    m = fields.MODULUS[sf]
    n = 1 << k
    cs = make_cs()
    usable = n - (cs.blinding_factors + 1)
    fixed, advice, mapping, inst = make_witness(random.Random(16), m, n, usable)
    g = co.generate_bases(curve, 986, n)
    w, u = co.generate_bases(curve, 60, 1)[0], co.generate_bases(curve, 61, 1)[0]
    params = h.Params.from_generators(curve, k, g, None, w, u)
    pk = keygen_pk(params, cs, fixed, mapping, 12345)
    dvk = hv.keygen_vk(params, pk)
    proofs = []
    for i in range(2):
        tr = Blake2bWrite(curve)
        create_proof(params, pk, advice, inst, _rng(sf, 800 + i), tr)
        proofs.append(tr.finalize())
    del pk
    bv = hb.BatchVerifier()
    for i in range(48):
        bv.add_proof([inst], proofs[i % 2])
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    assert bv.finalize(params, dvk)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    assert growth <= 16 * n * 32, growth
    params.close()
