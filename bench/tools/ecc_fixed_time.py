#!/usr/bin/env python3
"""Times fixed-base scalar multiplication on one MI355X: one process, inputs resident, a warm-up call per shape, then the median
[min, max] of --reps in milliseconds of GPU time (HIP events around the call); host clock where it says so.

  (a) the table build of the Pallas generator at 85 windows (`ecc.FixedBase`), host clock around the call, which returns with the stream
      idle: the whole build; a build cut short by z_limit = 1 after the points, the coefficients and one search round of one candidate;
      the difference, which is the search with the 680 roots (the roots are not timed apart)
  (b) `ecc.mul_fixed` of 2^20 scalars, beside `ecc.mul` of 2^20 pairs on the same base in the same run
  (c) `ecc.mul_fixed_trace` of 1 024 and 2^15 scalars
  (d) a k = 16 circuit of 700 multiplications through `mul_fixed_many`: the witness synthesis, `keygen_pk` and `create_proof`, host clock
  (e) beside them on this box's host, one core: `oracle.pasta.ec_mul` and the C oracle per product; the Python search
      (tests/ecc_fixed_cases.py) run in full over window 42 of the generator, whose z = 1684 is the smallest, and its rate in candidates
      per second over the first 400 candidates of every one of the 85 windows, from which the whole search is estimated, not run

No thresholds: nobody had measured any of this.  Writes profiles/ecc_fixed.txt (or --out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from ecc_time import gpu_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-proof", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ecc_fixed.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import halo2_amd as h
    from halo2_amd import ecc, fields
    from halo2_amd._lib import NotFound
    dev = fields.current_device()
    gen = torch.Generator(device=dev)
    gen.manual_seed(6)
    sync = torch.cuda.synchronize
    p, q = fields.MODULUS[h.FP], fields.MODULUS[h.FQ]
    generator = fields.to_limbs([p - 1, 2], h.FP).reshape(8)

    def uniform(n, top_bits):                                              # n values of 192 + top_bits bits
        out = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 4), dtype=torch.int64, device=dev, generator=gen)
        out[:, 3] &= (1 << top_bits) - 1
        return out

    def clock(fn):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        return round(1e3 * (time.perf_counter() - t0), 2), out

    def cut_short():
        try:
            ecc.FixedBase(generator, 85, z_limit=1)
        except NotFound:
            pass
    res = {"reps": args.reps}
    # (a)
    clock(lambda: ecc.FixedBase(generator, 85))                              # warm-up
    builds = [clock(lambda: ecc.FixedBase(generator, 85)) for _ in range(3)]
    base = builds[0][1]
    cuts = [clock(cut_short)[0] for _ in range(4)][1:]
    res["a_build_ms"], res["a_points_coefficients_ms"] = sorted(b[0] for b in builds), sorted(cuts)
    res["a_search_roots_ms"] = round(statistics.median(res["a_build_ms"]) - statistics.median(cuts), 2)
    res["a_largest_z"], res["a_candidates"] = max(base.z()), sum(z + 1 for z in base.z())
    # (b)
    n = 1 << 20
    scalars = uniform(n, 63)
    res["b_mul_fixed_ms"] = gpu_ms(lambda: ecc.mul_fixed(base, scalars), args.reps)
    bases = torch.from_numpy(generator.view(np.int64)).to(dev).reshape(1, 8).repeat(n, 1)
    res["b_mul_variable_ms"] = gpu_ms(lambda: ecc.mul(bases, scalars, with_status=True), args.reps)
    res["b_ratio_variable_over_fixed"] = round(res["b_mul_variable_ms"][0] / res["b_mul_fixed_ms"][0], 2)
    res["b_same_points"] = bool((ecc.mul_fixed(base, scalars[:4096]) == ecc.mul(bases[:4096], scalars[:4096])).all())
    del bases
    # (c)
    for count in (1 << 10, 1 << 15):
        ks = uniform(count, 63)
        ms = gpu_ms(lambda: ecc.mul_fixed_trace(base, ks), args.reps)
        res[f"c_trace_{count}_ms"], res[f"c_trace_{count}_us_per_mul"] = ms, round(1e3 * ms[0] / count, 3)
    # (e) the host
    from oracle import c_oracle as co
    from oracle import pasta as o
    import ecc_fixed_cases as fx
    ks = [int.from_bytes(os.urandom(32), "little") % q for _ in range(8)]
    t0 = time.perf_counter()
    want = [o.ec_mul(k, fx.GENERATOR, p) for k in ks]
    res["e_python_ec_mul_us_per_product"] = round(1e6 * (time.perf_counter() - t0) / len(ks), 1)
    problems = [(co.to_mont(h.FQ, co.ints_to_limbs([k])), co.points_to_mont(h.PALLAS, [fx.GENERATOR])) for k in ks]
    t0 = time.perf_counter()
    sums = [co.msm_naive(h.PALLAS, s_, b_) for s_, b_ in problems]
    res["e_c_oracle_us_per_product"] = round(1e6 * (time.perf_counter() - t0) / len(ks), 1)
    assert co.jac_to_affine_ints(h.PALLAS, sums[0]) == want[0]
    table = base.window_table()
    assert fx.find_z([pt[1] for pt in table[42]]) == base.z()[42] == 1684      # the one window the host finishes quickly, in full
    sample = 400                                                             # then the first candidates of EVERY window, for the rate
    t0 = time.perf_counter()
    for row in table:
        ys = [pt[1] for pt in row]
        for z in range(sample):
            fx.z_is_valid(z, ys)
    res["e_python_search_sampled"] = sample * len(table)
    res["e_python_search_candidates_per_s"] = round(sample * len(table) / (time.perf_counter() - t0))
    res["e_python_search_estimate_s"] = round(res["a_candidates"] / res["e_python_search_candidates_per_s"])
    # (d) the circuit
    if not args.skip_proof:
        from circuit_api import make_rng
        from ecc_fixed_mul import EccFixedMulCircuit
        from halo2_amd import circuit as front
        from halo2_amd.gadgets.ecc import FixedBaseTables
        from halo2_amd.transcript import Blake2bWrite
        from halo2_amd.verifier import verify_proof
        k, count = 16, 700
        ks = [int.from_bytes(os.urandom(32), "little") % q for _ in range(count)]
        products = fields.from_limbs(ecc.mul_fixed(base, fields.to_limbs(ks, h.FQ, montgomery=False)).reshape(-1, 4), h.FP)
        circuit = EccFixedMulCircuit(ks, FixedBaseTables.of(base))
        clock(lambda: front.synthesize(circuit, k, h.FP, fixed=False, advice=True, instances=[products]))      # warm-up
        res["d_witness_synthesis_ms"], _ = clock(lambda: front.synthesize(circuit, k, h.FP, fixed=False, advice=True, instances=[products]))
        params = h.Params.new(h.VESTA, k)
        clock(lambda: h.keygen_pk(params, circuit))                        # warm-up
        res["d_keygen_pk_ms"], pk = clock(lambda: h.keygen_pk(params, circuit))
        rng_ = make_rng()

        def prove():
            tr = Blake2bWrite(h.VESTA)
            h.create_proof(params, pk, [circuit], [[products]], rng_, tr)
            return tr.finalize()
        res["d_create_proof_first_ms"], proof = clock(prove)
        res["d_create_proof_ms"], proof = clock(prove)
        res["d_verifies"], res["d_proof_bytes"], res["d_count"] = bool(verify_proof(params, pk.vk, [products], proof)), len(proof), count
        params.close()

    lines = ["Fixed-base scalar multiplication over Pallas on one MI355X, one process; a warm-up call per shape, then median [min, max]",
             f"of {args.reps} in milliseconds of GPU time (events around the call); host clock where it says so", "",
             f"(a) tables of the generator, 85 windows, host clock, ms, three builds      {res['a_build_ms']}",
             f"    points, coefficients and one search launch (z_limit = 1), three runs  {res['a_points_coefficients_ms']}",
             f"    the search and the 680 roots (difference of the medians)              {res['a_search_roots_ms']}",
             f"    candidates up to each window's z: {res['a_candidates']}; the largest z: {res['a_largest_z']}",
             f"(b) mul_fixed, 2^20 scalars of 255 bits                  {res['b_mul_fixed_ms']}",
             f"    ecc.mul, the same scalars on the same base           {res['b_mul_variable_ms']}   variable / fixed = "
             f"{res['b_ratio_variable_over_fixed']}; same points: {res['b_same_points']}"]
    for count in (1 << 10, 1 << 15):
        lines.append(f"(c) mul_fixed_trace, {count:>6} scalars (85 rows and 11 aux each)   {res[f'c_trace_{count}_ms']}   "
                     f"{res[f'c_trace_{count}_us_per_mul']} us per multiplication")
    if not args.skip_proof:
        lines += [f"(d) the k = 16 circuit of {res['d_count']} multiplications through mul_fixed_many, host clock, ms; proof of "
                  f"{res['d_proof_bytes']} bytes verifies: {res['d_verifies']}",
                  f"    witness synthesis                               {res['d_witness_synthesis_ms']}",
                  f"    keygen_pk                                       {res['d_keygen_pk_ms']}",
                  f"    create_proof, first / second                    {res['d_create_proof_first_ms']} / {res['d_create_proof_ms']}"]
    lines += [f"(e) on this host, one core: oracle.pasta.ec_mul {res['e_python_ec_mul_us_per_product']} us per product; C oracle (its naive "
              f"multiexp of the one term) {res['e_c_oracle_us_per_product']} us",
              f"    the Python search over the first 400 candidates of each of the 85 windows ({res['e_python_search_sampled']} in all): "
              f"{res['e_python_search_candidates_per_s']} candidates per second,",
              f"    an ESTIMATE of {res['e_python_search_estimate_s']} s for the candidates of (a) at that rate; the whole search was not run",
              "", json.dumps(res)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
