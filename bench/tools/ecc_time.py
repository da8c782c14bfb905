#!/usr/bin/env python3
"""Times variable-base scalar multiplication on one MI355X: one process, inputs resident, a warm-up call per shape, then the median
[min, max] of --reps in milliseconds of GPU time (HIP events around the call).

  (a) `ecc.mul` of 2^16 and 2^20 (base, scalar) pairs, random 255-bit scalars
  (b) `ecc.mul_trace` of 1 024 and 2^15 pairs: both passes over the incomplete range, the batched inversion between them and the kernel
      of the 8 complete additions with its inversion per addition on the lane (--trace-only stops here: the run a kernel trace is
      taken of, to split (b) by kernel)
  (c) a k = 16 circuit of 400 multiplications through `mul_many`: the witness synthesis, `keygen_pk` and `create_proof`, host clock
  (d) beside them, per product on this box's host: `oracle.pasta.ec_mul` and the C oracle's naive multiexp of one term, same run

No thresholds: nobody had measured any of this.  Writes profiles/ecc.txt (or --out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))


def gpu_ms(fn, reps):
    import torch
    fn()                                                                   # warm-up
    times = []
    for _ in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    return [round(statistics.median(times), 3), round(min(times), 3), round(max(times), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--skip-proof", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ecc.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import halo2_amd as h
    from halo2_amd import ecc, fields
    dev = fields.current_device()
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)

    def uniform(n, top_bits):                                              # n values of 192 + top_bits bits
        out = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 4), dtype=torch.int64, device=dev, generator=gen)
        out[:, 3] &= (1 << top_bits) - 1
        return out
    g = torch.from_numpy(np.asarray(h.hash_to_curve(h.PALLAS, "halo2_amd:ecc_time", [b"base"])).view(np.int64)).to(dev).reshape(1, 8)

    def points(n):                                                         # n points of the curve: random multiples of one
        return ecc.mul(g.repeat(n, 1), uniform(n, 62))
    res = {"reps": args.reps}
    if not args.trace_only:
        for log_n in (16, 20):
            bases, scalars = points(1 << log_n), uniform(1 << log_n, 63)
            ms = gpu_ms(lambda: ecc.mul(bases, scalars, with_status=True), args.reps)
            res[f"a_mul_2^{log_n}_ms"], res[f"a_mul_2^{log_n}_us_per_product"] = ms, round(1e3 * ms[0] / (1 << log_n), 3)
    for count in (1 << 10, 1 << 15):
        bases, alphas = points(count), uniform(count, 62)                  # below 2^254 < p: valid Montgomery representations
        ms = gpu_ms(lambda: ecc.mul_trace(bases, alphas, with_status=True), args.reps)
        res[f"b_trace_{count}_ms"], res[f"b_trace_{count}_us_per_mul"] = ms, round(1e3 * ms[0] / count, 3)
        _, _, status = ecc.mul_trace(bases, alphas, with_status=True)
        res[f"b_trace_{count}_flagged"] = int(status.sum())
    if args.trace_only:
        print(json.dumps(res))
        return

    # (d) the host
    from oracle import c_oracle as co
    from oracle import pasta as o
    p, q = fields.MODULUS[h.FP], fields.MODULUS[h.FQ]
    pts = fields.from_limbs(points(8).cpu().numpy().view(np.uint64).reshape(-1, 4), h.FP)
    pts = [(pts[2 * i], pts[2 * i + 1]) for i in range(8)]
    ks = [int.from_bytes(os.urandom(32), "little") % q for _ in pts]
    t0 = time.perf_counter()
    want = [o.ec_mul(k, pt, p) for k, pt in zip(ks, pts)]
    res["d_python_ec_mul_us_per_product"] = round(1e6 * (time.perf_counter() - t0) / len(pts), 1)
    problems = [(co.to_mont(h.FQ, co.ints_to_limbs([k])), co.points_to_mont(h.PALLAS, [pt])) for k, pt in zip(ks, pts)]
    t0 = time.perf_counter()
    sums = [co.msm_naive(h.PALLAS, s_, b_) for s_, b_ in problems]
    res["d_c_oracle_us_per_product"] = round(1e6 * (time.perf_counter() - t0) / len(pts), 1)
    assert co.jac_to_affine_ints(h.PALLAS, sums[0]) == want[0]

    # (c) the circuit
    if not args.skip_proof:
        from circuit_api import make_rng
        from ecc_mul import EccMulCircuit, random_pairs
        from halo2_amd import circuit as front
        from halo2_amd.transcript import Blake2bWrite
        from halo2_amd.verifier import verify_proof
        k, count = 16, 400
        pairs = random_pairs(count, 2)
        bases = fields.to_limbs([c for b, _ in pairs for c in b], h.FP).reshape(-1, 8)
        products = fields.from_limbs(ecc.mul(bases, fields.to_limbs([a for _, a in pairs], h.FP, montgomery=False)).reshape(-1, 4), h.FP)
        circuit = EccMulCircuit(pairs)
        sync = torch.cuda.synchronize

        def clock(fn):
            sync()
            t0 = time.perf_counter()
            out = fn()
            sync()
            return round(1e3 * (time.perf_counter() - t0), 1), out
        clock(lambda: front.synthesize(circuit, k, h.FP, fixed=False, advice=True, instances=[products]))      # warm-up
        res["c_witness_synthesis_ms"], _ = clock(lambda: front.synthesize(circuit, k, h.FP, fixed=False, advice=True, instances=[products]))
        params = h.Params.new(h.VESTA, k)
        clock(lambda: h.keygen_pk(params, circuit))                        # warm-up
        res["c_keygen_pk_ms"], pk = clock(lambda: h.keygen_pk(params, circuit))
        rng_ = make_rng()

        def prove():
            tr = Blake2bWrite(h.VESTA)
            h.create_proof(params, pk, [circuit], [[products]], rng_, tr)
            return tr.finalize()
        res["c_create_proof_first_ms"], proof = clock(prove)
        res["c_create_proof_ms"], proof = clock(prove)
        res["c_verifies"], res["c_proof_bytes"], res["c_count"] = bool(verify_proof(params, pk.vk, [products], proof)), len(proof), count
        params.close()

    lines = [f"Variable-base scalar multiplication over Pallas on one MI355X, one process; a warm-up call per shape, then median [min, max]",
             f"of {args.reps} in milliseconds of GPU time (events around the call)", ""]
    for log_n in (16, 20):
        lines.append(f"(a) mul, 2^{log_n} pairs, random 255-bit scalars          {res[f'a_mul_2^{log_n}_ms']}   "
                     f"{res[f'a_mul_2^{log_n}_us_per_product']} us per product")
    for count in (1 << 10, 1 << 15):
        lines.append(f"(b) mul_trace, {count:>6} pairs (137 rows and 16 aux each)   {res[f'b_trace_{count}_ms']}   "
                     f"{res[f'b_trace_{count}_us_per_mul']} us per multiplication; flagged: {res[f'b_trace_{count}_flagged']}")
    if not args.skip_proof:
        lines += [f"(c) the k = 16 circuit of {res['c_count']} multiplications through mul_many, host clock, ms; proof of {res['c_proof_bytes']} "
                  f"bytes verifies: {res['c_verifies']}",
                  f"    witness synthesis                               {res['c_witness_synthesis_ms']}",
                  f"    keygen_pk                                       {res['c_keygen_pk_ms']}",
                  f"    create_proof, first / second                    {res['c_create_proof_first_ms']} / {res['c_create_proof_ms']}"]
    lines += [f"(d) on this host, one core, per product: oracle.pasta.ec_mul {res['d_python_ec_mul_us_per_product']} us; "
              f"C oracle (its naive multiexp of the one term) {res['d_c_oracle_us_per_product']} us", "", json.dumps(res)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
