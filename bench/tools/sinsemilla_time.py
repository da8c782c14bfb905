#!/usr/bin/env python3
"""Times Sinsemilla on one MI355X: one process, inputs resident, a warm-up call per shape, then the median [min, max] of --reps in
milliseconds of GPU time (HIP events around the call).

  (a) `HashDomain.hash_to_point` of 2^16 and 2^20 messages of 52 words (the MerkleCRH length), with the table gathered from global
      memory (the product) and, in a child process on the laboratory build, with the table copied into LDS (H2_SINSEMILLA_LDS=1)
  (b) `sinsemilla.trace` of 1 024 and 2^15 messages of the structure [25, 25, 2]
  (c) `sinsemilla.merkle_root` of 2^16 leaves
  (d) the k = 11 Merkle circuit of examples/sinsemilla_merkle.py: `keygen_pk` and `create_proof`, host clock
  (e) beside them, per hash of 52 words on this box's host: the Python restatement of tests/sinsemilla_cases.py and the C oracle's
      naive multiexp (`oracle.c_oracle.msm_naive`) of the hash written as 53 terms, same run

No thresholds: nobody had measured any of this.  Writes profiles/sinsemilla.txt (or --out)."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
AB_LIB = os.path.join(ROOT, "build", "ab", "libhalo2_mi355x_ab.so")


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


def hash_times(reps):
    """(a) for the library this process loaded"""
    import torch
    from halo2_amd import fields, sinsemilla
    dev = fields.current_device()
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    dom = sinsemilla.HashDomain(sinsemilla.MERKLE_CRH_DOMAIN)
    sinsemilla.generator_table()
    out = {}
    for log_n in (16, 20):
        words = torch.randint(0, 1024, (1 << log_n, 52), dtype=torch.int16, device=dev, generator=gen)
        out[f"hash_2^{log_n}_ms"] = gpu_ms(lambda: dom.hash_to_point(words, with_status=True), reps)
        if log_n == 16:                                                    # the two placements must agree on every point
            points, status = dom.hash_to_point(words, with_status=True)
            out["sha256_of_2^16_points"] = hashlib.sha256(points.cpu().numpy().tobytes() + status.cpu().numpy().tobytes()).hexdigest()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--hash-only", action="store_true", help="print (a) as JSON and stop: what the child process on the laboratory build runs")
    ap.add_argument("--skip-proof", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sinsemilla.txt"))
    args = ap.parse_args()
    if args.hash_only:
        print(json.dumps(hash_times(args.reps)))
        return
    import torch
    import halo2_amd as h
    from halo2_amd import fields, sinsemilla
    dev = fields.current_device()
    gen = torch.Generator(device=dev)
    gen.manual_seed(4)

    def uniform(*shape):                                                   # below 2^254 < p: valid Montgomery representations
        out = torch.randint(-(1 << 63), (1 << 63) - 1, shape + (4,), dtype=torch.int64, device=dev, generator=gen)
        out[..., 3] &= (1 << 62) - 1
        return out
    res = {"reps": args.reps}
    res["a_global"] = hash_times(args.reps)
    res["a_lds"] = None
    if os.path.exists(AB_LIB):
        env = dict(os.environ, H2_LIB_PATH=AB_LIB, H2_SINSEMILLA_LDS="1")
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--hash-only", "--reps", str(args.reps)], env=env,
                               capture_output=True, text=True, timeout=300)
        if child.returncode == 0:
            res["a_lds"] = json.loads(child.stdout.strip().splitlines()[-1])
        else:
            res["a_lds_error"] = child.stderr[-400:]
    q = sinsemilla.q_point(sinsemilla.MERKLE_CRH_DOMAIN)
    nw = [25, 25, 2]
    for count in (1 << 10, 1 << 15):
        pieces = uniform(count, 3)
        pieces[..., 3] = 0                                                 # canonical values under 2^192 (the kernel reads the low words)
        ms = gpu_ms(lambda: sinsemilla.trace(pieces, nw, q, with_status=True), args.reps)
        res[f"b_trace_{count}_ms"] = ms
        res[f"b_trace_{count}_us_per_hash"] = round(1e3 * ms[0] / count, 3)
    leaves = uniform(1 << 16)
    dom = sinsemilla.HashDomain(sinsemilla.MERKLE_CRH_DOMAIN)
    res["c_merkle_root_2^16_ms"] = gpu_ms(lambda: sinsemilla.merkle_root(leaves, dom), args.reps)

    # (e) the host
    import sinsemilla_cases as sc
    from oracle import c_oracle as co
    sc.table()
    msgs = [sc.merkle_words(0, 12345 + i, 67890 + i) for i in range(20)]
    t0 = time.perf_counter()
    for m in msgs:
        sc.hash_to_point(q, m)
    res["e_python_restatement_us_per_hash"] = round(1e6 * (time.perf_counter() - t0) / len(msgs), 1)
    # the C oracle has no single point addition: a hash of n words is the multiexp 2^n Q + sum 2^(n-1-i) S(m_i) of its naive routine
    # (complete arithmetic: the same point wherever the hash has a value)
    def as_msm(m):
        n = len(m)
        scalars = co.to_mont(h.FQ, co.ints_to_limbs([1 << n] + [1 << (n - 1 - i) for i in range(n)]))
        return scalars, co.points_to_mont(h.PALLAS, [q] + [sc.table()[w] for w in m])
    problems = [as_msm(m) for m in msgs]
    t0 = time.perf_counter()
    sums = [co.msm_naive(h.PALLAS, s_, b_) for s_, b_ in problems]
    res["e_c_oracle_us_per_hash"] = round(1e6 * (time.perf_counter() - t0) / len(msgs), 1)
    assert co.jac_to_affine_ints(h.PALLAS, sums[0]) == sc.hash_to_point(q, msgs[0])

    # (d) the circuit
    if not args.skip_proof:
        import random
        from circuit_api import make_rng
        from halo2_amd.transcript import Blake2bWrite
        from halo2_amd.verifier import verify_proof
        from sinsemilla_merkle import MerkleCircuit
        p = fields.MODULUS[h.FP]
        rng = random.Random(1)
        circuit = MerkleCircuit(rng.randrange(p), 0xA5A55A5A, [rng.randrange(p) for _ in range(32)])
        sync = torch.cuda.synchronize

        def clock(fn):
            sync()
            t0 = time.perf_counter()
            out = fn()
            sync()
            return round(1e3 * (time.perf_counter() - t0), 1), out
        params = h.Params.new(h.VESTA, 11)
        clock(lambda: h.keygen_pk(params, circuit))                        # warm-up
        res["d_keygen_pk_ms"], pk = clock(lambda: h.keygen_pk(params, circuit))
        rng_ = make_rng()

        def prove():
            tr = Blake2bWrite(h.VESTA)
            h.create_proof(params, pk, [circuit], [[]], rng_, tr)
            return tr.finalize()
        res["d_create_proof_first_ms"], proof = clock(prove)
        res["d_create_proof_ms"], proof = clock(prove)
        res["d_verifies"], res["d_proof_bytes"] = bool(verify_proof(params, pk.vk, [], proof)), len(proof)
        params.close()

    g, l = res["a_global"], res["a_lds"]
    lines = [f"Sinsemilla over Pallas on one MI355X, one process; a warm-up call per shape, then median [min, max] of {args.reps} in",
             "milliseconds of GPU time (events around the call)", ""]
    for log_n in (16, 20):
        ms = g[f"hash_2^{log_n}_ms"]
        lines.append(f"(a) hash_to_point, 2^{log_n} messages of 52 words, table gathered from global memory   {ms}   "
                     f"{round(1e6 * ms[0] / (1 << log_n), 1)} ns per hash")
        lines.append(f"    the same with the table copied into LDS by every workgroup (laboratory arm)     "
                     f"{l[f'hash_2^{log_n}_ms'] if l else 'not measured: ' + res.get('a_lds_error', 'no laboratory build')}")
    if l:
        same = l["sha256_of_2^16_points"] == g["sha256_of_2^16_points"]
        lines.append(f"    both placements give the same 2^16 points and statuses: {same}")
        kept = "not slower than the LDS copy at 2^20" if g["hash_2^20_ms"][0] <= l["hash_2^20_ms"][0] else "the LDS copy is faster in this run"
        lines.append(f"    table placement kept in the product: global gather ({kept})")
    for count in (1 << 10, 1 << 15):
        lines.append(f"(b) trace, {count:>6} messages of [25, 25, 2] words (53 rows each)    {res[f'b_trace_{count}_ms']}   "
                     f"{res[f'b_trace_{count}_us_per_hash']} us per hash")
    lines.append(f"(c) merkle_root of 2^16 leaves (16 launches)                      {res['c_merkle_root_2^16_ms']}")
    if not args.skip_proof:
        lines += [f"(d) the k = 11 Merkle circuit (32 layers), host clock, ms; proof of {res['d_proof_bytes']} bytes verifies: {res['d_verifies']}",
                  f"    keygen_pk                                       {res['d_keygen_pk_ms']}",
                  f"    create_proof, first / second                    {res['d_create_proof_first_ms']} / {res['d_create_proof_ms']}"]
    lines += [f"(e) on this host, one core, per hash of 52 words: Python restatement {res['e_python_restatement_us_per_hash']} us; "
              f"C oracle (its naive multiexp of the 53 terms) {res['e_c_oracle_us_per_hash']} us", "", json.dumps(res)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
