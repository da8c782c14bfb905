#!/usr/bin/env python3
"""Times Sinsemilla commitments and hashing from a private point on one MI355X: one process, inputs resident, a warm-up call per
shape, then the median [min, max] of --reps in milliseconds of GPU time (HIP events around the call); host clock where it says so.

  (a) `CommitDomain.commit` of 2^20 messages of 50 words (500 bits, a note-style commitment): the fused kernel, beside the three-call
      composition `ecc.add(hash_to_point(w), ecc.mul_fixed(R, r))` on the same inputs in the same run, and each of the three calls alone
  (b) `HashDomain.hash_to_point` of 2^20 messages of 50 words with one Q per message, beside the shared Q
  (c) `sinsemilla.trace_from` of 2^15 messages of the structure [25, 25], beside `sinsemilla.trace` (one row fewer per message)
  (d) `ecc.add_trace` of 2^20 pairs
  (e) the example's circuit (examples/sinsemilla_commit.py) of --count commitments through `commit_many`: the witness synthesis,
      `keygen_pk` and `create_proof`, host clock

No thresholds: nobody had measured any of this.  Writes profiles/sinsemilla_commit.txt (or --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ecc_time import gpu_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--count", type=int, default=400)
    ap.add_argument("--skip-proof", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sinsemilla_commit.txt"))
    args = ap.parse_args()
    import torch
    import halo2_amd as h
    from halo2_amd import ecc, fields, sinsemilla
    dev = fields.current_device()
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    sync = torch.cuda.synchronize
    q = fields.MODULUS[h.FQ]

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

    res = {"reps": args.reps}
    domain = sinsemilla.CommitDomain("z.cash:Orchard-NoteCommit")
    base = domain.fixed_base
    # (a)
    n, words = 1 << 20, 50
    w = torch.randint(0, 1024, (n, words), dtype=torch.int16, device=dev, generator=gen)
    r = uniform(n, 63)
    res["a_fused_ms"] = gpu_ms(lambda: domain.commit(w, r, with_status=True), args.reps)
    res["a_composition_ms"] = gpu_ms(lambda: ecc.add(domain.M.hash_to_point(w, with_status=True)[0], ecc.mul_fixed(base, r)), args.reps)
    res["a_hash_ms"] = gpu_ms(lambda: domain.M.hash_to_point(w, with_status=True), args.reps)
    res["a_mul_fixed_ms"] = gpu_ms(lambda: ecc.mul_fixed(base, r), args.reps)
    m, b = domain.M.hash_to_point(w, with_status=True)[0], ecc.mul_fixed(base, r)
    res["a_add_ms"] = gpu_ms(lambda: ecc.add(m, b), args.reps)
    res["a_same_points"] = bool((domain.commit(w, r, with_status=True)[0] == ecc.add(m, b)).all())
    res["a_composition_over_fused"] = round(res["a_composition_ms"][0] / res["a_fused_ms"][0], 3)
    # (b)
    res["b_shared_q_ms"] = res["a_hash_ms"]
    res["b_q_per_message_ms"] = gpu_ms(lambda: domain.M.hash_to_point(w, with_status=True, Q=b), args.reps)
    del m
    # (c)
    count, nw = 1 << 15, [25, 25]
    pieces = uniform(count * 2, 58).reshape(count, 2, 4)                     # 250 bits a piece
    qs = b[:count].contiguous()
    ms = gpu_ms(lambda: sinsemilla.trace_from(pieces, nw, qs, with_status=True), args.reps)
    res["c_trace_from_ms"], res["c_trace_from_us_per_message"] = ms, round(1e3 * ms[0] / count, 3)
    ms = gpu_ms(lambda: sinsemilla.trace(pieces, nw, domain.M.Q, with_status=True), args.reps)
    res["c_trace_ms"], res["c_trace_us_per_message"] = ms, round(1e3 * ms[0] / count, 3)
    # (d)
    res["d_add_trace_ms"] = gpu_ms(lambda: ecc.add_trace(b, b.roll(1, 0)), args.reps)
    del b, w, r
    # (e)
    if not args.skip_proof:
        import random
        from circuit_api import make_rng
        from halo2_amd import circuit as front
        from halo2_amd.gadgets.sinsemilla import CommitDomains
        from halo2_amd.transcript import Blake2bWrite
        from halo2_amd.verifier import verify_proof
        from sinsemilla_commit import CommitManyCircuit, rows_needed, words_of
        rng = random.Random(3)
        messages = [rng.getrandbits(500) for _ in range(args.count)]
        scalars = [rng.randrange(q) for _ in range(args.count)]
        points = domain.commit(words_of(messages), fields.to_limbs(scalars, h.FQ, montgomery=False).reshape(-1, 4))
        commitments = fields.from_limbs(points.reshape(-1, 4), h.FP)
        k = max(11, (rows_needed(args.count) - 1).bit_length())
        circuit = CommitManyCircuit(messages, scalars, CommitDomains.of(domain))
        clock(lambda: front.synthesize(circuit, k, h.FP, fixed=False, advice=True, instances=[commitments]))      # warm-up
        res["e_witness_synthesis_ms"], _ = clock(lambda: front.synthesize(circuit, k, h.FP, fixed=False, advice=True, instances=[commitments]))
        params = h.Params.new(h.VESTA, k)
        clock(lambda: h.keygen_pk(params, circuit))                        # warm-up
        res["e_keygen_pk_ms"], pk = clock(lambda: h.keygen_pk(params, circuit))
        rng_ = make_rng()

        def prove():
            tr = Blake2bWrite(h.VESTA)
            h.create_proof(params, pk, [circuit], [[commitments]], rng_, tr)
            return tr.finalize()
        res["e_create_proof_first_ms"], proof = clock(prove)
        res["e_create_proof_ms"], proof = clock(prove)
        res["e_verifies"], res["e_proof_bytes"] = bool(verify_proof(params, pk.vk, [commitments], proof)), len(proof)
        res["e_count"], res["e_k"] = args.count, k
        params.close()

    lines = ["Sinsemilla commitments over Pallas on one MI355X, one process; a warm-up call per shape, then median [min, max]",
             f"of {args.reps} in milliseconds of GPU time (events around the call); host clock where it says so", "",
             f"(a) commit, 2^20 messages of 50 words, scalars of 255 bits: fused kernel      {res['a_fused_ms']}",
             f"    the composition add(hash_to_point, mul_fixed), three launches             {res['a_composition_ms']}   "
             f"composition / fused = {res['a_composition_over_fused']}; same points: {res['a_same_points']}",
             f"    alone: hash_to_point {res['a_hash_ms']}   mul_fixed {res['a_mul_fixed_ms']}   add {res['a_add_ms']}",
             f"(b) hash_to_point, 2^20 messages of 50 words: one Q per message {res['b_q_per_message_ms']}   shared Q {res['b_shared_q_ms']}",
             f"(c) trace_from, 32768 messages of [25, 25] (52 rows each)   {res['c_trace_from_ms']}   {res['c_trace_from_us_per_message']} us per message",
             f"    trace, the same messages from one Q (51 rows each)      {res['c_trace_ms']}   {res['c_trace_us_per_message']} us per message",
             f"(d) add_trace, 2^20 pairs (11 elements each)                {res['d_add_trace_ms']}"]
    if not args.skip_proof:
        lines += [f"(e) the k = {res['e_k']} circuit of {res['e_count']} commitments through commit_many, host clock, ms; proof of "
                  f"{res['e_proof_bytes']} bytes verifies: {res['e_verifies']}",
                  f"    witness synthesis                               {res['e_witness_synthesis_ms']}",
                  f"    keygen_pk                                       {res['e_keygen_pk_ms']}",
                  f"    create_proof, first / second                    {res['e_create_proof_first_ms']} / {res['e_create_proof_ms']}"]
    lines += ["", json.dumps(res)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
