#!/usr/bin/env python3
"""Times Poseidon on one MI355X: one process, inputs resident, a warm-up call per shape, then the median [min, max] of --reps in
milliseconds of GPU time (HIP events around the call).

  (a) `poseidon.hash` of 2^20 pairs (ConstantLength<2>: one permutation each)
  (b) `poseidon.trace` of 2^10, 2^14 and 28 339 permutations (28 339 x 37 rows fill a k = 20 circuit)
  (c) a k = 20 circuit filled by `Pow5Chip.permute_many`: synthesis (the witness pass alone), `keygen_pk` and `create_proof`, host clock
  (d) beside them, the per-permutation time of the Python restatement `oracle.pasta.poseidon_permute` on this box's host, same run

No thresholds: nobody had measured any of this.  Writes profiles/poseidon_k20.txt (or --out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-proof", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poseidon_k20.txt"))
    args = ap.parse_args()
    import torch
    import halo2_amd as h
    from circuit_api import make_rng
    from halo2_amd import circuit as front
    from halo2_amd import fields, poseidon, poseidon_spec
    from halo2_amd.circuit import Circuit
    from halo2_amd.gadgets.poseidon import Pow5Chip
    from halo2_amd.transcript import Blake2bWrite
    from halo2_amd.verifier import verify_proof
    from oracle import pasta as o
    field, dev = h.FP, fields.current_device()
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)

    def uniform(*shape):                                               # below 2^254 < p: valid Montgomery representations
        out = torch.randint(-(1 << 63), (1 << 63) - 1, shape + (4,), dtype=torch.int64, device=dev, generator=gen)
        out[..., 3] &= (1 << 62) - 1
        return out

    def gpu_ms(fn):
        fn()                                                           # warm-up
        times = []
        for _ in range(args.reps):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            end.record()
            end.synchronize()
            times.append(start.elapsed_time(end))
        return [round(statistics.median(times), 3), round(min(times), 3), round(max(times), 3)]

    res = {"k": args.k, "reps": args.reps}
    pairs = uniform(1 << 20, 2)
    res["a_hash_2^20_pairs_ms"] = gpu_ms(lambda: poseidon.hash(pairs, field))
    res["a_ns_per_permutation"] = round(1e6 * res["a_hash_2^20_pairs_ms"][0] / (1 << 20), 2)
    fill = ((1 << args.k) - 6) // poseidon_spec.ROWS                   # 28 339 at k = 20
    for count in (1 << 10, 1 << 14, fill):
        states = uniform(count, 3)
        ms = gpu_ms(lambda: poseidon.trace(states, field))
        res[f"b_trace_{count}_ms"] = ms
        res[f"b_trace_{count}_ns_per_permutation"] = round(1e6 * ms[0] / count, 2)
        res[f"b_trace_{count}_store_GBps"] = round(count * 4 * poseidon_spec.ROWS * 32 / (ms[0] * 1e-3) / 1e9, 1)
    # (d) the restatement on the host
    rcs, mds, _ = poseidon_spec.constants(field)
    rng = o.SplitMix64(5)
    host_states = [[rng.field(o.P) for _ in range(3)] for _ in range(200)]
    t0 = time.perf_counter()
    for s in host_states:
        o.poseidon_permute(s, mds, rcs, o.P)
    res["d_host_restatement_us_per_permutation"] = round(1e6 * (time.perf_counter() - t0) / len(host_states), 1)

    # (c) the circuit
    if not args.skip_proof:
        class Filled(Circuit):
            def __init__(self, states=None):
                self.states = states

            def without_witnesses(self):
                return Filled()

            def configure(self, meta):
                state = [meta.advice_column() for _ in range(3)]
                sbox = meta.advice_column()
                rc_a = [meta.fixed_column() for _ in range(3)]
                rc_b = [meta.fixed_column() for _ in range(3)]
                return Pow5Chip.configure(meta, state, sbox, rc_a, rc_b)

            def synthesize(self, config, layouter):
                Pow5Chip(config).permute_many(layouter, fill, self.states)
        circuit = Filled(uniform(fill, 3))
        sync = torch.cuda.synchronize

        def clock(fn):
            sync()
            t0 = time.perf_counter()
            out = fn()
            sync()
            return round(1e3 * (time.perf_counter() - t0), 1), out
        params = h.Params.new(h.VESTA, args.k)
        clock(lambda: front.synthesize(circuit, args.k, field, fixed=False, advice=True, instances=[]))       # warm-up
        res["c_synthesis_ms"] = clock(lambda: front.synthesize(circuit, args.k, field, fixed=False, advice=True, instances=[]))[0]
        res["c_keygen_pk_ms"], pk = clock(lambda: h.keygen_pk(params, circuit))
        rng_ = make_rng()

        def prove():
            tr = Blake2bWrite(h.VESTA)
            h.create_proof(params, pk, [circuit], [[]], rng_, tr)
            return tr.finalize()
        res["c_create_proof_first_ms"], proof = clock(prove)
        res["c_create_proof_ms"], proof = clock(prove)
        res["c_verifies"] = bool(verify_proof(params, pk.vk, [], proof))
        res["c_permutations"], res["c_rows"] = fill, fill * poseidon_spec.ROWS
        params.close()
    lines = [f"Poseidon P128Pow5T3 over Fp on one MI355X, one process; a warm-up call per shape, then median [min, max] of {args.reps} in",
             "milliseconds of GPU time (events around the call)", "",
             f"(a) poseidon.hash, 2^20 pairs                      {res['a_hash_2^20_pairs_ms']}   {res['a_ns_per_permutation']} ns per permutation"]
    for count in (1 << 10, 1 << 14, fill):
        lines.append(f"(b) poseidon.trace, {count:>6} permutations          {res[f'b_trace_{count}_ms']}   "
                     f"{res[f'b_trace_{count}_ns_per_permutation']} ns per permutation, {res[f'b_trace_{count}_store_GBps']} GB/s stored")
    if not args.skip_proof:
        lines += [f"(c) k = {args.k} circuit of {fill} permutations ({fill * poseidon_spec.ROWS} rows) through permute_many, host clock, ms; proof verifies: {res['c_verifies']}",
                  f"    synthesis, witness pass (trace + assignment)    {res['c_synthesis_ms']}",
                  f"    keygen_pk                                       {res['c_keygen_pk_ms']}",
                  f"    create_proof, first / second                    {res['c_create_proof_first_ms']} / {res['c_create_proof_ms']}"]
    lines += [f"(d) oracle.pasta.poseidon_permute on this host      {res['d_host_restatement_us_per_permutation']} us per permutation (Python integers, one core)",
              "", json.dumps(res)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
