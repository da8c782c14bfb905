#!/usr/bin/env python3
"""Times halo2_amd.dev.MockProver.verify at k = 20 against the proof it guards: one process, one GPU, columns resident, a warm-up
call, then the median of 10 for
  * verify() of a satisfied witness of tests/plonk_circuits.make_cs("full"),
  * verify() of the same witness with ~100 planted faults (default max_failures),
  * create_proof of the same circuit -- the yardstick,
and the split of a verify() into its three checks (each followed by a synchronisation, so their sum exceeds the whole).
Writes profiles/mock_prover_k20.txt (or --out)."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mock_prover_k20.txt"))
    args = ap.parse_args()
    import torch
    import halo2_amd as h
    from halo2_amd import fields
    from halo2_amd.dev import MockProver
    from halo2_amd.plonk import create_proof, keygen_pk
    from halo2_amd.transcript import Blake2bWrite
    from oracle import c_oracle as co          # input generation only
    from plonk_circuits import make_cs, make_witness
    k, curve = args.k, h.VESTA
    n = 1 << k
    sf = fields.CURVE_FIELDS[curve][1]
    m = fields.MODULUS[sf]
    cs = make_cs("full")
    usable = n - (cs.blinding_factors + 1)
    fixed, advice, mapping, instance = make_witness(random.Random(7), m, n, usable)
    up = lambda col: torch.from_numpy(fields.to_limbs(col, sf, True).view(np.int64)).cuda()
    fixed_dev, advice_dev = [up(c) for c in fixed], [up(c) for c in advice]
    flat = np.array([[c2 * n + r2 for c2, r2 in col] for col in mapping], dtype=np.int64)
    rnd = random.Random(1)
    broken = [list(c) for c in advice]
    for i, r in enumerate(rnd.sample(range(1, usable), 100)):      # ~100 faults: outputs, copied cells and looked-up values
        col = i % 3
        broken[col][r] = (broken[col][r] + 1) % m
    broken_dev = [up(c) for c in broken]

    def median(fn):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return statistics.median(times), min(times), max(times)

    good = MockProver.run(k, cs, fixed_dev, advice_dev, instance, flat, sf)
    bad = MockProver.run(k, cs, fixed_dev, broken_dev, instance, flat, sf)
    res = {"k": k, "circuit": "make_cs('full')", "reps": args.reps}
    assert good.verify() == []
    res["verify_satisfied_ms"] = [round(1e3 * t, 3) for t in median(good.verify)]
    found = bad.verify()
    res["planted_faults"] = 100
    res["failures_reported"] = len(found)
    res["failure_counts"] = bad.failure_counts
    res["verify_faulty_ms"] = [round(1e3 * t, 3) for t in median(bad.verify)]
    split = {}
    n_gates = len(cs.gates)
    split["gates"] = median(lambda: good._check_expressions(good._gates, n_gates, False))
    split["lookups"] = median(lambda: [good._check_lookup(w, linked) for w, linked in good._lookups])
    split["permutation"] = median(good._check_permutation)
    res["split_satisfied_ms"] = {name: round(1e3 * t[0], 3) for name, t in split.items()}

    g = co.generate_bases(curve, 970 + k, n)
    w, u = co.generate_bases(curve, 60, 1)[0], co.generate_bases(curve, 61, 1)[0]
    params = h.Params.from_generators(curve, k, g, None, w, u)
    pk = keygen_pk(params, cs, fixed_dev, flat, 99)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    host = np.random.Generator(np.random.PCG64(5))

    def rng(count):
        if count >= 4096:
            out = torch.randint(-(1 << 63), (1 << 63) - 1, (count, 4), dtype=torch.int64, device="cuda", generator=gen)
            out[:, 3] &= (1 << 62) - 1
            return out
        out = host.integers(0, 1 << 64, size=(count, 4), dtype=np.uint64)
        out[:, 3] &= np.uint64((1 << 62) - 1)
        return out

    def prove():
        tr = Blake2bWrite(curve)
        create_proof(params, pk, advice_dev, instance, rng, tr)
        tr.finalize()
    res["create_proof_ms"] = [round(1e3 * t, 3) for t in median(prove)]
    res["verify_satisfied_over_create_proof"] = round(res["verify_satisfied_ms"][0] / res["create_proof_ms"][0], 3)
    params.close()
    lines = [f"MockProver.verify against create_proof, k = {k}, make_cs('full'), one MI355X, one process, columns resident;",
             f"a warm-up call, then median [min, max] of {args.reps} (milliseconds, host clock around a synchronised call)", "",
             f"verify(), satisfied witness            {res['verify_satisfied_ms']}",
             f"verify(), 100 planted faults           {res['verify_faulty_ms']}   ({res['failures_reported']} failures reported: {res['failure_counts']})",
             f"create_proof, same circuit             {res['create_proof_ms']}",
             f"verify(satisfied) / create_proof       {res['verify_satisfied_over_create_proof']}", "",
             f"the three checks of a satisfied verify(), each synchronised on its own (median): {res['split_satisfied_ms']}", "",
             json.dumps(res)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
