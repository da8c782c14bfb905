#!/usr/bin/env python3
"""BatchVerifier against B single verifications on the simple-example circuit (examples/simple_example.py) at k = 20, Vesta.

Prints ONE JSON line:
  single_verify_ms        verify_proof of one proof, median over the distinct proofs (warm)
  batch[B]                finalize of B proofs (the distinct proofs repeated), median; B x single beside it and the ratio
  breakdown_B64_ms        one finalize of 64 proofs in its phases: host parsing to the claims, instance commits, combine (host merges +
                          the s-combine launch), the commit over g, the small generic multiexp (+ the point sum)
  s_combine_kernel_ms     h2_ipa_s_combine_device alone at B = 64, k = 20 by HIP events (median of 20)

    python bench/batch_verify.py [--k 20] [--batches 1,8,64] [--profile-one]

--profile-one: set up, warm up, then run ONE finalize of the largest batch between two marker launches (`poly_powers`, the last two of the
run; the verifier never launches it), for `rocprofv3 --kernel-trace --stats -d D -o batch -- python bench/batch_verify.py --profile-one`;
--by-kernel D/batch_results.db (the rocpd database rocprofv3 writes by default; a `-f csv` kernel trace works too) then lists the
kernels between the markers by name (count, total and mean time)."""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def setup(k: int, distinct: int):
    import importlib.util

    import torch

    import halo2_amd as h
    from halo2_amd import fields
    from halo2_amd.plonk import ConstraintSystem, create_proof, keygen_pk
    from halo2_amd.transcript import Blake2bWrite
    from halo2_amd.verifier import keygen_vk
    from oracle import c_oracle as co
    spec = importlib.util.spec_from_file_location("simple_example", os.path.join(ROOT, "examples", "simple_example.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    curve, n = h.VESTA, 1 << k
    sf = fields.CURVE_FIELDS[curve][1]
    m = fields.MODULUS[sf]
    pv = co.generate_bases(curve, 0x56455354, n + 2)
    params = h.Params.from_generators(curve, k, np.ascontiguousarray(pv[:n]), None, pv[n], pv[n + 1])
    cs = ConstraintSystem(                                  # examples/simple_example.py prove_and_verify
        num_fixed_columns=2, num_advice_columns=2, num_instance_columns=1,
        gates=[lambda q: q.fixed(1) * (q.advice(0) * q.advice(1) - q.advice(0, 1))],
        advice_queries=[(0, 0), (1, 0), (0, 1)], instance_queries=[(0, 0)], fixed_queries=[(0, 0), (1, 0)],
        permutation_columns=[("instance", 0), ("fixed", 0), ("advice", 0), ("advice", 1)], degree=3, blinding_factors=5)
    dev = fields.current_device()
    up = lambda col: torch.from_numpy(fields.to_limbs(col, sf, True).view(np.int64)).to(dev)
    gen = np.random.Generator(np.random.PCG64(0xBA7C4))

    def rng(count):
        out = gen.integers(0, 1 << 64, size=(count, 4), dtype=np.uint64)
        out[:, 3] &= np.uint64((1 << 62) - 1)
        return out
    pk = vk = None
    items = []
    for i in range(distinct):
        advice, fixed, mapping, c = ex.build(m, n, 2 + 3 * i, 3 + 5 * i, 7)      # the same constant: the same key for every proof
        if pk is None:
            flat = np.arange(4 * n, dtype=np.int64).reshape(4, n)
            for col in range(4):
                for r, (c2, r2) in enumerate(mapping[col][:16]):
                    flat[col][r] = c2 * n + r2
            pk = keygen_pk(params, cs, [up(col) for col in fixed], flat)
            vk = keygen_vk(params, pk)
        tr = Blake2bWrite(curve)
        create_proof(params, pk, [up(col) for col in advice], [[c]], rng, tr)
        items.append(([[c]], tr.finalize()))
    del pk
    torch.cuda.synchronize()
    return params, vk, items


def _med(f, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts) * 1e3


def by_kernel(path: str) -> str:
    """The kernels of a rocprofv3 kernel trace between the last two `poly_powers` launches, by name."""
    if path.endswith(".db"):
        import sqlite3
        with sqlite3.connect(path) as db:
            rows = [tuple(r) for r in db.execute("select name, start, end from kernels")]
    else:
        rows = [(r["Kernel_Name"], r["Start_Timestamp"], r["End_Timestamp"]) for r in csv.DictReader(open(path))]
    rows = sorted(((name, int(t0), int(t1)) for name, t0, t1 in rows), key=lambda r: r[1])
    marks = [i for i, r in enumerate(rows) if "poly_powers" in r[0]]
    inside = rows[marks[-2] + 1:marks[-1]]               # the prover launches poly_powers too: the markers are the last two
    stats = {}
    for name, t0, t1 in inside:
        st = stats.setdefault(name, [0, 0])
        st[0] += 1
        st[1] += t1 - t0
    span = (inside[-1][2] - inside[0][1]) / 1e6 if inside else 0.0
    busy = sum(v[1] for v in stats.values())
    out = [f"{len(inside)} kernel launches in one finalize; first start to last end {span:.3f} ms; kernel time {busy / 1e6:.3f} ms",
           f"{'calls':>6} {'total_ms':>9} {'mean_us':>9}  kernel"]
    for name, (cnt, ns) in sorted(stats.items(), key=lambda kv: -kv[1][1]):
        out.append(f"{cnt:>6} {ns / 1e6:>9.3f} {ns / cnt / 1e3:>9.1f}  {name[:150]}")
    return "\n".join(out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--profile-one", action="store_true")
    ap.add_argument("--by-kernel", default=None, help="a rocprofv3 kernel trace of a --profile-one run: print its by-kernel listing")
    args = ap.parse_args(argv)
    if args.by_kernel is not None:
        print(by_kernel(args.by_kernel))
        return 0
    import torch

    import halo2_amd as h
    from halo2_amd import batch as hb
    from halo2_amd import fields
    from halo2_amd.arithmetic import best_multiexp, points_sum
    from halo2_amd.verifier import verify_proof
    batches = [int(b) for b in args.batches.split(",")]
    t0 = time.perf_counter()
    params, vk, items = setup(args.k, args.distinct)
    setup_s = time.perf_counter() - t0
    sf = fields.CURVE_FIELDS[params.curve][1]

    def make(B):
        bv = hb.BatchVerifier()
        for i in range(B):
            inst, proof = items[i % len(items)]
            bv.add_proof([inst], proof)
        return bv
    assert all(verify_proof(params, vk, inst, proof) for inst, proof in items)
    assert make(max(batches)).finalize(params, vk)                      # warm-up, and the batch is accepted
    if args.profile_one:
        bv = make(max(batches))
        marker = lambda: (h.powers(fields.scalar_limbs(3, sf), 8, sf, device=fields.current_device()), torch.cuda.synchronize())
        marker()
        ok = bv.finalize(params, vk)
        torch.cuda.synchronize()
        marker()
        print(json.dumps({"profile_one_finalize": max(batches), "k": args.k, "accepted": ok}))
        params.close()
        return 0

    single = []
    for inst, proof in items * 2:
        t = time.perf_counter()
        assert verify_proof(params, vk, inst, proof)
        single.append((time.perf_counter() - t) * 1e3)
    single_ms = statistics.median(single)
    res = {}
    for B in batches:
        bv = make(B)
        ms = _med(lambda: bv.finalize(params, vk), 3 if B <= 8 else 2)
        res[str(B)] = {"finalize_ms": round(ms, 2), "B_x_verify_proof_ms": round(B * single_ms, 2), "speedup": round(B * single_ms / ms, 2),
                       "finalize_per_proof_ms": round(ms / B, 3)}

    # one finalize of 64 in its phases (each phase synchronised)
    B = 64
    bv = make(B)
    ph = {}

    def tick(name, t):
        torch.cuda.synchronize()
        ph[name] = ph.get(name, 0.0) + (time.perf_counter() - t) * 1e3
    from halo2_amd.verifier import MSM, _check_instances, _verify_guard
    t = time.perf_counter()
    for inst, _ in bv.items:
        _check_instances(params, vk, inst)
    cms = hb.commit_instances(params, vk, bv.items)
    tick("instance_commits", t)
    t = time.perf_counter()
    claims = [hb.Claim.from_guard(_verify_guard(params, vk, inst, proof, MSM(params, defer_constant=True), instance_commitments=c))
              for (inst, proof), c in zip(bv.items, cms)]
    tick("host_parsing", t)
    t = time.perf_counter()
    msm = hb.combine_claims(params, claims, hb.draw_weights(B, sf))
    tick("combine_host_merge_and_s_combine", t)
    t = time.perf_counter()
    g_part = params.commit_unblinded(msm.g_scalars).cpu().numpy().view(np.uint64)
    tick("commit_over_g", t)
    t = time.perf_counter()
    bf = fields.CURVE_FIELDS[params.curve][0]
    scal = [s for s, _ in msm.other.values()] + [msm.w_scalar, msm.u_scalar]
    bases = [fields.to_limbs([x, y], bf, True).reshape(8) for x, (_, y) in msm.other.items()] + [params.w, params.u]
    small = best_multiexp(fields.to_limbs(scal, sf, True), np.stack(bases), params.curve)
    total = points_sum(np.stack([small, g_part]), params.curve)
    tick("small_multiexp_and_sum", t)
    assert not total[8:12].any()
    breakdown = {k_: round(v, 3) for k_, v in ph.items()}
    breakdown["small_multiexp_points"] = len(scal)

    # the kernel alone: B = 64, k by HIP events
    dev = fields.current_device()
    ch = np.stack([fields.to_limbs(c.u, sf, True) for c in claims])
    coeffs = fields.to_limbs([c.neg_c for c in claims], sf, True)
    out = torch.empty((params.n, 4), dtype=torch.int64, device=dev)
    for _ in range(3):
        h.ipa_s_combine(args.k, ch, coeffs, sf, out)
    ks = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        h.ipa_s_combine(args.k, ch, coeffs, sf, out)
        e1.record()
        e1.synchronize()
        ks.append(e0.elapsed_time(e1))
    print(json.dumps({"what": "BatchVerifier.finalize vs B x verify_proof, examples/simple_example.py circuit on Vesta, one GPU, one process; "
                              f"{len(items)} distinct proofs repeated", "k": args.k, "setup_s": round(setup_s, 1),
                      "single_verify_ms": round(single_ms, 2), "batch": res, "breakdown_B64_ms": breakdown,
                      "s_combine_kernel_ms": {"B": 64, "k": args.k, "median": round(statistics.median(ks), 4), "min": round(min(ks), 4)}}))
    params.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
