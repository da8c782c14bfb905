#!/usr/bin/env python3
"""Times the MockProver's regions on one MI355X, on the k = 16 circuit of 400 variable-base multiplications of bench/tools/ecc_time.py
(`mul_many`: whole columns assigned as vectors, selectors enabled by arrays of rows).  One process, a warm-up per measurement, host
clock with the device synchronised, the median [min, max] of --reps in milliseconds:

  (a) witness synthesis (fixed and advice cells, selectors, copies: what `run_circuit` runs) without and with `regions=True`
  (b) the regions' check on the records of (a): `h2_cells_assigned_check` (both kernels, the copies up and the answer back) and the
      host work around it in `MockProver`, against the nested loops of tests/region_model.py (dev.rs:581-641 over Python sets) on
      the same records, once
  (c) `MockProver.run_circuit(...).verify()` without and with regions

No thresholds: nobody had measured any of this.  Writes profiles/region_check.txt (or --out)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--count", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_check.txt"))
    args = ap.parse_args()
    import torch
    import halo2_amd as h
    import region_model as rm
    from ecc_mul import EccMulCircuit, random_pairs
    from halo2_amd import circuit as front
    from halo2_amd import ecc, fields
    from halo2_amd.dev import MockProver
    k, count = args.k, args.count
    pairs = random_pairs(count, 2)
    bases = fields.to_limbs([c for b, _ in pairs for c in b], h.FP).reshape(-1, 8)
    products = fields.from_limbs(ecc.mul(bases, fields.to_limbs([a for _, a in pairs], h.FP, montgomery=False)).reshape(-1, 4), h.FP)
    circuit = EccMulCircuit(pairs)

    def clock(fn, reps=args.reps):
        fn()                                                               # warm-up
        times = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        return [round(statistics.median(times), 2), round(min(times), 2), round(max(times), 2)], out
    res = {"reps": args.reps, "k": k, "count": count}
    synth = lambda regions: front.synthesize(circuit, k, h.FP, fixed=True, advice=True, instances=[products], regions=regions)
    res["a_synthesis_ms"], _ = clock(lambda: synth(False))
    res["a_synthesis_regions_ms"], (cs, assembly, _) = clock(lambda: synth(True))
    records = assembly.regions
    res["regions"], res["ranges"] = len(records), sum(len(r.cells) for r in records)
    res["range_cells"] = sum(c for r in records for _, _, c in r.cells)
    res["events"] = sum(len(at) for r in records for at in r.enabled_selectors.values())

    prover = MockProver.run_circuit(k, circuit, [products], h.FP, regions=True)
    res["pairs"] = sum(len(part) for part in prover.region_check_inputs()[2])
    res["b_check_regions_ms"], (unassigned, n_cells, n_instance) = clock(lambda: prover._check_regions(1024))
    res["b_failures"] = [len(unassigned), n_cells, n_instance]
    from halo2_amd import dev as dev_mod
    calls = []
    entry = dev_mod.cells_assigned_check

    def timed(*a):
        t0 = time.perf_counter()
        out = entry(*a)
        calls.append(1e3 * (time.perf_counter() - t0))
        return out
    dev_mod.cells_assigned_check = timed
    for _ in range(args.reps + 1):
        del calls[:]
        prover._check_regions(1024)
    dev_mod.cells_assigned_check = entry
    res["b_entry_point_ms"] = round(sum(calls), 2)                         # the last repetition's calls (one per kind of cell that occurs)

    # the model on the same records: regions as sets of cells, gates as tuples
    t0 = time.perf_counter()
    model_regions = [{"name": r.name, "columns": {(c.kind, c.index) for c in r.columns}, "rows": r.rows, "enabled_selectors": r.enabled_selectors,
                      "cells": {((c.kind, c.index), row) for c, first, n in r.cells for row in range(first, first + n)}} for r in records]
    gates = [(g.name, [s.index for s in g.queried_selectors], [((c.kind, c.index), rot) for c, rot in g.queried_cells]) for g in prover.circuit_cs.gates]
    res["b_model_sets_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    t0 = time.perf_counter()
    errors = rm.selector_errors(1 << k, model_regions, gates, [len(products)])
    res["b_model_loops_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    res["b_model_failures"] = len(errors)
    res["b_cells_checked"] = sum(len(at) * len(g[2]) for r in records for s, at in r.enabled_selectors.items() for g in gates if s in g[1])

    run = lambda regions: MockProver.run_circuit(k, circuit, [products], h.FP, regions=regions).verify()
    res["c_run_and_verify_ms"], plain = clock(lambda: run(False))
    res["c_run_and_verify_regions_ms"], full = clock(lambda: run(True))
    res["c_failures"] = [len(plain), len(full)]

    lines = [f"MockProver regions on one MI355X: the k = {k} circuit of {count} variable-base multiplications through mul_many; one process,",
             f"a warm-up per line, host clock with the device synchronised, median [min, max] of {args.reps} in ms", "",
             f"records: {res['regions']} regions, {res['ranges']} assigned ranges covering {res['range_cells']} cells, {res['events']} selector "
             f"enablings, {res['pairs']} (gate, selector) pairs, {res['b_cells_checked']} queried cells to check", "",
             f"(a) synthesis (fixed + advice), regions=False           {res['a_synthesis_ms']}",
             f"    synthesis (fixed + advice), regions=True            {res['a_synthesis_regions_ms']}",
             f"(b) the regions' check in MockProver (arrays, device, failures)   {res['b_check_regions_ms']}   failures {res['b_failures']}",
             f"    of which inside h2_cells_assigned_check (last repetition)     {res['b_entry_point_ms']}",
             f"    tests/region_model.py on the same records, once: building the sets {res['b_model_sets_ms']}, the loops {res['b_model_loops_ms']}   "
             f"failures {res['b_model_failures']}",
             f"(c) run_circuit(...).verify(), regions=False            {res['c_run_and_verify_ms']}",
             f"    run_circuit(...).verify(), regions=True             {res['c_run_and_verify_regions_ms']}   failures {res['c_failures']}", "",
             json.dumps(res)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
