#!/usr/bin/env python3
"""Times the V1 floor planner, host clock, on one seeded case: --regions (4000) random regions of 1 to 4 advice columns out of 10 and
1 to 40 rows (tests/floor_planner_cases.py `random_regions`).

  (a) the model -- tests/floor_planner_cases.py, the line-by-line port of the reference's strategy.rs, which clones and walks a
      column's allocations for every column of every placement -- and the shipped `slot_in_biggest_advice_first` on the same shapes,
      in the same run; the starts must agree.  Target: the planner at least 10 times faster than the model
  (b) the two synthesis passes of a circuit of those regions (each region one `assign_advice_column` per column), beside the
      planner's own time: what planning adds to a synthesis.  Not gated
  (c) with a device: keygen, and witness synthesis + create_proof, of the circuit of examples/floor_planner_v1.py under both
      planners.  Not gated; skipped, and said so, without a device

Writes profiles/floor_planner_v1.txt (or --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

TARGET = 10.0


def clock(f, reps):
    """-> (the last result, sorted milliseconds of `reps` runs)"""
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        times.append(round(1e3 * (time.perf_counter() - t0), 2))
    return out, sorted(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=64, help="pairs of the example circuit of (c)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "floor_planner_v1.txt"))
    args = ap.parse_args()
    import numpy as np

    import floor_planner_cases as fc
    from halo2_amd import circuit as front
    from halo2_amd import floor_planner as fp
    res = {"regions": args.regions, "reps": args.reps}
    shapes = fc.random_regions(args.regions)
    # (a)
    want, res["a_model_ms"] = clock(lambda: fc.model_slot_in_biggest_advice_first(shapes), 1)
    got, res["a_planner_ms"] = clock(lambda: fp.slot_in_biggest_advice_first(shapes), args.reps)
    assert got == want, "the planner and the model disagree"
    res["a_rows_v1"] = fc.rows_used(got[0], shapes)
    res["a_rows_simple"] = fc.rows_used(fc.simple_starts(shapes), shapes)
    median = res["a_planner_ms"][len(res["a_planner_ms"]) // 2]
    res["a_model_over_planner"] = round(res["a_model_ms"][0] / median, 1)
    res["a_target_met"] = res["a_model_over_planner"] >= TARGET

    # (b)
    class Regions(front.Circuit):
        floor_planner = fp.V1

        def without_witnesses(self):
            return Regions()

        @staticmethod
        def configure(meta):
            return [meta.advice_column() for _ in range(10)]

        def synthesize(self, advice, layouter):
            blank = np.zeros((40, 4), dtype=np.uint64)
            for columns, rows in shapes:
                layouter.assign_region("region", lambda region, columns=columns, rows=rows: [
                    region.assign_advice_column(advice[c.index], 0, blank[:rows]) for c in columns])
    k = max(4, (res["a_rows_simple"] + 16).bit_length())
    cs = front.ConstraintSystem(fc.M)
    config = Regions.configure(cs)
    circuit = Regions()

    def measure():
        assembly = front.Assembly(k, cs, fc.FP, fixed=False, advice=True, instances=[])
        pass_ = fp.MeasurementPass(assembly)
        circuit.without_witnesses().synthesize(config, pass_)
        return assembly, pass_
    (assembly, measured), res["b_measurement_pass_ms"] = clock(measure, args.reps)
    assert [(set(c), r) for c, r in measured.shapes] == [(set(c), r) for c, r in shapes]
    _, res["b_assignment_pass_ms"] = clock(lambda: circuit.synthesize(config, fp.AssignmentPass(assembly, got[0], measured.shapes)), args.reps)
    _, res["b_v1_synthesize_ms"] = clock(lambda: fp.V1.synthesize(front.Assembly(k, cs, fc.FP, fixed=False, advice=True, instances=[]),
                                                                  circuit, config, cs.constants), args.reps)
    # (c)
    import torch
    res["c_device"] = bool(torch.cuda.is_available())
    if res["c_device"]:
        import floor_planner_v1 as example
        import halo2_amd as h
        import random
        rng = random.Random(1)
        values = [rng.getrandbits(130) for _ in range(2 * args.pairs)]
        digest = example.public_digest(values, True)
        for name, kind in example.PLANNERS.items():
            rows, kk = example.layout(kind, args.pairs)
            params = h.Params.new(h.VESTA, kk)
            witnessed = kind(args.pairs, values, True)
            example.prove(params, witnessed, digest)                          # tables, first launches
            runs = sorted(example.prove(params, witnessed, digest)[2:] for _ in range(args.reps))
            params.close()
            res["c_" + name] = {"rows": rows, "k": kk, "keygen_ms": sorted(round(1e3 * r[0], 1) for r in runs),
                                "synthesis_and_create_proof_ms": sorted(round(1e3 * r[1], 1) for r in runs)}

    lines = [f"The V1 floor planner on {args.regions} seeded regions of 1 to 4 advice columns out of 10 and 1 to 40 rows; host clock, ms, "
             f"sorted runs", "",
             f"(a) rows used: SimpleFloorPlanner {res['a_rows_simple']}, V1 {res['a_rows_v1']}",
             f"    the model (line-by-line strategy.rs), one run      {res['a_model_ms']}",
             f"    slot_in_biggest_advice_first, {args.reps} runs              {res['a_planner_ms']}",
             f"    model / planner = {res['a_model_over_planner']}   target {TARGET:g}x: {'met' if res['a_target_met'] else 'NOT met'}; the same starts",
             f"(b) a circuit of those regions at k = {k}, one assign_advice_column per column of a region",
             f"    measurement pass                                   {res['b_measurement_pass_ms']}",
             f"    assignment pass                                    {res['b_assignment_pass_ms']}",
             f"    V1.synthesize: both passes and the plan            {res['b_v1_synthesize_ms']}"]
    if res["c_device"]:
        lines.append(f"(c) the circuit of examples/floor_planner_v1.py, {args.pairs} pairs, one MI355X, a warm-up run, then {args.reps}")
        for name in ("SimpleFloorPlanner", "V1"):
            r = res["c_" + name]
            lines.append(f"    {name:<18} {r['rows']:>5} rows, k = {r['k']}: keygen {r['keygen_ms']}, witness synthesis + create_proof "
                         f"{r['synthesis_and_create_proof_ms']}")
    else:
        lines.append("(c) no device: the example's keygen and create_proof were not timed")
    lines += ["", json.dumps(res)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
