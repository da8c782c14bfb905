#!/usr/bin/env python3
"""Times the bulk short and base-field fixed-base multiplications on one MI355X: one process, inputs and tables resident, a warm-up
call per shape, then the median [min, max] of --reps in milliseconds of GPU time (HIP events around the call), the sides of a
comparison taken in turn; host clock where it says so.  Every figure stands beside something that exists without the feature,
measured in the same run.

  (a) `ecc.mul_fixed_base_field_trace` and `ecc.mul_fixed_short_trace` of 2^15 items, each beside `ecc.mul_fixed_trace` of 2^15
      full-width scalars: the same 85-window chain as the base-field form, which adds one field multiplication and one row of
      stores per window (the running sum's z_w instead of the small window value, and row 85); the short form walks 22 windows
  (b) the witness synthesis of the circuit of examples/value_commitment.py (64 commitments [v]V + [rcv]R, k = 13) through
      `mul_fixed_short_many`, `mul_fixed_many` and `add_many`, against the same circuit from a loop of single calls on the same
      inputs, host clock

No thresholds: nobody had measured any of this.  Writes profiles/ecc_fixed_sum.txt (or --out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))


def in_turn(fns, reps):
    """every function warmed once, then timed `reps` times, one after the other in each round -> [median, min, max] ms per function"""
    import torch
    for fn in fns:
        fn()
    times = [[] for _ in fns]
    for _ in range(reps):
        for fn, ts in zip(fns, times):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            end.record()
            end.synchronize()
            ts.append(start.elapsed_time(end))
    return [[round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)] for ts in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log-items", type=int, default=15)
    ap.add_argument("--count", type=int, default=64, help="commitments of the example's circuit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ecc_fixed_sum.txt"))
    args = ap.parse_args()
    import torch
    import halo2_amd as h
    from halo2_amd import circuit as front
    from halo2_amd import ecc, fields
    from value_commitment import ValueCommitmentsCircuit, fixed_base, notes_and_commitments
    dev = fields.current_device()
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    sync = torch.cuda.synchronize
    res = {"reps": args.reps}
    n = 1 << args.log_items
    tables_v, tables_r = fixed_base(b"V", ecc.NUM_WINDOWS_SHORT), fixed_base(b"R", ecc.NUM_WINDOWS)

    # (a) canonical elements below 2^254 < p (and below the group's order for the full-width form); magnitudes of 64 bits
    scalars = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 4), dtype=torch.int64, device=dev, generator=gen)
    scalars[:, 3] &= (1 << 62) - 1
    magnitudes = scalars.clone()
    magnitudes[:, 1:] = 0
    signs = torch.from_numpy(fields.to_limbs([1, fields.MODULUS[h.FP] - 1], h.FP, montgomery=False).view("int64")).to(dev).repeat(n // 2, 1)
    full = ecc.mul_fixed_trace(tables_r.device, scalars)
    base_field = ecc.mul_fixed_base_field_trace(tables_r.device, scalars)
    rows = torch.arange(n, device=dev)[:, None] * 86 + torch.arange(85, device=dev)[None, :]
    for c in (0, 1, 2, 3, 5):                              # the same chain: every column but `window` agrees row for row
        assert torch.equal(base_field[0][c][rows.reshape(-1)], full[0][c]), c
    assert torch.equal(base_field[1][:, :11], full[1])
    del full, base_field, rows
    res["a_items"] = n
    res["a_full_width_ms"], res["a_base_field_ms"], res["a_short_ms"] = in_turn(
        [lambda: ecc.mul_fixed_trace(tables_r.device, scalars), lambda: ecc.mul_fixed_base_field_trace(tables_r.device, scalars),
         lambda: ecc.mul_fixed_short_trace(tables_v.device, magnitudes, signs)], args.reps)
    res["a_base_field_over_full_width"] = round(res["a_base_field_ms"][0] / res["a_full_width_ms"][0], 2)
    res["a_short_over_full_width"] = round(res["a_short_ms"][0] / res["a_full_width_ms"][0], 2)
    del scalars, magnitudes, signs

    # (b)
    notes, _ = notes_and_commitments(args.count, 1, tables_v, tables_r)
    k = max(11, (args.count * 116 + 16).bit_length())

    def clock(circuit):
        times = []
        for _ in range(args.reps + 1):                     # the first is the warm-up
            sync()
            t0 = time.perf_counter()
            front.synthesize(circuit, k, h.FP, fixed=False, advice=True, instances=[[0] * (2 * args.count)])
            sync()
            times.append(round(1e3 * (time.perf_counter() - t0), 2))
        rest = times[1:]
        return [round(statistics.median(rest), 2), min(rest), max(rest)]
    res["b_k"], res["b_count"] = k, args.count
    res["b_bulk_ms"] = clock(ValueCommitmentsCircuit(notes, tables_v, tables_r))
    res["b_loop_ms"] = clock(ValueCommitmentsCircuit(notes, tables_v, tables_r, bulk=False))
    res["b_loop_over_bulk"] = round(res["b_loop_ms"][0] / res["b_bulk_ms"][0], 1)

    lines = ["The bulk short and base-field fixed-base multiplications on one MI355X, one process; a warm-up call per shape, then median "
             f"[min, max] of {args.reps}", "in milliseconds of GPU time (events around the call, the sides of a comparison in turn); host clock where it says so",
             "",
             f"(a) ecc.mul_fixed_trace, 2^{args.log_items} full-width scalars, 85 windows (exists without the feature)   {res['a_full_width_ms']}",
             f"    ecc.mul_fixed_base_field_trace, 2^{args.log_items} elements, 85 windows, 86 rows                     {res['a_base_field_ms']}   "
             f"base-field / full-width = {res['a_base_field_over_full_width']}",
             f"    ecc.mul_fixed_short_trace, 2^{args.log_items} pairs, 22 windows, 23 rows                             {res['a_short_ms']}   "
             f"short / full-width = {res['a_short_over_full_width']}",
             "    (each call allocates its outputs and its scratch; the base-field form's columns but `window` and its addition record",
             "     were checked equal to the full-width form's on these scalars before timing)",
             f"(b) witness synthesis of the k = {k} circuit of {args.count} value commitments [v]V + [rcv]R, host clock, ms",
             f"    mul_fixed_short_many + mul_fixed_many + add_many         {res['b_bulk_ms']}",
             f"    a loop of mul_fixed_short, mul_fixed and add            {res['b_loop_ms']}   loop / bulk = {res['b_loop_over_bulk']}",
             "", json.dumps(res)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
