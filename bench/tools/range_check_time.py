#!/usr/bin/env python3
"""Times the bulk range check on one MI355X: one process, inputs resident, a warm-up call per shape, then the median [min, max] of
--reps in milliseconds of GPU time (HIP events around the call); host clock where it says so.

  (a) `h2_range_check_trace_device` of 2^20 values at 25 words into a buffer allocated once (the kernel alone), and beside it in the
      same run a device-to-device copy of as many bytes as the kernel stores: the floor of a kernel that does nothing but store;
      and, in a child process on the laboratory build, the kernel's other arm, one lane per value (H2_RANGE_CHECK_PER_VALUE=1)
  (b) `range_check.decompose` of the same values (the entry point with its allocations), and `range_check.short` of 2^20 values
  (c) the witness synthesis of the circuit of examples/range_check.py -- 2048 values to 130 bits, 2048 each to 4 and to 5 bits over
      the 4_5b lookup -- through `range_check_many` / `short_range_check_many`, against the same circuit filled by a loop of
      `witness_check` / `witness_short_check`, host clock

No thresholds: nobody had measured any of this.  Writes profiles/range_check.txt (or --out)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ecc_time import gpu_ms  # noqa: E402

AB_LIB = os.path.join(ROOT, "build", "ab", "libhalo2_mi355x_ab.so")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--count", type=int, default=2048, help="values of each kind in the circuit of (c)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_check.txt"))
    ap.add_argument("--kernel-only", action="store_true", help="print the kernel's times as JSON and stop (the child of the A/B arm)")
    args = ap.parse_args()
    import torch
    import halo2_amd as h
    from halo2_amd import circuit as front
    from halo2_amd import fields, range_check
    from halo2_amd._lib import check, lib
    dev = fields.current_device()
    gen = torch.Generator(device=dev)
    gen.manual_seed(8)
    sync = torch.cuda.synchronize
    res = {"reps": args.reps}
    # (a)
    n, words = 1 << 20, 25
    values = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 4), dtype=torch.int64, device=dev, generator=gen)
    values[:, 3] &= (1 << 58) - 1                                            # 250 bits: canonical, and every word is live
    rows = torch.empty((n, words + 1, 4), dtype=torch.int64, device=dev)
    status = torch.empty((n,), dtype=torch.uint8, device=dev)
    other = torch.empty_like(rows)
    entry = lib().h2_range_check_trace_device

    def kernel():
        check(entry(h.FP, values.data_ptr(), n, words, rows.data_ptr(), status.data_ptr(), None), "h2_range_check_trace_device")
    if args.kernel_only:
        ms = gpu_ms(kernel, args.reps)
        print(json.dumps({"ms": ms, "checksum": int(rows.sum()), "too_wide": int(status.sum())}))
        return
    res["a_stored_bytes"] = rows.numel() * 8
    res["a_kernel_ms"] = gpu_ms(kernel, args.reps)
    checksum = int(rows.sum())
    res["a_per_value_ms"] = None
    if os.path.exists(AB_LIB):
        env = dict(os.environ, H2_LIB_PATH=AB_LIB, H2_RANGE_CHECK_PER_VALUE="1")
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernel-only", "--reps", str(args.reps)], env=env,
                               capture_output=True, text=True, timeout=300)
        if child.returncode == 0:
            other_arm = json.loads(child.stdout.strip().splitlines()[-1])
            assert other_arm["checksum"] == checksum, "the two arms disagree"
            res["a_per_value_ms"] = other_arm["ms"]
        else:
            res["a_per_value_error"] = child.stderr[-400:]
    res["a_copy_ms"] = gpu_ms(lambda: other.copy_(rows), args.reps)
    res["a_kernel_over_copy"] = round(res["a_kernel_ms"][0] / res["a_copy_ms"][0], 2)
    res["a_kernel_gb_per_s"] = round(res["a_stored_bytes"] / res["a_kernel_ms"][0] / 1e6, 1)
    res["a_copy_gb_per_s_written"] = round(res["a_stored_bytes"] / res["a_copy_ms"][0] / 1e6, 1)
    del other
    # (b)
    res["b_decompose_ms"] = gpu_ms(lambda: range_check.decompose(values, words, with_status=True), args.reps)
    res["b_short_ms"] = gpu_ms(lambda: range_check.short(values, 5, with_status=True), args.reps)
    del rows
    # (c)
    from range_check import RangeCheckCircuit, k_for, witness
    k = k_for(args.count, "4_5b")
    wide, four, five = witness(args.count, 1)

    def clock(circuit):
        times = []
        for _ in range(4):                                                   # the first is the warm-up
            sync()
            t0 = time.perf_counter()
            front.synthesize(circuit, k, h.FP, fixed=False, advice=True, instances=[])
            sync()
            times.append(round(1e3 * (time.perf_counter() - t0), 2))
        return sorted(times[1:])
    res["c_k"], res["c_count"] = k, args.count
    res["c_bulk_ms"] = clock(RangeCheckCircuit(wide, four, five, "4_5b", bulk=True))
    res["c_loop_ms"] = clock(RangeCheckCircuit(wide, four, five, "4_5b", bulk=False))
    res["c_loop_over_bulk"] = round(res["c_loop_ms"][1] / res["c_bulk_ms"][1], 1)

    lines = ["The bulk range check on one MI355X, one process; a warm-up call per shape, then median [min, max] of "
             f"{args.reps} in milliseconds of GPU time", "(events around the call); host clock where it says so", "",
             f"(a) h2_range_check_trace_device, 2^20 values at 25 words ({res['a_stored_bytes']} bytes stored)   {res['a_kernel_ms']}   "
             f"{res['a_kernel_gb_per_s']} GB/s stored",
             f"    device-to-device copy of as many bytes                                          {res['a_copy_ms']}   "
             f"{res['a_copy_gb_per_s_written']} GB/s written",
             f"    kernel / copy = {res['a_kernel_over_copy']}",
             f"    the other arm, one lane per value (laboratory build, child process; same cells)  {res['a_per_value_ms']}",
             f"(b) range_check.decompose, the same call with its allocations                       {res['b_decompose_ms']}",
             f"    range_check.short, 2^20 values at 5 bits (three rows each)                      {res['b_short_ms']}",
             f"(c) witness synthesis of the k = {k} circuit of {args.count} values to 130 bits and {args.count} each to 4 and 5 bits, host clock, ms, three runs",
             f"    range_check_many / short_range_check_many      {res['c_bulk_ms']}",
             f"    a loop of witness_check / witness_short_check  {res['c_loop_ms']}   loop / bulk = {res['c_loop_over_bulk']}",
             "", json.dumps(res)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
