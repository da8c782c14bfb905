#!/usr/bin/env python3
"""Times the bulk Merkle paths on one MI355X: one process, inputs resident, a warm-up call per shape, then the median [min, max] of
--reps in milliseconds of GPU time (HIP events around the call), the two sides of a comparison taken in turn; host clock where it
says so.  Every figure stands beside something that exists without the feature, measured in the same run.

  (a) `sinsemilla.merkle_paths` of 2^16 paths x depth 32, and of 16 x 32, against the loop a caller writes without it on the same
      inputs: 32 x `sinsemilla.merkle_crh` with a `torch.where` swap (and the `stack` inside merkle_crh); the roots must agree
  (b) `h2_sinsemilla_merkle_trace_device` of 2^16 x 32 items into a buffer allocated once, against a device-to-device copy of as many
      bytes as it writes; and, in a child process on the laboratory build, the kernel's other arm, one lane per output element
      (H2_MERKLE_TRACE_PER_CELL=1)
  (c) the witness synthesis of the circuit of examples/sinsemilla_merkle_many.py (16 paths x 32 over two chips) through
      `MerklePaths.calculate_roots`, against the same circuit from a loop of 16 `MerklePath.calculate_root`, host clock
  (d) registers, scratch and code size of the two kernels beside sinsemilla.hip's layer kernel, from the compiler
      (`make -C halo2_amd/csrc merkle_path_resources`, or --resources FILE with its output)

No thresholds: nobody had measured any of this.  Writes profiles/merkle_paths.txt (or --out)."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

AB_LIB = os.path.join(ROOT, "build", "ab", "libhalo2_mi355x_ab.so")
KERNELS = ("merkle_paths", "merkle_trace", "sinsemilla_merkle")


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


def resources(text):
    """the compiler's remarks -> {kernel: (VGPRs, scratch bytes per lane, code bytes, occupancy)}"""
    found = {}
    sizes = {name: int(size) for size, name in re.findall(r"^\s*\d+:\s+[0-9a-f]+\s+(\d+)\s+FUNC\s.*?(_ZN2h2\w+)\s*$", text, flags=re.M)}
    for block in re.split(r"remark: Function Name: ", text)[1:]:
        name = next((k for k in sorted(KERNELS, key=len, reverse=True) if re.match(rf"_ZN2h2\d+_GLOBAL__N_1\d+{k}E", block)), None)
        if name:
            grab = lambda key: int(re.search(rf"{key}: (\d+)", block).group(1))
            found[name] = (grab("VGPRs"), grab(r"ScratchSize \[bytes/lane\]"), sizes.get(re.match(r"\w+", block).group(0)),
                           grab(r"Occupancy \[waves/SIMD\]"))
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log-paths", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle_paths.txt"))
    ap.add_argument("--resources", help="a file with the output of `make merkle_path_resources`; made here when absent")
    ap.add_argument("--trace-only", action="store_true", help="print the trace kernel's times as JSON and stop (the child of the A/B arm)")
    args = ap.parse_args()
    import torch
    import halo2_amd as h
    from halo2_amd import circuit as front
    from halo2_amd import fields, sinsemilla
    from halo2_amd._lib import MerklePaths, check, lib
    dev = fields.current_device()
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    sync = torch.cuda.synchronize
    res = {"reps": args.reps}
    depth = 32
    domain = sinsemilla.HashDomain(sinsemilla.MERKLE_CRH_DOMAIN)

    def random_elements(*shape):
        """Montgomery limbs of reduced elements: the top limb below the modulus's"""
        t = torch.randint(-(1 << 63), (1 << 63) - 1, shape + (4,), dtype=torch.int64, device=dev, generator=gen)
        t[..., 3] &= (1 << 61) - 1
        return t

    def inputs(n):
        return random_elements(n), torch.randint(-(1 << 31), (1 << 31) - 1, (n,), dtype=torch.int32, device=dev, generator=gen), random_elements(n, depth)

    def loop(leaves, positions, siblings):
        node = leaves
        for l in range(depth):                                              # noqa: E741
            bit = ((positions >> l) & 1).bool()[:, None]
            sibling = siblings[:, l]
            node = sinsemilla.merkle_crh(l, torch.where(bit, sibling, node), torch.where(bit, node, sibling), domain)
        return node

    big = inputs(1 << args.log_paths)
    if not args.trace_only:
        # (a)
        for key, data in (("a_big", big), ("a_small", inputs(16))):
            walked = sinsemilla.merkle_paths(*data, domain=domain)
            assert torch.equal(walked[:, depth], loop(*data)), "the walk and the loop disagree"
            res[key + "_walk_ms"], res[key + "_loop_ms"] = in_turn([lambda: sinsemilla.merkle_paths(*data, domain=domain), lambda: loop(*data)],
                                                                   args.reps)
            res[key + "_loop_over_walk"] = round(res[key + "_loop_ms"][0] / res[key + "_walk_ms"][0], 2)
    # (b)
    n = 1 << args.log_paths
    nodes = sinsemilla.merkle_paths(*big, domain=domain)
    count = n * depth
    out = torch.empty((23 * count, 4), dtype=torch.int64, device=dev)
    descriptor = MerklePaths(depth, None, None, torch.cuda.current_stream().cuda_stream)

    def kernel():
        check(lib().h2_sinsemilla_merkle_trace_device(C.byref(descriptor), nodes.data_ptr(), big[2].data_ptr(), big[1].data_ptr(), n, 0, depth,
                                                      out.data_ptr()), "h2_sinsemilla_merkle_trace_device")
    if args.trace_only:
        ms = in_turn([kernel], args.reps)[0]
        print(json.dumps({"ms": ms, "checksum": int(out.sum())}))
        return
    other = torch.empty_like(out)
    res["b_stored_bytes"] = out.numel() * 8
    res["b_kernel_ms"], res["b_copy_ms"] = in_turn([kernel, lambda: other.copy_(out)], args.reps)
    checksum = int(out.sum())
    res["b_kernel_over_copy"] = round(res["b_kernel_ms"][0] / res["b_copy_ms"][0], 2)
    res["b_kernel_gb_per_s"] = round(res["b_stored_bytes"] / res["b_kernel_ms"][0] / 1e6, 1)
    res["b_copy_gb_per_s_written"] = round(res["b_stored_bytes"] / res["b_copy_ms"][0] / 1e6, 1)
    del other, out
    res["b_per_cell_ms"] = None
    if os.path.exists(AB_LIB):
        env = dict(os.environ, H2_LIB_PATH=AB_LIB, H2_MERKLE_TRACE_PER_CELL="1")
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-only", "--reps", str(args.reps), "--log-paths", str(args.log_paths)],
                               env=env, capture_output=True, text=True, timeout=300)
        if child.returncode == 0:
            other_arm = json.loads(child.stdout.strip().splitlines()[-1])
            assert other_arm["checksum"] == checksum, "the two arms disagree"
            res["b_per_cell_ms"] = other_arm["ms"]
        else:
            res["b_per_cell_error"] = child.stderr[-400:]
    del nodes, big
    # (c)
    from sinsemilla_merkle_many import MerklePathsCircuit, planned_rows, smallest_k, witness
    paths = 16
    k = smallest_k(planned_rows(paths, depth))
    leaves, positions, siblings = witness(paths, depth, 1)

    def clock(circuit):
        times = []
        for _ in range(4):                                                   # the first is the warm-up
            sync()
            t0 = time.perf_counter()
            front.synthesize(circuit, k, h.FP, fixed=False, advice=True, instances=[])
            sync()
            times.append(round(1e3 * (time.perf_counter() - t0), 2))
        return sorted(times[1:])
    res["c_k"] = k
    res["c_bulk_ms"] = clock(MerklePathsCircuit(paths, depth, leaves, positions, siblings))
    res["c_loop_ms"] = clock(MerklePathsCircuit(paths, depth, leaves, positions, siblings, bulk=False))
    res["c_loop_over_bulk"] = round(res["c_loop_ms"][1] / res["c_bulk_ms"][1], 1)
    # (d)
    if args.resources:
        text = open(args.resources).read()
    else:
        made = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "halo2_amd", "csrc"), "merkle_path_resources"], capture_output=True, text=True)
        text = made.stdout + made.stderr
    res["d_resources"] = resources(text)

    def slower(key):
        walk, loop_ = res[key + "_walk_ms"], res[key + "_loop_ms"]
        spread = max(walk[2] - walk[1], loop_[2] - loop_[1])
        return walk[0] - loop_[0] > spread
    lines = ["The bulk Merkle paths on one MI355X, one process; a warm-up call per shape, then median [min, max] of "
             f"{args.reps} in milliseconds of GPU time", "(events around the call, the two sides of a comparison in turn); host clock where it says so", "",
             f"(a) sinsemilla.merkle_paths, 2^{args.log_paths} paths x depth 32, one launch                   {res['a_big_walk_ms']}",
             f"    the loop without it: 32 x merkle_crh, torch.where swap, stack; same roots       {res['a_big_loop_ms']}   loop / walk = {res['a_big_loop_over_walk']}",
             f"    sinsemilla.merkle_paths, 16 paths x depth 32                                    {res['a_small_walk_ms']}",
             f"    the loop without it                                                             {res['a_small_loop_ms']}   loop / walk = {res['a_small_loop_over_walk']}"]
    for key, what in (("a_big", f"2^{args.log_paths} paths"), ("a_small", "16 paths")):
        if slower(key):
            lines.append(f"    AT {what.upper()} THE ONE-LAUNCH WALK IS SLOWER THAN THE LOOP BY MORE THAN THE SPREAD OF THE REPEATS (see DESIGN.md)")
    lines += [f"(b) h2_sinsemilla_merkle_trace_device, 2^{args.log_paths} x 32 items ({res['b_stored_bytes']} bytes stored)   {res['b_kernel_ms']}   "
              f"{res['b_kernel_gb_per_s']} GB/s stored",
              f"    device-to-device copy of as many bytes                                          {res['b_copy_ms']}   "
              f"{res['b_copy_gb_per_s_written']} GB/s written",
              f"    kernel / copy = {res['b_kernel_over_copy']}",
              f"    the other arm, one lane per output element (laboratory build, child process; same bytes summed)  {res['b_per_cell_ms']}",
              f"(c) witness synthesis of the k = {k} circuit of 16 paths x 32 layers over two MerkleChips, host clock, ms, three runs",
              f"    MerklePaths.calculate_roots               {res['c_bulk_ms']}",
              f"    a loop of 16 MerklePath.calculate_root    {res['c_loop_ms']}   loop / bulk = {res['c_loop_over_bulk']}",
              "(d) the compiler's account (gfx950, -O3): VGPRs, scratch bytes per lane, code bytes, waves per SIMD"]
    for name in KERNELS:
        lines.append(f"    {name:<20}{res['d_resources'].get(name)}" + ("   (sinsemilla.hip, the layer kernel, for comparison)" if name == "sinsemilla_merkle" else ""))
    lines += ["", json.dumps(res)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
