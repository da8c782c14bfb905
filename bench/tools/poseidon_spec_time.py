#!/usr/bin/env python3
"""Times Poseidon for a run-time Spec on one MI355X: one process, inputs resident, a warm-up call per shape, then the median [min, max]
of --reps in milliseconds of GPU time (HIP events around the call).

  (a) `Spec.hash` of 2^20 messages of `rate` elements (ConstantLength<rate>: one permutation each) at (3, 2), (9, 8), (12, 11)
  (b) `Spec.trace` of 1024 and 32768 permutations at the same three
  (c) the (3, 2, 8, 56) spec kernels beside the P128Pow5T3 kernels of csrc/poseidon.hip, same inputs, same run, and their ratio
  (d) what the compiler reports for the six kernels of csrc/poseidon_spec.hip: registers, scratch, LDS, code size

No thresholds: nobody had measured any of this.  Writes profiles/poseidon_spec.txt (or --out)."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
SHAPES = [(3, 2), (9, 8), (12, 11)]
CSRC = os.path.join(ROOT, "halo2_amd", "csrc")


def resources():
    """{kernel: {vgprs, sgprs, scratch, spills, code_bytes}} from -Rpass-analysis=kernel-resource-usage and the device object's symbols;
    None where the compiler is not at hand."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    readelf = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "llvm-readelf")
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "--no-gpu-bundle-output", "-c", "poseidon_spec.hip"]
    try:
        with tempfile.TemporaryDirectory() as tmp:
            obj = os.path.join(tmp, "poseidon_spec.o")
            remarks = subprocess.run([hipcc, *flags, "-Rpass-analysis=kernel-resource-usage", "-o", obj], cwd=CSRC, capture_output=True, text=True, check=True).stderr
            symbols = subprocess.run([readelf, "-sW", obj], capture_output=True, text=True, check=True).stdout
    except (OSError, subprocess.CalledProcessError):
        return None
    out, name = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if m and name:
            out[name][m.group(1).strip()] = m.group(2)
    for line in symbols.splitlines():
        parts = line.split()
        if len(parts) >= 8 and parts[3] == "FUNC" and parts[7] in out:
            out[parts[7]]["code_bytes"] = int(parts[2])
    return out


def short(mangled):
    m = re.search(r"(poseidon_spec_[a-z]+)ILi([01])E", mangled)
    return f"{m.group(1)}<{'FP' if m.group(2) == '0' else 'FQ'}>" if m else mangled


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poseidon_spec.txt"))
    args = ap.parse_args()
    import torch
    import halo2_amd as h
    from halo2_amd import fields, poseidon
    from halo2_amd.poseidon_spec import Spec
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

    n = 1 << args.log_n
    res = {"reps": args.reps, "log_n": args.log_n}
    lines = [f"Poseidon for a run-time Spec (csrc/poseidon_spec.hip) over Fp on one MI355X, one process; a warm-up call per shape, then median",
             f"[min, max] of {args.reps} in milliseconds of GPU time (events around the call); 8 full and 56 partial rounds everywhere", ""]
    for width, rate in SHAPES:
        spec = Spec(field, width, rate)
        poseidon.spec_constants(spec, dev)                             # the one upload
        messages = uniform(n, rate)
        ms = gpu_ms(lambda: spec.hash(messages))
        res[f"a_hash_{width}_{rate}_ms"] = ms
        lines.append(f"(a) Spec({width:>2}, {rate:>2}).hash, 2^{args.log_n} messages of {rate:>2}        {ms}   {1e6 * ms[0] / n:.2f} ns per permutation")
        del messages
    for width, rate in SHAPES:
        spec = Spec(field, width, rate)
        for count in (1 << 10, 1 << 15):
            states = uniform(count, width)
            ms = gpu_ms(lambda: spec.trace(states))
            res[f"b_trace_{width}_{rate}_{count}_ms"] = ms
            gbps = count * (width + 1) * spec.rows * 32 / (ms[0] * 1e-3) / 1e9
            lines.append(f"(b) Spec({width:>2}, {rate:>2}).trace, {count:>6} permutations        {ms}   {1e6 * ms[0] / count:.2f} ns per permutation, {gbps:.1f} GB/s stored")
    # (c) the same work through both sets of kernels
    t3 = Spec.p128pow5t3(field)
    pairs, pairs_states, states = uniform(n, 2), uniform(n, 3), uniform(1 << 15, 3)
    assert torch.equal(t3.hash(pairs[:4096]), poseidon.hash(pairs[:4096], field)) and torch.equal(t3.trace(states[:1024]), poseidon.trace(states[:1024], field))
    rows = [("hash, 2^%d pairs" % args.log_n, lambda: t3.hash(pairs), lambda: poseidon.hash(pairs, field)),
            ("permute, 2^%d states" % args.log_n, lambda: t3.permute(pairs_states), lambda: poseidon.permute(pairs_states, field)),
            ("trace, 32768 states", lambda: t3.trace(states), lambda: poseidon.trace(states, field))]
    lines += ["", "(c) the (3, 2, 8, 56) spec kernel beside the P128Pow5T3 kernel of csrc/poseidon.hip: same inputs, same bytes out"]
    worst = 0.0
    for what, new, old in rows:
        a, b = gpu_ms(new), gpu_ms(old)
        ratio = a[0] / b[0]
        worst = max(worst, ratio)
        res[f"c_{what.split(',')[0]}_spec_ms"], res[f"c_{what.split(',')[0]}_t3_ms"], res[f"c_{what.split(',')[0]}_ratio"] = a, b, round(ratio, 2)
        lines.append(f"    {what:<24} spec {a}   T3 {b}   ratio {ratio:.2f}")
    if worst > 2:
        lines += ["    A ratio above 2 is the price of the run-time width: the T3 kernel holds its three words in registers and reads its constants",
                  "    with scalar loads, while the spec kernel moves every word of the state through LDS (eight 32-bit reads per operand of each",
                  "    of the width^2 products, eight writes per result) and keeps one multiplier body for all products, so nothing overlaps the",
                  "    LDS latency inside a lane; its LDS footprint (4096 * width bytes a wave) also bounds the waves per CU."]
    # (d) the compiler's figures
    usage = resources()
    res["d_resources"] = usage
    lines += ["", "(d) kernels of csrc/poseidon_spec.hip, hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; LDS is dynamic,",
              "    4096 * width bytes a workgroup of one wave (12 KiB at width 3, 36 KiB at 9, 48 KiB at 12)"]
    if usage is None:
        lines.append("    not measured: no compiler on this machine")
    else:
        for name, u in sorted(usage.items(), key=lambda kv: short(kv[0])):
            lines.append(f"    {short(name):<28} VGPRs {u.get('VGPRs')}  SGPRs {u.get('TotalSGPRs')}  scratch {u.get('ScratchSize')} B/lane  spills {u.get('VGPRs Spill')}/{u.get('SGPRs Spill')}  "
                         f"code {u.get('code_bytes')} B")
    lines += ["", json.dumps(res)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
