#!/usr/bin/env python3
"""Times the device side of the circuit front-end at k = 20: one process, one GPU, inputs resident, a warm-up call per shape, then
the median [min, max] of --reps, the two arms of a comparison alternating inside one loop.

  (a) `assigned_to_field` over 8 advice columns of all-rational values (one launch over 8 * 2^k elements) against what the same
      result took before it existed: `h2_batch_invert_device` over the denominators, then an element-wise product by the
      evaluation kernel (`Evaluator(LAGRANGE)`, num * inv) into a new vector.
  (b) `selector_conflicts` + `selector_combine` for 32 selectors (8 columns of 4).
  (c) `keygen_pk` and `create_proof` of the simple-example circuit through the front-end, its two advice columns assigned as
      whole vectors (examples/circuit_api.BulkCircuit), against examples/simple_example.prove_and_verify -- the same circuit lowered
      by hand -- on the same params.

Writes profiles/circuit_frontend_k20.txt (or --out)."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Rows:
    """What Evaluator.compile / run ask of a domain for a Lagrange-basis product: the field, its modulus and the length."""

    def __init__(self, n, field, m):
        self.n, self.k, self.field, self.m, self.omega = n, n.bit_length() - 1, field, m, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--columns", type=int, default=8)
    ap.add_argument("--selectors", type=int, default=32)
    ap.add_argument("--skip-proofs", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "circuit_frontend_k20.txt"))
    args = ap.parse_args()
    import torch
    import halo2_amd as h
    from halo2_amd import fields
    from halo2_amd.arithmetic import assigned_to_field, batch_invert, selector_combine, selector_conflicts
    from halo2_amd.circuit import pack_selectors
    from halo2_amd.evaluator import LAGRANGE, Evaluator
    from halo2_amd.transcript import Blake2bWrite
    k, curve = args.k, h.VESTA
    n = 1 << k
    sf = fields.CURVE_FIELDS[curve][1]
    m = fields.MODULUS[sf]
    dev = fields.current_device()
    sync = torch.cuda.synchronize

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return time.perf_counter() - t0

    def summary(times):
        return [round(1e3 * statistics.median(times), 3), round(1e3 * min(times), 3), round(1e3 * max(times), 3)]

    def alternate(*fns):
        for fn in fns:
            timed(fn)                                                  # warm-up of every arm
        times = [[] for _ in fns]
        for _ in range(args.reps):
            for i, fn in enumerate(fns):
                times[i].append(timed(fn))
        return [summary(t) for t in times]

    res = {"k": k, "reps": args.reps}
    # ---- (a) -------------------------------------------------------------------------------------------------------------------------
    total = args.columns * n
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)

    def uniform(count):                                                # values below 2^254 < p: valid Montgomery representations, non-zero
        out = torch.randint(-(1 << 63), (1 << 63) - 1, (count, 4), dtype=torch.int64, device=dev, generator=gen)
        out[:, 3] &= (1 << 62) - 1
        out[:, 0] |= 1
        return out
    num, den = uniform(total), uniform(total)
    fused_out = torch.empty_like(num)
    rows = _Rows(total, sf, m)
    scratch = torch.empty_like(den)
    ev = Evaluator(LAGRANGE)
    leaf_num, leaf_inv = ev.register_poly(num), ev.register_poly(scratch)
    program = ev.compile(leaf_num * leaf_inv, rows)
    two_call_out = []

    def fused():
        assigned_to_field(num, den, sf, out=fused_out)

    def two_calls():
        scratch.copy_(den)                                             # batch_invert works in place; the denominators are kept, as above
        batch_invert(scratch, sf)
        two_call_out[:] = [ev.run(program, rows)]

    def two_calls_in_place():                                          # the cheapest form of the old way: the denominators are consumed
        batch_invert(scratch, sf)
        two_call_out[:] = [ev.run(program, rows)]
    scratch.copy_(den)
    fused()
    two_calls()
    sync()
    res["a_same_result"] = bool(torch.equal(fused_out, two_call_out[0]))
    a = alternate(fused, two_calls, two_calls_in_place)
    res["a_elements"] = total
    res["a_assigned_to_field_ms"], res["a_invert_then_multiply_ms"], res["a_invert_in_place_then_multiply_ms"] = a
    bytes_moved = total * 32 * 3
    res["a_assigned_to_field_GBps"] = round(bytes_moved / (a[0][0] * 1e-3) / 1e9, 1)
    # ---- (b) -------------------------------------------------------------------------------------------------------------------------
    s = args.selectors
    rng = np.random.default_rng(5)
    owner = rng.integers(0, s, size=n)
    act = np.stack([owner == i for i in range(s)])                     # every row enables exactly one selector: no conflicts
    act[1, 12345 % n] = True                                           # ... but one
    bits = torch.from_numpy(pack_selectors(act)).to(dev)
    columns = [i // 4 for i in range(s)]
    roots = [i % 4 + 1 for i in range(s)]
    held = []
    b = alternate(lambda: held.__setitem__(slice(None), [selector_conflicts(bits)]),
                  lambda: held.__setitem__(slice(None), [selector_combine(bits, roots, columns, n, (s + 3) // 4, sf)]))
    res["b_selectors"] = s
    res["b_conflicts_found"] = int(selector_conflicts(bits).sum().item())
    res["b_selector_conflicts_ms"], res["b_selector_combine_ms"] = b
    # ---- (c) -------------------------------------------------------------------------------------------------------------------------
    if not args.skip_proofs:
        api, by_hand = _load("circuit_api"), _load("simple_example")
        params = h.Params.new(curve, k)
        usable = n - 6
        a_, b_, constant = 2, 3, 7
        c = constant * a_ * a_ * b_ * b_
        circuit = api.BulkCircuit(constant, a_, b_, rows=usable)
        rng_ = api.make_rng()
        keys = []

        def keygen():
            keys[:] = [h.keygen_pk(params, circuit)]

        def prove():
            tr = Blake2bWrite(curve)
            h.create_proof(params, keys[0], [circuit], [[[c]]], rng_, tr)
            return tr.finalize()
        keygen_ms = alternate(keygen)[0]
        proof = prove()
        from halo2_amd.verifier import verify_proof
        res["c_front_end_verifies"] = bool(verify_proof(params, keys[0].vk, [[c]], proof))
        prove_ms = alternate(prove)[0]
        res["c_front_end_keygen_pk_ms"], res["c_front_end_create_proof_ms"] = keygen_ms, prove_ms
        hand = [by_hand.prove_and_verify(params, quiet=True) for _ in range(3)]
        res["c_by_hand_ok"] = all(r["ok"] for r in hand)
        pick = lambda key: [round(1e3 * statistics.median(r[key] for r in hand), 3), round(1e3 * min(r[key] for r in hand), 3),
                            round(1e3 * max(r[key] for r in hand), 3)]
        res["c_by_hand_keygen_ms"] = pick("keygen_s")
        res["c_by_hand_create_proof_warm_ms"] = pick("create_proof_s")
        res["c_by_hand_create_proof_from_host_columns_ms"] = pick("create_proof_from_host_columns_s")
        params.close()
    lines = [f"The circuit front-end's device work at k = {k}, one MI355X, one process; a warm-up call per shape, then median [min, max] of",
             f"{args.reps} (milliseconds, host clock around a synchronised call), the arms of a comparison alternating in one loop", "",
             f"(a) {args.columns} columns x 2^{k} all-rational cells = {total} elements; the two ways give the same bits: {res['a_same_result']}",
             f"    assigned_to_field, one launch                                  {res['a_assigned_to_field_ms']}   ({res['a_assigned_to_field_GBps']} GB/s of 3 x 32 B per element)",
             f"    copy + h2_batch_invert_device + evaluation-kernel product      {res['a_invert_then_multiply_ms']}",
             f"    the same without the copy (denominators consumed)              {res['a_invert_in_place_then_multiply_ms']}", "",
             f"(b) {s} selectors over 2^{k} rows, 4 to a column ({res['b_conflicts_found']} non-zero matrix entries)",
             f"    selector_conflicts                                             {res['b_selector_conflicts_ms']}",
             f"    selector_combine                                               {res['b_selector_combine_ms']}"]
    if not args.skip_proofs:
        lines += ["", f"(c) simple-example circuit, advice columns assigned as two vectors of {usable} rows (proof verifies: {res['c_front_end_verifies']})",
                  f"    front-end keygen_pk (configure, synthesize, compress, keygen)  {res['c_front_end_keygen_pk_ms']}",
                  f"    front-end create_proof (synthesize, upload, invert, prove)     {res['c_front_end_create_proof_ms']}",
                  f"    by hand: keygen_pk + keygen_vk (3 runs)                         {res['c_by_hand_keygen_ms']}",
                  f"    by hand: create_proof, columns resident, warm                   {res['c_by_hand_create_proof_warm_ms']}",
                  f"    by hand: create_proof from host columns                         {res['c_by_hand_create_proof_from_host_columns_ms']}"]
    lines += ["", json.dumps(res)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
