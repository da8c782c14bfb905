#!/usr/bin/env python3
"""The reference's `examples/simple-example.rs` written against `halo2_amd.circuit`: a chip with its instructions, a `Circuit` with
`configure` and `synthesize`, and nothing lowered by hand -- examples/simple_example.py spells out what the floor planner, selector
compression and the copy-constraint assembly derive here.  The circuit is mock-proved, proved and verified on an MI355X.

Prove knowledge of a, b with constant * a^2 * b^2 = c for a public c.

    python examples/circuit_api.py [--k 4]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from halo2_amd.circuit import Circuit, Rotation, Value  # noqa: E402


class FieldConfig:
    def __init__(self, advice, instance, s_mul):
        self.advice, self.instance, self.s_mul = advice, instance, s_mul


class FieldChip:
    """Numbers are cells of the first advice column; `mul` takes two rows: | lhs | rhs | s_mul | above | out |."""

    def __init__(self, config: FieldConfig):
        self.config = config

    @staticmethod
    def configure(meta, advice, instance, constant) -> FieldConfig:
        meta.enable_equality(instance)
        meta.enable_constant(constant)
        for column in advice:
            meta.enable_equality(column)
        s_mul = meta.selector()

        def mul(cells):
            lhs = cells.query_advice(advice[0], Rotation.cur())
            rhs = cells.query_advice(advice[1], Rotation.cur())
            out = cells.query_advice(advice[0], Rotation.next())
            return [cells.query_selector(s_mul) * (lhs * rhs - out)]
        meta.create_gate("mul", mul)
        return FieldConfig(advice, instance, s_mul)

    def load_private(self, layouter, value):
        return layouter.assign_region("load private", lambda region: region.assign_advice(self.config.advice[0], 0, lambda: Value(value)))

    def load_constant(self, layouter, constant):
        return layouter.assign_region("load constant",
                                      lambda region: region.assign_advice_from_constant(self.config.advice[0], 0, constant))

    def mul(self, layouter, a, b):
        config = self.config

        def assign(region):
            config.s_mul.enable(region, 0)
            a.copy_advice(region, config.advice[0], 0)
            b.copy_advice(region, config.advice[1], 0)
            return region.assign_advice(config.advice[0], 1, lambda: a.value() * b.value())
        return layouter.assign_region("mul", assign)

    def expose_public(self, layouter, number, row: int) -> None:
        layouter.constrain_instance(number.cell(), self.config.instance, row)


class MyCircuit(Circuit):
    def __init__(self, constant: int, a=None, b=None):
        self.constant, self.a, self.b = constant, a, b

    def without_witnesses(self):
        return MyCircuit(self.constant)

    @staticmethod
    def configure(meta) -> FieldConfig:
        advice = [meta.advice_column(), meta.advice_column()]
        instance = meta.instance_column()
        constant = meta.fixed_column()
        return FieldChip.configure(meta, advice, instance, constant)

    def synthesize(self, config, layouter) -> None:
        chip = FieldChip(config)
        a = chip.load_private(layouter, self.a)
        b = chip.load_private(layouter, self.b)
        constant = chip.load_constant(layouter, self.constant)
        ab = chip.mul(layouter, a, b)
        absq = chip.mul(layouter, ab, ab)
        c = chip.mul(layouter, constant, absq)
        chip.expose_public(layouter, c, 0)


class BulkCircuit(MyCircuit):
    """The same cells in one region, the two advice columns assigned as whole vectors (`Region.assign_advice_column`): what a large
    circuit does instead of one Python call per cell.  `rows`: the vectors' length (zeros past the nine rows in use)."""

    def __init__(self, constant: int, a=None, b=None, rows: int = 9):
        super().__init__(constant, a, b)
        self.rows = rows

    def without_witnesses(self):
        return BulkCircuit(self.constant, rows=self.rows)

    def synthesize(self, config, layouter) -> None:
        from halo2_amd import fields
        m = fields.MODULUS[0]
        a, b, constant = self.a or 0, self.b or 0, self.constant           # keygen ignores the advice values
        ab = a * b % m
        absq = ab * ab % m
        a0 = np.zeros((self.rows, 4), dtype=np.uint64)
        a1 = np.zeros((self.rows, 4), dtype=np.uint64)
        a0[:9] = fields.to_limbs([a, b, constant, a, ab, ab, absq, constant, constant * absq % m], 0, True)
        a1[[3, 5, 7]] = fields.to_limbs([b, ab, absq], 0, True)

        def assign(region):
            left = region.assign_advice_column(config.advice[0], 0, a0)
            right = region.assign_advice_column(config.advice[1], 0, a1)
            for row in (3, 5, 7):
                config.s_mul.enable(region, row)
            region.constrain_constant(left.cell(2), constant)
            for x, y in ((left.cell(0), left.cell(3)), (left.cell(1), right.cell(3)), (left.cell(2), left.cell(7)),
                         (left.cell(4), left.cell(5)), (left.cell(4), right.cell(5)), (left.cell(6), right.cell(7))):
                region.constrain_equal(x, y)
            return left.cell(8)
        c = layouter.assign_region("all of it", assign)
        layouter.constrain_instance(c, config.instance, 0)


def make_rng(seed: int = 0x9E3779B97F4A7C15):
    """Any source of uniform scalars; NOT cryptographic here.  Large draws (a random polynomial's coefficients) stay on the device."""
    import torch
    from halo2_amd import fields
    gen = np.random.Generator(np.random.PCG64(seed))
    tgen = torch.Generator(device=fields.current_device())
    tgen.manual_seed(seed)

    def rng(count):
        if count >= 4096:
            out = torch.randint(-(1 << 63), (1 << 63) - 1, (count, 4), dtype=torch.int64, device=tgen.device, generator=tgen)
            out[:, 3] &= (1 << 62) - 1
            return out
        out = gen.integers(0, 1 << 64, size=(count, 4), dtype=np.uint64)
        out[:, 3] &= np.uint64((1 << 62) - 1)                              # below 2^254 < p: a valid Montgomery representation
        return out
    return rng


def prove_and_verify(params, circuit, c: int, quiet: bool = False) -> dict:
    """MockProver, keygen, create_proof and verify_proof of `circuit` with public input c; returns the verdicts and timings."""
    import halo2_amd as h
    from halo2_amd import fields
    from halo2_amd.dev import MockProver
    from halo2_amd.transcript import Blake2bWrite
    from halo2_amd.verifier import verify_proof
    sf = fields.CURVE_FIELDS[params.curve][1]
    mock = MockProver.run_circuit(params.k, circuit, [[c]], sf).verify()
    mock_wrong = MockProver.run_circuit(params.k, circuit, [[c + 1]], sf).verify()
    t0 = time.perf_counter()
    pk = h.keygen_pk(params, circuit)
    t1 = time.perf_counter()
    transcript = Blake2bWrite(params.curve)
    h.create_proof(params, pk, [circuit], [[[c]]], make_rng(), transcript)
    proof = transcript.finalize()
    t2 = time.perf_counter()
    ok = verify_proof(params, pk.vk, [[c]], proof)
    wrong = verify_proof(params, pk.vk, [[c + 1]], proof)
    if not quiet:
        print(f"k = {params.k}: MockProver {'satisfied' if not mock else mock}; keygen {t1 - t0:.3f} s, create_proof {t2 - t1:.3f} s "
              f"({len(proof)} bytes); c = {c}: {'accepted' if ok else 'REJECTED'}; c + 1: {'ACCEPTED' if wrong else 'rejected'}")
        print(f"transcript_repr = {pk.vk_repr:#066x}")
    return {"ok": bool(ok and not wrong and not mock and mock_wrong), "keygen_s": t1 - t0, "create_proof_s": t2 - t1,
            "proof_bytes": len(proof), "vk_repr": pk.vk_repr, "pinned": pk.pinned()}


def main(argv=None) -> bool:
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=4)
    args = ap.parse_args(argv)
    import halo2_amd as h
    params = h.Params.new(h.VESTA, args.k)
    a, b, constant = 2, 3, 7                                               # simple-example.rs:314-317
    c = constant * a * a * b * b
    chips = prove_and_verify(params, MyCircuit(constant, a, b), c)
    bulk = prove_and_verify(params, BulkCircuit(constant, a, b), c)
    params.close()
    return chips["ok"] and bulk["ok"]


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
