#!/usr/bin/env python3
"""The most common mistake while writing a chip, found by `dev::MockProver` on an MI355X: a cell a gate reads and nobody assigned.

The circuit is the reference's `unassigned_cell` (halo2_proofs/src/dev.rs:941-1012): a gate `q * (a[-1] - b)`, enabled at offset 1 of a
region that assigns a = 0 at offset 0 and forgets b.  An unassigned cell reads as zero, so the gate HOLDS and a proof would verify --
until some other witness needs b.  With `regions=True` the MockProver keeps the regions of the synthesis and says what the reference
says; with b assigned it is satisfied.

    python examples/unassigned_cell.py
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from halo2_amd.circuit import Circuit, Rotation, Value                                             # noqa: E402

K = 4
SENTENCE = ("Region 0 ('Faulty synthesis') uses Gate 0 ('Equality check') at offset 1, which requires cell in column "
            "Column { index: 1, column_type: Advice } at offset 1 to be assigned.")


class FaultyCircuit(Circuit):
    """forget_b=False is the fix."""

    def __init__(self, forget_b: bool = True):
        self.forget_b = forget_b

    def without_witnesses(self):
        return FaultyCircuit(self.forget_b)

    @staticmethod
    def configure(meta):
        a, b = meta.advice_column(), meta.advice_column()
        q = meta.selector()

        def equality(cells):
            a_ = cells.query_advice(a, Rotation.prev())
            b_ = cells.query_advice(b, Rotation.cur())
            q_ = cells.query_selector(q)
            return [q_ * (a_ - b_)]                                            # if q is enabled, a and b must be assigned to
        meta.create_gate("Equality check", equality)
        return dict(a=a, b=b, q=q)

    def synthesize(self, config, layouter):
        def assign(region):
            config["q"].enable(region, 1)                                      # enable the equality gate
            region.assign_advice(config["a"], 0, lambda: Value.known(0))       # a = 0
            if not self.forget_b:                                              # BUG when forgotten: b = 0 is what the column holds anyway
                region.assign_advice(config["b"], 1, lambda: Value.known(0))
        layouter.assign_region("Faulty synthesis", assign)


def main() -> bool:
    import halo2_amd as h
    from halo2_amd.dev import CellNotAssigned, MockProver
    plain = MockProver.run_circuit(K, FaultyCircuit(), [], h.FP).verify()
    print(f"without regions: {len(plain)} failure(s) -- the forgotten cell reads as zero and the gate holds")
    failures = MockProver.run_circuit(K, FaultyCircuit(), [], h.FP, regions=True).verify()
    for f in failures:
        print(f)
    expected = [CellNotAssigned(gate=(0, "Equality check"), region=(0, "Faulty synthesis"), gate_offset=1, column=("advice", 1), offset=1)]
    if plain or failures != expected or str(failures[0]) != SENTENCE:
        print("unexpected failures for the faulty circuit")
        return False
    fixed = MockProver.run_circuit(K, FaultyCircuit(forget_b=False), [], h.FP, regions=True)
    fixed.assert_satisfied()
    print("with b assigned: MockProver is satisfied")
    return fixed.failure_counts["CellNotAssigned"] == 0


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
