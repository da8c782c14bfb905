#!/usr/bin/env python3
"""`dev::MockProver` on an MI355X: find out WHY a witness would not verify, before proving it.

1. The reference's documentation example (halo2_proofs/src/dev.rs:166-261): an R1CS gate written as s * (a * b + c) instead of
   s * (a * b - c), with a = 2, b = 4, c = 8 in row 0.  The checker names the gate, the row and the cell values.
2. The circuit of examples/simple_example.py: `assert_satisfied()` first, as the reference's own examples do
   (examples/simple-example.rs:331-337), then the real proof.

    python examples/mock_prover.py [--k 4]
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def buggy_r1cs():
    """The documentation example in lowered form: advice a, b, c; the selector s is a fixed column; K = 5."""
    import halo2_amd as h
    from halo2_amd.dev import MockProver
    from halo2_amd.plonk import ConstraintSystem
    k = 5
    n = 1 << k
    cs = ConstraintSystem(num_fixed_columns=1, num_advice_columns=3, num_instance_columns=0,
                          gates=[lambda q: q.fixed(0) * (q.advice(0) * q.advice(1) + q.advice(2))],       # BUG: should be a * b - c
                          advice_queries=[(0, 0), (1, 0), (2, 0)], instance_queries=[], fixed_queries=[(0, 0)], degree=3, blinding_factors=5)
    column = lambda v: [v] + [0] * (n - 1)
    prover = MockProver.run(k, cs, [column(1)], [column(2), column(4), column(2 * 4)], [], [], h.FP)
    return prover.verify()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=4)
    args = ap.parse_args(argv)
    import halo2_amd as h
    import simple_example
    from halo2_amd import fields
    from halo2_amd.dev import ConstraintNotSatisfied, MockProver
    from halo2_amd.plonk import ConstraintSystem

    failures = buggy_r1cs()
    for f in failures:
        print(f)
    expected = [ConstraintNotSatisfied(0, 0, (("fixed", 0, 0, 1), ("advice", 0, 0, 2), ("advice", 1, 0, 4), ("advice", 2, 0, 8)))]
    if failures != expected:
        print("unexpected failures for the documentation example")
        return False

    # simple-example: checked, then proved
    curve = h.VESTA
    sf = fields.CURVE_FIELDS[curve][1]
    m, n = fields.MODULUS[sf], 1 << args.k
    cs = ConstraintSystem(
        num_fixed_columns=2, num_advice_columns=2, num_instance_columns=1,
        gates=[lambda q: q.fixed(1) * (q.advice(0) * q.advice(1) - q.advice(0, 1))],
        advice_queries=[(0, 0), (1, 0), (0, 1)], instance_queries=[(0, 0)], fixed_queries=[(0, 0), (1, 0)],
        permutation_columns=[("instance", 0), ("fixed", 0), ("advice", 0), ("advice", 1)], degree=3, blinding_factors=5)
    advice, fixed, mapping, c = simple_example.build(m, n, 2, 3, 7)
    MockProver.run(args.k, cs, fixed, advice, [[c]], mapping, sf).assert_satisfied()
    print(f"simple-example (k = {args.k}): MockProver is satisfied")
    wrong = MockProver.run(args.k, cs, fixed, advice, [[c + 1]], mapping, sf).verify()
    for f in wrong:
        print("with the public input c + 1:", f)
    params = simple_example.toy_params(h, curve, args.k)
    res = simple_example.prove_and_verify(params)
    params.close()
    return bool(res["ok"] and len(wrong) == 2)


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
