#!/usr/bin/env python3
"""One circuit under both floor planners: `SimpleFloorPlanner` stacks every region below all that came before it in any of its
columns; `V1` measures the regions first and fits each into the lowest gap that takes it.  The planner decides the rows a circuit
needs, so it decides k, and k the size of every commitment and transform of keygen and create_proof.

The circuit: 2 x pairs values are range-checked to 130 bits in bulk (`range_check_many`: one region of 14 rows each on the running-sum
column); a secret bit orders the first two (`CondSwapChip.mux`, twice: one row each across five columns, the running-sum column among
them); every pair is hashed (`Pow5Chip.hash2_many`: one region of 37 rows each on the four Poseidon columns), the inputs tied to the
range-checked cells, and the first digest is the public input.  The two one-row regions touch all five columns, so the single pass
puts them, and with them all hashes, below the range checks: 28 x pairs + 2 + 37 x pairs rows.  V1 lays the hashes and the range
checks side by side: 37 x pairs + 3 rows.  At 64 pairs that is k = 13 against k = 12.

    python examples/floor_planner_v1.py [--pairs 64]
"""
from __future__ import annotations

import argparse
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from halo2_amd.circuit import AssignedCell, Circuit, NotEnoughRowsAvailable, SimpleFloorPlanner  # noqa: E402
from halo2_amd.floor_planner import V1  # noqa: E402
from halo2_amd.gadgets.poseidon import Pow5Chip  # noqa: E402
from halo2_amd.gadgets.utilities import CondSwapChip, LookupRangeCheckConfig, load_private  # noqa: E402

NUM_WORDS = 13


class OrderedHashesCircuit(Circuit):
    """values: 2 x pairs integers below 2^130, swap: a bool (None each for keygen).  Subclasses choose the planner."""

    def __init__(self, pairs: int, values=None, swap=None):
        self.pairs, self.values, self.swap = pairs, values, swap

    def without_witnesses(self):
        return type(self)(self.pairs)

    @staticmethod
    def configure(meta):
        advices = [meta.advice_column() for _ in range(5)]
        rc_a = [meta.fixed_column() for _ in range(3)]
        rc_b = [meta.fixed_column() for _ in range(3)]
        meta.enable_constant(meta.fixed_column())
        instance = meta.instance_column()
        meta.enable_equality(instance)
        for column in advices:
            meta.enable_equality(column)
        poseidon = Pow5Chip.configure(meta, advices[:3], advices[3], rc_a, rc_b)
        lookup = LookupRangeCheckConfig.configure(meta, advices[4], meta.lookup_table_column())
        return poseidon, lookup, CondSwapChip.configure(meta, advices), instance, advices

    def synthesize(self, config, layouter) -> None:
        from halo2_amd import fields
        poseidon, lookup, cond_swap, instance, advices = config
        values = [None] * (2 * self.pairs) if self.values is None else self.values
        lookup.load_range_check_table(layouter)
        checked = lookup.range_check_many(layouter, values, NUM_WORDS, True)
        low, high = (AssignedCell(values[i], checked[i][0]) for i in (0, 1))
        choice = load_private(layouter, advices[0], None if self.swap is None else int(self.swap))
        swap = CondSwapChip(cond_swap)
        first, second = swap.mux(layouter, choice, low, high), swap.mux(layouter, choice, high, low)
        left = right = None
        if self.values is not None:
            ordered = [values[1], values[0]] if self.swap else values[:2]
            left = fields.to_limbs([ordered[0]] + values[2::2], 0, True)
            right = fields.to_limbs([ordered[1]] + values[3::2], 0, True)
        hashes = Pow5Chip(poseidon).hash2_many(layouter, self.pairs, left, right)

        def tie(region):
            region.constrain_equal(hashes.left_cell(0), first.cell())
            region.constrain_equal(hashes.right_cell(0), second.cell())
            for i in range(1, self.pairs):
                region.constrain_equal(hashes.left_cell(i), checked[2 * i][0])
                region.constrain_equal(hashes.right_cell(i), checked[2 * i + 1][0])
        layouter.assign_region("inputs", tie)
        layouter.constrain_instance(hashes.output_cell(0), instance, 0)


class OrderedHashesCircuitV1(OrderedHashesCircuit):
    floor_planner = V1


PLANNERS = {"SimpleFloorPlanner": OrderedHashesCircuit, "V1": OrderedHashesCircuitV1}
assert OrderedHashesCircuit.floor_planner is SimpleFloorPlanner


def layout(kind, pairs: int):
    """-> (rows used, smallest k): keygen's synthesis of the circuit without witnesses at the first k that has the rows"""
    from halo2_amd import circuit as front
    k = 11                                                                    # the lookup table alone is 2^10 rows
    while True:
        try:
            _, _, layouter = front.synthesize(kind(pairs), k, 0, fixed=True, advice=False)
            return max(start + rows for start, (columns, rows) in zip(layouter.regions, layouter.shapes) if columns), k
        except NotEnoughRowsAvailable:
            k += 1


def public_digest(values, swap) -> int:
    """Poseidon(first, second) of the ordered first pair, outside the circuit"""
    import numpy as np
    from halo2_amd import fields, poseidon
    ordered = [values[1], values[0]] if swap else values[:2]
    digest = poseidon.hash(fields.to_limbs(ordered, 0, True).reshape(1, 2, 4), 0)
    return fields.from_limbs(np.ascontiguousarray(digest).view(np.uint64).reshape(-1, 4), 0, True)[0]


def prove(params, circuit, digest):
    """keygen and create_proof -> (pk, proof bytes, seconds of keygen, seconds of witness synthesis + create_proof)"""
    import halo2_amd as h
    from circuit_api import make_rng
    from halo2_amd.transcript import Blake2bWrite
    t0 = time.perf_counter()
    pk = h.keygen_pk(params, circuit)
    t1 = time.perf_counter()
    transcript = Blake2bWrite(params.curve)
    h.create_proof(params, pk, [circuit], [[[digest]]], make_rng(), transcript)
    proof = transcript.finalize()
    return pk, proof, t1 - t0, time.perf_counter() - t1


def main(argv=None) -> bool:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args(argv)
    import halo2_amd as h
    from halo2_amd.dev import MockProver
    from halo2_amd.verifier import verify_proof
    rng = random.Random(args.seed)
    values, swap = [rng.getrandbits(130) for _ in range(2 * args.pairs)], True
    digest = public_digest(values, swap)
    plans = {name: layout(kind, args.pairs) for name, kind in PLANNERS.items()}
    for name, (rows, k) in plans.items():
        print(f"{name:<18} {rows:>6} rows, k = {k}")
    ok = True
    for name, kind in PLANNERS.items():
        k = plans[name][1]
        circuit = kind(args.pairs, values, swap)
        params = h.Params.new(h.VESTA, k)
        line = f"{name}, k = {k}: "
        if kind is OrderedHashesCircuitV1:
            mock = MockProver.run_circuit(k, circuit, [[digest]], h.FP).verify()
            mock_wrong = MockProver.run_circuit(k, circuit, [[digest + 1]], h.FP).verify()
            ok = ok and not mock and bool(mock_wrong)
            line += f"MockProver {'satisfied' if not mock else mock[:3]}; "
        prove(params, circuit, digest)                                        # once unmeasured: tables and first launches
        pk, proof, keygen_s, prove_s = prove(params, circuit, digest)
        accepted = verify_proof(params, pk.vk, [[digest]], proof)
        wrong = verify_proof(params, pk.vk, [[digest + 1]], proof)
        params.close()
        ok = ok and accepted and not wrong
        print(line + f"keygen {keygen_s:.3f} s, witness synthesis + create_proof {prove_s:.3f} s ({len(proof)} bytes): "
              f"{'accepted' if accepted else 'REJECTED'}; digest + 1: {'ACCEPTED' if wrong else 'rejected'}")
    return bool(ok and plans["V1"][0] <= plans["SimpleFloorPlanner"][0])


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
