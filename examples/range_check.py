#!/usr/bin/env python3
"""Range checks in bulk: constrain a few thousand values to 130 bits and as many again to 4 and to 5 bits, the checks every
Orchard-shaped circuit is full of.

The circuit stands on `LookupRangeCheck4_5BConfig` (halo2_gadgets utilities/lookup_range_check.rs): the K = 10 lookup table with a tag
column, over which a 4- or 5-bit check is ONE row -- a lookup of (value, tag) -- where the plain `LookupRangeCheckConfig` takes three
(the value, its shift by 2^(10 - s), and the constant 2^-s).  Every check goes through the bulk path: `range_check_many` lays all
130-bit checks into one region of 14 rows each (13 words, strict) whose running sums come from one launch of
`halo2_amd.range_check.decompose`; `short_range_check_many` does the same for the short checks.  The circuit is mock-proved, proved and
verified on an MI355X.

    python examples/range_check.py [--count 2048] [--lookup 4_5b|plain] [--loop]
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

from halo2_amd.circuit import Circuit  # noqa: E402
from halo2_amd.gadgets.utilities import LookupRangeCheck4_5BConfig, LookupRangeCheckConfig  # noqa: E402

NUM_WORDS = 13                            # 130 bits: the width of the ECC chip's overflow check
LOOKUPS = {"plain": LookupRangeCheckConfig, "4_5b": LookupRangeCheck4_5BConfig}
TABLE_ROWS = {"plain": 1 << 10, "4_5b": (1 << 10) + (1 << 4) + (1 << 5)}


class RangeCheckCircuit(Circuit):
    """wide: integers below 2^130; four, five: integers below 2^4 and 2^5 (None each for keygen).  bulk=False assigns the same cells
    one Python integer at a time, by a loop of witness_check and witness_short_check."""

    def __init__(self, wide, four, five, lookup="4_5b", bulk=True):
        self.wide, self.four, self.five, self.lookup, self.bulk = list(wide), list(four), list(five), lookup, bulk
        self.short_rows = None

    def without_witnesses(self):
        return RangeCheckCircuit([None] * len(self.wide), [None] * len(self.four), [None] * len(self.five), self.lookup, self.bulk)

    def configure(self, meta):
        running_sum = meta.advice_column()
        table_idx = meta.lookup_table_column()
        constants = meta.fixed_column()
        meta.enable_constant(constants)
        return LOOKUPS[self.lookup].configure(meta, running_sum, table_idx)

    def synthesize(self, config, layouter) -> None:
        config.load_range_check_table(layouter)
        if self.bulk:
            config.range_check_many(layouter, self.wide, NUM_WORDS, True)
            before = len(layouter.regions)
            config.short_range_check_many(layouter, self.four, 4)
            config.short_range_check_many(layouter, self.five, 5)
        else:
            for v in self.wide:
                config.witness_check(layouter, v, NUM_WORDS, True)
            before = len(layouter.regions)
            for bits, values in ((4, self.four), (5, self.five)):
                for v in values:
                    config.witness_short_check(layouter, v, bits)
        self.short_rows = sum(rows for _, rows in layouter.shapes[before:])


def rows_needed(count: int, lookup: str) -> int:
    short = 1 if lookup == "4_5b" else 3
    return max(count * (NUM_WORDS + 1) + 2 * count * short, TABLE_ROWS[lookup])


def k_for(count: int, lookup: str) -> int:
    k = 11
    while (1 << k) - 16 < rows_needed(count, lookup):                         # the last rows of the domain are the blinding rows
        k += 1
    return k


def witness(count: int, seed: int):
    rng = random.Random(seed)
    return ([rng.getrandbits(130) for _ in range(count)], [rng.getrandbits(4) for _ in range(count)],
            [rng.getrandbits(5) for _ in range(count)])


def prove(params, circuit: RangeCheckCircuit):
    """keygen (the circuit without its witness) and create_proof -> (pk, proof bytes, seconds of each)."""
    import halo2_amd as h
    from circuit_api import make_rng
    from halo2_amd.transcript import Blake2bWrite
    t0 = time.perf_counter()
    pk = h.keygen_pk(params, circuit)
    t1 = time.perf_counter()
    transcript = Blake2bWrite(params.curve)
    h.create_proof(params, pk, [circuit], [[]], make_rng(), transcript)
    proof = transcript.finalize()
    return pk, proof, t1 - t0, time.perf_counter() - t1


def main(argv=None) -> bool:
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=2048)
    ap.add_argument("--lookup", choices=sorted(LOOKUPS), default="4_5b")
    ap.add_argument("--loop", action="store_true", help="assign cell by cell instead of through the bulk path")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args(argv)
    import halo2_amd as h
    from halo2_amd.dev import MockProver
    from halo2_amd.verifier import verify_proof
    k = k_for(args.count, args.lookup)
    wide, four, five = witness(args.count, args.seed)
    circuit = RangeCheckCircuit(wide, four, five, args.lookup, bulk=not args.loop)
    mock = MockProver.run_circuit(k, circuit, [], h.FP).verify()
    short_rows = circuit.short_rows
    # one value too wide: the MockProver names the rows
    bad = RangeCheckCircuit(wide, [16] + four[1:], five, args.lookup, bulk=not args.loop)
    caught = MockProver.run_circuit(k, bad, [], h.FP).verify()
    params = h.Params.new(h.VESTA, k)
    pk, proof, keygen_s, prove_s = prove(params, circuit)
    ok = verify_proof(params, pk.vk, [], proof)
    flipped = bytearray(proof)
    flipped[100] ^= 1
    wrong = verify_proof(params, pk.vk, [], bytes(flipped))
    params.close()
    other = "plain" if args.lookup == "4_5b" else "4_5b"
    per = {"4_5b": 1, "plain": 3}
    print(f"{args.count} values to 130 bits and {args.count} each to 4 and to 5 bits over the {args.lookup} lookup, k = {k}: "
          f"MockProver {'satisfied' if not mock else mock[:3]}; 16 in place of a 4-bit value: {len(caught)} failure(s)")
    print(f"the 4- and 5-bit checks took {short_rows} rows ({per[args.lookup]} each); over the {other} lookup they take "
          f"{2 * args.count * per[other]} ({per[other]} each)")
    print(f"keygen {keygen_s:.3f} s, create_proof {prove_s:.3f} s ({len(proof)} bytes): {'accepted' if ok else 'REJECTED'}; "
          f"one byte flipped: {'ACCEPTED' if wrong else 'rejected'}")
    return bool(ok and not wrong and not mock and caught and short_rows == 2 * args.count * per[args.lookup])


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
