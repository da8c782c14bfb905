#!/usr/bin/env python3
"""N value commitments in bulk: prove knowledge of values v_i (64 bits and a sign) and blinding scalars rcv_i with
cv_i = [v_i]V + [rcv_i]R for N public commitments cv_i, the value commitment of an Orchard action N times over.

Where examples/ecc_fixed_mul.py lays each commitment out cell by cell, `ValueCommitmentsCircuit` lays all N out in five regions:
`EccChip.mul_fixed_short_many` (the running sums and window points of all [v_i]V from halo2_amd/csrc/ecc_fixed_sum.hip, then their
closing additions with the sign's gate), `EccChip.mul_fixed_many` (all [rcv_i]R from halo2_amd/csrc/ecc_fixed.hip, then their closing
additions) and `EccChip.add_many` (the N sums from `ecc.add_trace`).  Per commitment the gates, cells and equality constraints are those
of the loop; bulk=False is that loop, on the same inputs, for bench/tools/ecc_fixed_sum_time.py to measure beside it.  The circuit is
mock-proved, proved and verified on an MI355X at k = 13, and the proof is rejected against one wrong commitment.

    python examples/value_commitment.py [--count 64] [--seed 1]
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

from ecc_fixed_mul import ValueCommitCircuit, configure, fixed_base  # noqa: E402
from halo2_amd.circuit import Circuit  # noqa: E402
from halo2_amd.gadgets.ecc import EccChip  # noqa: E402
from halo2_amd.gadgets.utilities import load_private  # noqa: E402


class ValueCommitmentsCircuit(Circuit):
    """notes: (magnitude below 2^64, sign 1 or -1, rcv below the group's order); tables_v, tables_r: the `FixedBaseTables` of V (22
    windows) and R (85); the commitments' coordinates are the public inputs x_0, y_0, x_1, y_1, ...  bulk=False: one `mul_fixed_short`,
    `mul_fixed` and `add` per note.  witness=False lays the same circuit out for keygen."""

    def __init__(self, notes, tables_v, tables_r, witness=True, bulk=True):
        self.notes, self.tables_v, self.tables_r, self.witness, self.bulk = notes, tables_v, tables_r, witness, bulk

    def without_witnesses(self):
        return ValueCommitmentsCircuit(self.notes, self.tables_v, self.tables_r, witness=False, bulk=self.bulk)

    def configure(self, meta):
        return configure(self, meta)

    def synthesize(self, config, layouter) -> None:
        if not self.bulk:
            loop = ValueCommitCircuit(self.notes, self.tables_v, self.tables_r, self.witness)
            loop.instance = self.instance
            return loop.synthesize(config, layouter)
        from halo2_amd import ecc
        config.lookup_config.load_range_check_table(layouter)
        chip = EccChip(config)
        p, count = config.add.modulus, len(self.notes)
        v = (lambda x: x) if self.witness else (lambda x: None)
        magnitudes = [load_private(layouter, config.advices[0], v(m)) for m, _, _ in self.notes]
        signs = [load_private(layouter, config.advices[0], v(s % p)) for _, s, _ in self.notes]
        values = chip.mul_fixed_short_many(layouter, self.tables_v, magnitudes, signs)
        blinds = chip.mul_fixed_many(layouter, self.tables_r, [v(r) for _, _, r in self.notes])
        trace = None
        if values.outputs is not None:                                        # the operands are bare cells: their values are on the device
            trace = ecc.add_trace(values.outputs.reshape(count, 8), blinds.outputs.reshape(count, 8))
        sums = chip.add_many(layouter, [values.point(i) for i in range(count)],
                             [(blinds.result_x(i), blinds.result_y(i)) for i in range(count)], trace=trace)
        for i in range(count):
            layouter.constrain_instance(sums.result_x(i), self.instance, 2 * i)
            layouter.constrain_instance(sums.result_y(i), self.instance, 2 * i + 1)


def notes_and_commitments(count: int, seed: int, tables_v, tables_r):
    """`count` random notes and, outside the circuit, their commitments v V + rcv R as multiexps of two terms -> (notes, the public
    inputs x_0, y_0, ...)"""
    import numpy as np
    import halo2_amd as h
    from halo2_amd import fields
    q = fields.MODULUS[h.FQ]
    rng = random.Random(seed)
    notes = [(rng.randrange(1 << 64), rng.choice((1, -1)), rng.randrange(q)) for _ in range(count)]
    bases = fields.to_limbs(list(tables_v.generator + tables_r.generator), h.FP).reshape(2, 8)
    commitments = []
    for magnitude, sign, r in notes:
        cm = h.best_multiexp(fields.to_limbs([sign * magnitude % q, r], h.FQ), bases, h.PALLAS, affine=True)
        commitments += fields.from_limbs(np.asarray(cm).reshape(2, 4), h.FP)
    return notes, commitments


def main(argv=None) -> bool:
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=64)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args(argv)
    import halo2_amd as h
    from circuit_api import make_rng
    from halo2_amd import ecc, fields
    from halo2_amd.dev import MockProver
    from halo2_amd.transcript import Blake2bWrite
    from halo2_amd.verifier import verify_proof
    p = fields.MODULUS[h.FP]
    tables_v, tables_r = fixed_base(b"V", ecc.NUM_WINDOWS_SHORT), fixed_base(b"R", ecc.NUM_WINDOWS)
    notes, commitments = notes_and_commitments(args.count, args.seed, tables_v, tables_r)
    rows = args.count * (2 + 23 + 2 + 85 + 2 + 2)
    k = max(11, (rows + 16).bit_length())
    circuit = ValueCommitmentsCircuit(notes, tables_v, tables_r)
    mock = MockProver.run_circuit(k, circuit, [commitments], h.FP).verify()
    params = h.Params.new(h.VESTA, k)
    t0 = time.perf_counter()
    pk = h.keygen_pk(params, circuit)
    t1 = time.perf_counter()
    transcript = Blake2bWrite(params.curve)
    h.create_proof(params, pk, [circuit], [[commitments]], make_rng(), transcript)
    proof = transcript.finalize()
    t2 = time.perf_counter()
    ok = verify_proof(params, pk.vk, [commitments], proof)
    changed = list(commitments)
    changed[2 * (args.count // 2) + 1] = (changed[2 * (args.count // 2) + 1] + 1) % p
    wrong = verify_proof(params, pk.vk, [changed], proof)
    params.close()
    print(f"{args.count} value commitments in bulk, k = {k}: MockProver {'satisfied' if not mock else mock[:3]}; keygen {t1 - t0:.3f} s, "
          f"create_proof {t2 - t1:.3f} s ({len(proof)} bytes)")
    print(f"the multiexp's commitments: {'accepted' if ok else 'REJECTED'}; one commitment changed: {'ACCEPTED' if wrong else 'rejected'}")
    return bool(ok and not wrong and not mock)


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
