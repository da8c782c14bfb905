#!/usr/bin/env python3
"""Value commitments in a circuit: prove knowledge of values v_i (64 bits and a sign) and blinding scalars r_i with
cm_i = [v_i]V + [r_i]R for public commitments cm_i and two fixed bases V and R, the shape of Orchard's value commitment.

The bases' tables -- the window table, the Lagrange coefficients, z and u -- are built on the device (`halo2_amd.ecc.FixedBase`: the
search for z runs there), 22 windows for V and 85 for R.  `ValueCommitCircuit` multiplies through the chip's `mul_fixed_short` and
`mul_fixed` and adds with `add`, instruction for instruction what a circuit over the reference's chip does
(halo2_gadgets/src/ecc/chip/mul_fixed/{short,full_width}.rs).  The commitments outside the circuit come from a two-term multiexp each.
The circuit is mock-proved, proved and verified on an MI355X at k = 11.

`EccFixedMulCircuit` beside it is the bulk form of the blinding half alone: `count` products [r_i]R through `EccChip.mul_fixed_many`,
one region of 85 rows per product whose six advice columns come from the device trace kernel (halo2_amd/csrc/ecc_fixed.hip) and whose
fixed columns are the tables tiled; bench/tools/ecc_fixed_time.py fills a k = 16 circuit with it.

    python examples/ecc_fixed_mul.py [--count 4] [--seed 1]
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
from halo2_amd.gadgets.ecc import EccChip, FixedPoint, FixedPoints, FixedPointShort, ScalarFixed, ScalarFixedShort  # noqa: E402
from halo2_amd.gadgets.utilities import LookupRangeCheckConfig, load_private  # noqa: E402


def configure(circuit, meta):
    """the reference's test configuration (ecc.rs:783-812) with an instance column: ten advice columns, the table column, eight
    Lagrange columns, the constants in a fixed column of their own"""
    advices = [meta.advice_column() for _ in range(10)]
    lookup_table = meta.lookup_table_column()
    lagrange_coeffs = [meta.fixed_column() for _ in range(8)]
    constants = meta.fixed_column()
    meta.enable_constant(constants)
    range_check = LookupRangeCheckConfig.configure(meta, advices[9], lookup_table)
    config = EccChip.configure(meta, advices, lagrange_coeffs, range_check, fixed_bases=FixedPoints(full_width=("R",), short=("V",)))
    circuit.instance = meta.instance_column()
    meta.enable_equality(circuit.instance)
    return config


class ValueCommitCircuit(Circuit):
    """notes: (magnitude below 2^64, sign 1 or -1, r below the group's order); tables_v, tables_r: the `FixedBaseTables` of V (22
    windows) and R (85); the commitments' coordinates are the public inputs x_0, y_0, x_1, y_1, ..."""

    def __init__(self, notes, tables_v, tables_r, witness=True):
        self.notes, self.tables_v, self.tables_r, self.witness = notes, tables_v, tables_r, witness

    def without_witnesses(self):
        return ValueCommitCircuit(self.notes, self.tables_v, self.tables_r, witness=False)

    def configure(self, meta):
        return configure(self, meta)

    def synthesize(self, config, layouter) -> None:
        config.lookup_config.load_range_check_table(layouter)
        chip = EccChip(config)
        p = config.add.modulus
        v_base, r_base = FixedPointShort.from_inner(chip, self.tables_v), FixedPoint.from_inner(chip, self.tables_r)
        for i, (magnitude, sign, r) in enumerate(self.notes):
            magnitude, sign, r = (magnitude, sign % p, r) if self.witness else (None, None, None)
            cells = (load_private(layouter, config.advices[0], magnitude), load_private(layouter, config.advices[0], sign))
            value_point, _ = v_base.mul(layouter, ScalarFixedShort.new(chip, layouter, cells))
            blind_point, _ = r_base.mul(layouter, ScalarFixed.new(chip, layouter, r))
            cm = value_point.add(layouter, blind_point).inner()
            layouter.constrain_instance(cm.x().cell(), self.instance, 2 * i)
            layouter.constrain_instance(cm.y().cell(), self.instance, 2 * i + 1)


class EccFixedMulCircuit(Circuit):
    """scalars: integers below the group's order; tables: the base's `FixedBaseTables`; the products' coordinates are the public
    inputs x_0, y_0, x_1, y_1, ...  witness=False lays the same circuit out for keygen."""

    def __init__(self, scalars, tables, witness=True):
        self.scalars, self.tables, self.witness, self.many = scalars, tables, witness, None

    def without_witnesses(self):
        return EccFixedMulCircuit(self.scalars, self.tables, witness=False)

    def configure(self, meta):
        return configure(self, meta)

    def synthesize(self, config, layouter) -> None:
        config.lookup_config.load_range_check_table(layouter)
        chip = EccChip(config)
        self.many = chip.mul_fixed_many(layouter, self.tables, [k if self.witness else None for k in self.scalars])
        for i in range(len(self.scalars)):
            layouter.constrain_instance(self.many.result_x(i), self.instance, 2 * i)
            layouter.constrain_instance(self.many.result_y(i), self.instance, 2 * i + 1)


def fixed_base(name: bytes, num_windows: int):
    """a point nobody knows the logarithm of, and its tables from the device"""
    import numpy as np
    import halo2_amd as h
    from halo2_amd import ecc
    from halo2_amd.gadgets.ecc import FixedBaseTables
    point = np.asarray(h.hash_to_curve(h.PALLAS, "halo2_amd:ecc_fixed_mul example", [name])).reshape(8)
    return FixedBaseTables.of(ecc.FixedBase(point, num_windows))


def main(argv=None) -> bool:
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args(argv)
    import numpy as np
    import halo2_amd as h
    from circuit_api import make_rng
    from halo2_amd import ecc, fields
    from halo2_amd.dev import MockProver
    from halo2_amd.transcript import Blake2bWrite
    from halo2_amd.verifier import verify_proof
    p, q = fields.MODULUS[h.FP], fields.MODULUS[h.FQ]
    t0 = time.perf_counter()
    tables_v, tables_r = fixed_base(b"V", ecc.NUM_WINDOWS_SHORT), fixed_base(b"R", ecc.NUM_WINDOWS)
    t_tables = time.perf_counter() - t0
    rng = random.Random(args.seed)
    notes = [(rng.randrange(1 << 64), rng.choice((1, -1)), rng.randrange(q)) for _ in range(args.count)]
    # the public inputs outside the circuit: v V + r R as a multiexp of two terms
    bases = fields.to_limbs(list(tables_v.generator + tables_r.generator), h.FP).reshape(2, 8)
    commitments = []
    for magnitude, sign, r in notes:
        cm = h.best_multiexp(fields.to_limbs([sign * magnitude % q, r], h.FQ), bases, h.PALLAS, affine=True)
        commitments += fields.from_limbs(np.asarray(cm).reshape(2, 4), h.FP)
    k = 11
    circuit = ValueCommitCircuit(notes, tables_v, tables_r)
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
    changed[0] = (changed[0] + 1) % p
    wrong = verify_proof(params, pk.vk, [changed], proof)
    params.close()
    print(f"tables of V (22 windows) and R (85 windows) in {t_tables:.3f} s (largest z {max(tables_v.z + tables_r.z)}); {args.count} "
          f"commitments, k = {k}: MockProver {'satisfied' if not mock else mock[:3]}; keygen {t1 - t0:.3f} s, create_proof {t2 - t1:.3f} s "
          f"({len(proof)} bytes)")
    print(f"the multiexp's commitments: {'accepted' if ok else 'REJECTED'}; one public input changed: {'ACCEPTED' if wrong else 'rejected'}")
    return bool(ok and not wrong and not mock)


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
