#!/usr/bin/env python3
"""64 variable-base scalar multiplications in one circuit: prove knowledge of 64 scalars alpha_i with [alpha_i] P_i = R_i for public
products R_i, the way an Orchard action multiplies a private point.

The circuit lays the 64 multiplications through `EccChip.mul_many`: one region of 64 x 137 rows whose ten advice columns come from the
device trace kernel (halo2_amd/csrc/ecc.hip), and the 64 overflow checks in three bulk regions; gate for gate and copy for copy the
layout of 64 calls of the reference's `mul` (halo2_gadgets/src/ecc/chip/mul.rs).  k = 14.  The circuit is mock-proved, proved and
verified on an MI355X.

    python examples/ecc_mul.py [--count 64] [--seed 1]
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
from halo2_amd.gadgets.ecc import EccChip, NonIdentityPoint  # noqa: E402
from halo2_amd.gadgets.utilities import LookupRangeCheckConfig, load_private  # noqa: E402


class EccMulCircuit(Circuit):
    """pairs: (base (x, y), alpha) integers; the products' coordinates are the public inputs x_0, y_0, x_1, y_1, ...
    witness=False lays the same circuit out for keygen."""

    def __init__(self, pairs, witness=True):
        self.pairs, self.witness, self.many = pairs, witness, None

    def without_witnesses(self):
        return EccMulCircuit(self.pairs, witness=False)

    def configure(self, meta):
        advices = [meta.advice_column() for _ in range(10)]
        lookup_table = meta.lookup_table_column()
        lagrange_coeffs = [meta.fixed_column() for _ in range(8)]
        meta.enable_constant(lagrange_coeffs[0])
        range_check = LookupRangeCheckConfig.configure(meta, advices[9], lookup_table)
        config = EccChip.configure(meta, advices, lagrange_coeffs, range_check)
        self.instance = meta.instance_column()
        meta.enable_equality(self.instance)
        return config

    def synthesize(self, config, layouter) -> None:
        config.lookup_config.load_range_check_table(layouter)
        chip = EccChip(config)
        bases = [NonIdentityPoint.new(chip, layouter, b if self.witness else None).inner() for b, _ in self.pairs]
        alphas = [load_private(layouter, config.advices[0], a if self.witness else None) for _, a in self.pairs]
        self.many = chip.mul_many(layouter, bases, alphas)
        for i in range(len(self.pairs)):
            layouter.constrain_instance(self.many.result_x(i), self.instance, 2 * i)
            layouter.constrain_instance(self.many.result_y(i), self.instance, 2 * i + 1)


def random_pairs(count: int, seed: int):
    """`count` points of the curve (multiples of a hashed point, on the device) and as many scalars"""
    import numpy as np
    import halo2_amd as h
    from halo2_amd import ecc, fields
    p, q = fields.MODULUS[h.FP], fields.MODULUS[h.FQ]
    rng = random.Random(seed)
    g = np.asarray(h.hash_to_curve(h.PALLAS, "halo2_amd:ecc_mul example", [b"base"])).reshape(1, 8)
    ks = [rng.randrange(1, q) for _ in range(count)]
    pts = fields.from_limbs(ecc.mul(np.repeat(g, count, axis=0), fields.to_limbs(ks, h.FQ, montgomery=False)).reshape(-1, 4), h.FP)
    return [((pts[2 * i], pts[2 * i + 1]), rng.randrange(p)) for i in range(count)]


def main(argv=None) -> bool:
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=64)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args(argv)
    import numpy as np
    import halo2_amd as h
    from circuit_api import make_rng
    from halo2_amd import ecc, fields
    from halo2_amd.dev import MockProver
    from halo2_amd.transcript import Blake2bWrite
    from halo2_amd.verifier import verify_proof
    p = fields.MODULUS[h.FP]
    pairs = random_pairs(args.count, args.seed)
    # the public inputs, by the product kernel outside the circuit: [alpha]P with alpha taken as an integer below 2^255
    bases = fields.to_limbs([c for b, _ in pairs for c in b], h.FP).reshape(-1, 8)
    products = fields.from_limbs(ecc.mul(bases, fields.to_limbs([a for _, a in pairs], h.FP, montgomery=False)).reshape(-1, 4), h.FP)
    k = 14
    circuit = EccMulCircuit(pairs)
    mock = MockProver.run_circuit(k, circuit, [products], h.FP).verify()
    inside = fields.from_limbs(circuit.many.outputs.cpu().numpy().view(np.uint64).reshape(-1, 4), h.FP)
    params = h.Params.new(h.VESTA, k)
    t0 = time.perf_counter()
    pk = h.keygen_pk(params, circuit)
    t1 = time.perf_counter()
    transcript = Blake2bWrite(params.curve)
    h.create_proof(params, pk, [circuit], [[products]], make_rng(), transcript)
    proof = transcript.finalize()
    t2 = time.perf_counter()
    ok = verify_proof(params, pk.vk, [products], proof)
    changed = list(products)
    changed[0] = (changed[0] + 1) % p
    wrong = verify_proof(params, pk.vk, [changed], proof)
    params.close()
    print(f"{args.count} multiplications, k = {k}: MockProver {'satisfied' if not mock else mock[:3]}; keygen {t1 - t0:.3f} s, "
          f"create_proof {t2 - t1:.3f} s ({len(proof)} bytes)")
    print(f"the products {'equal' if inside == products else 'DIFFER FROM'} ecc.mul's outside the circuit: "
          f"{'accepted' if ok else 'REJECTED'}; one public input changed: {'ACCEPTED' if wrong else 'rejected'}")
    return bool(ok and not wrong and not mock and inside == products)


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
