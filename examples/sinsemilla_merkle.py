#!/usr/bin/env python3
"""A Sinsemilla Merkle path in a circuit: prove knowledge of a leaf and its 32 siblings under a root, the way Orchard's
note-commitment tree is opened.

The circuit is the reference's `MyMerkleCircuit` (halo2_gadgets/src/sinsemilla/merkle.rs): two Sinsemilla chips, two Merkle chips
and a lookup range check side by side over ten advice columns; layers 0-15 of the path go to the first chip, 16-31 to the second.
Each layer is a conditional swap, the three message pieces of MerkleCRH(l, left, right), two 5-bit range checks, one 52-word
Sinsemilla hash and the decomposition check: 16 x 53 rows of hashing in each of the two sets of columns, k = 11.  The key it generates is the
reference's, byte for byte.  The circuit is mock-proved, proved and verified on an MI355X.

    python examples/sinsemilla_merkle.py [--pos 0xA5A55A5A]
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
from halo2_amd.gadgets.sinsemilla import MerkleChip, MerklePath, SinsemillaChip  # noqa: E402
from halo2_amd.gadgets.utilities import LookupRangeCheckConfig  # noqa: E402

MERKLE_DEPTH = 32
DOMAIN = "MerkleCRH-M"                    # the reference's TestHashDomain: CommitDomain::new("MerkleCRH").Q()


class MerkleCircuit(Circuit):
    """leaf, leaf_pos, path: integers (path: 32 of them, from the leaf up), None for keygen.  q, table: the domain's Q and the
    generator table as integers where the caller supplies them; None for the library's own, derived on the device."""

    def __init__(self, leaf=None, leaf_pos=None, path=None, q=None, table=None):
        self.leaf, self.leaf_pos, self.path, self.q, self.table = leaf, leaf_pos, path, q, table
        self.root = None

    def without_witnesses(self):
        return type(self)(q=self.q, table=self.table)

    def domain_q(self):
        if self.q is None:
            from halo2_amd import sinsemilla
            self.q = sinsemilla.q_point(DOMAIN)
        return self.q

    def configure(self, meta):
        advices = [meta.advice_column() for _ in range(10)]
        constants = meta.fixed_column()
        meta.enable_constant(constants)
        fixed_y_q_1, fixed_y_q_2 = meta.fixed_column(), meta.fixed_column()
        lookup = (meta.lookup_table_column(), meta.lookup_table_column(), meta.lookup_table_column())
        range_check = LookupRangeCheckConfig.configure(meta, advices[9], lookup[0])
        sinsemilla_1 = SinsemillaChip.configure(meta, advices[5:], advices[7], fixed_y_q_1, lookup, range_check, table=self.table)
        config_1 = MerkleChip.configure(meta, sinsemilla_1)
        sinsemilla_2 = SinsemillaChip.configure(meta, advices[:5], advices[2], fixed_y_q_2, lookup, range_check, table=self.table)
        config_2 = MerkleChip.configure(meta, sinsemilla_2)
        return config_1, config_2

    def synthesize(self, config, layouter) -> None:
        SinsemillaChip.load(config[0].sinsemilla_config, layouter)            # the generator table, shared by both chips
        chip_1, chip_2 = MerkleChip(config[0]), MerkleChip(config[1])
        leaf = chip_1.load_private(layouter, config[0].cond_swap_config.a, self.leaf)
        path = MerklePath([chip_1, chip_2], self.domain_q(), self.leaf_pos, self.path, MERKLE_DEPTH)
        self.root = path.calculate_root(layouter, leaf)


def root_outside_the_circuit(leaf: int, pos: int, path) -> int:
    """The same fold with one `sinsemilla.merkle_crh` launch per layer (l counts from the leaf, as the circuit does)."""
    import numpy as np
    from halo2_amd import FP, fields, sinsemilla
    domain = sinsemilla.HashDomain(DOMAIN)
    node = leaf
    for l, sibling in enumerate(path):                                        # noqa: E741
        left, right = (node, sibling) if pos >> l & 1 == 0 else (sibling, node)
        out = sinsemilla.merkle_crh(l, fields.to_limbs([left], FP), fields.to_limbs([right], FP), domain)
        node = fields.from_limbs(np.asarray(out), FP)[0]
    return node


def prove(params, circuit: MerkleCircuit):
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
    ap.add_argument("--pos", type=lambda s: int(s, 0), default=0xA5A55A5A)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args(argv)
    import halo2_amd as h
    from halo2_amd import fields
    from halo2_amd.dev import MockProver
    from halo2_amd.verifier import verify_proof
    p = fields.MODULUS[h.FP]
    rng = random.Random(args.seed)
    leaf, path = rng.randrange(p), [rng.randrange(p) for _ in range(MERKLE_DEPTH)]
    k = 11
    params = h.Params.new(h.VESTA, k)
    circuit = MerkleCircuit(leaf, args.pos, path)
    mock = MockProver.run_circuit(k, circuit, [], h.FP).verify()
    root = circuit.root.value().inner.evaluate(p)
    outside = root_outside_the_circuit(leaf, args.pos, path)
    pk, proof, keygen_s, prove_s = prove(params, circuit)
    ok = verify_proof(params, pk.vk, [], proof)
    flipped = bytearray(proof)
    flipped[100] ^= 1
    wrong = verify_proof(params, pk.vk, [], bytes(flipped))
    params.close()
    print(f"a path of {MERKLE_DEPTH} layers at position {args.pos:#010x}, k = {k}: MockProver {'satisfied' if not mock else mock[:3]}; "
          f"keygen {keygen_s:.3f} s, create_proof {prove_s:.3f} s ({len(proof)} bytes)")
    print(f"root = {root:#066x} ({'equals' if root == outside else 'DIFFERS FROM'} the fold outside the circuit): "
          f"{'accepted' if ok else 'REJECTED'}; one byte flipped: {'ACCEPTED' if wrong else 'rejected'}")
    return bool(ok and not wrong and not mock and root == outside)


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
