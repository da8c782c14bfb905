#!/usr/bin/env python3
"""A Merkle tree of Poseidon hashes in a circuit: prove knowledge of 64 leaves under a public root.

The 63 hashes are laid out by `Pow5Chip.hash2_many`, one call per layer of the tree (32, 16, 8, 4, 2, 1 hashes): the witness of every
layer comes from the device in one launch (`halo2_amd.poseidon.trace`), the digests of a layer feed the next without leaving the
device, children are tied to their parents with copy constraints and the root is copied to the instance column.  63 x 37 = 2331 rows
of the three state columns: k = 12.  The circuit is mock-proved, proved and verified on an MI355X.

    python examples/poseidon_merkle.py [--leaves 64] [--k 12]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from circuit_api import make_rng  # noqa: E402
from halo2_amd.circuit import Circuit  # noqa: E402
from halo2_amd.gadgets.poseidon import Pow5Chip  # noqa: E402


class MerkleConfig:
    def __init__(self, poseidon, instance):
        self.poseidon, self.instance = poseidon, instance


class MerkleCircuit(Circuit):
    """leaves: an (n, 4) array or tensor of Montgomery limbs, n a power of two; None for keygen."""

    def __init__(self, n_leaves: int, leaves=None):
        if n_leaves < 2 or n_leaves & (n_leaves - 1):
            raise ValueError("a power-of-two number of leaves, at least two")
        self.n_leaves, self.leaves = n_leaves, leaves

    def without_witnesses(self):
        return MerkleCircuit(self.n_leaves)

    @staticmethod
    def configure(meta) -> MerkleConfig:
        state = [meta.advice_column() for _ in range(3)]
        partial_sbox = meta.advice_column()
        rc_a = [meta.fixed_column() for _ in range(3)]
        rc_b = [meta.fixed_column() for _ in range(3)]
        meta.enable_constant(meta.fixed_column())                              # the capacity 2^65 of every hash
        instance = meta.instance_column()
        meta.enable_equality(instance)
        return MerkleConfig(Pow5Chip.configure(meta, state, partial_sbox, rc_a, rc_b), instance)

    def synthesize(self, config, layouter) -> None:
        chip = Pow5Chip(config.poseidon)
        nodes, below, count = self.leaves, None, self.n_leaves // 2
        while count:
            left, right = (None, None) if nodes is None else (nodes[0::2], nodes[1::2])
            layer = chip.hash2_many(layouter, count, left, right)
            if below is not None:                                              # a parent's inputs are its children's outputs
                def tie(region, layer=layer, below=below, count=count):
                    for i in range(count):
                        region.constrain_equal(layer.left_cell(i), below.output_cell(2 * i))
                        region.constrain_equal(layer.right_cell(i), below.output_cell(2 * i + 1))
                layouter.assign_region("children", tie)
            nodes, below, count = layer.digests, layer, count // 2
        layouter.constrain_instance(below.output_cell(0), config.instance, 0)


def random_leaves(n: int, seed: int = 1):
    """n field elements as device limbs (below 2^254: valid Montgomery representations)."""
    import torch
    from halo2_amd import fields
    gen = torch.Generator(device=fields.current_device())
    gen.manual_seed(seed)
    out = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 4), dtype=torch.int64, device=gen.device, generator=gen)
    out[:, 3] &= (1 << 62) - 1
    return out


def public_root(leaves, field: int) -> int:
    """The root outside the circuit: one `poseidon.hash` launch per layer."""
    import numpy as np
    from halo2_amd import fields, poseidon
    root = poseidon.merkle_root(leaves, field)
    return fields.from_limbs(root.cpu().numpy().view(np.uint64), field, True)[0]


def prove(params, circuit: MerkleCircuit):
    """keygen (the circuit without its witness) and create_proof -> (pk, proof bytes, seconds of each)."""
    import halo2_amd as h
    from halo2_amd.transcript import Blake2bWrite
    t0 = time.perf_counter()
    pk = h.keygen_pk(params, circuit)
    t1 = time.perf_counter()
    transcript = Blake2bWrite(params.curve)
    h.create_proof(params, pk, [circuit], [[[public_root(circuit.leaves, 0)]]], make_rng(), transcript)
    proof = transcript.finalize()
    return pk, proof, t1 - t0, time.perf_counter() - t1


def main(argv=None) -> bool:
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", type=int, default=64)
    ap.add_argument("--k", type=int, default=12)
    args = ap.parse_args(argv)
    import halo2_amd as h
    from halo2_amd.dev import MockProver
    from halo2_amd.verifier import verify_proof
    params = h.Params.new(h.VESTA, args.k)
    circuit = MerkleCircuit(args.leaves, random_leaves(args.leaves))
    root = public_root(circuit.leaves, h.FP)
    mock = MockProver.run_circuit(args.k, circuit, [[root]], h.FP).verify()
    mock_wrong = MockProver.run_circuit(args.k, circuit, [[root + 1]], h.FP).verify()
    pk, proof, keygen_s, prove_s = prove(params, circuit)
    ok = verify_proof(params, pk.vk, [[root]], proof)
    wrong = verify_proof(params, pk.vk, [[root + 1]], proof)
    params.close()
    print(f"{args.leaves} leaves, {args.leaves - 1} hashes, k = {args.k}: MockProver {'satisfied' if not mock else mock[:3]}; "
          f"keygen {keygen_s:.3f} s, create_proof {prove_s:.3f} s ({len(proof)} bytes)")
    print(f"root = {root:#066x}: {'accepted' if ok else 'REJECTED'}; root + 1: {'ACCEPTED' if wrong else 'rejected'}")
    return bool(ok and not wrong and not mock and mock_wrong)


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
