#!/usr/bin/env python3
"""Many Sinsemilla Merkle paths in one circuit: prove knowledge of 16 leaves and their 32 siblings each under 16 public roots, the way a
batch of note-commitment-tree openings is proved.

The columns, gates and lookups are those of `examples/sinsemilla_merkle.py` (the reference's `MyMerkleCircuit`: two Sinsemilla chips, two
Merkle chips and a lookup range check over ten advice columns) plus one instance column for the roots.  What differs is the synthesis:
`MerklePaths.calculate_roots` walks all paths on the device in one launch and lays layers 0-15 of every path out in bulk regions of the
first chip, layers 16-31 in the second, each region's columns written whole from the device.  The circuit is mock-proved, proved and
verified on an MI355X.

    python examples/sinsemilla_merkle_many.py [--paths 16] [--depth 32]
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
from halo2_amd.gadgets.sinsemilla import MerkleChip, MerklePath, MerklePaths, SinsemillaChip  # noqa: E402
from halo2_amd.gadgets.utilities import LookupRangeCheck4_5BConfig, LookupRangeCheckConfig  # noqa: E402

DOMAIN = "MerkleCRH-M"                    # the reference's TestHashDomain
HASH_ROWS = 53                            # 52 words and the final row


class MerklePathsCircuit(Circuit):
    """leaves, positions, paths: n integers, n integers below 2^32, n lists of `depth` siblings from the leaf up; None for keygen.
    chips: 1 or 2 MerkleChips share the layers; tagged: the range check is LookupRangeCheck4_5BConfig; public: the roots are
    constrained to rows 0 .. n - 1 of an instance column; bulk=False builds the same circuit from n `MerklePath.calculate_root`
    calls.  q, table: the domain's Q and the generator table where the caller supplies them."""

    def __init__(self, n, depth, leaves=None, positions=None, paths=None, chips=2, tagged=False, public=False, bulk=True, q=None, table=None):
        self.n, self.depth, self.leaves, self.positions, self.paths = n, depth, leaves, positions, paths
        self.chips, self.tagged, self.public, self.bulk, self.q, self.table = chips, tagged, public, bulk, q, table
        self.roots = None

    def without_witnesses(self):
        return type(self)(self.n, self.depth, chips=self.chips, tagged=self.tagged, public=self.public, bulk=self.bulk, q=self.q, table=self.table)

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
        range_check = (LookupRangeCheck4_5BConfig if self.tagged else LookupRangeCheckConfig).configure(meta, advices[9], lookup[0])
        sinsemilla_1 = SinsemillaChip.configure(meta, advices[5:], advices[7], fixed_y_q_1, lookup, range_check, table=self.table)
        config_1 = MerkleChip.configure(meta, sinsemilla_1)
        sinsemilla_2 = SinsemillaChip.configure(meta, advices[:5], advices[2], fixed_y_q_2, lookup, range_check, table=self.table)
        config_2 = MerkleChip.configure(meta, sinsemilla_2)
        instance = None
        if self.public:
            instance = meta.instance_column()
            meta.enable_equality(instance)
        return config_1, config_2, instance

    def synthesize(self, config, layouter) -> None:
        SinsemillaChip.load(config[0].sinsemilla_config, layouter)            # the generator table, shared by both chips
        chips = [MerkleChip(config[0]), MerkleChip(config[1])][:self.chips]
        known = self.leaves is not None
        leaves = [chips[0].load_private(layouter, config[0].cond_swap_config.a, self.leaves[i] if known else None) for i in range(self.n)]
        if self.bulk:
            self.roots = MerklePaths(chips, self.domain_q(), self.positions, self.paths, self.depth).calculate_roots(layouter, leaves)
        else:
            self.roots = [MerklePath(chips, self.domain_q(), self.positions[i] if known else None, self.paths[i] if known else None,
                                     self.depth).calculate_root(layouter, leaves[i]) for i in range(self.n)]
        if self.public:
            for i, root in enumerate(self.roots):
                layouter.constrain_instance(root.cell(), config[2], i)


def planned_rows(n: int, depth: int, chips: int = 2, tagged: bool = False) -> int:
    """The rows the fullest advice column takes: the range-check column is also the first chip's last column, so it carries that chip's
    swaps, hashes and decomposition rows and the range checks of EVERY chip (two per item, three rows each, one with the tag column);
    the first chip's swap column also carries the n leaves."""
    per_chip = -(-depth // chips)
    spans = [min(depth, (at + 1) * per_chip) - at * per_chip for at in range(chips) if at * per_chip < depth]
    first = n * spans[0]
    checks = 2 * (1 if tagged else 3) * n * depth
    return max(n + first * (1 + HASH_ROWS + 2), first * (1 + HASH_ROWS + 2) + checks)


def smallest_k(rows: int, blinding: int = 6) -> int:
    k = 11                                                                    # the 1024-row generator table
    while (1 << k) - blinding < rows:
        k += 1
    return k


def roots_outside_the_circuit(leaves, positions, paths) -> list:
    """The same walks through `sinsemilla.merkle_paths`, outside any circuit"""
    import numpy as np
    from halo2_amd import FP, fields, sinsemilla
    n, depth = len(leaves), len(paths[0])
    nodes = sinsemilla.merkle_paths(fields.to_limbs(leaves, FP), np.array(positions, dtype=np.uint32),
                                    fields.to_limbs([s for p in paths for s in p], FP).reshape(n, depth, 4), sinsemilla.HashDomain(DOMAIN))
    return fields.from_limbs(np.ascontiguousarray(nodes[:, depth]), FP)


def witness(n: int, depth: int, seed: int = 1):
    import halo2_amd as h
    from halo2_amd import fields
    p = fields.MODULUS[h.FP]
    rng = random.Random(seed)
    return ([rng.randrange(p) for _ in range(n)], [rng.getrandbits(32) for _ in range(n)],
            [[rng.randrange(p) for _ in range(depth)] for _ in range(n)])


def main(argv=None) -> bool:
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=16)
    ap.add_argument("--depth", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args(argv)
    import halo2_amd as h
    from circuit_api import make_rng
    from halo2_amd import fields
    from halo2_amd.dev import MockProver
    from halo2_amd.transcript import Blake2bWrite
    from halo2_amd.verifier import verify_proof
    n, depth = args.paths, args.depth
    leaves, positions, paths = witness(n, depth, args.seed)
    rows = planned_rows(n, depth)
    k = smallest_k(rows)
    print(f"{n} paths of {depth} layers over two MerkleChips: {rows} rows planned in the fullest column, k = {k}")
    roots = roots_outside_the_circuit(leaves, positions, paths)
    instance = list(roots)
    circuit = MerklePathsCircuit(n, depth, leaves, positions, paths, public=True)
    t0 = time.perf_counter()
    mock = MockProver.run_circuit(k, circuit, [instance], h.FP).verify()
    t1 = time.perf_counter()
    p = fields.MODULUS[h.FP]
    inside = [root.value().inner.evaluate(p) for root in circuit.roots]
    params = h.Params.new(h.VESTA, k)
    pk = h.keygen_pk(params, circuit)
    t2 = time.perf_counter()
    transcript = Blake2bWrite(params.curve)
    h.create_proof(params, pk, [circuit], [[instance]], make_rng(), transcript)
    proof = transcript.finalize()
    t3 = time.perf_counter()
    ok = verify_proof(params, pk.vk, [instance], proof)
    wrong_roots = list(roots)
    wrong_roots[n // 2] = (wrong_roots[n // 2] + 1) % p
    wrong = verify_proof(params, pk.vk, [wrong_roots], proof)
    params.close()
    print(f"MockProver {'satisfied' if not mock else mock[:3]} ({t1 - t0:.3f} s); keygen {t2 - t1:.3f} s, create_proof {t3 - t2:.3f} s "
          f"({len(proof)} bytes)")
    print(f"the {n} roots {'equal' if inside == roots else 'DIFFER FROM'} the walks outside the circuit: {'accepted' if ok else 'REJECTED'}; "
          f"one wrong root: {'ACCEPTED' if wrong else 'rejected'}")
    return bool(ok and not wrong and not mock and inside == roots)


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
