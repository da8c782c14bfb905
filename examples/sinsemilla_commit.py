#!/usr/bin/env python3
"""Note-style commitments in a circuit: prove knowledge of 500-bit messages m_i and blinding scalars r_i with
cm_i = SinsemillaHashToPoint(D || "-M", m_i) + [r_i] GroupHash(D || "-r", "") for public commitments cm_i -- SinsemillaCommit (Zcash
protocol specification 5.4.8.4), the shape of Orchard's note commitment.

`halo2_amd.sinsemilla.CommitDomain` derives Q and R, builds R's window tables on the device and computes the public commitments in
one launch, hash and blinding product fused (halo2_amd/csrc/sinsemilla_commit.hip).  `CommitManyCircuit` witnesses every message as two
pieces of 25 words and lays all the commitments out through `CommitDomain.commit_many`: one bulk region of fixed-base products, one of
hashes, one of complete additions, their advice columns from the device's trace kernels.  The circuit is mock-proved, proved and
verified on an MI355X; bench/tools/sinsemilla_commit_time.py fills a larger one.

    python examples/sinsemilla_commit.py [--count 4] [--seed 1] [--domain z.cash:Orchard-NoteCommit]
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
from halo2_amd.gadgets.ecc import EccChip, FixedPoints  # noqa: E402
from halo2_amd.gadgets.sinsemilla import CommitDomain, SinsemillaChip  # noqa: E402
from halo2_amd.gadgets.utilities import LookupRangeCheckConfig  # noqa: E402

MESSAGE_BITS, PIECE_BITS = 500, 250


class CommitManyCircuit(Circuit):
    """messages: integers of 500 bits; scalars: integers below the group's order; domain: a gadget `CommitDomains`; the commitments'
    coordinates are the public inputs x_0, y_0, x_1, y_1, ...  witness=False lays the same circuit out for keygen."""

    def __init__(self, messages, scalars, domain, witness=True):
        self.messages, self.scalars, self.domain, self.witness, self.many = messages, scalars, domain, witness, None

    def without_witnesses(self):
        return CommitManyCircuit(self.messages, self.scalars, self.domain, witness=False)

    def configure(self, meta):
        """ten advice columns: the ECC chip on all of them, the Sinsemilla chip on the upper five, the range check on the last"""
        advices = [meta.advice_column() for _ in range(10)]
        constants = meta.fixed_column()
        meta.enable_constant(constants)
        table_idx = meta.lookup_table_column()
        lagrange_coeffs = [meta.fixed_column() for _ in range(8)]
        lookup = (table_idx, meta.lookup_table_column(), meta.lookup_table_column())
        range_check = LookupRangeCheckConfig.configure(meta, advices[9], table_idx)
        ecc_config = EccChip.configure(meta, advices, lagrange_coeffs, range_check, fixed_bases=FixedPoints(full_width=("R",)))
        sinsemilla_config = SinsemillaChip.configure(meta, advices[5:], advices[7], lagrange_coeffs[0], lookup, range_check)
        self.instance = meta.instance_column()
        meta.enable_equality(self.instance)
        return ecc_config, sinsemilla_config

    def synthesize(self, config, layouter) -> None:
        ecc_config, sinsemilla_config = config
        SinsemillaChip.load(sinsemilla_config, layouter)
        chip = SinsemillaChip(sinsemilla_config)
        domain = CommitDomain(chip, EccChip(ecc_config), self.domain)
        mask = (1 << PIECE_BITS) - 1
        pieces = [[chip.witness_message_piece(layouter, (m >> (PIECE_BITS * k)) & mask if self.witness else None, 25) for k in range(2)]
                  for m in self.messages]
        self.many = domain.commit_many(layouter, pieces, [25, 25], [k if self.witness else None for k in self.scalars])
        for i in range(len(self.messages)):
            layouter.constrain_instance(self.many.result_x(i), self.instance, 2 * i)
            layouter.constrain_instance(self.many.result_y(i), self.instance, 2 * i + 1)


def words_of(messages):
    """(n, 50) 10-bit words, low bits first"""
    import numpy as np
    return np.array([[(m >> (10 * j)) & 1023 for j in range(MESSAGE_BITS // 10)] for m in messages], dtype=np.uint16).reshape(len(messages), 50)


def rows_needed(count: int) -> int:
    """the bulk regions sit one under the other: 85 + 2 rows of the product, 51 of the hash, 2 of the addition, 2 of the pieces"""
    return max(1 << 10, (85 + 2 + 51 + 2 + 2) * count) + 16


def main(argv=None) -> bool:
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--domain", default="z.cash:Orchard-NoteCommit")
    args = ap.parse_args(argv)
    import halo2_amd as h
    from circuit_api import make_rng
    from halo2_amd import fields, sinsemilla
    from halo2_amd.dev import MockProver
    from halo2_amd.gadgets.sinsemilla import CommitDomains
    from halo2_amd.transcript import Blake2bWrite
    from halo2_amd.verifier import verify_proof
    p, q = fields.MODULUS[h.FP], fields.MODULUS[h.FQ]
    t0 = time.perf_counter()
    primitive = sinsemilla.CommitDomain(args.domain)
    domain = CommitDomains.of(primitive)
    t_tables = time.perf_counter() - t0
    rng = random.Random(args.seed)
    messages = [rng.getrandbits(MESSAGE_BITS) for _ in range(args.count)]
    scalars = [rng.randrange(q) for _ in range(args.count)]
    # the public inputs outside the circuit: one fused launch
    points = primitive.commit(words_of(messages), fields.to_limbs(scalars, h.FQ, montgomery=False).reshape(-1, 4))
    commitments = fields.from_limbs(points.reshape(-1, 4), h.FP)
    k = max(11, (rows_needed(args.count) - 1).bit_length())
    circuit = CommitManyCircuit(messages, scalars, domain)
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
    print(f"domain {args.domain!r}: Q, R and R's tables (85 windows) in {t_tables:.3f} s; {args.count} commitments of {MESSAGE_BITS} bits, "
          f"k = {k}: MockProver {'satisfied' if not mock else mock[:3]}; keygen {t1 - t0:.3f} s, create_proof {t2 - t1:.3f} s "
          f"({len(proof)} bytes)")
    print(f"the device's commitments: {'accepted' if ok else 'REJECTED'}; one public input changed: {'ACCEPTED' if wrong else 'rejected'}")
    return bool(ok and not wrong and not mock)


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
