#!/usr/bin/env python3
"""A wide Poseidon sponge in a circuit: the reference benchmark's HashCircuit<MySpec<9, 8>, 9, 8, 8>
(halo2_gadgets/benches/poseidon.rs) -- width 9, rate 8, 8 full and 56 partial rounds, a message of eight elements hashed by one
permutation, the digest public.

The specification is `halo2_amd.poseidon_spec.Spec(field, 9, 8)`: its round constants and MDS matrix come from the Grain procedure,
`Pow5Chip.configure(..., spec=spec)` builds the gates of that width, and `spec.hash` computes the public digest on the device.  Nine
state columns and the partial S-box, 42 rows: k = 7.  The circuit is mock-proved, proved and verified on an MI355X.

    python examples/poseidon_wide.py [--width 9] [--k 7]
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
from halo2_amd.gadgets.poseidon import ConstantLength, Hash, Pow5Chip  # noqa: E402
from halo2_amd.poseidon_spec import Spec  # noqa: E402

FP = 0


class HashConfig:
    def __init__(self, poseidon, expected):
        self.poseidon, self.expected = poseidon, expected


class HashCircuit(Circuit):
    """message: `rate` integers, None for keygen."""

    def __init__(self, spec: Spec, message=None):
        self.spec, self.message = spec, message

    def without_witnesses(self):
        return HashCircuit(self.spec)

    def configure(self, meta) -> HashConfig:
        width = self.spec.width
        state = [meta.advice_column() for _ in range(width)]
        expected = meta.instance_column()
        meta.enable_equality(expected)
        partial_sbox = meta.advice_column()
        rc_a = [meta.fixed_column() for _ in range(width)]
        rc_b = [meta.fixed_column() for _ in range(width)]
        meta.enable_constant(rc_b[0])
        return HashConfig(Pow5Chip.configure(meta, state, partial_sbox, rc_a, rc_b, spec=self.spec), expected)

    def synthesize(self, config: HashConfig, layouter) -> None:
        chip = Pow5Chip.construct(config.poseidon)
        rate = self.spec.rate
        word = lambda i: None if self.message is None else self.message[i]
        message = layouter.assign_region("load message", lambda region: [
            region.assign_advice(config.poseidon.state[i], 0, lambda i=i: word(i)) for i in range(rate)])
        hasher = Hash.init(chip, layouter.namespace("init"), ConstantLength(rate))
        output = hasher.hash(layouter.namespace("hash"), message)
        layouter.constrain_instance(output.cell(), config.expected, 0)


def public_digest(message, spec: Spec | None = None) -> int:
    """The digest outside the circuit: one `Spec.hash` launch."""
    import numpy as np
    from halo2_amd import fields
    spec = Spec(FP, 9, 8) if spec is None else spec
    limbs = fields.to_limbs([int(v) for v in message], spec.field, True).reshape(1, len(message), 4)
    return fields.from_limbs(np.ascontiguousarray(spec.hash(limbs)).reshape(-1, 4), spec.field, True)[0]


def main(argv=None) -> bool:
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=9)
    ap.add_argument("--k", type=int, default=7)
    args = ap.parse_args(argv)
    import halo2_amd as h
    from halo2_amd.dev import MockProver
    from halo2_amd.transcript import Blake2bWrite
    from halo2_amd.verifier import verify_proof
    spec = Spec(FP, args.width, args.width - 1)
    message = [(0x9E3779B97F4A7C15 * (i + 1)) ** 3 % spec.modulus for i in range(spec.rate)]
    digest = public_digest(message, spec)
    assert digest == spec.hash_ints(message), "the device and the host disagree"
    circuit = HashCircuit(spec, message)
    mock = MockProver.run_circuit(args.k, circuit, [[digest]], FP).verify()
    mock_wrong = MockProver.run_circuit(args.k, circuit, [[(digest + 1) % spec.modulus]], FP).verify()
    params = h.Params.new(h.VESTA, args.k)
    t0 = time.perf_counter()
    pk = h.keygen_pk(params, circuit)
    t1 = time.perf_counter()
    transcript = Blake2bWrite(params.curve)
    h.create_proof(params, pk, [circuit], [[[digest]]], make_rng(), transcript)
    proof = transcript.finalize()
    t2 = time.perf_counter()
    ok = verify_proof(params, pk.vk, [[digest]], proof)
    wrong = verify_proof(params, pk.vk, [[(digest + 1) % spec.modulus]], proof)
    params.close()
    print(f"{spec!r}, ConstantLength<{spec.rate}>, k = {args.k}: MockProver {'satisfied' if not mock else mock[:3]}; "
          f"keygen {t1 - t0:.3f} s, create_proof {t2 - t1:.3f} s ({len(proof)} bytes)")
    print(f"digest = {digest:#066x}: {'accepted' if ok else 'REJECTED'}; digest + 1: {'ACCEPTED' if wrong else 'rejected'}")
    return bool(ok and not wrong and not mock and mock_wrong)


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
