"""Shared by test_poseidon_host.py and test_gpu_poseidon.py: the fixtures, host restatements of the sponge and of the Pow5 chip's
witness over `oracle.pasta.poseidon_permute` and Python integers, the three test circuits of halo2_gadgets/src/poseidon/pow5.rs
(:621-716 MyPermuteCircuit, :727-816 MyHashCircuit) against `halo2_amd.circuit`, the bulk circuits, and a host evaluation of a
synthesized circuit's gates and copy constraints."""
import json
import os

import numpy as np

from halo2_amd import circuit as front
from halo2_amd import fields
from halo2_amd.circuit import Circuit
from halo2_amd.gadgets.poseidon import ConstantLength, Hash, Pow5Chip
from oracle import pasta as o

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KAT = json.load(open(os.path.join(GOLDEN, "poseidon_kat.json")))
HASH_KAT = json.load(open(os.path.join(GOLDEN, "poseidon_hash_kat.json")))
FP, FQ = 0, 1
NAME = {FP: "fp", FQ: "fq"}
MOD = {FP: o.P, FQ: o.Q}
WIDTH, RATE, ROWS = 3, 2, 37


def kat_constants(field):
    d = KAT[NAME[field]]
    return [[int(x, 16) for x in r] for r in d["round_constants"]], [[int(x, 16) for x in r] for r in d["mds"]]


def permute_ints(state, field):
    rcs, mds = kat_constants(field)
    return o.poseidon_permute(state, mds, rcs, MOD[field])


def hash_ints(message, field):
    """Hash<_, P128Pow5T3, ConstantLength<L>, 3, 2> (halo2_poseidon/src/lib.rs:197-397) restated: capacity L * 2^64, two words absorbed
    per permutation, zero padding, word 0 of the last state."""
    m = MOD[field]
    state = [0, 0, len(message) << 64]
    padded = list(message) + [0] * (-len(message) % RATE)
    for at in range(0, len(padded), RATE):
        state = [(state[0] + padded[at]) % m, (state[1] + padded[at + 1]) % m, state[2]]
        state = permute_ints(state, field)
    return state[0]


def merkle_root_ints(leaves, field):
    layer = list(leaves)
    while len(layer) > 1:
        layer = [hash_ints(layer[i:i + 2], field) for i in range(0, len(layer), 2)]
    return layer[0]


def trace_ints(state, field):
    """The Pow5 chip's 37 rows of one permutation, round by round: ([state0], [state1], [state2], [partial_sbox])."""
    m = MOD[field]
    rcs, mds = kat_constants(field)
    mul = lambda s: [sum(mds[i][j] * s[j] for j in range(3)) % m for i in range(3)]
    state = [w % m for w in state]
    rows, sbox = [list(state)], [0] * ROWS
    for r in range(4):
        state = mul([pow((w + c) % m, 5, m) for w, c in zip(state, rcs[r])])
        rows.append(list(state))
    for i in range(28):
        for half in range(2):
            r = 4 + 2 * i + half
            state = [(w + c) % m for w, c in zip(state, rcs[r])]
            state[0] = pow(state[0], 5, m)
            if half == 0:
                sbox[4 + i] = state[0]
            state = mul(state)
        rows.append(list(state))
    for r in range(60, 64):
        state = mul([pow((w + c) % m, 5, m) for w, c in zip(state, rcs[r])])
        rows.append(list(state))
    assert len(rows) == ROWS
    return [[row[j] for row in rows] for j in range(3)] + [sbox]


def trace_limbs(states, field):
    """(4, 37 * count, 4) Montgomery limbs of the restated trace of `states` (lists of three integers)."""
    columns = [[], [], [], []]
    for s in states:
        for j, col in enumerate(trace_ints(s, field)):
            columns[j] += col
    return np.stack([fields.to_limbs(col, field, True) for col in columns])


def states_limbs(states, field):
    return fields.to_limbs([w for s in states for w in s], field, True).reshape(-1, 3, 4)


def random_states(count, field, seed):
    rng = o.SplitMix64(seed)
    return [[rng.field(MOD[field]) for _ in range(3)] for _ in range(count)]


# ---- the reference's test circuits ----------------------------------------------------------------------------------------------------
def configure_chip(meta, constant=False):
    state = [meta.advice_column() for _ in range(WIDTH)]
    partial_sbox = meta.advice_column()
    rc_a = [meta.fixed_column() for _ in range(WIDTH)]
    rc_b = [meta.fixed_column() for _ in range(WIDTH)]
    if constant:
        meta.enable_constant(rc_b[0])
    return Pow5Chip.configure(meta, state, partial_sbox, rc_a, rc_b)


class PermuteCircuit(Circuit):
    """MyPermuteCircuit: the permutation of (0, 1, 2), the expected final state computed outside the circuit."""

    def __init__(self, final_state=None):
        self.final_state = permute_ints([0, 1, 2], FP) if final_state is None else final_state

    def without_witnesses(self):
        return PermuteCircuit(self.final_state)

    def configure(self, meta):
        return configure_chip(meta)

    def synthesize(self, config, layouter):
        initial = layouter.assign_region(
            "prepare initial state", lambda region: [region.assign_advice(config.state[i], 0, i) for i in range(WIDTH)])
        final = Pow5Chip.construct(config).permute(layouter, initial)

        def constrain(region):
            for i in range(WIDTH):
                var = region.assign_advice(config.state[i], 0, self.final_state[i])
                region.constrain_equal(final[i].cell(), var.cell())
        layouter.assign_region("constrain final state", constrain)


class HashCircuit(Circuit):
    """MyHashCircuit<_, 3, 2, L>: message and output are witnessed."""

    def __init__(self, length, message=None, output=None):
        self.length, self.message, self.output = length, message, output

    def without_witnesses(self):
        return HashCircuit(self.length)

    def configure(self, meta):
        return configure_chip(meta, constant=True)

    def synthesize(self, config, layouter):
        chip = Pow5Chip.construct(config)
        word = lambda i: None if self.message is None else self.message[i]
        message = layouter.assign_region(
            "load message", lambda region: [region.assign_advice(config.state[i], 0, lambda i=i: word(i)) for i in range(self.length)])
        hasher = Hash.init(chip, layouter.namespace("init"), ConstantLength(self.length))
        output = hasher.hash(layouter.namespace("hash"), message)

        def constrain(region):
            expected = region.assign_advice(config.state[0], 0, lambda: self.output)
            region.constrain_equal(output.cell(), expected.cell())
        layouter.assign_region("constrain output", constrain)


# ---- the bulk path ----------------------------------------------------------------------------------------------------------------------
class PermuteManyCircuit(Circuit):
    """`count` permutations through `permute_many` alone: the region starts on row 0.  states: (count, 3, 4) limbs, or None;
    trace: the chip's columns when the test wants to hand in its own (a tampered witness)."""

    def __init__(self, count, states=None, trace=None):
        self.count, self.states, self.trace = count, states, trace
        self.result = None

    def without_witnesses(self):
        return PermuteManyCircuit(self.count)

    def configure(self, meta):
        return configure_chip(meta)

    def synthesize(self, config, layouter):
        self.result = Pow5Chip.construct(config).permute_many(layouter, self.count, self.states, trace=self.trace)


class MirrorCircuit(Circuit):
    """An inputs region of 3 columns x `count` rows, then either `count` calls of `permute` (bulk=False) or one `permute_many` whose
    input cells are copy-constrained to the same input cells (bulk=True)."""

    def __init__(self, inputs, bulk, witness=True):
        self.inputs, self.bulk, self.witness = inputs, bulk, witness            # inputs: lists of three integers

    def without_witnesses(self):
        return MirrorCircuit(self.inputs, self.bulk, witness=False)

    def configure(self, meta):
        return configure_chip(meta)

    def synthesize(self, config, layouter):
        count = len(self.inputs)
        value = lambda i, j: self.inputs[i][j] if self.witness else None
        cells = layouter.assign_region("inputs", lambda region: [
            [region.assign_advice(config.state[j], i, lambda i=i, j=j: value(i, j)) for j in range(WIDTH)] for i in range(count)])
        chip = Pow5Chip.construct(config)
        if not self.bulk:
            for i in range(count):
                chip.permute(layouter, cells[i])
            return
        states = states_limbs(self.inputs, config.field) if self.witness else None
        many = chip.permute_many(layouter, count, states)

        def tie(region):
            for i in range(count):
                for j in range(WIDTH):
                    region.constrain_equal(many.input_cell(i, j), cells[i][j].cell())
        layouter.assign_region("tie inputs", tie)


# ---- a synthesized circuit checked on the host --------------------------------------------------------------------------------------------
def gate_of_polynomial(cs, index):
    """(gate name, constraint index within the gate) of the index-th polynomial of the constraint system."""
    for gate in cs.gates:
        if index < len(gate.polys):
            return gate.name, index
        index -= len(gate.polys)
    raise IndexError(index)


def host_failures(circuit, k, field=FP, instances=()):
    """Synthesize with the witness and evaluate every gate on every usable row and every copy constraint with Python integers:
    [("gate", name, constraint, row)] + [("copy", column, row)].  Selectors are read from the assembly, uncompressed."""
    cs, assembly, _ = front.synthesize(circuit, k, field, fixed=True, advice=True, instances=[list(c) for c in instances])
    m, n = MOD[field], 1 << k
    fixed, advice = assembly.host_columns(assembly.fixed), assembly.host_columns(assembly.advice)
    instance = [list(c) + [0] * (n - len(c)) for c in instances]
    failures = []
    for gate in cs.gates:
        for c, poly in enumerate(gate.polys):
            for row in range(assembly.usable):
                value = poly.evaluate(
                    lambda v: v % m, lambda s: int(assembly.selectors[s.index][row]), lambda q: fixed[q[1]][(row + q[2]) % n],
                    lambda q: advice[q[1]][(row + q[2]) % n], lambda q: instance[q[1]][(row + q[2]) % n], lambda a: -a % m, lambda a, b: (a + b) % m,
                    lambda a, b: a * b % m, lambda a, f: a * f % m)
                if value:
                    failures.append(("gate", gate.name, c, row))
    by_kind = {"advice": advice, "fixed": fixed, "instance": instance}
    columns = assembly.permutation.columns
    for c, mapped in enumerate(assembly.permutation.pairs()):
        for row, (c2, row2) in enumerate(mapped):
            if by_kind[columns[c].kind][columns[c].index][row] != by_kind[columns[c2].kind][columns[c2].index][row2]:
                failures.append(("copy", (columns[c].kind, columns[c].index), row))
    return failures
