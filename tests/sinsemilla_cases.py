"""Shared by test_sinsemilla_host.py and test_gpu_sinsemilla.py: the restatement of Sinsemilla over `oracle.pasta` and
`oracle.hash_to_curve` -- a fold with affine INCOMPLETE addition that returns None (the specification's bottom) on exceptional
operands -- the restated witness of the chip, MerkleCRH, and the messages the tests share."""
import functools
import random

from oracle import hash_to_curve as h2c
from oracle import pasta as o

P = o.P                                   # Pallas base field: coordinates, and the field of the circuits
ORDER = o.Q                               # the order of the Pallas group
K, C = 10, 253
MERKLE_DOMAIN = b"z.cash:Orchard-MerkleCRH"
STRUCTURES = {"one": [1], "merkle": [25, 25, 2], "full": [1] + [25] * 10 + [2]}


@functools.lru_cache(maxsize=None)
def table():
    """S(0) .. S(1023) as (x, y) integers"""
    s = h2c.hash_to_curve("pallas", "z.cash:SinsemillaS")
    return [s(j.to_bytes(4, "little")) for j in range(1 << K)]


@functools.lru_cache(maxsize=None)
def q_of(domain: bytes):
    return h2c.hash_to_curve("pallas", "z.cash:SinsemillaQ")(domain)


def incomplete_add(a, b):
    """The specification's incomplete addition: None when either operand is None or the identity, or when they share their x."""
    if a is None or b is None or a[0] == b[0]:
        return None
    lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return (x, (lam * (a[0] - x) - a[1]) % P)


def hash_to_point(q, words, upto=None):
    """fold Acc <- (Acc + S(m)) + Acc from Q; `upto`: the accumulators after the prefixes of those lengths instead"""
    acc, seen = q, {}
    for i, w in enumerate(words):
        if upto is not None and i in upto:
            seen[i] = acc
        acc = incomplete_add(incomplete_add(acc, table()[w]), acc)
    if upto is None:
        return acc
    if len(words) in upto:
        seen[len(words)] = acc
    return seen


def words_of(pieces, num_words):
    return [(p >> (K * j)) & 1023 for p, n in zip(pieces, num_words) for j in range(n)]


def merkle_words(layer, left, right):
    v = layer | (left << 10) | (right << 265)
    return [(v >> (K * j)) & 1023 for j in range(52)]


def merkle_crh(q, layer, left, right):
    pt = hash_to_point(q, merkle_words(layer, left, right))
    return None if pt is None else pt[0]


def merkle_root(q, leaves):
    layer, depth = list(leaves), len(leaves).bit_length() - 1
    for level in range(depth):
        layer = [merkle_crh(q, depth - 1 - level, layer[i], layer[i + 1]) for i in range(0, len(layer), 2)]
    return layer[0]


def trace(q, pieces, num_words):
    """The five columns SinsemillaChip::hash_message assigns (hash_to_point.rs:295-493) for one message, as integers: x_a, x_p, bits,
    lambda_1, lambda_2, each of sum(num_words) + 1 rows.  Division is the reference's Assigned division (x / 0 = 0)."""
    inv = lambda v: pow(v % P, -1, P) if v % P else 0
    x_a, y_a = q
    cols = [[], [], [], [], []]
    for piece, n in zip(pieces, num_words):
        for j in range(n):
            z = piece >> (K * j)
            x_p, y_p = table()[z & 1023]
            l1 = (y_a - y_p) * inv(x_a - x_p) % P
            x_r = (l1 * l1 - x_a - x_p) % P
            l2 = (2 * y_a * inv(x_a - x_r) - l1) % P
            for col, v in zip(cols, (x_a, x_p, z, l1, l2)):
                col.append(v)
            x_new = (l2 * l2 - x_a - x_r) % P
            x_a, y_a = x_new, (l2 * (x_a - x_new) - y_a) % P
    for col, v in zip(cols, (x_a, 0, 0, y_a, 0)):
        col.append(v)
    return cols


def random_pieces(num_words, seed, high_zero=False):
    """one message of this structure; high_zero: the longest piece keeps only its lowest word"""
    rng = random.Random(seed)
    pieces = [rng.getrandbits(K * n) for n in num_words]
    if high_zero:
        k = max(range(len(num_words)), key=lambda i: num_words[i])
        pieces[k] &= 1023
    return pieces


@functools.lru_cache(maxsize=None)
def message_pool():
    """257 messages of 253 words -- all zero, all 1023, random -- and for each the accumulator after 0, 1, 2, 52 and 253 words"""
    rng = random.Random(20)
    msgs = [[0] * C, [1023] * C] + [[rng.randrange(1024) for _ in range(C)] for _ in range(255)]
    q = q_of(MERKLE_DOMAIN)
    return q, msgs, [hash_to_point(q, m, upto=(0, 1, 2, 52, 253)) for m in msgs]


def halve(pt):
    return o.ec_mul(pow(2, -1, ORDER), pt, P)


def exceptional_cases():
    """(name, Q, message) whose chain has no value; every message has 5 words and m_0 = 5"""
    s = table()
    rng = random.Random(6)
    tail = [rng.randrange(1024) for _ in range(4)]
    cases = [("doubling", s[5], [5] + tail), ("identity", o.ec_neg(s[5], P), [5] + tail),
             ("second addition", o.ec_neg(halve(s[5]), P), [5] + tail)]
    # round 3 of 5: choose Acc_3 = S(m_3) and undo rounds 2, 1, 0: Acc_i = (Acc_{i+1} - S(m_i)) / 2
    m = [5, 77, 901, 333, 12]
    acc = s[m[3]]
    for i in (2, 1, 0):
        acc = halve(o.ec_add(acc, o.ec_neg(s[m[i]], P), P))
    assert hash_to_point(acc, m[:3]) == s[m[3]]                  # rounds 0 to 2 are clean and do arrive at S(m_3)
    cases.append(("round 3 of 5", acc, m))
    return cases


# ---- the reference's test circuits and the circuits of the bulk path -----------------------------------------------------------------------
# (imported lazily by the tests that build circuits: the restatement above needs nothing of the package)
import gzip                                                                   # noqa: E402
import importlib.util                                                         # noqa: E402
import os                                                                     # noqa: E402

import numpy as np                                                            # noqa: E402

from halo2_amd import circuit as front                                        # noqa: E402
from halo2_amd.circuit import Circuit                                         # noqa: E402
from halo2_amd.gadgets.sinsemilla import SinsemillaChip                       # noqa: E402
from halo2_amd.gadgets.utilities import LookupRangeCheckConfig               # noqa: E402
from oracle import plonk_api                                                  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FP = 0
TEST_DOMAIN = b"MerkleCRH-M"              # the reference's TestHashDomain: CommitDomain::new("MerkleCRH").Q()
MERKLE_DEPTH = 32
LEAF_POS = 0xA5A55A5A


def fixture_text(name):
    path = os.path.join(GOLDEN, name)
    raw = gzip.open(path).read() if name.endswith(".gz") else open(path, "rb").read()
    return raw.decode().replace("\r\n", "\n")


def fixture_cs(text):
    """the `cs:` section of a pinned key in its one-line form"""
    flat = plonk_api.compact_debug(text)
    return flat[flat.index("cs: ") + 4:flat.index(", fixed_commitments: ")]


def merkle_witness():
    rng = random.Random(32)
    return rng.randrange(P), LEAF_POS, [rng.randrange(P) for _ in range(MERKLE_DEPTH)]


def merkle_path_root(q, leaf, pos, path):
    """the reference's fold (merkle.rs:351-385): l counts from the leaf; a hash without a value counts as 0"""
    node = leaf
    for l, sibling in enumerate(path):                                        # noqa: E741
        left, right = (node, sibling) if pos >> l & 1 == 0 else (sibling, node)
        node = merkle_crh(q, l, left, right) or 0
    return node


def _example(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.dirname(GOLDEN)), "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# MyMerkleCircuit (sinsemilla/merkle.rs:213-393) is the circuit of examples/sinsemilla_merkle.py
MerkleCircuit = _example("sinsemilla_merkle").MerkleCircuit


class TamperedMerkleCircuit(MerkleCircuit):
    """The hash of layer 7 is handed a right node with one bit flipped: its pieces no longer decompose the node the swap produced."""

    def synthesize(self, config, layouter):
        from halo2_amd.gadgets import sinsemilla as g
        original = g.MerkleChip.hash_layer

        def hash_layer(chip, layouter_, q, l, left, right):                  # noqa: E741
            value = right.value().inner
            if l == 7 and value is not None:
                right = g.AssignedCell(g.Assigned.trivial(value.evaluate(P) ^ 1, P), right.cell())
            return original(chip, layouter_, q, l, left, right)
        g.MerkleChip.hash_layer = hash_layer
        try:
            super().synthesize(config, layouter)
        finally:
            g.MerkleChip.hash_layer = original


class LookupCircuit(Circuit):
    """MyLookupCircuit (lookup_range_check.rs:884-976): a value of exactly num_words K bits, strict, and one of one bit more, not strict."""

    def __init__(self, num_words):
        self.num_words = num_words

    def without_witnesses(self):
        return LookupCircuit(self.num_words)

    def configure(self, meta):
        running_sum = meta.advice_column()
        table_idx = meta.lookup_table_column()
        constants = meta.fixed_column()
        meta.enable_constant(constants)
        return LookupRangeCheckConfig.configure(meta, running_sum, table_idx)

    def synthesize(self, config, layouter):
        config.load_range_check_table(layouter)
        bits = self.num_words * K
        for element, final_z, strict in (((1 << bits) - 1, 0, True), (1 << bits, 1, False)):
            zs = config.witness_check(layouter, element, self.num_words, strict)
            known = [z.value().inner for z in zs]
            if all(v is not None for v in known):
                assert [v.evaluate(P) for v in known] == [element >> (K * i) for i in range(self.num_words + 1)] and known[-1].evaluate(P) == final_z


class RangeCircuit(Circuit):
    """checks: ("witness", value, num_words, strict) and ("short", value, num_bits) through one LookupRangeCheckConfig"""

    def __init__(self, checks):
        self.checks = checks

    def without_witnesses(self):
        return RangeCircuit([c[:1] + (None,) + c[2:] for c in self.checks])

    configure = LookupCircuit.configure

    def synthesize(self, config, layouter):
        config.load_range_check_table(layouter)
        for check in self.checks:
            if check[0] == "witness":
                config.witness_check(layouter, check[1], check[2], check[3])
            else:
                config.witness_short_check(layouter, check[1], check[2])


def configure_hash_chip(meta, table):
    """one Sinsemilla chip as the reference's circuits set it up: five advice columns, the pieces witnessed in the third (`bits`),
    the range check in a sixth"""
    advices = [meta.advice_column() for _ in range(6)]
    constants = meta.fixed_column()
    meta.enable_constant(constants)
    fixed_y_q = meta.fixed_column()
    lookup = (meta.lookup_table_column(), meta.lookup_table_column(), meta.lookup_table_column())
    range_check = LookupRangeCheckConfig.configure(meta, advices[5], lookup[0])
    return SinsemillaChip.configure(meta, advices[:5], advices[2], fixed_y_q, lookup, range_check, table=table)


class HashCircuit(Circuit):
    """messages: lists of piece integers of one structure; every message is witnessed piece by piece, then hashed -- by one
    `hash_to_point` each (bulk=False) or by one `hash_to_point_many` (bulk=True)."""

    def __init__(self, num_words, messages, q, table=None, bulk=False, witness=True):
        self.num_words, self.messages, self.q, self.table, self.bulk, self.witness = num_words, messages, q, table, bulk, witness
        self.points, self.many = None, None

    def without_witnesses(self):
        return HashCircuit(self.num_words, self.messages, self.q, self.table, self.bulk, witness=False)

    def configure(self, meta):
        return configure_hash_chip(meta, self.table)

    def synthesize(self, config, layouter):
        SinsemillaChip.load(config, layouter)
        chip = SinsemillaChip(config)
        pieces = [[chip.witness_message_piece(layouter, p if self.witness else None, n) for p, n in zip(m, self.num_words)]
                  for m in self.messages]
        if self.bulk:
            self.many = chip.hash_to_point_many(layouter, self.q, self.num_words, pieces)
        else:
            self.points = [chip.hash_to_point(layouter, self.q, p)[0] for p in pieces]


def host_keygen_cs(circuit, k):
    """keygen's synthesis and selector compression on the host: the conflict matrix comes from numpy instead of the device"""
    cs, assembly, _ = front.synthesize(circuit.without_witnesses(), k, FP, fixed=True, advice=False)
    sel = assembly.selectors.astype(np.int64)
    conflicts = (sel @ sel.T) > 0
    np.fill_diagonal(conflicts, False)
    cs.compress_selectors(conflicts)
    return cs


def host_failures(circuit, k):
    """Synthesize with the witness and evaluate, with Python integers, every gate and every lookup on every usable row and every copy
    constraint: [("gate", name, constraint name, row)] + [("lookup", index, row)] + [("copy", (kind, column), row)].  Selectors are
    read from the assembly, uncompressed.  -> (failures, assembly, layouter)"""
    cs, assembly, layouter = front.synthesize(circuit, k, FP, fixed=True, advice=True, instances=[])
    n = 1 << k
    fixed, advice = assembly.host_columns(assembly.fixed), assembly.host_columns(assembly.advice)
    selectors = assembly.selectors

    def value(e, row):
        return e.evaluate(
            lambda v: v % P, lambda s: int(selectors[s.index][row]), lambda q: fixed[q[1]][(row + q[2]) % n],
            lambda q: advice[q[1]][(row + q[2]) % n], lambda q: 0, lambda a: -a % P, lambda a, b: (a + b) % P,
            lambda a, b: a * b % P, lambda a, f: a * f % P)
    failures = []
    for gate in cs.gates:
        for name, poly in zip(gate.constraint_names, gate.polys):
            rows = range(assembly.usable)
            if poly.kind == "Product" and poly.args[0].kind == "Selector":    # selector * constraint: only where it is enabled
                rows = np.flatnonzero(selectors[poly.args[0].args[0].index][:assembly.usable])
            failures += [("gate", gate.name, name, int(row)) for row in rows if value(poly, int(row))]
    for index, (inputs, tables) in enumerate(cs.lookups):
        table = {tuple(value(t, row) for t in tables) for row in range(assembly.usable)}
        failures += [("lookup", index, row) for row in range(assembly.usable) if tuple(value(e, row) for e in inputs) not in table]
    by_kind = {"advice": advice, "fixed": fixed}
    columns = assembly.permutation.columns
    for c, mapped in enumerate(assembly.permutation.pairs()):
        for row, (c2, row2) in enumerate(mapped):
            if by_kind[columns[c].kind][columns[c].index][row] != by_kind[columns[c2].kind][columns[c2].index][row2]:
                failures.append(("copy", (columns[c].kind, columns[c].index), row))
    return failures, assembly, layouter
