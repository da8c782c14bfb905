"""Shared by test_sinsemilla_commit_host.py and test_gpu_sinsemilla_commit.py: the restatement of SinsemillaCommit (Zcash protocol
specification 5.4.8.4) and of hashing from a private point over the restatements of sinsemilla_cases.py, ecc_cases.py and
ecc_fixed_cases.py -- `commit`, the crafted initial points that steer a hash onto [r]R or its negative, the witness of a hash whose Q
is a cell -- and the messages, points and scalars the tests share."""
import functools
import random

from oracle import hash_to_curve as h2c
from oracle import pasta as o

import ecc_cases as ec
import ecc_fixed_cases as fx
import sinsemilla_cases as sc
from sinsemilla_cases import ORDER, P

PERSONALIZATION = "MerkleCRH"             # the reference's test domain (sinsemilla.rs, tests): Q = Q("MerkleCRH-M"), R = R("MerkleCRH-r")
COMMIT_WORDS = [25, 25]                   # a 500-bit message as Message::from_bitstring cuts it: 50 words in two pieces
UPTO = (0, 1, 50, 52, 253)


@functools.lru_cache(maxsize=None)
def r_of(name: str):
    """CommitDomain::new(name).R(): the personalisation is the domain string itself"""
    return h2c.hash_to_curve("pallas", name + "-r")(b"")


@functools.lru_cache(maxsize=None)
def q_of(name: str):
    return sc.q_of((name + "-M").encode())


def point(pt):
    """the identity as (0, 0)"""
    return (0, 0) if pt is None else pt


def group_add(a, b):
    """the group's sum of two points with the identity as (0, 0), by oracle.pasta's ec_add"""
    return point(o.ec_add(None if a == (0, 0) else a, None if b == (0, 0) else b, P))


def blind(r, name=PERSONALIZATION):
    """[r]R with r read as the device reads it: 255 bits, not reduced"""
    return o.ec_mul(r % ORDER, r_of(name), P) if r % ORDER else None


def commit(q, words, r, name=PERSONALIZATION):
    """None where the HASH is bottom; otherwise the group's sum, the identity as (0, 0)"""
    m = sc.hash_to_point(q, words)
    return None if m is None else point(o.ec_add(m, blind(r, name), P))


def crafted_q(words, target):
    """the Q from which `words` hashes to `target` with every round clean: Acc_i = (Acc_{i+1} - S(m_i)) / 2 undone from the end"""
    acc = target
    for w in reversed(words):
        acc = sc.halve(o.ec_add(acc, o.ec_neg(sc.table()[w], P), P))
    return acc


CRAFT_WORDS = [5, 77, 901, 333, 12]
CRAFT_R = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100ABCD


@functools.lru_cache(maxsize=None)
def crafted_cases():
    """{"doubling": Q with hash = [r]R, "identity": Q with hash = -[r]R}, for CRAFT_WORDS and CRAFT_R"""
    t = blind(CRAFT_R)
    return {"doubling": crafted_q(CRAFT_WORDS, t), "identity": crafted_q(CRAFT_WORDS, o.ec_neg(t, P))}


@functools.lru_cache(maxsize=None)
def private_qs(n=257):
    """Q_i alternating among Q(Orchard's MerkleCRH), Q("MerkleCRH-M") and random points of the curve"""
    fixed = (sc.q_of(sc.MERKLE_DOMAIN), sc.q_of(sc.TEST_DOMAIN))
    rand = ec.random_bases(n)
    return [fixed[i % 3] if i % 3 < 2 else rand[i] for i in range(n)]


@functools.lru_cache(maxsize=None)
def private_pool():
    """for each message of sc.message_pool(), the accumulators from its own Q after 0, 1, 50, 52 and 253 words"""
    _, msgs, _ = sc.message_pool()
    return [sc.hash_to_point(q, m, upto=UPTO) for q, m in zip(private_qs(len(msgs)), msgs)]


@functools.lru_cache(maxsize=None)
def shared_pool():
    """the same from the one Q of the test domain"""
    _, msgs, _ = sc.message_pool()
    q = q_of(PERSONALIZATION)
    return [sc.hash_to_point(q, m, upto=UPTO) for m in msgs]


@functools.lru_cache(maxsize=None)
def scalar_pool(n=257):
    """the edge scalars of the fixed-base product in front, random ones behind, and [r]R of each (None for the identity)"""
    scalars = fx.EDGE_SCALARS + ec.random_scalars(n - len(fx.EDGE_SCALARS), seed=31)
    return scalars, [blind(r) for r in scalars]


def shared_words_hash(message):
    """the hash of a 500-bit message (an integer) from the test domain's Q"""
    return sc.hash_to_point(q_of(PERSONALIZATION), sc.words_of([message], [50]))


def trace_from(q, pieces, num_words):
    """sc.trace from q under the row that holds y_Q in x_p (hash_to_point.rs:117-121, :179-182): five columns of sum(num_words) + 2"""
    cols = sc.trace(q, pieces, num_words)
    return [[v] + col for v, col in zip((0, q[1], 0, 0, 0), cols)]


def add_pairs(n):
    """n pairs that go round the six branches of add.rs: P + Q, P + P, P + (-P), P + 0, 0 + Q, 0 + 0"""
    pts = ec.random_bases(2 * n + 2, seed=41)
    kinds = [lambda a, b: (a, b), lambda a, b: (a, a), lambda a, b: (a, o.ec_neg(a, P)), lambda a, b: (a, (0, 0)),
             lambda a, b: ((0, 0), b), lambda a, b: ((0, 0), (0, 0))]
    return [kinds[i % 6](pts[2 * i], pts[2 * i + 1]) for i in range(n)]


def add_row(p, q):
    """the 11 elements of one addition: x_p y_p x_qr y_qr lambda alpha beta gamma delta x_r y_r, with the reference's inv0"""
    r, witnesses = ec.complete_add(p, q)
    return list(p + q + witnesses + r)


def random_messages(structure, count, seed=0):
    rng = random.Random(1000 * seed + count)
    return [[rng.getrandbits(10 * n) for n in structure] for _ in range(count)]


# ---- the reference's test circuit (halo2_gadgets/src/sinsemilla.rs tests::MySinsemillaCircuit) and the circuit of the bulk path -----------
# (imported lazily by the tests that build circuits: the restatement above needs nothing of the package)
from halo2_amd.circuit import Circuit                                         # noqa: E402
from halo2_amd.gadgets import sinsemilla as g                                 # noqa: E402
from halo2_amd.gadgets.ecc import EccChip, FixedBaseTables, FixedPoints, NonIdentityPoint, ScalarFixed      # noqa: E402
from halo2_amd.gadgets.sinsemilla import SinsemillaChip                       # noqa: E402
from halo2_amd.gadgets.utilities import LookupRangeCheckConfig               # noqa: E402

# the z of R("MerkleCRH-r") over 85 windows, from a host run of fx.find_z; the reference's pinned vk_sinsemilla_chip commits to them
Z_R_85 = [
    167376, 2789, 42871, 36486, 60638, 54161, 150446, 120407, 24225, 27122, 269798, 33939, 42385, 23157, 61278, 87764, 1059,
    175554, 15331, 176775, 42509, 2066, 24643, 8727, 36434, 97337, 36165, 38159, 15597, 79290, 25069, 46683, 16156, 1006, 63890,
    8055, 216002, 92487, 67446, 30996, 1911, 144236, 105394, 1569, 14705, 178387, 49076, 46359, 44569, 115479, 24951, 1888,
    29492, 7878, 82817, 73540, 43091, 21, 84304, 17872, 33547, 7661, 65793, 79781, 67471, 55716, 138403, 8200, 327803, 59268,
    16361, 52282, 35713, 27308, 121140, 79264, 15054, 221, 63304, 66176, 41661, 5364, 9863, 66829, 41274]
assert len(Z_R_85) == fx.NUM_WINDOWS


def bits_of(value, n):
    return [bool(value >> i & 1) for i in range(n)]


@functools.lru_cache(maxsize=None)
def host_r_tables() -> FixedBaseTables:
    """R's tables on the host: the z of the list above (each checked valid here), the roots from the oracle"""
    r = r_of(PERSONALIZATION)
    table = fx.window_table(r, fx.NUM_WINDOWS)
    assert all(fx.z_is_valid(z, [pt[1] for pt in row]) for z, row in zip(Z_R_85, table))
    return FixedBaseTables(r, table, fx.lagrange_coeffs(table), Z_R_85, fx.roots(table, Z_R_85))


def host_domain() -> g.CommitDomains:
    return g.CommitDomains(q_of(PERSONALIZATION), host_r_tables())


def configure_chips(meta, table, allow_init_from_private_point):
    """sinsemilla.rs tests::configure: ten advices, the constants' column, the table index, eight Lagrange columns, two more table
    columns, the range check on advices[9], the ECC chip on all ten, and one Sinsemilla chip on each half"""
    advices = [meta.advice_column() for _ in range(10)]
    constants = meta.fixed_column()
    meta.enable_constant(constants)
    table_idx = meta.lookup_table_column()
    lagrange = [meta.fixed_column() for _ in range(8)]
    lookup = (table_idx, meta.lookup_table_column(), meta.lookup_table_column())
    range_check = LookupRangeCheckConfig.configure(meta, advices[9], table_idx)
    ecc_config = EccChip.configure(meta, advices, lagrange, range_check,
                                   fixed_bases=FixedPoints(full_width=("R",), short=("R",), base_field=("R",)))
    config1 = SinsemillaChip.configure(meta, advices[:5], advices[2], lagrange[0], lookup, range_check, table=table,
                                       allow_init_from_private_point=allow_init_from_private_point)
    config2 = SinsemillaChip.configure(meta, advices[5:], advices[7], lagrange[1], lookup, range_check, table=table,
                                       allow_init_from_private_point=allow_init_from_private_point)
    return ecc_config, config1, config2


class MySinsemillaCircuit(Circuit):
    """The reference's synthesis: with chip 1 the MerkleCRH hash of l (10 bits) || left (250) || right (250) constrained to a witnessed
    parent; with chip 2 the commitment of 500 bits under a random r constrained to a witnessed result.  The pinned key depends on the
    shapes, fixed cells and copies, not on the witnesses, which come from `seed`.  domain: a gadget CommitDomains.
    private: the chips allow hashing from a private point, and chip 2 goes on to hash 50 bits from a witnessed Q.
    mutate: the y_Q of that hash (row 0 of its region, column x_p) is overwritten with its value + 1."""

    def __init__(self, domain, table=None, seed=1, witness=True, private=False, mutate=False, flag=None):
        self.domain, self.table, self.seed, self.witness, self.private, self.mutate = domain, table, seed, witness, private, mutate
        self.flag = private if flag is None else flag                        # flag=False with private=True: the call must raise
        self.mutated_row = None

    def without_witnesses(self):
        return MySinsemillaCircuit(self.domain, self.table, self.seed, witness=False, private=self.private, flag=self.flag)

    def configure(self, meta):
        return configure_chips(meta, self.table, self.flag)

    def synthesize(self, config, layouter):
        rng = random.Random(self.seed)
        v = (lambda x: x) if self.witness else (lambda x: None)
        vbits = (lambda value, n: bits_of(value, n)) if self.witness else (lambda value, n: [None] * n)
        ecc_chip = EccChip(config[0])
        SinsemillaChip.load(config[1], layouter)
        q = self.domain.Q
        # the MerkleCRH example
        chip1 = SinsemillaChip(config[1])
        merkle_crh = g.HashDomain(chip1, q)
        left_v, right_v = rng.getrandbits(250), rng.getrandbits(250)
        l = g.MessagePiece.from_bitstring(chip1, layouter, vbits(0, 10))     # noqa: E741
        left = g.MessagePiece.from_bitstring(chip1, layouter, vbits(left_v, 250))
        right = g.MessagePiece.from_bitstring(chip1, layouter, vbits(right_v, 250))
        want = sc.hash_to_point(q, sc.words_of([0, left_v, right_v], [1, 25, 25]))
        expected_parent = NonIdentityPoint.new(ecc_chip, layouter, v(want))
        parent, _ = merkle_crh.hash_to_point(layouter, g.Message.from_pieces(chip1, [l, left, right]))
        NonIdentityPoint(ecc_chip, parent).constrain_equal(layouter, expected_parent)
        # the commitment
        chip2 = SinsemillaChip(config[2])
        test_commit = g.CommitDomain(chip2, ecc_chip, self.domain)
        r_val, message_v = rng.randrange(ORDER), rng.getrandbits(500)
        r = ScalarFixed.new(ecc_chip, layouter, v(r_val))
        message = g.Message.from_bitstring(chip2, layouter, vbits(message_v, 500))
        result, _ = test_commit.commit(layouter, message, r)
        want = commit(q, sc.words_of([message_v], [50]), r_val)
        expected_result = NonIdentityPoint.new(ecc_chip, layouter, v(want))
        result.constrain_equal(layouter, expected_result)
        if not self.private:
            return
        # a hash from a witnessed point
        q_val, short_v = ec.random_bases(1, seed=300 + self.seed)[0], rng.getrandbits(50)
        q_point = NonIdentityPoint.new(ecc_chip, layouter, v(q_val))
        message = g.Message.from_bitstring(chip2, layouter, vbits(short_v, 50))
        hashed, _ = test_commit.hash_with_private_init(layouter, q_point, message)
        hashed.constrain_equal(layouter, NonIdentityPoint.new(ecc_chip, layouter, v(sc.hash_to_point(q_val, sc.words_of([short_v], [5])))))
        if self.mutate:
            self.mutated_row = layouter.regions[hashed.inner().x().cell().region_index]
            if layouter.cs.collect_advice:
                column = config[2].double_and_add.x_p
                value = layouter.cs.advice[column.index].integers(layouter.cs.n, FP)[self.mutated_row]
                layouter.cs.assign_advice(column, self.mutated_row, lambda: (value + 1) % P)


FP = 0


class CommitCircuit(Circuit):
    """messages: one integer of 500 bits each, witnessed as two pieces of 25 words; scalars: the blinding factors.  One `commit` each
    (many=False), kept in `results` as (Point, running sums, ScalarFixed), or all through one `commit_many` (many=True), kept in `bulk`."""

    def __init__(self, messages, scalars, domain, table=None, many=False, witness=True):
        self.messages, self.scalars, self.domain, self.table, self.many, self.witness = messages, scalars, domain, table, many, witness
        self.results, self.bulk, self.pieces, self.config = [], None, None, None

    def without_witnesses(self):
        return CommitCircuit(self.messages, self.scalars, self.domain, self.table, self.many, witness=False)

    def configure(self, meta):
        return configure_chips(meta, self.table, False)

    def synthesize(self, config, layouter):
        v = (lambda x: x) if self.witness else (lambda x: None)
        self.config = config
        ecc_chip = EccChip(config[0])
        SinsemillaChip.load(config[1], layouter)
        chip = SinsemillaChip(config[2])
        domain = g.CommitDomain(chip, ecc_chip, self.domain)
        mask = (1 << 250) - 1
        self.pieces = [[chip.witness_message_piece(layouter, v(m >> (250 * k) & mask), 25) for k in range(2)] for m in self.messages]
        if self.many:
            self.bulk = domain.commit_many(layouter, self.pieces, [25, 25], [v(k) for k in self.scalars])
            return
        self.results = []
        for pieces, k in zip(self.pieces, self.scalars):
            r = ScalarFixed.new(ecc_chip, layouter, v(k))
            self.results.append(domain.commit(layouter, g.Message.from_pieces(chip, pieces), r))


class FlaggedHashCircuit(Circuit):
    """Hashes on a chip configured with allow_init_from_private_point.  messages: lists of piece integers of one structure; start: one
    (x, y) pair, public and shared, or a list of points, one witnessed Q per message.  One `hash_to_point` or
    `hash_to_point_with_private_init` each (bulk=False), kept in `points`, or one `hash_to_point_many` (bulk=True), kept in `many`."""

    def __init__(self, num_words, messages, start, table=None, bulk=False, witness=True):
        self.num_words, self.messages, self.start, self.table, self.bulk, self.witness = num_words, messages, start, table, bulk, witness
        self.private = isinstance(start, list)
        self.points, self.many = None, None

    def without_witnesses(self):
        return FlaggedHashCircuit(self.num_words, self.messages, self.start, self.table, self.bulk, witness=False)

    def configure(self, meta):
        return configure_chips(meta, self.table, True)

    def synthesize(self, config, layouter):
        v = (lambda x: x) if self.witness else (lambda x: None)
        ecc_chip = EccChip(config[0])
        SinsemillaChip.load(config[1], layouter)
        chip = SinsemillaChip(config[2])
        start = [NonIdentityPoint.new(ecc_chip, layouter, v(q)).inner() for q in self.start] if self.private else self.start
        pieces = [[chip.witness_message_piece(layouter, v(p), n) for p, n in zip(m, self.num_words)] for m in self.messages]
        if self.bulk:
            self.many = chip.hash_to_point_many(layouter, start, self.num_words, pieces)
        elif self.private:
            self.points = [chip.hash_to_point_with_private_init(layouter, q, p)[0] for q, p in zip(start, pieces)]
        else:
            self.points = [chip.hash_to_point(layouter, start, p)[0] for p in pieces]
