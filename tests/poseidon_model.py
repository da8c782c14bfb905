"""Poseidon for any specification in Python integers, restated from halo2_poseidon/src/{lib,grain,mds}.rs line by line and
independently of halo2_amd/poseidon_spec.py: the Grain register is an 80-entry list refilled eight bits at a time as grain.rs does it,
the inverse MDS is the Lagrange form of mds.rs:79-101 (not an elimination), the sponge is lib.rs's Absorbing / Squeezing pair.

What stands behind it: at (3, 2, 8, 56) the model's constants, permutations and hashes are the reference's own vectors
(tests/golden/poseidon_kat.json, poseidon_hash_kat.json -- tests/test_poseidon_spec_host.py).  For every other width NO reference value
exists in this repository: the reference is Rust, no toolchain builds it here, and oracle/ is closed.  The wide cases therefore rest
on this restatement and on those pins alone; the device and the gadget are held to it bit for bit.

Also here: the Pow5 chip's row list of one permutation (pow5.rs:435-597), the trace as limbs, and the test circuits of
halo2_gadgets/benches/poseidon.rs (HashCircuit<S, WIDTH, RATE, L>) against halo2_amd.circuit."""
import functools

P = 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001
Q = 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001
FP, FQ = 0, 1
MOD = {FP: P, FQ: Q}
NUM_BITS = 255


# ---- grain.rs ---------------------------------------------------------------------------------------------------------------------------
class Grain:
    def __init__(self, t, r_f, r_p):
        state = [1] * 80                                                      # bitarr![1; 80], Msb0: index 0 is the first bit

        def set_bits(offset, length, value):
            for i in range(length):
                state[offset + length - 1 - i] = (value >> i) & 1
        set_bits(0, 2, 1)                                                     # FieldType::PrimeOrder
        set_bits(2, 4, 0)                                                     # SboxType::Pow
        set_bits(6, 12, NUM_BITS)
        set_bits(18, 12, t)
        set_bits(30, 10, r_f)
        set_bits(40, 10, r_p)
        self.state, self.next_bit = state, 80
        for _ in range(20):                                                   # discard the first 160 bits
            self.load_next_8_bits()
            self.next_bit = 80

    def load_next_8_bits(self):
        s = self.state
        new = [s[i + 62] ^ s[i + 51] ^ s[i + 38] ^ s[i + 23] ^ s[i + 13] ^ s[i] for i in range(8)]
        self.state = s[8:] + s[:8]                                            # rotate_left(8)
        self.next_bit -= 8
        for i in range(8):
            self.state[self.next_bit + i] = new[i]

    def get_next_bit(self):
        if self.next_bit == 80:
            self.load_next_8_bits()
        bit = self.state[self.next_bit]
        self.next_bit += 1
        return bit

    def next(self):                                                           # the self-shrinking filter (Iterator::next)
        while not self.get_next_bit():
            self.get_next_bit()
        return self.get_next_bit()

    def _bits(self):
        v = 0
        for i in range(NUM_BITS):
            if self.next():
                v |= 1 << (NUM_BITS - 1 - i)
        return v

    def next_field_element(self, m):
        while True:
            v = self._bits()
            if v < m:                                                         # from_repr_vartime rejects what is not canonical
                return v

    def next_field_element_without_rejection(self, m):
        return self._bits() % m                                               # from_uniform_bytes of the 64-byte little-endian form


# ---- mds.rs -----------------------------------------------------------------------------------------------------------------------------
def generate_mds(grain, t, m, select):
    while True:
        while True:
            vals = [grain.next_field_element_without_rejection(m) for _ in range(2 * t)]
            if len(set(vals)) == len(vals):
                xs, ys = vals[:t], vals[t:]
                break
        if select != 0:
            select -= 1
            continue
        mds = [[0] * t for _ in range(t)]
        for i in range(t):
            for j in range(t):
                total = (xs[i] + ys[j]) % m
                assert total != 0
                mds[i][j] = pow(total, m - 2, m)
        break

    def lagrange(points, j, x):
        acc = 1
        for k, x_k in enumerate(points):
            if k != j:
                acc = acc * (x - x_k) % m * pow((points[j] - x_k) % m, m - 2, m) % m
        return acc
    neg_ys = [-y % m for y in ys]
    inv = [[(xs[j] - neg_ys[i]) * lagrange(xs, j, neg_ys[i]) % m * lagrange(neg_ys, i, xs[j]) % m for j in range(t)] for i in range(t)]
    return mds, inv


# ---- lib.rs -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def constants(field, t, r_f, r_p, secure_mds=0):
    """generate_constants (lib.rs:64-91) -> (round_constants, mds, mds_inv)"""
    m = MOD[field]
    grain = Grain(t, r_f, r_p)
    round_constants = [[grain.next_field_element(m) for _ in range(t)] for _ in range(r_f + r_p)]
    mds, inv = generate_mds(grain, t, m, secure_mds)
    return round_constants, mds, inv


class Model:
    """One specification: (field, width, rate, full rounds, partial rounds, secure_mds)."""

    def __init__(self, field, width, rate, full=8, partial=56, secure_mds=0):
        self.field, self.m, self.width, self.rate, self.full, self.partial, self.secure_mds = field, MOD[field], width, rate, full, partial, secure_mds
        self.round_constants, self.mds, self.mds_inv = constants(field, width, full, partial, secure_mds)
        self.rows = full + partial // 2 + 1

    def apply_mds(self, state):
        return [sum(self.mds[i][j] * state[j] for j in range(self.width)) % self.m for i in range(self.width)]

    def full_round(self, state, rcs):
        return self.apply_mds([pow((w + rc) % self.m, 5, self.m) for w, rc in zip(state, rcs)])

    def part_round(self, state, rcs):
        state = [(w + rc) % self.m for w, rc in zip(state, rcs)]
        state[0] = pow(state[0], 5, self.m)
        return self.apply_mds(state)

    def permute(self, state):                                                 # lib.rs:106-151
        assert len(state) == self.width
        r_f = self.full // 2
        rounds = [self.full_round] * r_f + [self.part_round] * self.partial + [self.full_round] * r_f
        state = [w % self.m for w in state]
        for fn, rcs in zip(rounds, self.round_constants):
            state = fn(state, rcs)
        return state

    def hash(self, message):                                                  # Hash<_, S, ConstantLength<L>, T, RATE>::hash (lib.rs:289-430)
        length = len(message)
        state = [0] * self.width
        state[self.rate] = (length << 64) % self.m                           # initial_capacity_element
        words = list(message) + [0] * (-length % self.rate)                  # ConstantLength::padding
        absorbing = []
        for value in words:                                                   # Sponge::absorb
            if len(absorbing) < self.rate:
                absorbing.append(value)
                continue
            state = self._sponge(state, absorbing)
            absorbing = [value]
        return self._sponge(state, absorbing)[0]                              # finish_absorbing, squeeze

    def _sponge(self, state, absorbed):                                       # poseidon_sponge (lib.rs:153-174)
        state = list(state)
        for i, value in enumerate(absorbed):
            state[i] = (state[i] + value) % self.m
        return self.permute(state)

    def merkle_root(self, leaves, arity=None):
        arity = self.rate if arity is None else arity
        layer = list(leaves)
        while len(layer) > 1:
            layer = [self.hash(layer[i:i + arity]) for i in range(0, len(layer), arity)]
        return layer[0]

    def trace(self, state):
        """The chip's rows of one permutation (pow5.rs:435-597): width lists of `rows` state cells, then the partial_sbox column."""
        assert self.partial % 2 == 0
        half, rcs = self.full // 2, self.round_constants
        state = [w % self.m for w in state]
        rows, sbox = [list(state)], [0] * self.rows
        for r in range(half):
            state = self.full_round(state, rcs[r])
            rows.append(list(state))
        for i in range(self.partial // 2):
            r = half + 2 * i
            mid = [(w + rc) % self.m for w, rc in zip(state, rcs[r])]
            mid[0] = pow(mid[0], 5, self.m)
            sbox[half + i] = mid[0]
            state = self.part_round(self.apply_mds(mid), rcs[r + 1])
            rows.append(list(state))
        for r in range(half + self.partial, self.full + self.partial):
            state = self.full_round(state, rcs[r])
            rows.append(list(state))
        assert len(rows) == self.rows and state == self.permute(rows[0])
        return [[row[j] for row in rows] for j in range(self.width)] + [sbox]

    def trace_limbs(self, states):
        """(width + 1, rows * count, 4) Montgomery limbs"""
        import numpy as np

        from halo2_amd import fields
        columns = [[] for _ in range(self.width + 1)]
        for s in states:
            for j, col in enumerate(self.trace(s)):
                columns[j] += col
        return np.stack([fields.to_limbs(col, self.field, True) for col in columns])

    def states_limbs(self, states):
        from halo2_amd import fields
        return fields.to_limbs([w for s in states for w in s], self.field, True).reshape(-1, self.width, 4)

    def spec(self):
        """the library's Spec of the same parameters"""
        from halo2_amd.poseidon_spec import Spec
        return Spec(self.field, self.width, self.rate, self.full, self.partial, self.secure_mds)


@functools.lru_cache(maxsize=None)
def model(field, width, rate, full=8, partial=56, secure_mds=0):
    return Model(field, width, rate, full, partial, secure_mds)


def random_states(count, width, field, seed):
    """deterministic field elements without the library: SplitMix64 words, four to an element, reduced"""
    x = [seed & 0xFFFFFFFFFFFFFFFF]

    def word():
        x[0] = (x[0] + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = x[0]
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        return z ^ (z >> 31)
    return [[(word() | word() << 64 | word() << 128 | word() << 192) % MOD[field] for _ in range(width)] for _ in range(count)]
