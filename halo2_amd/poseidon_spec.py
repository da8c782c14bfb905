"""Poseidon specifications over both Pasta fields: P128Pow5T3 (halo2_poseidon/src/p128pow5t3.rs: width 3, rate 2, 8 full and 56
partial rounds, S-box x^5) as module constants, and `Spec` for any other width, rate and round counts (halo2_poseidon::Spec<F, T,
RATE> with `generate_constants`).  The constants are generated here by the published parameter procedure of the Poseidon paper (Grassi,
Khovratovich, Rechberger, Roy, Schofnegger: "Poseidon: a new hash function for zero-knowledge proof systems", appendix F and the
authors' generate_parameters_grain script), not copied:

  * an 80-bit Grain LFSR, seeded most significant bit first with  field tag (2 bits) = 1 | S-box tag (4) = 0 | field size (12) = 255 |
    t (12) | R_F (10) | R_P (10) | thirty ones;  feedback b62 ^ b51 ^ b38 ^ b23 ^ b13 ^ b0;  the first 160 bits are discarded
  * the self-shrinking filter: bits are read in pairs, the second bit of a pair is emitted when the first is 1
  * a field element is 255 emitted bits, most significant first; the (R_F + R_P) * t round constants reject values >= p
  * the MDS matrix is the Cauchy matrix 1 / (x_i + y_j) of 2 t further elements drawn WITHOUT rejection (reduced mod p), redrawn
    while two of them are equal; `secure_mds` matrices are passed over and the next one drawn is used (0 for P128Pow5T3)

`constants(field)` -> (round_constants[64][3], mds[3][3], mds_inv[3][3]) as Python integers; tests/golden/poseidon_kat.json pins the
first two.  Everything the device code and the circuit gadget know about Poseidon comes from this module: csrc/gen_poseidon_consts.py
writes the table the P128Pow5T3 kernels read, a `Spec` uploads its own for the kernels of csrc/poseidon_spec.hip, and
halo2_amd/gadgets/poseidon.py builds its gates from the integers."""
from __future__ import annotations

import functools

FP, FQ = 0, 1                                               # H2_FP, H2_FQ; no import: csrc/gen_poseidon_consts.py loads this file alone

P = 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001
Q = 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001
MODULUS = {FP: P, FQ: Q}
WIDTH, RATE = 3, 2
FULL_ROUNDS, PARTIAL_ROUNDS = 8, 56
ROUNDS = FULL_ROUNDS + PARTIAL_ROUNDS
FIELD_BITS = 255
ALPHA = 5
ROWS = FULL_ROUNDS + PARTIAL_ROUNDS // 2 + 1                # rows of one permutation in the Pow5 chip: 36 gate rows and the output


class Grain:
    """The bit source of the parameter procedure."""

    def __init__(self, t: int = WIDTH, r_f: int = FULL_ROUNDS, r_p: int = PARTIAL_ROUNDS, field_bits: int = FIELD_BITS):
        bits = []
        for width, value in ((2, 1), (4, 0), (12, field_bits), (12, t), (10, r_f), (10, r_p), (30, (1 << 30) - 1)):
            bits += [(value >> (width - 1 - i)) & 1 for i in range(width)]
        self.state, self.field_bits = bits, field_bits
        for _ in range(160):
            self._step()

    def _step(self) -> int:
        s = self.state                                        # the register is the last 80 entries of a growing list
        i = len(s) - 80
        new = s[i + 62] ^ s[i + 51] ^ s[i + 38] ^ s[i + 23] ^ s[i + 13] ^ s[i]
        s.append(new)
        return new

    def bit(self) -> int:
        while not self._step():
            self._step()
        return self._step()

    def integer(self) -> int:
        v = 0
        for _ in range(self.field_bits):
            v = (v << 1) | self.bit()
        return v

    def element(self, m: int) -> int:
        while True:
            v = self.integer()
            if v < m:
                return v


def invert_matrix(a, m: int):
    """Gauss-Jordan elimination mod m."""
    n = len(a)
    rows = [[x % m for x in row] + [int(i == j) for j in range(n)] for i, row in enumerate(a)]
    for c in range(n):
        pivot = next(r for r in range(c, n) if rows[r][c])
        rows[c], rows[pivot] = rows[pivot], rows[c]
        inv = pow(rows[c][c], -1, m)
        rows[c] = [x * inv % m for x in rows[c]]
        for r in range(n):
            if r != c and rows[r][c]:
                f = rows[r][c]
                rows[r] = [(x - f * y) % m for x, y in zip(rows[r], rows[c])]
    return [row[n:] for row in rows]


def generate(m: int, t: int = WIDTH, r_f: int = FULL_ROUNDS, r_p: int = PARTIAL_ROUNDS, secure_mds: int = 0):
    """secure_mds: how many drawn matrices to pass over before the one that is used (halo2_poseidon/src/mds.rs:33-36)."""
    grain = Grain(t, r_f, r_p)
    round_constants = [[grain.element(m) for _ in range(t)] for _ in range(r_f + r_p)]
    while True:
        drawn = [grain.integer() % m for _ in range(2 * t)]
        if len(set(drawn)) != 2 * t:
            continue
        if secure_mds == 0:
            break
        secure_mds -= 1
    xs, ys = drawn[:t], drawn[t:]
    mds = [[pow(xs[i] + ys[j], -1, m) for j in range(t)] for i in range(t)]
    return round_constants, mds, invert_matrix(mds, m)


@functools.lru_cache(maxsize=None)
def constants(field: int):
    """(round_constants, mds, mds_inv) of P128Pow5T3 over Fp (field 0) or Fq (field 1)."""
    return generate(MODULUS[field])


MAX_WIDTH, MAX_ROUNDS = 12, 1024                           # H2_POSEIDON_MAX_WIDTH; full + partial rounds of one call


class Spec:
    """halo2_poseidon::Spec<F, T, RATE> with S-box x^5: a field, a width, a rate, the round counts and `secure_mds`, the number of
    drawn MDS matrices to pass over.  `round_constants`, `mds` and `mds_inv` are Python integers from the Grain procedure above.
    Spec(...) of equal parameters is the same object, so the constants are generated once and uploaded once per device.

    permute / hash / trace / merkle_root run on the device (halo2_amd/csrc/poseidon_spec.hip) and follow halo2_amd.poseidon's array
    conventions; permute_ints / hash_ints are the same on the host with Python integers."""
    _instances: dict = {}

    def __new__(cls, field: int, width: int, rate: int, full_rounds: int = FULL_ROUNDS, partial_rounds: int = PARTIAL_ROUNDS, secure_mds: int = 0):
        key = (field, width, rate, full_rounds, partial_rounds, secure_mds)
        if key in cls._instances:
            return cls._instances[key]
        if field not in MODULUS:
            raise ValueError("Spec: field is FP or FQ")
        if not (2 <= width <= MAX_WIDTH and 1 <= rate < width):
            raise ValueError(f"Spec: a width of 2 .. {MAX_WIDTH} and a rate of 1 .. width - 1")
        if full_rounds < 2 or full_rounds % 2 or partial_rounds < 0 or full_rounds + partial_rounds > MAX_ROUNDS or secure_mds < 0:
            raise ValueError(f"Spec: an even number of full rounds, at least 2, and at most {MAX_ROUNDS} rounds in all")
        self = super().__new__(cls)
        self.field, self.modulus, self.width, self.rate = field, MODULUS[field], width, rate
        self.full_rounds, self.partial_rounds, self.secure_mds = full_rounds, partial_rounds, secure_mds
        if key == (field, WIDTH, RATE, FULL_ROUNDS, PARTIAL_ROUNDS, 0):
            self.round_constants, self.mds, self.mds_inv = constants(field)
        else:
            self.round_constants, self.mds, self.mds_inv = generate(self.modulus, width, full_rounds, partial_rounds, secure_mds)
        self.rows = full_rounds + partial_rounds // 2 + 1                # of one permutation in the Pow5 chip (partial_rounds even)
        self._device_constants = {}                                      # torch device -> the table the kernels read
        cls._instances[key] = self
        return self

    @classmethod
    def p128pow5t3(cls, field: int) -> "Spec":
        return cls(field, WIDTH, RATE, FULL_ROUNDS, PARTIAL_ROUNDS, 0)

    def key(self):
        return (self.field, self.width, self.rate, self.full_rounds, self.partial_rounds, self.secure_mds)

    def __repr__(self):
        return "Spec(field=%d, width=%d, rate=%d, full_rounds=%d, partial_rounds=%d, secure_mds=%d)" % self.key()

    # ---- the host, Python integers -----------------------------------------------------------------------------------------------------
    def permute_ints(self, state):
        return permute_spec(state, self)

    def hash_ints(self, message):
        """Hash<_, S, ConstantLength<len(message)>, T, RATE> (halo2_poseidon/src/lib.rs:289-345)."""
        m, rate = self.modulus, self.rate
        state = [0] * self.width
        state[rate] = capacity(len(message)) % m
        padded = list(message) + [0] * (-len(message) % rate)
        for at in range(0, len(padded), rate):
            state = [(w + v) % m for w, v in zip(state, padded[at:at + rate])] + state[rate:]
            state = permute_spec(state, self)
        return state[0]

    # ---- the device: halo2_amd.poseidon has the bodies (this file is also loaded alone, without the package) ---------------------------------
    def permute(self, states, out=None):
        """(n, width, 4) -> (n, width, 4).  torch: `out` may be `states` itself (in place)."""
        from . import poseidon
        return poseidon.spec_permute(self, states, out)

    def hash(self, messages):                                                 # noqa: A003 -- the reference's name
        """(n, len, 4) -> (n, 4)"""
        from . import poseidon
        return poseidon.spec_hash(self, messages)

    def trace(self, states):
        """(count, width, 4) -> (width + 1, rows * count, 4): the columns state0 .. state(width - 1), partial_sbox."""
        from . import poseidon
        return poseidon.spec_trace(self, states)

    def merkle_root(self, leaves, arity: int | None = None):
        """The root of the `arity`-ary tree (default: the rate) over arity^d leaves, a node being hash(children): (n, 4) -> (4,)."""
        from . import poseidon
        return poseidon.spec_merkle_root(self, leaves, arity)


def capacity(length: int) -> int:
    """ConstantLength<L>::initial_capacity_element: L * 2^64."""
    return length << 64


def permute(state, field: int):
    """One permutation of three integers on the host: what the gadget's cell-by-cell assignment computes (`permute_spec` takes a Spec)."""
    m = MODULUS[field]
    rcs, mds, _ = constants(field)
    state = list(state)
    half = FULL_ROUNDS // 2
    for r, rc in enumerate(rcs):
        state = [(w + c) % m for w, c in zip(state, rc)]
        if r < half or r >= half + PARTIAL_ROUNDS:
            state = [pow(w, ALPHA, m) for w in state]
        else:
            state[0] = pow(state[0], ALPHA, m)
        state = [sum(mds[i][j] * state[j] for j in range(WIDTH)) % m for i in range(WIDTH)]
    return state


def permute_spec(state, spec: Spec):
    """One permutation of spec.width integers on the host (halo2_poseidon/src/lib.rs:106-151)."""
    m, width = spec.modulus, spec.width
    half = spec.full_rounds // 2
    state = list(state)
    if len(state) != width:
        raise ValueError(f"a state of {width} words")
    for r, rc in enumerate(spec.round_constants):
        state = [(w + c) % m for w, c in zip(state, rc)]
        if r < half or r >= half + spec.partial_rounds:
            state = [pow(w, ALPHA, m) for w in state]
        else:
            state[0] = pow(state[0], ALPHA, m)
        state = [sum(spec.mds[i][j] * state[j] for j in range(width)) % m for i in range(width)]
    return state
