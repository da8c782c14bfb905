"""Shared by test_ecc_host.py and test_gpu_ecc.py: the restatement, over `oracle.pasta` with affine arithmetic and inv0, of what
the ECC chip's complete addition (ecc/chip/add.rs:195-323) and variable-base multiplication (ecc/chip/mul.rs:164-382,
mul/incomplete.rs:228-373, mul/complete.rs:87-192, mul/overflow.rs:101-208) assign -- the ten advice columns of the
"variable-base scalar mul" region and the overflow check's witnesses of one multiplication -- and the scalars and bases the tests share."""
import functools
import random

from oracle import pasta as o

P = o.P                                   # Pallas base field: coordinates, and the field of the circuits
ORDER = o.Q                               # the order of the Pallas group
T_Q = ORDER - (1 << 254)
ROWS = 137
NUM_BITS = 255
HI_LEN, LO_LEN, COMPLETE_LEN = 125, 126, 3

# chip.rs:280-292 and mul.rs:71-79: the columns of complete addition and of the two incomplete halves
X_P, Y_P, X_QR, Y_QR, LAMBDA, ALPHA, BETA, GAMMA, DELTA = range(9)
HI = dict(z=9, x_a=3, lambda_1=4, lambda_2=5)
LO = dict(z=6, x_a=7, lambda_1=8, lambda_2=2)
Z_COMPLETE = 9

EDGE_SCALARS = [0, 1, 2, 3, 7, 8, 9, 15, 16, 17,
                (1 << 130) - T_Q - 1, (1 << 130) - T_Q, (1 << 130) - 1, 1 << 130,
                (1 << 254) - T_Q - 1, (1 << 254) - T_Q,
                P - 2, P - 1]


def inv0(v):
    return pow(v % P, -1, P) if v % P else 0


class Vanishing(ValueError):
    """a denominator of the incomplete range is zero, or an operand is the identity: the reference's Error::Synthesis"""


def complete_add(p, q):
    """add.rs:213-295 -> ((x_r, y_r), (lambda, alpha, beta, gamma, delta))"""
    (x_p, y_p), (x_q, y_q) = p, q
    alpha, beta, gamma = inv0(x_q - x_p), inv0(x_p), inv0(x_q)
    delta = inv0(y_q + y_p) if x_q == x_p else 0
    if x_q != x_p:
        lam = (y_q - y_p) * alpha % P
    elif y_p:
        lam = 3 * x_p * x_p * inv0(2 * y_p) % P
    else:
        lam = 0
    if x_p == 0:
        r = (x_q, y_q)
    elif x_q == 0:
        r = (x_p, y_p)
    elif x_q == x_p and y_q == -y_p % P:
        r = (0, 0)
    else:
        x_r = (lam * lam - x_p - x_q) % P
        r = (x_r, (lam * (x_p - x_r) - y_p) % P)
    return r, (lam, alpha, beta, gamma, delta)


def incomplete_add(p, q):
    """add_incomplete.rs:76-133: None where the reference errors"""
    if p == (0, 0) or q == (0, 0) or p[0] == q[0]:
        return None
    lam = (q[1] - p[1]) * inv0(q[0] - p[0]) % P
    x = (lam * lam - p[0] - q[0]) % P
    return (x, (lam * (p[0] - x) - p[1]) % P)


def decompose(alpha):
    """mul.rs:421-455: the 255 bits of k = alpha + t_q, unreduced, most significant first"""
    k = alpha + T_Q
    return [k >> i & 1 for i in range(NUM_BITS - 1, -1, -1)]


def mul_trace(base, alpha):
    """-> (columns, aux, result): columns[c][row] for the ten advice columns and ROWS rows (0 where nothing is assigned); aux the 16
    witnesses of the overflow check: s, the 14 running sums of its thirteen 10-bit words, eta; result = [alpha]base as (x, y)."""
    if base == (0, 0):
        raise Vanishing("the base is the identity")
    cols = [[0] * ROWS for _ in range(10)]
    bits = decompose(alpha)

    def put_add(row, p, q):
        r, witnesses = complete_add(p, q)
        for c, v in zip((X_P, Y_P, X_QR, Y_QR, LAMBDA, ALPHA, BETA, GAMMA, DELTA), p + q + witnesses):
            cols[c][row] = v
        cols[X_QR][row + 1], cols[Y_QR][row + 1] = r
        return r

    acc = put_add(0, base, base)                                              # mul.rs:187-189
    z = 0                                                                     # z_init at (hi.z, 1) is zero already
    zs = [z]
    for half, these in ((HI, bits[:HI_LEN]), (LO, bits[HI_LEN:HI_LEN + LO_LEN])):
        x_a, y_a = acc                                                        # incomplete.rs:240-289
        x_p, y_p = base
        if acc == (0, 0) or x_p == x_a:
            raise Vanishing("double_and_add starts on an exceptional pair")
        cols[half["z"]][1] = z
        cols[half["x_a"]][2] = x_a
        cols[half["lambda_1"]][1] = y_a
        for r, k in enumerate(these):                                         # incomplete.rs:298-362
            row = 2 + r
            z = (2 * z + k) % P
            zs.append(z)
            cols[half["z"]][row] = z
            cols[X_P][row], cols[Y_P][row] = x_p, y_p
            y = y_p if k else -y_p % P
            if (x_a - x_p) % P == 0:
                raise Vanishing(f"x_a = x_p at row {row}")
            l1 = (y_a - y) * inv0(x_a - x_p) % P
            x_r = (l1 * l1 - x_a - x_p) % P
            if (x_a - x_r) % P == 0:
                raise Vanishing(f"x_a = x_r at row {row}")
            l2 = (2 * y_a * inv0(x_a - x_r) - l1) % P
            cols[half["lambda_1"]][row], cols[half["lambda_2"]][row] = l1, l2
            x_new = (l2 * l2 - x_a - x_r) % P
            x_a, y_a = x_new, (l2 * (x_a - x_new) - y_a) % P
            cols[half["x_a"]][row + 1] = x_a
        cols[half["lambda_1"]][2 + len(these)] = y_a                          # incomplete.rs:365-370
        acc = (x_a, y_a)
    offset = 1 + LO_LEN + 2                                                   # mul.rs:233
    cols[Z_COMPLETE][offset] = z                                              # complete.rs:115-123
    for it, k in enumerate(bits[HI_LEN + LO_LEN:HI_LEN + LO_LEN + COMPLETE_LEN]):
        row = offset + 2 * it
        z = (2 * z + k) % P
        zs.append(z)
        cols[Z_COMPLETE][row + 2] = z
        cols[Z_COMPLETE][row + 1] = base[1]
        u = (base[0], base[1] if k else -base[1] % P)
        tmp = put_add(row, u, acc)
        acc = put_add(row + 1, acc, tmp)
    offset += 2 * COMPLETE_LEN                                                # mul.rs:253, process_lsb
    lsb = bits[-1]
    z = (2 * z + lsb) % P
    zs.append(z)
    cols[Z_COMPLETE][offset + 1] = z
    p = (0, 0) if lsb else (base[0], -base[1] % P)
    result = put_add(offset, p, acc)
    cols[X_P][offset + 1], cols[Y_P][offset + 1] = base
    assert offset + 2 == ROWS and len(zs) == NUM_BITS + 1
    zs.reverse()                                                              # z_0 .. z_255
    s = (alpha + zs[254] * (1 << 130)) % P                                    # overflow.rs:111-129
    aux = [s] + [s >> (10 * i) for i in range(14)] + [inv0(zs[130])]
    return cols, aux, result


def ec_mul(k, pt):
    """[k]pt with the identity as (0, 0)"""
    r = o.ec_mul(k % ORDER, None if pt == (0, 0) else pt, P) if k % ORDER else None
    return (0, 0) if r is None else r


@functools.lru_cache(maxsize=None)
def random_bases(n, seed=11):
    rng = o.SplitMix64(seed)
    return [o.synth_point(rng, P) for _ in range(n)]


def random_scalars(n, bits=255, seed=12):
    rng = random.Random(seed)
    return [rng.getrandbits(bits) for _ in range(n)]


# ---- the circuits ---------------------------------------------------------------------------------------------------------------------------
# (imported lazily by the tests that build circuits: the restatement above needs nothing of the package)
import numpy as np                                                            # noqa: E402

import mock_prover_model as model                                             # noqa: E402
from halo2_amd import circuit as front                                        # noqa: E402
from halo2_amd.circuit import Circuit                                         # noqa: E402
from halo2_amd.gadgets.ecc import EccChip, NonIdentityPoint, Point, ScalarVar  # noqa: E402
from halo2_amd.gadgets.utilities import LookupRangeCheckConfig, load_private  # noqa: E402

FP = 0
GATE_NAMES = ["witness point", "witness non-identity point", "incomplete addition", "complete addition",
              "q_mul_1 == 1 checks", "q_mul_2 == 1 checks", "q_mul_3 == 1 checks",
              "q_mul_1 == 1 checks", "q_mul_2 == 1 checks", "q_mul_3 == 1 checks",
              "Decompose scalar for complete bits of variable-base mul", "overflow checks", "LSB check"]


def configure_ecc_chip(meta):
    """the reference's test circuits (ecc.rs:783-812): ten advice columns, eight fixed ones for the Lagrange coefficients, the first of
    which holds the constants, and the range check on the last advice column"""
    advices = [meta.advice_column() for _ in range(10)]
    lookup_table = meta.lookup_table_column()
    lagrange_coeffs = [meta.fixed_column() for _ in range(8)]
    meta.enable_constant(lagrange_coeffs[0])
    range_check = LookupRangeCheckConfig.configure(meta, advices[9], lookup_table)
    return EccChip.configure(meta, advices, lagrange_coeffs, range_check)


class PointOpsCircuit(Circuit):
    """ops: ("witness", (x, y)), ("witness_non_id", (x, y)), ("add", p, q), ("add_incomplete", p, q) with (0, 0) the identity;
    ("add", p, q, r) also constrains the sum equal to a witnessed r, as the reference's test_add does.  The results are kept in
    `results` as cells"""

    def __init__(self, ops, witness=True):
        self.ops, self.witness, self.results = ops, witness, []

    def without_witnesses(self):
        return PointOpsCircuit(self.ops, witness=False)

    configure = staticmethod(configure_ecc_chip)

    def synthesize(self, config, layouter):
        config.lookup_config.load_range_check_table(layouter)
        chip = EccChip(config)
        v = (lambda pt: pt) if self.witness else (lambda pt: None)
        self.results = []
        for op in self.ops:
            if op[0] == "witness":
                self.results.append(Point.new(chip, layouter, v(op[1])))
            elif op[0] == "witness_non_id":
                self.results.append(NonIdentityPoint.new(chip, layouter, v(op[1])))
            elif op[0] == "add":
                p, q = (Point.new(chip, layouter, v(pt)) for pt in op[1:3])
                self.results.append(p.add(layouter, q))
                if len(op) == 4:
                    self.results[-1].constrain_equal(layouter, Point.new(chip, layouter, v(op[3])))
            else:
                p, q = (NonIdentityPoint.new(chip, layouter, v(pt)) for pt in op[1:])
                self.results.append(p.add_incomplete(layouter, q))


# (column, row) of the cell a test overwrites with its value + 2 (a running sum off by 2 is a bit on neither of its two rows): rows of the
# multiplication's region; eta's row is that of its overflow check
MUTATIONS = {"z_hi": (9, 50), "lambda": (4, 131), "eta": (6, 2)}


class MulCircuit(Circuit):
    """one `mul` per (base, alpha) pair; mutate: (index of the multiplication, a key of MUTATIONS): that cell is written over after
    synthesis, and `mutated_row` is the row of the circuit it sits on"""

    def __init__(self, pairs, witness=True, mutate=None):
        self.pairs, self.witness, self.mutate, self.products, self.mutated_row = pairs, witness, mutate, [], None

    def without_witnesses(self):
        return type(self)(self.pairs, witness=False)

    configure = staticmethod(configure_ecc_chip)

    def _inputs(self, config, layouter):
        config.lookup_config.load_range_check_table(layouter)
        chip = EccChip(config)
        bases = [NonIdentityPoint.new(chip, layouter, b if self.witness else None) for b, _ in self.pairs]
        alphas = [load_private(layouter, config.advices[0], a if self.witness else None) for _, a in self.pairs]
        return chip, bases, alphas

    def synthesize(self, config, layouter):
        chip, bases, alphas = self._inputs(config, layouter)
        self.products = [b.mul(layouter, ScalarVar.from_base(chip, layouter, a))[0] for b, a in zip(bases, alphas)]
        if self.mutate:
            i, what = self.mutate
            region = self.products[i].inner().x().cell().region_index + (3 if what == "eta" else 0)      # s, its range check, the gate
            self._overwrite(config, layouter, layouter.regions[region] + MUTATIONS[what][1], MUTATIONS[what][0])

    def _overwrite(self, config, layouter, row, column):
        self.mutated_row = row
        if layouter.cs.collect_advice:
            cells = layouter.cs.advice[config.advices[column].index]
            value = cells.integers(layouter.cs.n, FP)[row]
            layouter.cs.assign_advice(config.advices[column], row, lambda: (value + 2) % P)


class MulManyCircuit(MulCircuit):
    """the same multiplications through one `mul_many`; the products' cells are exposed in an instance column when `expose`"""

    def __init__(self, pairs, witness=True, mutate=None, expose=False):
        super().__init__(pairs, witness, mutate)
        self.expose, self.many = expose, None

    def without_witnesses(self):
        return MulManyCircuit(self.pairs, witness=False, expose=self.expose)

    def configure(self, meta):
        config = configure_ecc_chip(meta)
        if self.expose:
            self.instance = meta.instance_column()
            meta.enable_equality(self.instance)
        return config

    def synthesize(self, config, layouter):
        chip, bases, alphas = self._inputs(config, layouter)
        self.many = chip.mul_many(layouter, [b.inner() for b in bases], alphas)
        if self.expose:
            for i in range(len(self.pairs)):
                layouter.constrain_instance(self.many.result_x(i), self.instance, 2 * i)
                layouter.constrain_instance(self.many.result_y(i), self.instance, 2 * i + 1)
        if self.mutate:
            i, what = self.mutate
            column, row = MUTATIONS[what]
            if what == "eta":
                row += layouter.regions[self.many.region_index + 3] + 3 * i
            else:
                row += layouter.regions[self.many.region_index] + ROWS * i
            self._overwrite(config, layouter, row, column)


def host_model(circuit, k, instances=()):
    """Synthesize on the host, compress the selectors with numpy in place of the device, lower, and hand the integer columns to
    tests/mock_prover_model.py.  -> (failures, names, assembly, layouter, cs); names[g] = (gate name, constraint name) of the lowered
    polynomial g, the index a ConstraintNotSatisfied carries."""
    instances = [list(c) for c in instances]
    cs, assembly, layouter = front.synthesize(circuit, k, FP, fixed=True, advice=True, instances=instances)
    names = [(g.name, n) for g in cs.gates for n in g.constraint_names]
    sel = assembly.selectors.astype(np.int64)
    conflicts = (sel @ sel.T) > 0
    np.fill_diagonal(conflicts, False)
    combinations = cs.compress_selectors(conflicts)
    fixed = assembly.host_columns(assembly.fixed)
    for members in combinations:
        column = [0] * assembly.n
        for s, root in members:
            for row in np.flatnonzero(assembly.selectors[s]):
                column[int(row)] = root
        fixed.append(column)
    advice = assembly.host_columns(assembly.advice)
    failures = model.verify(k, front.lower(cs), fixed, advice, instances, assembly.permutation.pairs(), P)
    return failures, names, assembly, layouter, cs
