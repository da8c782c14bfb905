"""Shared by test_ecc_fixed_host.py and test_gpu_ecc_fixed.py: the restatement, over `oracle.pasta`, of a fixed base's tables
(ecc/chip/constants.rs: compute_window_table, compute_lagrange_coeffs, find_zs_and_us) and of what the full-width fixed-base
multiplication assigns (ecc/chip/mul_fixed.rs:172-405, mul_fixed/full_width.rs:116-163), with the scalars and the generator's z the
tests share; below it the circuits: one per form of fixed-base multiplication, and the mirror of the reference's `MyEccCircuit`
(halo2_gadgets/src/ecc.rs, tests) whose pinned key and stored proof are tests/golden/vk_ecc_chip.rdata.gz and proof_ecc_chip.bin."""
import functools

from oracle import pasta as o

import ecc_cases as ec
from ecc_cases import ORDER, P

H = 8
NUM_WINDOWS, NUM_WINDOWS_SHORT = 85, 22
GENERATOR = (P - 1, 2)                                     # pallas::Affine::generator()
X_P, Y_P, X_QR, Y_QR, WINDOW, U = range(6)

# full_width.rs:256-260: the two window sequences whose last addition is a doubling, the second one not reduced
LAST_DOUBLING = int("1333333333333333333333333333333333333333333333333333333333333333333333333333333333334", 8)
LAST_DOUBLING_NON_CANONICAL = int("5333333333333333333333333333333333333333332711161673731021062440252244051273333333333", 8)
EDGE_SCALARS = [0, 1, ORDER - 1, (1 << 255) - 1, LAST_DOUBLING, LAST_DOUBLING_NON_CANONICAL]
EDGE_SCALARS_SHORT = [0, 1, (1 << 64) - 1, (1 << 66) - 1]  # 22 windows read 66 bits

# the z of the Pallas generator, from a host run of find_z below; the reference's pinned vk_ecc_chip commits to the same values
Z_GENERATOR_22 = [43655, 109180, 61855, 22792, 14323, 49340, 44106, 6761, 47940, 79582, 3365, 51667, 23557, 71715, 72411, 81323, 42306,
                  170594, 153399, 123967, 45210, 47381]
Z_GENERATOR_85 = Z_GENERATOR_22[:21] + [
    33828, 35916, 41584, 6170, 11193, 33522, 172258, 14241, 49210, 116579, 9614, 3395, 72959, 19163, 65943, 73370, 34409, 64584, 105594,
    55203, 153173, 1684, 45351, 94119, 122571, 34870, 23350, 216891, 6656, 38186, 119457, 14327, 48142, 8340, 38666, 196327, 39318, 236217,
    45314, 25824, 201273, 246768, 146377, 20458, 126526, 472656, 207233, 182140, 28692, 68225, 53602, 159006, 140116, 88050, 45619, 58608,
    177089, 113359, 36185, 195431, 2923, 74622, 20536, 4210]
Z_GENERATOR_2 = [43655, 5583]                             # window 1 is the last window here: other points than window 1 above
assert len(Z_GENERATOR_22) == NUM_WINDOWS_SHORT and len(Z_GENERATOR_85) == NUM_WINDOWS


def window_scalars(num_windows):
    """constants.rs:40-82 -> [w][k], integers mod q"""
    rows = [[(k + 2) * H ** w % ORDER for k in range(H)] for w in range(num_windows - 1)]
    offset = sum(1 << (3 * j + 1) for j in range(num_windows - 1))
    rows.append([(k * H ** (num_windows - 1) - offset) % ORDER for k in range(H)])
    return rows


@functools.lru_cache(maxsize=None)
def window_table(base, num_windows):
    """[w][k] = (x, y), the identity (0, 0)"""
    return [[ec.ec_mul(s, base) for s in row] for row in window_scalars(num_windows)]


def lagrange_coeffs(table):
    """constants.rs:86-106: per window the coefficients, lowest degree first, of the polynomial through (k, x(table[w][k]))"""
    basis = []
    for i in range(H):
        num, den = [1], 1
        for j in range(H):
            if j != i:
                num = [(a - j * b) % P for a, b in zip([0] + num, num + [0])]
                den = den * (i - j) % P
        inv = pow(den, -1, P)
        basis.append([c * inv % P for c in num])
    return [[sum(basis[k][c] * row[k][0] for k in range(H)) % P for c in range(H)] for row in table]


def evaluate(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % P
    return acc


def is_square(a):
    """as `sqrt().is_some()`: zero counts"""
    return a % P == 0 or pow(a % P, (P - 1) // 2, P) == 1


def z_is_valid(z, ys):
    return all(is_square(z + y) and not is_square(z - y) for y in ys)


def find_z(ys, start=0, limit=1000 << 16):
    """constants.rs:122-141: the smallest z in [start, limit) valid for the window, or None"""
    return next((z for z in range(start, limit) if z_is_valid(z, ys)), None)


def roots(table, zs):
    return [[o.sqrt_mod(pt[1] + z, P) for pt in row] for row, z in zip(table, zs)]


def windows_of(k, num_windows):
    return [k >> (3 * w) & 7 for w in range(num_windows)]


def mul_fixed_trace(table, us, k):
    """-> (columns, aux, result): columns[c][w] for x_p, y_p, x_qr, y_qr, window, u (0 where nothing is assigned); aux the nine cells
    of the closing complete addition's row and the result's two coordinates; us[w][k] may hold None where a test has no root to give"""
    nw = len(table)
    cols = [[0] * nw for _ in range(6)]
    acc = None
    for w, d in enumerate(windows_of(k, nw)):
        cols[X_P][w], cols[Y_P][w] = point = table[w][d]
        cols[WINDOW][w], cols[U][w] = d, us[w][d]
        if w == 0:
            acc = point
        else:
            cols[X_QR][w], cols[Y_QR][w] = acc
            if w < nw - 1:
                acc = ec.incomplete_add(point, acc)                             # mul_fixed.rs:355-357
                assert acc is not None
    result, witnesses = ec.complete_add(table[nw - 1][d], acc)                 # full_width.rs:150-159
    return cols, list(table[nw - 1][d] + acc + witnesses + result), result


@functools.lru_cache(maxsize=None)
def generator_tables(num_windows=NUM_WINDOWS):
    """the generator's tables on the host: the z of the lists above (each checked valid here), the roots from the oracle"""
    table = window_table(GENERATOR, num_windows)
    zs = {NUM_WINDOWS: Z_GENERATOR_85, NUM_WINDOWS_SHORT: Z_GENERATOR_22}[num_windows]
    assert all(z_is_valid(z, [pt[1] for pt in row]) for z, row in zip(zs, table))
    return table, lagrange_coeffs(table), zs, roots(table, zs)


# ---- the circuits ---------------------------------------------------------------------------------------------------------------------------
from halo2_amd.circuit import Circuit                                         # noqa: E402
from halo2_amd.gadgets.ecc import (EccChip, FixedBaseTables, FixedPoint, FixedPointBaseField, FixedPoints, FixedPointShort,      # noqa: E402
                                   Point, ScalarFixed, ScalarFixedShort)
from halo2_amd.gadgets.utilities import LookupRangeCheckConfig, load_private  # noqa: E402

GATE_NAMES_FIXED = ["range check", "Running sum coordinates check", "Full-width fixed-base scalar mul", "Short fixed-base mul gate",
                    "Canonicity checks"]


def host_tables(num_windows=NUM_WINDOWS) -> FixedBaseTables:
    table, coeffs, zs, us = generator_tables(num_windows)
    return FixedBaseTables(GENERATOR, table, coeffs, zs, us)


def configure_fixed(meta):
    """the reference's MyCircuit::configure (ecc.rs:783-812): ten advice columns, the table column, eight Lagrange columns, and the
    constants in a fixed column of their own"""
    advices = [meta.advice_column() for _ in range(10)]
    lookup_table = meta.lookup_table_column()
    lagrange = [meta.fixed_column() for _ in range(8)]
    constants = meta.fixed_column()
    meta.enable_constant(constants)
    range_check = LookupRangeCheckConfig.configure(meta, advices[9], lookup_table)
    return EccChip.configure(meta, advices, lagrange, range_check,
                             fixed_bases=FixedPoints(full_width=("generator",), short=("generator",), base_field=("generator",)))


# (column, row of the multiplication's region) a test overwrites with its value + 1
MUTATIONS = {"window": (4, 40), "u": (5, 17)}


class MulFixedCircuit(Circuit):
    """one full-width `mul_fixed` per scalar over `tables`, or all of them through one `mul_fixed_many` (many=True).  mutate: (index of
    the multiplication, a key of MUTATIONS)"""

    def __init__(self, scalars, tables, witness=True, mutate=None, many=False):
        self.scalars, self.tables, self.witness, self.mutate, self.many = scalars, tables, witness, mutate, many
        self.products, self.mutated_row, self.bulk = [], None, None

    def without_witnesses(self):
        return MulFixedCircuit(self.scalars, self.tables, witness=False, many=self.many)

    configure = staticmethod(configure_fixed)

    def synthesize(self, config, layouter):
        config.lookup_config.load_range_check_table(layouter)
        chip = EccChip(config)
        values = [k if self.witness else None for k in self.scalars]
        if self.many:
            self.bulk = chip.mul_fixed_many(layouter, self.tables, values)
            return
        base = FixedPoint.from_inner(chip, self.tables)
        self.products = [base.mul(layouter, ScalarFixed.new(chip, layouter, k)) for k in values]
        if self.mutate:
            i, what = self.mutate
            column, row = MUTATIONS[what]
            region = self.products[i][1].windows[0].cell().region_index
            self.mutated_row = layouter.regions[region] + row
            if layouter.cs.collect_advice:
                cells = layouter.cs.advice[config.advices[column].index]
                value = cells.integers(layouter.cs.n, ec.FP)[self.mutated_row]
                layouter.cs.assign_advice(config.advices[column], self.mutated_row, lambda: (value + 1) % P)


class ShortCircuit(Circuit):
    """one `mul_fixed_short` per (magnitude, sign) over the 22-window `tables` (mul_fixed/short.rs tests::test_mul_fixed_short), then
    one `mul_sign` per (point, sign) of `signed`; magnitudes and signs are elements of Fp, the sign 1 or p - 1 where it is valid"""

    def __init__(self, pairs, tables, signed=(), witness=True):
        self.pairs, self.tables, self.signed, self.witness, self.products, self.signed_points = pairs, tables, signed, witness, [], []

    def without_witnesses(self):
        return ShortCircuit(self.pairs, self.tables, self.signed, witness=False)

    configure = staticmethod(configure_fixed)

    def synthesize(self, config, layouter):
        config.lookup_config.load_range_check_table(layouter)
        chip = EccChip(config)
        v = (lambda x: x) if self.witness else (lambda x: None)
        base = FixedPointShort.from_inner(chip, self.tables)
        self.products = []
        for magnitude, sign in self.pairs:
            cells = (load_private(layouter, config.advices[0], v(magnitude)), load_private(layouter, config.advices[0], v(sign)))
            self.products.append(base.mul(layouter, ScalarFixedShort.new(chip, layouter, cells))[0])
        # the identity is a constant of the circuit, as in the reference's test_mul_sign; the other points are witnessed
        def new(pt):
            return Point.new_from_constant(chip, layouter, pt) if pt == (0, 0) else Point.new(chip, layouter, v(pt))
        self.signed_points = [new(pt).mul_sign(layouter, load_private(layouter, config.advices[0], v(sign)))
                              for pt, sign in self.signed]


T_P = P - (1 << 254)
# base_field_elem.rs tests: 0, -1, and the corners of the canonicity gate -- t_p, t_p - 1 and 2^254 - 1 with the top bit clear, 2^254
# the first value with it set
EDGE_BASE_FIELD = [0, P - 1, T_P, T_P - 1, (1 << 254) - 1, 1 << 254]


class BaseFieldCircuit(Circuit):
    """one `mul_fixed_base_field_elem` per alpha over the 85-window `tables`.  mutate: the index of the multiplication whose alpha_1
    cell (row 1 of its "Canonicity checks" region, advice 7) is overwritten with its value + 1"""

    def __init__(self, alphas, tables, witness=True, mutate=None):
        self.alphas, self.tables, self.witness, self.mutate, self.products, self.mutated_row = alphas, tables, witness, mutate, [], None

    def without_witnesses(self):
        return BaseFieldCircuit(self.alphas, self.tables, witness=False)

    configure = staticmethod(configure_fixed)

    def synthesize(self, config, layouter):
        config.lookup_config.load_range_check_table(layouter)
        chip = EccChip(config)
        base = FixedPointBaseField.from_inner(chip, self.tables)
        self.products = []
        for i, alpha in enumerate(self.alphas):
            cell = load_private(layouter, config.advices[0], alpha if self.witness else None)
            self.products.append(base.mul(layouter, cell))
            if self.mutate == i:                                              # the region laid out last is this one's canonicity check
                self.mutated_row = layouter.regions[-1] + 1
                if layouter.cs.collect_advice:
                    cells = layouter.cs.advice[config.advices[7].index]
                    value = cells.integers(layouter.cs.n, ec.FP)[self.mutated_row]
                    layouter.cs.assign_advice(config.advices[7], self.mutated_row, lambda: (value + 1) % P)


# ---- the reference's test circuit (halo2_gadgets/src/ecc.rs tests::MyEccCircuit, test_errors = false) ------------------------------------
class MyEccCircuit(Circuit):
    """The reference's synthesis order: P, -P, Q, the identity, then test_witness_non_id, test_add, test_add_incomplete, test_mul,
    test_mul_sign, test_mul_fixed, test_mul_fixed_short and test_mul_fixed_base_field of the chip's modules, region for region.  The
    pinned key depends on the shapes, fixed cells and copies, not on the witnesses, which come from `seed`.  full, short: the
    generator's tables at 85 and 22 windows.  witness=False is keygen's view; the identity, which the reference passes as a known
    value either way, stays known."""

    def __init__(self, full, short, seed=1, witness=True):
        self.full, self.short, self.seed, self.witness = full, short, seed, witness

    def without_witnesses(self):
        return MyEccCircuit(self.full, self.short, self.seed, witness=False)

    configure = staticmethod(configure_fixed)

    def synthesize(self, config, layouter):
        import random

        from halo2_amd import fields
        from halo2_amd.circuit import Synthesis
        from halo2_amd.gadgets.ecc import NonIdentityPoint, ScalarVar
        rng = random.Random(self.seed)
        chip = EccChip(config)
        column = config.advices[0]
        v = (lambda x: x) if self.witness else (lambda x: None)
        zero_pt = (0, 0)

        def neg(pt):
            return (pt[0], -pt[1] % P)

        def non_id(pt):
            return NonIdentityPoint.new(chip, layouter, v(pt))

        def must_fail(pt):
            try:
                NonIdentityPoint.new(chip, layouter, pt)
            except Synthesis:
                return
            raise AssertionError("witnessing the identity as a non-identity point should fail")

        def equal_non_id(result, expected):
            result.constrain_equal(layouter, non_id(expected))

        config.lookup_config.load_range_check_table(layouter)
        p_val, q_val = ec.random_bases(2, seed=100 + self.seed)
        p, p_neg, q = non_id(p_val), non_id(neg(p_val)), non_id(q_val)
        Point.new(chip, layouter, zero_pt)                                    # the identity as a point ...
        must_fail(zero_pt)                                                    # ... but not as a non-identity point
        must_fail(zero_pt)                                                    # witness_point.rs tests::test_witness_non_id

        # add.rs tests::test_add
        zero = p.add(layouter, p_neg)
        zero.add(layouter, zero).constrain_equal(layouter, zero)
        equal_non_id(p.add(layouter, q), ec.o.ec_add(p_val, q_val, P))
        equal_non_id(p.add(layouter, p), ec.ec_mul(2, p_val))
        p.add(layouter, zero).constrain_equal(layouter, p)
        zero.add(layouter, p).constrain_equal(layouter, p)
        zeta = fields.zeta(ec.FP)
        for endo in ((zeta * p_val[0] % P, p_val[1]), (zeta * p_val[0] % P, -p_val[1] % P),
                     (zeta * zeta * p_val[0] % P, p_val[1]), (zeta * zeta * p_val[0] % P, -p_val[1] % P)):
            p.add(layouter, non_id(endo))

        # add_incomplete.rs tests::test_add_incomplete
        equal_non_id(p.add_incomplete(layouter, q), ec.o.ec_add(p_val, q_val, P))

        # mul.rs tests::test_mul: a random scalar, zero, -1
        for scalar in (rng.randrange(P), 0, P - 1):
            cell = load_private(layouter, column, v(scalar))
            result, _ = p.mul(layouter, ScalarVar.from_base(chip, layouter, cell))
            if scalar:
                equal_non_id(result, ec.ec_mul(scalar, p_val))

        # short.rs tests::test_mul_sign
        s_val = ec.random_bases(1, seed=200 + self.seed)[0]
        s, s_neg, identity = (Point.new(chip, layouter, pt) for pt in (v(s_val), v(neg(s_val)), zero_pt))
        pos_sign = load_private(layouter, config.advices[0], v(1))
        neg_sign = load_private(layouter, config.advices[1], v(P - 1))
        s.mul_sign(layouter, pos_sign).constrain_equal(layouter, s)
        s.mul_sign(layouter, neg_sign).constrain_equal(layouter, s_neg)
        identity.mul_sign(layouter, pos_sign).constrain_equal(layouter, identity)
        identity.mul_sign(layouter, neg_sign).constrain_equal(layouter, identity)

        # full_width.rs tests::test_mul_fixed: a random scalar, the doubling string, zero, -1
        base = FixedPoint.from_inner(chip, self.full)
        for scalar in (rng.randrange(ORDER), LAST_DOUBLING, 0, ORDER - 1):
            result, _ = base.mul(layouter, ScalarFixed.new(chip, layouter, v(scalar)))
            if scalar:
                equal_non_id(result, ec.ec_mul(scalar, GENERATOR))

        # short.rs tests::test_mul_fixed_short
        short = FixedPointShort.from_inner(chip, self.short)
        top, double = (1 << 64) - 1, 0xB6DB6DB6DB6DB6DC
        pairs = [(rng.randrange(1 << 64), rng.choice((1, P - 1))), (top, 1), (top, P - 1), (double, 1), (double, P - 1), (0, 1), (0, P - 1)]
        for magnitude, sign in pairs:
            cells = (load_private(layouter, column, v(magnitude)), load_private(layouter, column, v(sign)))
            result, _ = short.mul(layouter, ScalarFixedShort.new(chip, layouter, cells))
            if magnitude:
                equal_non_id(result, ec.ec_mul(magnitude if sign == 1 else -magnitude, GENERATOR))

        # base_field_elem.rs tests::test_mul_fixed_base_field: a random element, the doubling string, zero, -1
        base_field = FixedPointBaseField.from_inner(chip, self.full)
        for scalar in (rng.randrange(P), LAST_DOUBLING, 0, P - 1):
            result = base_field.mul(layouter, load_private(layouter, column, v(scalar)))
            if scalar:
                equal_non_id(result, ec.ec_mul(scalar, GENERATOR))
