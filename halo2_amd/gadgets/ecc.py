"""The variable-base half of the ECC gadget of halo2_gadgets (src/ecc.rs, ecc/chip.rs, chip/witness_point.rs, chip/add_incomplete.rs,
chip/add.rs, chip/mul.rs, mul/incomplete.rs, mul/complete.rs, mul/overflow.rs) against `halo2_amd.circuit`, over Pallas: `EccChip`
with `witness_point`, `witness_point_non_id`, `add_incomplete`, `add` and variable-base `mul`, and the wrappers `Point`,
`NonIdentityPoint` and `ScalarVar`.

The mirror assigns cell by cell with Python integers and inv0 (x / 0 = 0, what the reference's `Assigned` evaluates to) -- the same
regions, offsets, gates, constraint names and copy constraints as the reference:

    config = EccChip.configure(meta, advices[10], lagrange_coeffs[8], range_check)
    base = NonIdentityPoint.new(chip, layouter, (x, y))
    product, scalar = base.mul(layouter, ScalarVar.from_base(chip, layouter, alpha_cell))

What the reference does not have is the bulk path: `EccChip.mul_many` lays `count` multiplications back to back in ONE region whose
ten advice columns come from the device (`halo2_amd.ecc.mul_trace`), then three bulk regions with their overflow checks; per
multiplication the same gates, cells and equality constraints as `mul`, grouped differently.

Fixed-base multiplication (full-width, short, base-field) and `CommitDomain` are not built."""
from __future__ import annotations

import numpy as np

from .. import ecc as primitive
from .. import fields
from ..circuit import AssignedCell, Cell, ConstraintSystem, Expression, Rotation, Synthesis
from .sinsemilla import DoubleAndAdd, NonIdentityEccPoint
from .utilities import K, LookupRangeCheckConfig, bool_check, ternary, value_int

FP = 0
ROWS = primitive.ROWS
NUM_BITS = 255                                                                # pallas::Scalar::NUM_BITS
NUM_COMPLETE_BITS = 3                                                         # mul.rs:27-46
INCOMPLETE_LEN = NUM_BITS - 1 - NUM_COMPLETE_BITS
INCOMPLETE_HI_LEN = INCOMPLETE_LEN // 2
INCOMPLETE_LO_LEN = INCOMPLETE_LEN - INCOMPLETE_HI_LEN
CURVE_B = 5


class EccPoint:
    """chip.rs:32-83: affine coordinates in two cells, the identity as (0, 0)."""

    def __init__(self, x: AssignedCell, y: AssignedCell):
        self._x, self._y = x, y

    def x(self) -> AssignedCell:
        return self._x

    def y(self) -> AssignedCell:
        return self._y

    @staticmethod
    def of(point) -> "EccPoint":
        """impl From<NonIdentityEccPoint> for EccPoint"""
        return point if isinstance(point, EccPoint) else EccPoint(point.x(), point.y())


def _inv0(v: int, m: int) -> int:
    return pow(v, -1, m) if v % m else 0


def _xy(point, m: int):
    """the coordinates as integers, or None where either is unknown"""
    x, y = value_int(point.x().value(), m), value_int(point.y().value(), m)
    return None if x is None or y is None else (x, y)


# ---- witness_point.rs ----------------------------------------------------------------------------------------------------------------------
class WitnessPointConfig:
    def __init__(self, q_point, q_point_non_id, x, y):
        self.q_point, self.q_point_non_id, self.x, self.y = q_point, q_point_non_id, x, y

    @staticmethod
    def configure(meta: ConstraintSystem, x, y) -> "WitnessPointConfig":    # witness_point.rs:31-86
        config = WitnessPointConfig(meta.selector(), meta.selector(), x, y)

        def curve_eqn(cells):                                                 # y^2 = x^3 + b
            x_ = cells.query_advice(config.x, Rotation.cur())
            y_ = cells.query_advice(config.y, Rotation.cur())
            return y_.square() - (x_.square() * x_) - Expression.constant(CURVE_B)

        def witness_point(cells):
            q_point = cells.query_selector(config.q_point)
            x_ = cells.query_advice(config.x, Rotation.cur())
            y_ = cells.query_advice(config.y, Rotation.cur())
            # (q_point * x) * curve_eqn, without parentheses: the shape the pinned key has
            return [("x == 0 v on_curve", q_point * x_ * curve_eqn(cells)), ("y == 0 v on_curve", q_point * y_ * curve_eqn(cells))]
        meta.create_gate("witness point", witness_point)

        def witness_non_id(cells):
            q = cells.query_selector(config.q_point_non_id)
            return [("on_curve", q * curve_eqn(cells))]
        meta.create_gate("witness non-identity point", witness_non_id)
        return config

    def point(self, value, offset: int, region) -> EccPoint:                 # witness_point.rs:121-142; the identity is (0, 0)
        self.q_point.enable(region, offset)
        x = region.assign_advice(self.x, offset, lambda: value[0])
        y = region.assign_advice(self.y, offset, lambda: value[1])
        return EccPoint(x, y)

    def point_non_id(self, value, offset: int, region) -> NonIdentityEccPoint:      # witness_point.rs:167-187
        self.q_point_non_id.enable(region, offset)
        if value is not None and tuple(value) == (0, 0):
            raise Synthesis("witness_point_non_id: the identity")
        x = region.assign_advice(self.x, offset, lambda: value[0])
        y = region.assign_advice(self.y, offset, lambda: value[1])
        return NonIdentityEccPoint(x, y)


# ---- add_incomplete.rs ---------------------------------------------------------------------------------------------------------------------
class AddIncompleteConfig:
    def __init__(self, modulus, q_add_incomplete, x_p, y_p, x_qr, y_qr):
        self.modulus, self.q_add_incomplete = modulus, q_add_incomplete
        self.x_p, self.y_p, self.x_qr, self.y_qr = x_p, y_p, x_qr, y_qr

    @staticmethod
    def configure(meta: ConstraintSystem, x_p, y_p, x_qr, y_qr) -> "AddIncompleteConfig":      # add_incomplete.rs:25-80
        for column in (x_p, y_p, x_qr, y_qr):
            meta.enable_equality(column)
        config = AddIncompleteConfig(meta.modulus, meta.selector(), x_p, y_p, x_qr, y_qr)

        def gate(cells):
            q = cells.query_selector(config.q_add_incomplete)
            x_p_ = cells.query_advice(x_p, Rotation.cur())
            y_p_ = cells.query_advice(y_p, Rotation.cur())
            x_q = cells.query_advice(x_qr, Rotation.cur())
            y_q = cells.query_advice(y_qr, Rotation.cur())
            x_r = cells.query_advice(x_qr, Rotation.next())
            y_r = cells.query_advice(y_qr, Rotation.next())
            poly1 = (x_r + x_q + x_p_) * (x_p_ - x_q) * (x_p_ - x_q) - (y_p_ - y_q).square()
            poly2 = (y_r + y_q) * (x_p_ - x_q) - (y_p_ - y_q) * (x_q - x_r)
            return [("x_r", q * poly1), ("y_r", q * poly2)]
        meta.create_gate("incomplete addition", gate)
        return config

    def assign_region(self, p, q, offset: int, region) -> NonIdentityEccPoint:      # add_incomplete.rs:82-146
        m = self.modulus
        self.q_add_incomplete.enable(region, offset)
        pv, qv = _xy(p, m), _xy(q, m)
        if pv is not None and qv is not None and (pv == (0, 0) or qv == (0, 0) or pv[0] == qv[0]):
            raise Synthesis("add_incomplete: an identity operand or equal x")
        p.x().copy_advice(region, self.x_p, offset)
        p.y().copy_advice(region, self.y_p, offset)
        q.x().copy_advice(region, self.x_qr, offset)
        q.y().copy_advice(region, self.y_qr, offset)
        r = None
        if pv is not None and qv is not None:
            lam = (qv[1] - pv[1]) * _inv0(qv[0] - pv[0], m) % m
            x_r = (lam * lam - pv[0] - qv[0]) % m
            r = (x_r, (lam * (pv[0] - x_r) - pv[1]) % m)
        x_r = region.assign_advice(self.x_qr, offset + 1, lambda: r[0])
        y_r = region.assign_advice(self.y_qr, offset + 1, lambda: r[1])
        return NonIdentityEccPoint(x_r, y_r)


# ---- add.rs ----------------------------------------------------------------------------------------------------------------------------------
def complete_add_values(p, q, m: int):
    """add.rs:213-295 on integers -> ((x_r, y_r), (lambda, alpha, beta, gamma, delta))"""
    (x_p, y_p), (x_q, y_q) = p, q
    alpha, beta, gamma = _inv0(x_q - x_p, m), _inv0(x_p, m), _inv0(x_q, m)
    delta = _inv0(y_q + y_p, m) if x_q == x_p else 0
    if x_q != x_p:
        lam = (y_q - y_p) * alpha % m
    elif y_p:
        lam = 3 * x_p * x_p * _inv0(2 * y_p, m) % m
    else:
        lam = 0
    if x_p == 0:
        r = (x_q, y_q)
    elif x_q == 0:
        r = (x_p, y_p)
    elif x_q == x_p and y_q == -y_p % m:
        r = (0, 0)
    else:
        x_r = (lam * lam - x_p - x_q) % m
        r = (x_r, (lam * (x_p - x_r) - y_p) % m)
    return r, (lam, alpha, beta, gamma, delta)


class AddConfig:
    def __init__(self, modulus, q_add, x_p, y_p, x_qr, y_qr, lambda_, alpha, beta, gamma, delta):
        self.modulus, self.q_add = modulus, q_add
        self.x_p, self.y_p, self.x_qr, self.y_qr = x_p, y_p, x_qr, y_qr
        self.lambda_, self.alpha, self.beta, self.gamma, self.delta = lambda_, alpha, beta, gamma, delta

    def output_columns(self) -> set:
        return {self.x_qr, self.y_qr}

    @staticmethod
    def configure(meta: ConstraintSystem, x_p, y_p, x_qr, y_qr, lambda_, alpha, beta, gamma, delta) -> "AddConfig":      # add.rs:38-193
        for column in (x_p, y_p, x_qr, y_qr):
            meta.enable_equality(column)
        config = AddConfig(meta.modulus, meta.selector(), x_p, y_p, x_qr, y_qr, lambda_, alpha, beta, gamma, delta)

        def gate(cells):
            q_add = cells.query_selector(config.q_add)
            x_p_ = cells.query_advice(x_p, Rotation.cur())
            y_p_ = cells.query_advice(y_p, Rotation.cur())
            x_q = cells.query_advice(x_qr, Rotation.cur())
            y_q = cells.query_advice(y_qr, Rotation.cur())
            x_r = cells.query_advice(x_qr, Rotation.next())
            y_r = cells.query_advice(y_qr, Rotation.next())
            lam = cells.query_advice(lambda_, Rotation.cur())
            alpha_ = cells.query_advice(alpha, Rotation.cur())               # inv0(x_q - x_p)
            beta_ = cells.query_advice(beta, Rotation.cur())                 # inv0(x_p)
            gamma_ = cells.query_advice(gamma, Rotation.cur())               # inv0(x_q)
            delta_ = cells.query_advice(delta, Rotation.cur())               # inv0(y_p + y_q) if x_q = x_p, 0 otherwise
            x_q_minus_x_p = x_q - x_p_
            x_p_minus_x_r = x_p_ - x_r
            y_q_plus_y_p = y_q + y_p_
            if_alpha = x_q_minus_x_p * alpha_
            if_beta = x_p_ * beta_
            if_gamma = x_q * gamma_
            if_delta = y_q_plus_y_p * delta_
            one, two, three = Expression.constant(1), Expression.constant(2), Expression.constant(3)
            y_q_minus_y_p = y_q - y_p_
            incomplete = x_q_minus_x_p * lam - y_q_minus_y_p
            poly1 = x_q_minus_x_p * incomplete
            three_x_p_sq = three * x_p_.square()
            two_y_p = two * y_p_
            tangent_line = two_y_p * lam - three_x_p_sq
            poly2 = (one - if_alpha) * tangent_line
            nonexceptional_x_r = lam.square() - x_p_ - x_q - x_r
            nonexceptional_y_r = lam * x_p_minus_x_r - y_p_ - y_r
            poly3a = x_p_ * x_q * x_q_minus_x_p * nonexceptional_x_r
            poly3b = x_p_ * x_q * x_q_minus_x_p * nonexceptional_y_r
            poly3c = x_p_ * x_q * y_q_plus_y_p * nonexceptional_x_r
            poly3d = x_p_ * x_q * y_q_plus_y_p * nonexceptional_y_r
            poly4a = (one - if_beta) * (x_r - x_q)
            poly4b = (one - if_beta) * (y_r - y_q)
            poly5a = (one - if_gamma) * (x_r - x_p_)
            poly5b = (one - if_gamma) * (y_r - y_p_)
            poly6a = (one - if_alpha - if_delta) * x_r
            poly6b = (one - if_alpha - if_delta) * y_r
            names = ("1", "2", "3a", "3b", "3c", "3d", "4a", "4b", "5a", "5b", "6a", "6b")
            polys = (poly1, poly2, poly3a, poly3b, poly3c, poly3d, poly4a, poly4b, poly5a, poly5b, poly6a, poly6b)
            return [(name, q_add * poly) for name, poly in zip(names, polys)]
        meta.create_gate("complete addition", gate)
        return config

    def assign_region(self, p: EccPoint, q: EccPoint, offset: int, region) -> EccPoint:      # add.rs:195-323
        m = self.modulus
        self.q_add.enable(region, offset)
        p.x().copy_advice(region, self.x_p, offset)
        p.y().copy_advice(region, self.y_p, offset)
        q.x().copy_advice(region, self.x_qr, offset)
        q.y().copy_advice(region, self.y_qr, offset)
        pv, qv = _xy(p, m), _xy(q, m)
        r, w = (None, None) if pv is None or qv is None else complete_add_values(pv, qv, m)
        for column, index in ((self.alpha, 1), (self.beta, 2), (self.gamma, 3), (self.delta, 4), (self.lambda_, 0)):
            region.assign_advice(column, offset, lambda i=index: w[i])
        x_r = region.assign_advice(self.x_qr, offset + 1, lambda: r[0])
        y_r = region.assign_advice(self.y_qr, offset + 1, lambda: r[1])
        return EccPoint(x_r, y_r)


# ---- mul/incomplete.rs ---------------------------------------------------------------------------------------------------------------------
class IncompleteConfig:
    def __init__(self, modulus, num_bits, q_mul_1, q_mul_2, q_mul_3, z, double_and_add, y_p):
        self.modulus, self.num_bits = modulus, num_bits
        self.q_mul_1, self.q_mul_2, self.q_mul_3, self.z, self.double_and_add, self.y_p = q_mul_1, q_mul_2, q_mul_3, z, double_and_add, y_p

    @staticmethod
    def configure(meta: ConstraintSystem, num_bits, z, x_a, x_p, y_p, lambda_1, lambda_2) -> "IncompleteConfig":      # incomplete.rs:75-218
        meta.enable_equality(z)
        meta.enable_equality(lambda_1)
        config = IncompleteConfig(meta.modulus, num_bits, meta.selector(), meta.selector(), meta.selector(), z,
                                  DoubleAndAdd(x_a, x_p, lambda_1, lambda_2), y_p)
        dna = config.double_and_add
        two_inv = pow(2, -1, meta.modulus)

        def y_a(cells, rotation):                                             # y_A = (lambda_1 + lambda_2) (x_a - x_r) / 2
            return dna.Y_A(cells, rotation) * two_inv

        def for_loop(cells, y_a_next):
            one = Expression.constant(1)
            z_cur = cells.query_advice(config.z, Rotation.cur())
            z_prev = cells.query_advice(config.z, Rotation.prev())
            x_a_cur = cells.query_advice(dna.x_a, Rotation.cur())
            x_a_next = cells.query_advice(dna.x_a, Rotation.next())
            x_p_cur = cells.query_advice(dna.x_p, Rotation.cur())
            y_p_cur = cells.query_advice(config.y_p, Rotation.cur())
            lambda1_cur = cells.query_advice(dna.lambda_1, Rotation.cur())
            lambda2_cur = cells.query_advice(dna.lambda_2, Rotation.cur())
            y_a_cur = y_a(cells, Rotation.cur())
            k = z_cur - z_prev * 2                                            # k_i = z_i - 2 z_{i+1}
            check = bool_check(k)
            gradient_1 = lambda1_cur * (x_a_cur - x_p_cur) - y_a_cur + (k * 2 - one) * y_p_cur
            secant_line = lambda2_cur.square() - x_a_next - dna.x_r(cells, Rotation.cur()) - x_a_cur
            gradient_2 = lambda2_cur * (x_a_cur - x_a_next) - y_a_cur - y_a_next
            return [("bool_check", check), ("gradient_1", gradient_1), ("secant_line", secant_line), ("gradient_2", gradient_2)]

        def q_mul_1(cells):
            q = cells.query_selector(config.q_mul_1)
            y_a_next = y_a(cells, Rotation.next())
            y_a_witnessed = cells.query_advice(dna.lambda_1, Rotation.cur())
            return [("init y_a", q * (y_a_witnessed - y_a_next))]
        meta.create_gate("q_mul_1 == 1 checks", q_mul_1)

        def q_mul_2(cells):
            q = cells.query_selector(config.q_mul_2)
            y_a_next = y_a(cells, Rotation.next())
            x_p_cur = cells.query_advice(dna.x_p, Rotation.cur())
            x_p_next = cells.query_advice(dna.x_p, Rotation.next())
            y_p_cur = cells.query_advice(config.y_p, Rotation.cur())
            y_p_next = cells.query_advice(config.y_p, Rotation.next())
            checks = [("x_p_check", x_p_cur - x_p_next), ("y_p_check", y_p_cur - y_p_next)] + for_loop(cells, y_a_next)
            return [(name, q * poly) for name, poly in checks]
        meta.create_gate("q_mul_2 == 1 checks", q_mul_2)

        def q_mul_3(cells):
            q = cells.query_selector(config.q_mul_3)
            y_a_final = cells.query_advice(dna.lambda_1, Rotation.next())
            return [(name, q * poly) for name, poly in for_loop(cells, y_a_final)]
        meta.create_gate("q_mul_3 == 1 checks", q_mul_3)
        return config

    def assign(self, region, offset: int, base: NonIdentityEccPoint, bits, acc):      # incomplete.rs:228-373, double_and_add
        """acc: (x cell, y cell, z cell).  -> (x_a cell, y_a cell, the z cells of this half)"""
        m, dna, n = self.modulus, self.double_and_add, self.num_bits
        assert len(bits) == n
        base_v = _xy(base, m)
        acc_v = _xy(EccPoint(acc[0], acc[1]), m)
        if base_v is not None and acc_v is not None and (base_v == (0, 0) or acc_v == (0, 0) or base_v[0] == acc_v[0]):
            raise Synthesis("double_and_add: an identity operand or equal x")
        self.q_mul_1.enable(region, offset)
        for idx in range(n - 1):
            self.q_mul_2.enable(region, offset + 1 + idx)
        self.q_mul_3.enable(region, offset + n)
        z = acc[2].copy_advice(region, self.z, offset)
        x_a = acc[0].copy_advice(region, dna.x_a, offset + 1)
        acc[1].copy_advice(region, dna.lambda_1, offset)
        known = base_v is not None and acc_v is not None and bits[0] is not None
        z_v = value_int(z.value(), m)
        x_a_v, y_a_v = acc_v if known else (None, None)
        x_p, y_p = base_v if known else (None, None)
        offset += 1
        zs = []
        for row, k in enumerate(bits):
            if known:
                z_v = (2 * z_v + k) % m
            z = region.assign_advice(self.z, row + offset, lambda v=z_v: v)
            zs.append(z)
            region.assign_advice(dna.x_p, row + offset, lambda: x_p)
            region.assign_advice(self.y_p, row + offset, lambda: y_p)
            lambda_1 = lambda_2 = x_a_new = None
            if known:
                y = y_p if k else -y_p % m
                lambda_1 = (y_a_v - y) * _inv0(x_a_v - x_p, m) % m
                x_r = (lambda_1 * lambda_1 - x_a_v - x_p) % m
                lambda_2 = (2 * y_a_v * _inv0(x_a_v - x_r, m) - lambda_1) % m
                x_a_new = (lambda_2 * lambda_2 - x_a_v - x_r) % m
                y_a_v = (lambda_2 * (x_a_v - x_a_new) - y_a_v) % m
                x_a_v = x_a_new
            region.assign_advice(dna.lambda_1, row + offset, lambda v=lambda_1: v)
            region.assign_advice(dna.lambda_2, row + offset, lambda v=lambda_2: v)
            x_a = region.assign_advice(dna.x_a, row + offset + 1, lambda v=x_a_new: v)
        y_a = region.assign_advice(dna.lambda_1, offset + n, lambda: y_a_v)
        return x_a, y_a, zs


# ---- mul/complete.rs -----------------------------------------------------------------------------------------------------------------------
class CompleteConfig:
    def __init__(self, modulus, q_mul_decompose_var, z_complete, add_config):
        self.modulus, self.q_mul_decompose_var, self.z_complete, self.add_config = modulus, q_mul_decompose_var, z_complete, add_config

    @staticmethod
    def configure(meta: ConstraintSystem, z_complete, add_config: AddConfig) -> "CompleteConfig":      # complete.rs:24-82
        meta.enable_equality(z_complete)
        config = CompleteConfig(meta.modulus, meta.selector(), z_complete, add_config)

        def gate(cells):
            q = cells.query_selector(config.q_mul_decompose_var)
            z_prev = cells.query_advice(z_complete, Rotation.prev())
            z_next = cells.query_advice(z_complete, Rotation.next())
            k = z_next - Expression.constant(2) * z_prev                      # k_i = z_i - 2 z_{i+1}
            check = bool_check(k)
            base_y = cells.query_advice(z_complete, Rotation.cur())
            y_p = cells.query_advice(add_config.y_p, Rotation.prev())
            y_switch = ternary(k, base_y - y_p, base_y + y_p)                 # k_i = 0: y_p = -base_y; k_i = 1: y_p = base_y
            return [("bool_check", q * check), ("y_switch", q * y_switch)]
        meta.create_gate("Decompose scalar for complete bits of variable-base mul", gate)
        return config

    def assign_region(self, region, offset: int, bits, base: EccPoint, x_a, y_a, z):      # complete.rs:87-192
        m = self.modulus
        assert len(bits) == NUM_COMPLETE_BITS
        for row in range(NUM_COMPLETE_BITS):
            self.q_mul_decompose_var.enable(region, 2 * row + offset + 1)
        acc = EccPoint(x_a, y_a)
        z = z.copy_advice(region, self.z_complete, offset)
        z_v = value_int(z.value(), m)
        zs = []
        for it, k in enumerate(bits):
            row = 2 * it
            z_v = None if z_v is None or k is None else (2 * z_v + k) % m
            z = region.assign_advice(self.z_complete, row + offset + 2, lambda v=z_v: v)
            zs.append(z)
            base_y = base.y().copy_advice(region, self.z_complete, row + offset + 1)
            b = value_int(base_y.value(), m)
            y_p_v = None if b is None or k is None else (b if k else -b % m)
            y_p = region.assign_advice(self.add_config.y_p, row + offset, lambda v=y_p_v: v)
            u = EccPoint(base.x(), y_p)
            tmp_acc = self.add_config.assign_region(u, acc, row + offset, region)
            acc = self.add_config.assign_region(acc, tmp_acc, row + offset + 1, region)
        return acc, zs


# ---- mul/overflow.rs -----------------------------------------------------------------------------------------------------------------------
class OverflowConfig:
    def __init__(self, modulus, q_mul_overflow, lookup_config, advices):
        self.modulus, self.q_mul_overflow, self.lookup_config, self.advices = modulus, q_mul_overflow, lookup_config, list(advices)

    @staticmethod
    def configure(meta: ConstraintSystem, lookup_config: LookupRangeCheckConfig, advices) -> "OverflowConfig":      # overflow.rs:29-99
        for advice in advices:
            meta.enable_equality(advice)
        config = OverflowConfig(meta.modulus, meta.selector(), lookup_config, advices)
        a = config.advices
        t_q = _t_q(meta.modulus)

        def gate(cells):
            q = cells.query_selector(config.q_mul_overflow)
            one = Expression.constant(1)
            two_pow_124 = Expression.constant(1 << 124)
            two_pow_130 = two_pow_124 * Expression.constant(1 << 6)
            z_0 = cells.query_advice(a[0], Rotation.prev())
            z_130 = cells.query_advice(a[0], Rotation.cur())
            eta = cells.query_advice(a[0], Rotation.next())
            k_254 = cells.query_advice(a[1], Rotation.prev())
            alpha = cells.query_advice(a[1], Rotation.cur())
            s_minus_lo_130 = cells.query_advice(a[1], Rotation.next())
            s = cells.query_advice(a[2], Rotation.cur())
            s_check = s - (alpha + k_254 * two_pow_130)
            recovery = z_0 - alpha - Expression.constant(t_q)                 # z_0 = alpha + t_q (mod p)
            lo_zero = k_254 * (z_130 - two_pow_124)
            s_minus_lo_130_check = k_254 * s_minus_lo_130
            canonicity = (one - k_254) * (one - z_130 * eta) * s_minus_lo_130
            checks = (("s_check", s_check), ("recovery", recovery), ("lo_zero", lo_zero), ("s_minus_lo_130_check", s_minus_lo_130_check),
                      ("canonicity", canonicity))
            return [(name, q * poly) for name, poly in checks]
        meta.create_gate("overflow checks", gate)
        return config

    def overflow_check(self, layouter, alpha: AssignedCell, zs) -> None:     # overflow.rs:101-208; zs = [z_0 .. z_255]
        m, a = self.modulus, self.advices
        alpha_v, k_254_v = value_int(alpha.value(), m), value_int(zs[254].value(), m)
        s_val = None if alpha_v is None or k_254_v is None else (alpha_v + k_254_v * (1 << 130)) % m
        s = layouter.assign_region("s = alpha + k_254 ⋅ 2^130", lambda region: region.assign_advice(a[0], 0, lambda: s_val))
        s_minus_lo_130 = self.lookup_config.copy_check(layouter, s, 130 // K, False)[-1]
        z_130_v = value_int(zs[130].value(), m)

        def assign(region):
            self.q_mul_overflow.enable(region, 1)
            zs[0].copy_advice(region, a[0], 0)
            zs[130].copy_advice(region, a[0], 1)
            region.assign_advice(a[0], 2, lambda: _inv0(z_130_v, m))          # eta = inv0(z_130)
            zs[254].copy_advice(region, a[1], 0)
            alpha.copy_advice(region, a[1], 1)
            s_minus_lo_130.copy_advice(region, a[1], 2)
            s.copy_advice(region, a[2], 1)
        layouter.assign_region("overflow check", assign)


def _t_q(modulus: int) -> int:
    """q = 2^254 + t_q, the order of the curve over the field of this modulus (the other Pasta modulus)"""
    p, q = fields.MODULUS[0], fields.MODULUS[1]
    return (q if modulus == p else p) - (1 << 254)


def decompose_for_scalar_mul(alpha, t_q: int) -> list:
    """mul.rs:421-455: the 255 bits of k = alpha + t_q, not reduced, most significant first; None without a value"""
    if alpha is None:
        return [None] * NUM_BITS
    k = alpha + t_q
    return [k >> i & 1 for i in range(NUM_BITS - 1, -1, -1)]


# ---- mul.rs ----------------------------------------------------------------------------------------------------------------------------------
class MulConfig:
    def __init__(self, modulus, q_mul_lsb, add_config, hi_config, lo_config, complete_config, overflow_config):
        self.modulus, self.q_mul_lsb, self.add_config = modulus, q_mul_lsb, add_config
        self.hi_config, self.lo_config, self.complete_config, self.overflow_config = hi_config, lo_config, complete_config, overflow_config
        self.t_q = _t_q(modulus)

    @staticmethod
    def configure(meta: ConstraintSystem, add_config: AddConfig, lookup_config, advices) -> "MulConfig":      # mul.rs:65-162
        a = advices
        hi_config = IncompleteConfig.configure(meta, INCOMPLETE_HI_LEN, a[9], a[3], a[0], a[1], a[4], a[5])
        lo_config = IncompleteConfig.configure(meta, INCOMPLETE_LO_LEN, a[6], a[7], a[0], a[1], a[8], a[2])
        complete_config = CompleteConfig.configure(meta, a[9], add_config)
        overflow_config = OverflowConfig.configure(meta, lookup_config, a[6:9])
        config = MulConfig(meta.modulus, meta.selector(), add_config, hi_config, lo_config, complete_config, overflow_config)

        def lsb(cells):                                                       # lsb = 0: (x, y) = (x_p, -y_p); lsb = 1: (0, 0)
            q = cells.query_selector(config.q_mul_lsb)
            z_1 = cells.query_advice(complete_config.z_complete, Rotation.cur())
            z_0 = cells.query_advice(complete_config.z_complete, Rotation.next())
            x_p = cells.query_advice(add_config.x_p, Rotation.cur())
            y_p = cells.query_advice(add_config.y_p, Rotation.cur())
            base_x = cells.query_advice(add_config.x_p, Rotation.next())
            base_y = cells.query_advice(add_config.y_p, Rotation.next())
            bit = z_0 - z_1 * 2
            check = bool_check(bit)
            lsb_x = ternary(bit, x_p, x_p - base_x)
            lsb_y = ternary(bit, y_p, y_p + base_y)
            return [("bool_check", q * check), ("lsb_x", q * lsb_x), ("lsb_y", q * lsb_y)]
        meta.create_gate("LSB check", lsb)
        assert hi_config.double_and_add.x_p == lo_config.double_and_add.x_p and hi_config.y_p == lo_config.y_p
        outputs = add_config.output_columns()
        for half in (hi_config, lo_config):
            assert half.z not in outputs and half.double_and_add.lambda_1 not in outputs
        return config

    def assign(self, layouter, alpha: AssignedCell, base: NonIdentityEccPoint):      # mul.rs:164-302
        m = self.modulus
        bits = decompose_for_scalar_mul(value_int(alpha.value(), m), self.t_q)

        def assign(region):
            base_point = EccPoint.of(base)
            acc = self.add_config.assign_region(base_point, base_point, 0, region)
            offset = 1
            z_init = region.assign_advice_from_constant(self.hi_config.z, offset, 0)
            x_a, y_a, zs_hi = self.hi_config.assign(region, offset, base, bits[:INCOMPLETE_HI_LEN], (acc.x(), acc.y(), z_init))
            x_a, y_a, zs_lo = self.lo_config.assign(region, offset, base, bits[INCOMPLETE_HI_LEN:INCOMPLETE_LEN], (x_a, y_a, zs_hi[-1]))
            offset += INCOMPLETE_LO_LEN + 2
            acc, zs_complete = self.complete_config.assign_region(region, offset, bits[INCOMPLETE_LEN:INCOMPLETE_LEN + NUM_COMPLETE_BITS],
                                                                  base_point, x_a, y_a, zs_lo[-1])
            offset += NUM_COMPLETE_BITS * 2
            result, z_0 = self._process_lsb(region, offset, base, acc, zs_complete[-1], bits[-1])
            zs = [z_init] + zs_hi + zs_lo + zs_complete + [z_0]
            assert len(zs) == NUM_BITS + 1
            zs.reverse()                                                      # z_0 .. z_255
            return result, zs
        result, zs = layouter.assign_region("variable-base scalar mul", assign)
        self.overflow_config.overflow_check(layouter, alpha, zs)
        return result, ScalarVar(alpha)

    def _process_lsb(self, region, offset: int, base, acc: EccPoint, z_1: AssignedCell, lsb):      # mul.rs:321-382
        m = self.modulus
        self.q_mul_lsb.enable(region, offset)
        z_1_v = value_int(z_1.value(), m)
        z_0 = region.assign_advice(self.complete_config.z_complete, offset + 1,
                                   lambda: None if z_1_v is None or lsb is None else (2 * z_1_v + lsb) % m)
        base.x().copy_advice(region, self.add_config.x_p, offset + 1)
        base.y().copy_advice(region, self.add_config.y_p, offset + 1)
        base_v = _xy(base, m)
        p_v = None if base_v is None or lsb is None else ((0, 0) if lsb else (base_v[0], -base_v[1] % m))
        x = region.assign_advice(self.add_config.x_p, offset, lambda: p_v[0])
        y = region.assign_advice(self.add_config.y_p, offset, lambda: p_v[1])
        return self.add_config.assign_region(EccPoint(x, y), acc, offset, region), z_0


# ---- chip.rs -------------------------------------------------------------------------------------------------------------------------------
class EccConfig:
    def __init__(self, advices, add_incomplete, add, mul, witness_point, lookup_config, lagrange_coeffs):
        self.advices, self.add_incomplete, self.add, self.mul = list(advices), add_incomplete, add, mul
        self.witness_point, self.lookup_config, self.lagrange_coeffs = witness_point, lookup_config, list(lagrange_coeffs)


class ScalarVar:
    """chip.rs ScalarVar::BaseFieldElem: a scalar of variable-base multiplication given as an element of the base field."""

    def __init__(self, cell: AssignedCell):
        self.cell = cell

    @staticmethod
    def from_base(chip, layouter, base: AssignedCell) -> "ScalarVar":        # ecc.rs:233-245, chip.rs scalar_var_from_base
        return ScalarVar(base)


class MulMany:
    """What `mul_many` returns: the cells of multiplication i by position.  outputs: (count, 2, 4) Montgomery x and y of the products
    (None without a witness)."""

    def __init__(self, region_index, config: EccConfig, count: int, outputs):
        self.region_index, self.config, self.count, self.outputs = region_index, config, count, outputs
        self.alpha_cells = None

    def result_x(self, i: int) -> Cell:
        return Cell(self.region_index, ROWS * i + ROWS - 1, self.config.add.x_qr)

    def result_y(self, i: int) -> Cell:
        return Cell(self.region_index, ROWS * i + ROWS - 1, self.config.add.y_qr)

    def alpha(self, i: int) -> Cell:
        """the copy of alpha_i in its overflow check"""
        return self.alpha_cells.cell(3 * i + 1)


class EccChip:
    def __init__(self, config: EccConfig):
        self.config = config

    @staticmethod
    def configure(meta: ConstraintSystem, advices, lagrange_coeffs, range_check: LookupRangeCheckConfig) -> EccConfig:
        """chip.rs:273-333, the variable-base part: the gates of witness_point, add_incomplete, add and mul (hi, lo, complete, overflow,
        then the LSB gate) on the reference's columns, with enable_equality, selectors and gates created in the reference's order.
        The fixed-base configs are NOT created and `lagrange_coeffs` is stored unused: a follow-up appends the fixed-base gates after
        these, and only then does a circuit reproduce the reference's pinned vk_ecc_chip."""
        a = list(advices)
        assert len(a) == 10 and len(lagrange_coeffs) == 8
        witness_point = WitnessPointConfig.configure(meta, a[0], a[1])
        add_incomplete = AddIncompleteConfig.configure(meta, a[0], a[1], a[2], a[3])
        add = AddConfig.configure(meta, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8])
        mul = MulConfig.configure(meta, add, range_check, a)
        return EccConfig(a, add_incomplete, add, mul, witness_point, range_check, lagrange_coeffs)

    # ---- EccInstructions (chip.rs:431-600) -------------------------------------------------------------------------------------------------
    def constrain_equal(self, layouter, a, b) -> None:
        def assign(region):
            region.constrain_equal(a.x().cell(), b.x().cell())
            region.constrain_equal(a.y().cell(), b.y().cell())
        layouter.assign_region("constrain equal", assign)

    def witness_point(self, layouter, value) -> EccPoint:
        """value: (x, y) integers, (0, 0) or None for the identity... None alone is an unknown value"""
        return layouter.assign_region("witness point", lambda region: self.config.witness_point.point(value, 0, region))

    def witness_point_non_id(self, layouter, value) -> NonIdentityEccPoint:
        return layouter.assign_region("witness non-identity point", lambda region: self.config.witness_point.point_non_id(value, 0, region))

    @staticmethod
    def extract_p(point) -> AssignedCell:
        return point.x()

    def add_incomplete(self, layouter, a: NonIdentityEccPoint, b: NonIdentityEccPoint) -> NonIdentityEccPoint:
        return layouter.assign_region("incomplete point addition", lambda region: self.config.add_incomplete.assign_region(a, b, 0, region))

    def add(self, layouter, a, b) -> EccPoint:
        return layouter.assign_region("complete point addition",
                                      lambda region: self.config.add.assign_region(EccPoint.of(a), EccPoint.of(b), 0, region))

    def mul(self, layouter, scalar, base: NonIdentityEccPoint):
        """scalar: the AssignedCell of alpha, or a ScalarVar.  -> (EccPoint, ScalarVar)"""
        alpha = scalar.cell if isinstance(scalar, ScalarVar) else scalar
        return self.config.mul.assign(layouter, alpha, base)

    # ---- the bulk path ---------------------------------------------------------------------------------------------------------------------
    def mul_many(self, layouter, bases, alphas, values=None, trace=None) -> MulMany:
        """`count` multiplications [alpha_i] base_i: ONE region of ROWS * count rows whose ten advice columns come from the device,
        then three bulk regions with the overflow checks (the s cells; the 14-row range checks of s; the 3-row gate blocks).  Per
        multiplication the gates, cells and equality constraints of `mul`.

        bases: NonIdentityEccPoint cells; alphas: AssignedCells.  values: (bases (count, 8), alphas (count, 4)) Montgomery limbs where
        the caller has them on the device already (else they are read from the cells); trace: (columns, aux) where the caller has them
        (else `ecc.mul_trace`, once).  Without a witness (keygen) the same shape is laid out and nothing is launched."""
        import torch
        c, m = self.config, self.config.mul.modulus
        count = len(bases)
        if len(alphas) != count:
            raise ValueError("mul_many: as many alphas as bases")
        backend = layouter.cs
        total = ROWS * count
        if not backend.collect_advice:
            trace = None
        elif trace is None and count:
            if values is None:
                pts, ints = [_xy(b, m) for b in bases], [value_int(a.value(), m) for a in alphas]
                if any(p is None for p in pts) or any(v is None for v in ints):
                    raise Synthesis("mul_many: a witness is needed and there is none")
                values = (fields.to_limbs([v for p in pts for v in p], FP).reshape(count, 8), fields.to_limbs(ints, FP))
            on_device = [v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint64).view(np.int64))
                         .to(fields.current_device()) for v in values]
            try:
                trace = primitive.mul_trace(on_device[0], on_device[1])
            except primitive.Vanishing as e:
                raise Synthesis(str(e)) from e
        columns = aux = None
        if trace is not None:
            columns, aux = [t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t, dtype=np.uint64).view(np.int64))
                            for t in trace]
            if tuple(columns.shape) != (10, total, 4) or tuple(aux.shape) != (count, primitive.AUX, 4):
                raise ValueError("mul_many: the trace is ((10, ROWS * count, 4), (count, 16, 4))")

        def blank(rows):
            return np.broadcast_to(np.zeros((1, 4), dtype=np.uint64), (rows, 4))
        add, mul = c.add, c.mul
        hi, lo, complete, overflow = mul.hi_config, mul.lo_config, mul.complete_config, mul.overflow_config
        a = c.advices
        base_rows = ROWS * np.arange(count, dtype=np.int64)

        def rows_of(offsets):
            return (base_rows[:, None] + np.asarray(offsets, dtype=np.int64)[None, :]).reshape(-1)
        complete_at = 1 + INCOMPLETE_LO_LEN + 2                              # row 129
        lsb_at = complete_at + 2 * NUM_COMPLETE_BITS                          # row 135
        result = MulMany(None, c, count, None)

        def assign(region):
            index = region.region_index

            def cell(i, row, column):
                return Cell(index, ROWS * i + row, column)
            for j, column in enumerate(a):
                region.assign_advice_column(column, 0, blank(total) if columns is None else columns[j])
            region.enable_selector_rows(add.q_add, rows_of([0] + list(range(complete_at, lsb_at + 1))))
            for half in (hi, lo):
                n = half.num_bits
                region.enable_selector_rows(half.q_mul_1, rows_of([1]))
                region.enable_selector_rows(half.q_mul_2, rows_of(range(2, 2 + n - 1)))
                region.enable_selector_rows(half.q_mul_3, rows_of([1 + n]))
            region.enable_selector_rows(complete.q_mul_decompose_var, rows_of([complete_at + 2 * r + 1 for r in range(NUM_COMPLETE_BITS)]))
            region.enable_selector_rows(mul.q_mul_lsb, rows_of([lsb_at]))
            for i in range(count):
                bx, by = bases[i].x().cell(), bases[i].y().cell()
                # row 0: P + P copies the base four times (add.rs:205-211)
                for column, src in ((add.x_p, bx), (add.y_p, by), (add.x_qr, bx), (add.y_qr, by)):
                    region.constrain_equal(cell(i, 0, column), src)
                region.constrain_constant(cell(i, 1, hi.z), 0)                # z_init (mul.rs:200-205)
                # the hi half starts on [2]P (incomplete.rs:270-289; its z copies z_init onto itself)
                region.constrain_equal(cell(i, 2, hi.double_and_add.x_a), cell(i, 1, add.x_qr))
                region.constrain_equal(cell(i, 1, hi.double_and_add.lambda_1), cell(i, 1, add.y_qr))
                # the lo half starts where the hi half ends
                hi_end = 2 + INCOMPLETE_HI_LEN
                region.constrain_equal(cell(i, 1, lo.z), cell(i, hi_end - 1, hi.z))
                region.constrain_equal(cell(i, 2, lo.double_and_add.x_a), cell(i, hi_end, hi.double_and_add.x_a))
                region.constrain_equal(cell(i, 1, lo.double_and_add.lambda_1), cell(i, hi_end, hi.double_and_add.lambda_1))
                # complete addition starts where the lo half ends (complete.rs:112-123, add.rs:205-211)
                lo_end = 2 + INCOMPLETE_LO_LEN
                region.constrain_equal(cell(i, complete_at, complete.z_complete), cell(i, lo_end - 1, lo.z))
                region.constrain_equal(cell(i, complete_at, add.x_qr), cell(i, lo_end, lo.double_and_add.x_a))
                region.constrain_equal(cell(i, complete_at, add.y_qr), cell(i, lo_end, lo.double_and_add.lambda_1))
                for it in range(NUM_COMPLETE_BITS):
                    row = complete_at + 2 * it
                    region.constrain_equal(cell(i, row + 1, complete.z_complete), by)      # base_y
                    region.constrain_equal(cell(i, row, add.x_p), bx)                      # U = (base.x, +-base.y)
                    # Acc + (U + Acc): Acc is copied from the row above into x_p, y_p
                    region.constrain_equal(cell(i, row + 1, add.x_p), cell(i, row, add.x_qr))
                    region.constrain_equal(cell(i, row + 1, add.y_p), cell(i, row, add.y_qr))
                region.constrain_equal(cell(i, lsb_at + 1, add.x_p), bx)      # mul.rs:351-354
                region.constrain_equal(cell(i, lsb_at + 1, add.y_p), by)
            return index
        result.region_index = layouter.assign_region("variable-base scalar mul many", assign)

        # ---- the overflow checks (overflow.rs:101-208), region kind by region kind -----------------------------------------------------------
        def aux_rows(entries):
            """aux[:, entries] flattened multiplication by multiplication"""
            if aux is None:
                return blank(count * len(entries))
            return aux[:, entries, :].reshape(count * len(entries), 4)
        words = 130 // K
        s_cells = layouter.assign_region("s = alpha + k_254 ⋅ 2^130 many",
                                         lambda region: region.assign_advice_column(overflow.advices[0], 0, aux_rows([0])))
        lookup = overflow.lookup_config

        def decompose(region):
            sums = region.assign_advice_column(lookup.running_sum, 0, aux_rows(list(range(1, 2 + words))))
            word_rows = ((words + 1) * np.arange(count, dtype=np.int64)[:, None] + np.arange(words, dtype=np.int64)[None, :]).reshape(-1)
            region.enable_selector_rows(lookup.q_lookup, word_rows)
            region.enable_selector_rows(lookup.q_running, word_rows)
            for i in range(count):
                region.constrain_equal(sums.cell((words + 1) * i), s_cells.cell(i))
            return sums
        sums = layouter.assign_region("Decompose low 130 bits of s many", decompose)
        z_columns = [mul.complete_config.z_complete, hi.z, hi.z]              # the columns of z_0, z_130 and z_254 in the big region
        z_rows = [ROWS - 1, 1 + INCOMPLETE_HI_LEN, 2]

        def gate_blocks(region):
            first, second, third = overflow.advices
            if columns is None:
                col0 = col1 = col2 = blank(3 * count)
            else:
                dev = columns.device
                at = torch.from_numpy(base_rows).to(dev)
                z_0, z_130, k_254 = (columns[a.index(col)][at + row] for col, row in zip(z_columns, z_rows))
                aux_d = aux.to(dev)
                zero = torch.zeros_like(z_0)
                col0 = torch.stack([z_0, z_130, aux_d[:, 15]], dim=1).reshape(3 * count, 4)
                col1 = torch.stack([k_254, zero, aux_d[:, 14]], dim=1).reshape(3 * count, 4)
                col2 = torch.stack([zero, aux_d[:, 0], zero], dim=1).reshape(3 * count, 4)
            v0 = region.assign_advice_column(first, 0, col0)
            v1 = region.assign_advice_column(second, 0, col1)
            v2 = region.assign_advice_column(third, 0, col2)
            region.enable_selector_rows(overflow.q_mul_overflow, 3 * np.arange(count, dtype=np.int64) + 1)
            big = result.region_index
            for i in range(count):
                for v, row, (column, at_row) in ((v0, 0, (z_columns[0], z_rows[0])), (v0, 1, (z_columns[1], z_rows[1])),
                                                 (v1, 0, (z_columns[2], z_rows[2]))):
                    region.constrain_equal(v.cell(3 * i + row), Cell(big, ROWS * i + at_row, column))
                alphas[i].copy_advice(region, second, 3 * i + 1)              # the value of alpha comes from its cell
                region.constrain_equal(v1.cell(3 * i + 2), sums.cell((words + 1) * i + words))
                region.constrain_equal(v2.cell(3 * i + 1), s_cells.cell(i))
            return v1
        result.alpha_cells = layouter.assign_region("overflow check many", gate_blocks)
        if columns is not None and count:
            last = torch.from_numpy(base_rows + ROWS - 1).to(columns.device)
            result.outputs = torch.stack([columns[a.index(add.x_qr)][last], columns[a.index(add.y_qr)][last]], dim=1)
        return result


# ---- ecc.rs: the wrappers ------------------------------------------------------------------------------------------------------------------
class _PointBase:
    def __init__(self, chip: EccChip, inner):
        self.chip, self._inner = chip, inner

    def inner(self):
        return self._inner

    def constrain_equal(self, layouter, other) -> None:
        self.chip.constrain_equal(layouter, EccPoint.of(self._inner), EccPoint.of(other.inner()))

    def extract_p(self) -> AssignedCell:
        return self.chip.extract_p(self._inner)

    def add(self, layouter, other) -> "Point":
        assert self.chip is other.chip or self.chip.config is other.chip.config
        return Point(self.chip, self.chip.add(layouter, self._inner, other.inner()))


class Point(_PointBase):
    """ecc.rs:486-575: a point that may be the identity."""

    @staticmethod
    def new(chip: EccChip, layouter, value) -> "Point":
        return Point(chip, chip.witness_point(layouter, value))


class NonIdentityPoint(_PointBase):
    """ecc.rs:376-484"""

    @staticmethod
    def new(chip: EccChip, layouter, value) -> "NonIdentityPoint":
        return NonIdentityPoint(chip, chip.witness_point_non_id(layouter, value))

    def add_incomplete(self, layouter, other: "NonIdentityPoint") -> "NonIdentityPoint":
        return NonIdentityPoint(self.chip, self.chip.add_incomplete(layouter, self._inner, other.inner()))

    def mul(self, layouter, by: ScalarVar):
        """-> (Point, ScalarVar)"""
        point, scalar = self.chip.mul(layouter, by, self._inner)
        return Point(self.chip, point), scalar
