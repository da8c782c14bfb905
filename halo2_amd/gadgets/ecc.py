"""The ECC gadget of halo2_gadgets (src/ecc.rs, ecc/chip.rs, chip/witness_point.rs, chip/add_incomplete.rs, chip/add.rs, chip/mul.rs,
mul/incomplete.rs, mul/complete.rs, mul/overflow.rs, chip/mul_fixed.rs, mul_fixed/full_width.rs, mul_fixed/short.rs,
mul_fixed/base_field_elem.rs) against `halo2_amd.circuit`, over Pallas: `EccChip` with `witness_point`, `witness_point_non_id`,
`witness_point_from_constant`, `add_incomplete`, `add`, variable-base `mul`, fixed-base `mul_fixed` (full-width), `mul_fixed_short` and `mul_fixed_base_field_elem`,
and `mul_sign`, and the wrappers `Point`, `NonIdentityPoint`, `ScalarVar`, `ScalarFixed`, `ScalarFixedShort`, `FixedPoint`,
`FixedPointShort` and `FixedPointBaseField`.

The mirror assigns cell by cell with Python integers and inv0 (x / 0 = 0, what the reference's `Assigned` evaluates to) -- the same
regions, offsets, gates, constraint names and copy constraints as the reference:

    config = EccChip.configure(meta, advices[10], lagrange_coeffs[8], range_check)
    base = NonIdentityPoint.new(chip, layouter, (x, y))
    product, scalar = base.mul(layouter, ScalarVar.from_base(chip, layouter, alpha_cell))

What the reference does not have is the bulk path: `EccChip.mul_many` lays `count` multiplications back to back in ONE region whose
ten advice columns come from the device (`halo2_amd.ecc.mul_trace`), then three bulk regions with their overflow checks; per
multiplication the same gates, cells and equality constraints as `mul`, grouped differently.

`EccChip.configure(..., fixed_bases=FixedPoints(...))` goes on to the fixed-base configs in the reference's order: `mul_fixed`
(its running sum, `fixed_z` and the gate "Running sum coordinates check"), `full_width`, `short` and `base_field_elem`.  `FixedBaseTables` holds a base's
tables as integers, from the device (`FixedBaseTables.of(halo2_amd.ecc.FixedBase(...))`) or from anywhere else.
`EccChip.mul_fixed_many` is the bulk path of `mul_fixed`: one region of 85 rows per multiplication whose six advice columns come from
`halo2_amd.ecc.mul_fixed_trace` and whose fixed columns are the base's tables tiled, then one region with the complete additions.
`EccChip.mul_fixed_short_many` and `EccChip.mul_fixed_base_field_elem_many` are the bulk paths of the two forms whose scalar is a
running sum (23 and 86 rows per multiplication from `halo2_amd.ecc.mul_fixed_short_trace` / `mul_fixed_base_field_trace`, then the
additions, and for the base-field form the range check of alpha_0' and the canonicity gate's rows), and `EccChip.add_many` is the bulk
path of `add`; every bulk path closes on the one layout of `EccChip.additions_many`.

The mirror of the reference's test circuit (`MyEccCircuit`, tests/ecc_fixed_cases.py) reproduces the reference's pinned `vk_ecc_chip`
bit for bit and its stored proof verifies.  `CommitDomain`, which multiplies its R through `FixedPoint` and adds through `add`, is in
`halo2_amd/gadgets/sinsemilla.py`."""
from __future__ import annotations

import numpy as np

from .. import ecc as primitive
from .. import fields
from .. import range_check as range_primitive
from ..circuit import AssignedCell, Cell, ConstraintSystem, Expression, Rotation, Synthesis
from .sinsemilla import DoubleAndAdd, NonIdentityEccPoint
from .utilities import K, LookupRangeCheckConfig, RunningSumConfig, bool_check, decompose_word, range_check, ternary, value_int

FP = 0
ROWS = primitive.ROWS
NUM_BITS = 255                                                                # pallas::Scalar::NUM_BITS
NUM_COMPLETE_BITS = 3                                                         # mul.rs:27-46
INCOMPLETE_LEN = NUM_BITS - 1 - NUM_COMPLETE_BITS
INCOMPLETE_HI_LEN = INCOMPLETE_LEN // 2
INCOMPLETE_LO_LEN = INCOMPLETE_LEN - INCOMPLETE_HI_LEN
CURVE_B = 5
FIXED_BASE_WINDOW_SIZE, H = 3, 8                                              # constants.rs:12-15
NUM_WINDOWS, NUM_WINDOWS_SHORT = primitive.NUM_WINDOWS, primitive.NUM_WINDOWS_SHORT


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

    def constant_point(self, value, offset: int, region) -> EccPoint:       # witness_point.rs:145-164; the identity is (0, 0)
        self.q_point.enable(region, offset)
        x = region.assign_advice_from_constant(self.x, offset, value[0])
        y = region.assign_advice_from_constant(self.y, offset, value[1])
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


# ---- constants.rs, ecc.rs FixedPoint: a base's tables ------------------------------------------------------------------------------------
class FixedBaseTables:
    """What the chip reads of a fixed base (ecc/chip.rs FixedPoint: generator, u, z, lagrange_coeffs) as Python integers, and the window
    table the reference recomputes point by point while it assigns: window_table[w][k] = (x, y), lagrange_coeffs[w][c], z[w], u[w][k].
    `device` is the `halo2_amd.ecc.FixedBase` they were read from, which the bulk path multiplies over, or None."""

    def __init__(self, generator, window_table, lagrange_coeffs, z, u, device=None):
        self.generator, self.window_table, self.lagrange_coeffs, self.z, self.u = generator, window_table, lagrange_coeffs, z, u
        self.num_windows, self.device = len(window_table), device
        assert len(lagrange_coeffs) == len(z) == len(u) == self.num_windows

    @staticmethod
    def of(fixed_base: "primitive.FixedBase") -> "FixedBaseTables":
        return FixedBaseTables(fixed_base.generator(), fixed_base.window_table(), fixed_base.lagrange_coeffs(), fixed_base.z(),
                               fixed_base.u(), device=fixed_base)


class FixedPoints:
    """ecc.rs FixedPoints: the bases of a circuit by the form of their scalars."""

    def __init__(self, full_width=(), short=(), base_field=()):
        self.full_width, self.short, self.base_field = tuple(full_width), tuple(short), tuple(base_field)


# ---- mul_fixed.rs ----------------------------------------------------------------------------------------------------------------------------
class MulFixedConfig:
    def __init__(self, modulus, running_sum_config, lagrange_coeffs, fixed_z, window, u, add_config, add_incomplete_config):
        self.modulus, self.running_sum_config, self.lagrange_coeffs, self.fixed_z = modulus, running_sum_config, list(lagrange_coeffs), fixed_z
        self.window, self.u, self.add_config, self.add_incomplete_config = window, u, add_config, add_incomplete_config

    @staticmethod
    def configure(meta: ConstraintSystem, lagrange_coeffs, window, u, add_config: AddConfig,
                  add_incomplete_config: AddIncompleteConfig) -> "MulFixedConfig":      # mul_fixed.rs:56-104
        meta.enable_equality(window)
        meta.enable_equality(u)
        q_running_sum = meta.selector()
        running_sum_config = RunningSumConfig.configure(meta, q_running_sum, window, FIXED_BASE_WINDOW_SIZE)
        config = MulFixedConfig(meta.modulus, running_sum_config, lagrange_coeffs, meta.fixed_column(), window, u, add_config,
                                add_incomplete_config)
        assert add_config.x_p == add_incomplete_config.x_p and add_config.y_p == add_incomplete_config.y_p
        assert not {window, u} & add_config.output_columns()

        def running_sum_coords(cells):                                        # mul_fixed.rs:115-129
            q = cells.query_selector(running_sum_config.q_range_check)
            z_cur = cells.query_advice(window, Rotation.cur())
            z_next = cells.query_advice(window, Rotation.next())
            word = z_cur - z_next * H                                         # a_i = z_i - 8 z_(i+1)
            return [(name, q * poly) for name, poly in config.coords_check(cells, word)]
        meta.create_gate("Running sum coordinates check", running_sum_coords)
        return config

    def coords_check(self, cells, window: Expression) -> list:               # mul_fixed.rs:133-169
        y_p = cells.query_advice(self.add_config.y_p, Rotation.cur())
        x_p = cells.query_advice(self.add_config.x_p, Rotation.cur())
        z = cells.query_fixed(self.fixed_z)
        u = cells.query_advice(self.u, Rotation.cur())
        window_pow = []
        for power in range(H):
            acc = Expression.constant(1)
            for _ in range(power):
                acc = acc * window
            window_pow.append(acc)
        interpolated_x = Expression.constant(0)
        for power, coeff in zip(window_pow, self.lagrange_coeffs):
            interpolated_x = interpolated_x + (power * cells.query_fixed(coeff))
        x_check = interpolated_x - x_p
        y_check = u.square() - y_p - z
        on_curve = y_p.square() - x_p.square() * x_p - Expression.constant(CURVE_B)
        return [("check x", x_check), ("check y", y_check), ("on-curve", on_curve)]

    def assign_region_inner(self, region, offset: int, windows, base: FixedBaseTables, coords_check_toggle):      # mul_fixed.rs:172-193
        """windows: the scalar's num_windows values, integers or None.  -> (acc, mul_b): the sum of all windows but the last, and
        the last window's point, both NonIdentityEccPoint"""
        nw = base.num_windows
        assert len(windows) == nw
        for w in range(nw):                                                   # assign_fixed_constants, mul_fixed.rs:196-252
            coords_check_toggle.enable(region, w + offset)
            for k in range(H):
                region.assign_fixed(self.lagrange_coeffs[k], w + offset, lambda w=w, k=k: base.lagrange_coeffs[w][k])
            region.assign_fixed(self.fixed_z, w + offset, lambda w=w: base.z[w])
        acc = self._process_window(region, offset, 0, windows[0], base)       # initialize_accumulator
        for w in range(1, nw - 1):                                            # add_incomplete, mul_fixed.rs:323-360
            mul_b = self._process_window(region, offset, w, windows[w], base)
            acc = self.add_incomplete_config.assign_region(mul_b, acc, offset + w, region)
        return acc, self._process_window(region, offset, nw - 1, windows[nw - 1], base)      # process_msb

    def _process_window(self, region, offset: int, w: int, k, base: FixedBaseTables) -> NonIdentityEccPoint:      # mul_fixed.rs:255-305
        point = None if k is None else base.window_table[w][k]
        if point is not None and (point[0] == 0 or point[1] == 0):
            raise Synthesis("mul_fixed: a window's point has a zero coordinate")
        x = region.assign_advice(self.add_config.x_p, offset + w, lambda: point[0])
        y = region.assign_advice(self.add_config.y_p, offset + w, lambda: point[1])
        region.assign_advice(self.u, offset + w, lambda: base.u[w][k])
        return NonIdentityEccPoint(x, y)


# ---- mul_fixed/full_width.rs -----------------------------------------------------------------------------------------------------------------
class ScalarFixed:
    """chip.rs EccScalarFixed: a full-width scalar, an integer below 2^255 or None, and its window cells once it has been used"""

    def __init__(self, value, windows=None):
        self.value, self.windows = value, windows

    @staticmethod
    def new(chip, layouter, value) -> "ScalarFixed":                         # ecc.rs:251-259, chip.rs witness_scalar_fixed: lazily
        return chip.witness_scalar_fixed(layouter, value)


class FullWidthConfig:
    def __init__(self, q_mul_fixed_full, super_config: MulFixedConfig):
        self.q_mul_fixed_full, self.super_config = q_mul_fixed_full, super_config

    @staticmethod
    def configure(meta: ConstraintSystem, super_config: MulFixedConfig) -> "FullWidthConfig":      # full_width.rs:20-51
        config = FullWidthConfig(meta.selector(), super_config)

        def gate(cells):
            q = cells.query_selector(config.q_mul_fixed_full)
            window = cells.query_advice(super_config.window, Rotation.cur())
            checks = super_config.coords_check(cells, window) + [("window range check", range_check(window, H))]
            return [(name, q * poly) for name, poly in checks]
        meta.create_gate("Full-width fixed-base scalar mul", gate)
        return config

    def _witness(self, region, offset: int, value) -> ScalarFixed:          # full_width.rs:56-114
        for idx in range(NUM_WINDOWS):
            self.q_mul_fixed_full.enable(region, offset + idx)
        words = [None] * NUM_WINDOWS if value is None else decompose_word(value, NUM_BITS, FIXED_BASE_WINDOW_SIZE)
        cells = [region.assign_advice(self.super_config.window, offset + idx, lambda v=word: v) for idx, word in enumerate(words)]
        return ScalarFixed(value, cells)

    def assign(self, layouter, scalar: ScalarFixed, base: FixedBaseTables):  # full_width.rs:116-177
        """-> (EccPoint, ScalarFixed)"""
        assert scalar.windows is None and base.num_windows == NUM_WINDOWS
        if scalar.value is not None and not 0 <= scalar.value < 1 << NUM_BITS:
            raise ValueError("mul_fixed: a scalar of at most 255 bits")

        def incomplete(region):
            witnessed = self._witness(region, 0, scalar.value)
            words = [None] * NUM_WINDOWS if scalar.value is None else decompose_word(scalar.value, NUM_BITS, FIXED_BASE_WINDOW_SIZE)
            acc, mul_b = self.super_config.assign_region_inner(region, 0, words, base, self.q_mul_fixed_full)
            return witnessed, acc, mul_b
        witnessed, acc, mul_b = layouter.assign_region("Full-width fixed-base mul (incomplete addition)", incomplete)
        result = layouter.assign_region("Full-width fixed-base mul (last window, complete addition)",
                                        lambda region: self.super_config.add_config.assign_region(EccPoint.of(mul_b), EccPoint.of(acc), 0,
                                                                                                  region))
        return result, witnessed


# ---- mul_fixed/short.rs ----------------------------------------------------------------------------------------------------------------------
L_SCALAR_SHORT = 64                                                           # constants.rs:27


class ScalarFixedShort:
    """chip.rs EccScalarFixedShort: a magnitude of at most 64 bits and a sign of 1 or -1, both cells, and the running sum of the
    magnitude once it has been used"""

    def __init__(self, magnitude: AssignedCell, sign: AssignedCell, running_sum=None):
        self.magnitude, self.sign, self.running_sum = magnitude, sign, running_sum

    @staticmethod
    def new(chip, layouter, magnitude_sign) -> "ScalarFixedShort":          # ecc.rs:285-298
        return chip.scalar_fixed_from_signed_short(layouter, magnitude_sign)


def _running_sum_windows(zs, m: int) -> list:
    """mul_fixed.rs:438-495: word_i = z_i - 8 z_(i+1), its low three bits the index into the window's table"""
    values = [value_int(z.value(), m) for z in zs]
    if any(v is None for v in values):
        return [None] * (len(zs) - 1)
    return [(cur - nxt * H) % m & (H - 1) for cur, nxt in zip(values, values[1:])]


def _signed_y(sign: AssignedCell, y: AssignedCell, m: int):
    s, y_v = value_int(sign.value(), m), value_int(y.value(), m)
    return None if s is None or y_v is None else (-y_v % m if s == m - 1 else y_v)


class ShortConfig:
    def __init__(self, modulus, q_mul_fixed_short, super_config: MulFixedConfig):
        self.modulus, self.q_mul_fixed_short, self.super_config = modulus, q_mul_fixed_short, super_config

    @staticmethod
    def configure(meta: ConstraintSystem, super_config: MulFixedConfig) -> "ShortConfig":      # short.rs:21-77
        config = ShortConfig(meta.modulus, meta.selector(), super_config)

        def gate(cells):
            q = cells.query_selector(config.q_mul_fixed_short)
            y_p = cells.query_advice(super_config.add_config.y_p, Rotation.cur())
            y_a = cells.query_advice(super_config.add_config.y_qr, Rotation.cur())
            last_window = cells.query_advice(super_config.u, Rotation.cur())  # z_21 = k_21
            sign = cells.query_advice(super_config.window, Rotation.cur())
            one = Expression.constant(1)
            last_window_check = bool_check(last_window)
            sign_check = sign.square() - one
            y_check = (y_p - y_a) * (y_p + y_a)
            negation_check = sign * y_p - y_a
            checks = (("last_window_check", last_window_check), ("sign_check", sign_check), ("y_check", y_check),
                      ("negation_check", negation_check))
            return [(name, q * poly) for name, poly in checks]
        meta.create_gate("Short fixed-base mul gate", gate)
        return config

    def assign(self, layouter, scalar: ScalarFixedShort, base: FixedBaseTables):      # short.rs:108-243
        """-> (EccPoint, ScalarFixedShort)"""
        m, sup = self.modulus, self.super_config
        assert scalar.running_sum is None and base.num_windows == NUM_WINDOWS_SHORT

        def incomplete(region):
            zs = sup.running_sum_config.copy_decompose(region, 0, scalar.magnitude, True, L_SCALAR_SHORT, NUM_WINDOWS_SHORT)
            decomposed = ScalarFixedShort(scalar.magnitude, scalar.sign, zs)
            acc, mul_b = sup.assign_region_inner(region, 0, _running_sum_windows(zs, m), base, sup.running_sum_config.q_range_check)
            return decomposed, acc, mul_b
        decomposed, acc, mul_b = layouter.assign_region("Short fixed-base mul (incomplete addition)", incomplete)

        def last_window(region):
            magnitude_mul = sup.add_config.assign_region(EccPoint.of(mul_b), EccPoint.of(acc), 0, region)
            sign = decomposed.sign.copy_advice(region, sup.window, 1)
            decomposed.running_sum[21].copy_advice(region, sup.u, 1)          # the last window, in a free cell of the u column
            y_val = _signed_y(sign, magnitude_mul.y(), m)
            self.q_mul_fixed_short.enable(region, 1)
            y_var = region.assign_advice(sup.add_config.y_p, 1, lambda: y_val)
            return EccPoint(magnitude_mul.x(), y_var)
        return layouter.assign_region("Short fixed-base mul (most significant word)", last_window), decomposed

    def assign_scalar_sign(self, layouter, sign: AssignedCell, point: EccPoint) -> EccPoint:      # short.rs:247-305
        m, sup = self.modulus, self.super_config

        def assign(region):
            self.q_mul_fixed_short.enable(region, 0)
            region.assign_advice_from_constant(sup.u, 0, 0)                   # the "last window" is irrelevant here
            sign.copy_advice(region, sup.window, 0)
            point.y().copy_advice(region, sup.add_config.y_qr, 0)
            signed_y = region.assign_advice(sup.add_config.y_p, 0, lambda: _signed_y(sign, point.y(), m))
            return EccPoint(point.x(), signed_y)
        return layouter.assign_region("Signed point", assign)


# ---- mul_fixed/base_field_elem.rs ------------------------------------------------------------------------------------------------------------
class BaseFieldElemConfig:
    def __init__(self, modulus, q_mul_fixed_base_field, canon_advices, lookup_config, super_config: MulFixedConfig):
        self.modulus, self.q_mul_fixed_base_field, self.canon_advices = modulus, q_mul_fixed_base_field, list(canon_advices)
        self.lookup_config, self.super_config = lookup_config, super_config
        self.t_p = modulus - (1 << 254)

    @staticmethod
    def configure(meta: ConstraintSystem, canon_advices, lookup_config: LookupRangeCheckConfig,
                  super_config: MulFixedConfig) -> "BaseFieldElemConfig":    # base_field_elem.rs:32-163
        for advice in canon_advices:
            meta.enable_equality(advice)
        config = BaseFieldElemConfig(meta.modulus, meta.selector(), canon_advices, lookup_config, super_config)
        inc = super_config.add_incomplete_config
        assert not set(canon_advices) & {inc.x_p, inc.y_p, inc.x_qr, inc.y_qr}
        c = config.canon_advices

        def gate(cells):
            q = cells.query_selector(config.q_mul_fixed_base_field)
            alpha = cells.query_advice(c[0], Rotation.prev())
            z_84_alpha = cells.query_advice(c[2], Rotation.prev())            # the last three bits of alpha
            # alpha = alpha_0 (252 bits) || alpha_1 (2 bits) || alpha_2 (1 bit); alpha_0 is derived, not witnessed
            alpha_0 = alpha - (z_84_alpha * (1 << 252))
            alpha_1 = cells.query_advice(c[1], Rotation.cur())
            alpha_2 = cells.query_advice(c[2], Rotation.cur())
            alpha_0_prime = cells.query_advice(c[0], Rotation.cur())
            z_13_alpha_0_prime = cells.query_advice(c[0], Rotation.next())
            z_44_alpha = cells.query_advice(c[1], Rotation.next())
            z_43_alpha = cells.query_advice(c[2], Rotation.next())
            alpha_1_range_check = range_check(alpha_1, 1 << 2)
            alpha_2_range_check = bool_check(alpha_2)
            z_84_alpha_check = z_84_alpha - (alpha_1 + alpha_2 * (1 << 2))
            alpha_0_prime_check = alpha_0_prime - (alpha_0 + Expression.constant(1 << 130) - Expression.constant(config.t_p))
            # MSB = 1: alpha_1 = 0, alpha_0 < 2^130 (its top 120 bits and bits 130, 131 vanish) and alpha_0 + 2^130 - t_p < 2^130
            alpha_0_hi_120 = z_44_alpha - z_84_alpha * Expression.constant(1 << 120)
            a_43 = z_43_alpha - z_44_alpha * H
            checks = (("MSB = 1 => alpha_1 = 0", alpha_2 * alpha_1),
                      ("MSB = 1 => alpha_0_hi_120 = 0", alpha_2 * alpha_0_hi_120),
                      ("MSB = 1 => a_43 = 0 or 1", alpha_2 * bool_check(a_43)),
                      ("MSB = 1 => z_13_alpha_0_prime = 0", alpha_2 * z_13_alpha_0_prime),
                      ("alpha_1_range_check", alpha_1_range_check), ("alpha_2_range_check", alpha_2_range_check),
                      ("z_84_alpha_check", z_84_alpha_check), ("alpha_0_prime check", alpha_0_prime_check))
            return [(name, q * poly) for name, poly in checks]
        meta.create_gate("Canonicity checks", gate)
        return config

    def assign(self, layouter, scalar: AssignedCell, base: FixedBaseTables) -> EccPoint:      # base_field_elem.rs:165-378
        m, sup, c = self.modulus, self.super_config, self.canon_advices
        assert base.num_windows == NUM_WINDOWS

        def incomplete(region):
            zs = sup.running_sum_config.copy_decompose(region, 0, scalar, True, NUM_BITS, NUM_WINDOWS)
            acc, mul_b = sup.assign_region_inner(region, 0, _running_sum_windows(zs, m), base, sup.running_sum_config.q_range_check)
            return zs, acc, mul_b
        zs, acc, mul_b = layouter.assign_region("Base-field elem fixed-base mul (incomplete addition)", incomplete)
        result = layouter.assign_region("Base-field elem fixed-base mul (complete addition)",
                                        lambda region: sup.add_config.assign_region(EccPoint.of(mul_b), EccPoint.of(acc), 0, region))
        alpha, z_43_alpha, z_44_alpha, z_84_alpha = zs[0], zs[43], zs[44], zs[84]
        alpha_v, z_84_v = value_int(alpha.value(), m), value_int(z_84_alpha.value(), m)
        known = alpha_v is not None and z_84_v is not None
        alpha_0_prime_v = (alpha_v - z_84_v * (1 << 252) + (1 << 130) - self.t_p) % m if known else None
        sums = self.lookup_config.witness_check(layouter, alpha_0_prime_v, 13, False)
        alpha_0_prime, z_13_alpha_0_prime = sums[0], sums[13]

        def canonicity(region):
            self.q_mul_fixed_base_field.enable(region, 1)
            alpha.copy_advice(region, c[0], 0)
            z_84_alpha.copy_advice(region, c[2], 0)
            alpha_0_prime.copy_advice(region, c[0], 1)
            region.assign_advice(c[1], 1, lambda: alpha_v >> 252 & 3)         # alpha_1 = alpha[252..=253]
            region.assign_advice(c[2], 1, lambda: alpha_v >> 254 & 1)         # alpha_2 = alpha[254]
            z_13_alpha_0_prime.copy_advice(region, c[0], 2)
            z_44_alpha.copy_advice(region, c[1], 2)
            z_43_alpha.copy_advice(region, c[2], 2)
        layouter.assign_region("Canonicity checks", canonicity)
        return result


# ---- chip.rs -------------------------------------------------------------------------------------------------------------------------------
class EccConfig:
    def __init__(self, advices, add_incomplete, add, mul, witness_point, lookup_config, lagrange_coeffs, fixed_bases=None,
                 mul_fixed=None, mul_fixed_full=None, mul_fixed_short=None, mul_fixed_base_field=None):
        self.advices, self.add_incomplete, self.add, self.mul = list(advices), add_incomplete, add, mul
        self.witness_point, self.lookup_config, self.lagrange_coeffs = witness_point, lookup_config, list(lagrange_coeffs)
        self.fixed_bases, self.mul_fixed, self.mul_fixed_full, self.mul_fixed_short = fixed_bases, mul_fixed, mul_fixed_full, mul_fixed_short
        self.mul_fixed_base_field = mul_fixed_base_field


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


class MulFixedMany:
    """What `mul_fixed_many` returns: the cells of multiplication i by position.  outputs: (count, 2, 4) Montgomery x and y of the
    products (None without a witness)."""

    def __init__(self, config: EccConfig, count: int):
        self.config, self.count, self.region_index, self.add_region_index, self.outputs = config, count, None, None, None

    def result_x(self, i: int) -> Cell:
        return Cell(self.add_region_index, 2 * i + 1, self.config.add.x_qr)

    def result_y(self, i: int) -> Cell:
        return Cell(self.add_region_index, 2 * i + 1, self.config.add.y_qr)

    def window(self, i: int, w: int) -> Cell:
        return Cell(self.region_index, NUM_WINDOWS * i + w, self.config.mul_fixed.window)


class MulFixedSumMany:
    """What `mul_fixed_short_many` and `mul_fixed_base_field_elem_many` return: the cells of multiplication i by position.  outputs:
    (count, 2, 4) Montgomery x and y of the results (None without a witness); for the short form the y is the signed one."""

    def __init__(self, config: EccConfig, count: int, num_windows: int, short: bool):
        self.config, self.count, self.num_windows, self.short = config, count, num_windows, short
        self.region_index, self.add_region_index, self.canonicity_region_index, self.outputs = None, None, None, None
        self.alpha_0_prime = None                                             # base field: per multiplication the range check's cells

    def result_x(self, i: int) -> Cell:
        return Cell(self.add_region_index, 2 * i + 1, self.config.add.x_qr)

    def result_y(self, i: int) -> Cell:
        """the short form's result is the signed y, in y_p beside the sum (short.rs:186-190)"""
        return Cell(self.add_region_index, 2 * i + 1, self.config.add.y_p if self.short else self.config.add.y_qr)

    def point(self, i: int) -> tuple:
        return self.result_x(i), self.result_y(i)

    def z(self, i: int, w: int) -> Cell:
        """the running sum's z_w, w = 0 .. num_windows"""
        return Cell(self.region_index, (self.num_windows + 1) * i + w, self.config.mul_fixed.window)


class AddMany:
    """What `add_many` returns: sum i is in row 2 i + 1 of one region.  outputs: (count, 2, 4) Montgomery (None without a witness)."""

    def __init__(self, config: EccConfig, count: int):
        self.config, self.count, self.region_index, self.outputs = config, count, None, None

    def result_x(self, i: int) -> Cell:
        return Cell(self.region_index, 2 * i + 1, self.config.add.x_qr)

    def result_y(self, i: int) -> Cell:
        return Cell(self.region_index, 2 * i + 1, self.config.add.y_qr)

    def point(self, i: int) -> tuple:
        return self.result_x(i), self.result_y(i)


def _tensor(t):
    import torch
    return t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t, dtype=np.uint64).view(np.int64))


def _blank(rows: int):
    return np.broadcast_to(np.zeros((1, 4), dtype=np.uint64), (rows, 4))


def _cell_of(c) -> Cell:
    return c.cell() if isinstance(c, AssignedCell) else c


def _operand_cells(point) -> tuple:
    """the two cells of an operand of a bulk addition: an EccPoint or NonIdentityEccPoint, or a pair of cells"""
    x, y = (point.x(), point.y()) if hasattr(point, "x") else point
    return _cell_of(x), _cell_of(y)


class EccChip:
    def __init__(self, config: EccConfig):
        self.config = config

    @staticmethod
    def configure(meta: ConstraintSystem, advices, lagrange_coeffs, range_check: LookupRangeCheckConfig,
                  fixed_bases: FixedPoints | None = None) -> EccConfig:
        """chip.rs:273-333: the gates of witness_point, add_incomplete, add and mul (hi, lo, complete, overflow, then the LSB gate) on
        the reference's columns, with enable_equality, selectors and gates created in the reference's order.  With `fixed_bases` it goes
        on as chip.rs:296-320 does: mul_fixed (window and u on advices 4 and 5, the running sum's "range check" gate, fixed_z, "Running
        sum coordinates check"), then full_width, short and base_field_elem (on advices 6 - 8).  Without, nothing fixed-base is created
        and `lagrange_coeffs` is stored unused.  A circuit configured this way reproduces the reference's pinned vk_ecc_chip
        (tests/test_gpu_ecc_fixed_circuit.py)."""
        a = list(advices)
        assert len(a) == 10 and len(lagrange_coeffs) == 8
        witness_point = WitnessPointConfig.configure(meta, a[0], a[1])
        add_incomplete = AddIncompleteConfig.configure(meta, a[0], a[1], a[2], a[3])
        add = AddConfig.configure(meta, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8])
        mul = MulConfig.configure(meta, add, range_check, a)
        if fixed_bases is None:
            return EccConfig(a, add_incomplete, add, mul, witness_point, range_check, lagrange_coeffs)
        mul_fixed = MulFixedConfig.configure(meta, lagrange_coeffs, a[4], a[5], add, add_incomplete)
        mul_fixed_full = FullWidthConfig.configure(meta, mul_fixed)
        mul_fixed_short = ShortConfig.configure(meta, mul_fixed)
        mul_fixed_base_field = BaseFieldElemConfig.configure(meta, a[6:9], range_check, mul_fixed)
        return EccConfig(a, add_incomplete, add, mul, witness_point, range_check, lagrange_coeffs, fixed_bases, mul_fixed, mul_fixed_full,
                         mul_fixed_short, mul_fixed_base_field)

    # ---- EccInstructions (chip.rs:431-600) -------------------------------------------------------------------------------------------------
    def constrain_equal(self, layouter, a, b) -> None:
        def assign(region):
            region.constrain_equal(a.x().cell(), b.x().cell())
            region.constrain_equal(a.y().cell(), b.y().cell())
        layouter.assign_region("constrain equal", assign)

    def witness_point(self, layouter, value) -> EccPoint:
        """value: (x, y) integers, (0, 0) or None for the identity... None alone is an unknown value"""
        return layouter.assign_region("witness point", lambda region: self.config.witness_point.point(value, 0, region))

    def witness_point_from_constant(self, layouter, value) -> EccPoint:
        """value: (x, y) integers fixed by the circuit, (0, 0) the identity (chip.rs:471-481)"""
        return layouter.assign_region("witness point (constant)", lambda region: self.config.witness_point.constant_point(value, 0, region))

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

    def witness_scalar_fixed(self, layouter, value) -> ScalarFixed:          # chip.rs:536-548: witnessed lazily, where it is used
        return ScalarFixed(value)

    def mul_fixed(self, layouter, scalar: ScalarFixed, base: FixedBaseTables):
        """[scalar]base, full-width (chip.rs:602-613).  -> (EccPoint, ScalarFixed)"""
        if self.config.mul_fixed_full is None:
            raise ValueError("mul_fixed: the chip was configured without fixed_bases")
        return self.config.mul_fixed_full.assign(layouter, scalar, base)

    def scalar_fixed_from_signed_short(self, layouter, magnitude_sign) -> ScalarFixedShort:      # chip.rs:516-528: constrained lazily
        magnitude, sign = magnitude_sign
        return ScalarFixedShort(magnitude, sign)

    def mul_fixed_short(self, layouter, scalar: ScalarFixedShort, base: FixedBaseTables):
        """[sign magnitude]base over the base's 22-window tables (chip.rs:613-625).  -> (EccPoint, ScalarFixedShort)"""
        if self.config.mul_fixed_short is None:
            raise ValueError("mul_fixed_short: the chip was configured without fixed_bases")
        return self.config.mul_fixed_short.assign(layouter, scalar, base)

    def mul_fixed_base_field_elem(self, layouter, base_field_elem: AssignedCell, base: FixedBaseTables) -> EccPoint:
        """[alpha]base for a cell alpha of Fp read as an integer, with its canonicity checked (chip.rs:627-640)"""
        if self.config.mul_fixed_base_field is None:
            raise ValueError("mul_fixed_base_field_elem: the chip was configured without fixed_bases")
        return self.config.mul_fixed_base_field.assign(layouter, base_field_elem, base)

    def mul_sign(self, layouter, sign: AssignedCell, point: EccPoint) -> EccPoint:
        """[sign]point for a sign constrained to 1 or -1 by the short gate (chip.rs:564-578)"""
        if self.config.mul_fixed_short is None:
            raise ValueError("mul_sign: the chip was configured without fixed_bases")
        return self.config.mul_fixed_short.assign_scalar_sign(layouter, sign, EccPoint.of(point))

    # ---- the bulk paths --------------------------------------------------------------------------------------------------------------------
    def mul_fixed_many(self, layouter, fixed_base: FixedBaseTables, scalars, values=None, trace=None) -> MulFixedMany:
        """`count` full-width multiplications [k_i]B: ONE region of 85 * count rows whose advice columns 0 - 5 come from the device
        (`ecc.mul_fixed_trace`) and whose fixed columns are the base's tables tiled, then one region with the `count` complete
        additions, two rows each.  Per multiplication the gates, cells and equality constraints of `mul_fixed`.

        scalars: integers below 2^255 (None each without a witness).  values: (count, 4) canonical limbs where the caller has them on
        the device already; trace: (columns, aux) where the caller has them (else `ecc.mul_fixed_trace`, once, over
        `fixed_base.device`).  Without a witness (keygen) the same shape is laid out and nothing is launched."""
        import torch
        c = self.config
        if c.mul_fixed_full is None:
            raise ValueError("mul_fixed_many: the chip was configured without fixed_bases")
        count, nw = len(scalars), NUM_WINDOWS
        assert fixed_base.num_windows == nw
        total = nw * count
        if not layouter.cs.collect_advice:
            trace = None
        elif trace is None and count:
            if values is None:
                if any(k is None for k in scalars):
                    raise Synthesis("mul_fixed_many: a witness is needed and there is none")
                values = fields.to_limbs(list(scalars), FP, montgomery=False)
            if fixed_base.device is None:
                raise ValueError("mul_fixed_many: the tables have no device copy to multiply over")
            k = values if torch.is_tensor(values) else torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint64).view(np.int64)) \
                .to(fields.current_device())
            trace = primitive.mul_fixed_trace(fixed_base.device, k)
        columns = aux = None
        if trace is not None:
            columns, aux = [t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t, dtype=np.uint64).view(np.int64))
                            for t in trace]
            if tuple(columns.shape) != (6, total, 4) or tuple(aux.shape) != (count, primitive.FIXED_AUX, 4):
                raise ValueError("mul_fixed_many: the trace is ((6, 85 * count, 4), (count, 11, 4))")

        def blank(rows):
            return np.broadcast_to(np.zeros((1, 4), dtype=np.uint64), (rows, 4))
        add, inc, fixed, full = c.add, c.add_incomplete, c.mul_fixed, c.mul_fixed_full
        a = c.advices
        base_rows = nw * np.arange(count, dtype=np.int64)
        result = MulFixedMany(c, count)

        def assign(region):
            index = region.region_index
            for j in range(6):
                assert a[j] == (add.x_p, add.y_p, add.x_qr, add.y_qr, fixed.window, fixed.u)[j]
                region.assign_advice_column(a[j], 0, blank(total) if columns is None else columns[j])
            if count:
                for k in range(H):
                    coeffs = fields.to_limbs([row[k] for row in fixed_base.lagrange_coeffs], FP)
                    region.assign_fixed_column(fixed.lagrange_coeffs[k], 0, np.tile(coeffs, (count, 1)))
                region.assign_fixed_column(fixed.fixed_z, 0, np.tile(fields.to_limbs(list(fixed_base.z), FP), (count, 1)))
            region.enable_selector_rows(full.q_mul_fixed_full, np.arange(total, dtype=np.int64))
            region.enable_selector_rows(inc.q_add_incomplete, (base_rows[:, None] + np.arange(1, nw - 1, dtype=np.int64)[None, :]).reshape(-1))
            for i in range(count):                                            # window 1's addition starts from window 0's point
                region.constrain_equal(Cell(index, nw * i + 1, add.x_qr), Cell(index, nw * i, add.x_p))
                region.constrain_equal(Cell(index, nw * i + 1, add.y_qr), Cell(index, nw * i, add.y_p))
            return index
        result.region_index = layouter.assign_region("Full-width fixed-base mul (incomplete addition) many", assign)

        # the last window's point and the accumulator
        result.add_region_index = self.additions_many(
            layouter, "Full-width fixed-base mul (last window, complete addition) many", count, aux,
            lambda i: [Cell(result.region_index, nw * i + nw - 1, column) for column in (add.x_p, add.y_p, add.x_qr, add.y_qr)])
        if aux is not None and count:
            result.outputs = aux[:, 9:11].contiguous()
        return result

    def additions_many(self, layouter, name: str, count: int, aux, operands, second=None, extra=None) -> int:
        """`count` complete additions in ONE region of 2 * count rows, the layout every bulk path closes on: row 2 i holds the nine
        cells of addition i (aux[:, 0:9]: x_p, y_p, x_qr, y_qr, lambda, alpha, beta, gamma, delta) with q_add on, row 2 i + 1 the sum
        in x_qr, y_qr (aux[:, 9:11]) and zeros in the other seven -- but for a column of `second`, {column: (count, 4) Montgomery
        values}, which holds those.  operands(i) -> the four cells that x_p, y_p, x_qr, y_qr of row 2 i are constrained equal to.
        extra(region): what else the region holds.  aux None (keygen): zeros.  -> the region's index"""
        import torch
        add = self.config.add
        second = second or {}

        def additions(region):
            index = region.region_index
            for j, column in enumerate((add.x_p, add.y_p, add.x_qr, add.y_qr, add.lambda_, add.alpha, add.beta, add.gamma, add.delta)):
                if aux is None:
                    values_ = _blank(2 * count)
                else:
                    below = second[column] if column in second else aux[:, 9 + (j - 2)] if j in (2, 3) else torch.zeros_like(aux[:, j])
                    values_ = torch.stack([aux[:, j], below.to(aux.device)], dim=1).reshape(2 * count, 4)
                region.assign_advice_column(column, 0, values_)
            region.enable_selector_rows(add.q_add, 2 * np.arange(count, dtype=np.int64))
            for i in range(count):
                for column, source in zip((add.x_p, add.y_p, add.x_qr, add.y_qr), operands(i)):
                    region.constrain_equal(Cell(index, 2 * i, column), source)
            if extra is not None:
                extra(region)
            return index
        return layouter.assign_region(name, additions)

    def add_many(self, layouter, a_points, b_points, trace=None) -> AddMany:
        """`count` complete additions a_i + b_i in one region of 2 * count rows filled from `ecc.add_trace`; both operands of every
        row are copy-constrained to the given points, the gate and the cells are those of `add`.  A point is an EccPoint or a
        NonIdentityEccPoint, or the pair of cells a bulk result names (`point(i)`).  trace: the (count, 11, 4) rows of `ecc.add_trace`
        where the caller has them -- needed where the operands are bare cells, which carry no value; else the operands' values are read
        from their cells.  Without a witness (keygen) the same shape is laid out and nothing is launched."""
        c, m = self.config, self.config.add.modulus
        count = len(a_points)
        if len(b_points) != count:
            raise ValueError("add_many: as many b as a")
        aux = None
        if layouter.cs.collect_advice and count:
            if trace is None:
                pts = [[_xy(p, m) if hasattr(p, "x") else None for p in side] for side in (a_points, b_points)]
                if any(p is None for side in pts for p in side):
                    raise Synthesis("add_many: a witness is needed and there is none")
                on_device = [_tensor(fields.to_limbs([v for p in side for v in p], FP).reshape(count, 8)).to(fields.current_device())
                             for side in pts]
                trace = primitive.add_trace(on_device[0], on_device[1])
            aux = _tensor(trace)
            if tuple(aux.shape) != (count, primitive.FIXED_AUX, 4):
                raise ValueError("add_many: the trace is (count, 11, 4)")
        cells = [(_operand_cells(p) + _operand_cells(q)) for p, q in zip(a_points, b_points)]
        result = AddMany(c, count)
        result.region_index = self.additions_many(layouter, "complete point addition many", count, aux, lambda i: cells[i])
        if aux is not None:
            result.outputs = aux[:, 9:11].contiguous()
        return result

    def _running_sum_many(self, layouter, name: str, fixed_base: FixedBaseTables, sources, columns) -> int:
        """The first region of a fixed-base multiplication by a running sum, `count` times in one: num_windows + 1 rows each, advice
        columns 0 - 5 from `columns` (zeros without), the base's tables tiled with a zero last row, the running sum's q_range_check on
        rows 0 .. nw-1 and q_add_incomplete on rows 1 .. nw-2 of each; z_0 copied from sources[i], z_nw constrained to 0, window 1's
        addition starting from window 0's point.  -> the region's index"""
        c = self.config
        add, inc, fixed = c.add, c.add_incomplete, c.mul_fixed
        a, count, nw = c.advices, len(sources), fixed_base.num_windows
        rows = nw + 1
        base_rows = rows * np.arange(count, dtype=np.int64)

        def assign(region):
            index = region.region_index
            for j in range(6):
                assert a[j] == (add.x_p, add.y_p, add.x_qr, add.y_qr, fixed.window, fixed.u)[j]
                region.assign_advice_column(a[j], 0, _blank(rows * count) if columns is None else columns[j])
            if count:
                for k in range(H):
                    coeffs = fields.to_limbs([row[k] for row in fixed_base.lagrange_coeffs] + [0], FP)
                    region.assign_fixed_column(fixed.lagrange_coeffs[k], 0, np.tile(coeffs, (count, 1)))
                region.assign_fixed_column(fixed.fixed_z, 0, np.tile(fields.to_limbs(list(fixed_base.z) + [0], FP), (count, 1)))
            region.enable_selector_rows(fixed.running_sum_config.q_range_check,
                                        (base_rows[:, None] + np.arange(nw, dtype=np.int64)[None, :]).reshape(-1))
            region.enable_selector_rows(inc.q_add_incomplete, (base_rows[:, None] + np.arange(1, nw - 1, dtype=np.int64)[None, :]).reshape(-1))
            for i in range(count):
                region.constrain_equal(Cell(index, rows * i, fixed.window), sources[i].cell())
                region.constrain_constant(Cell(index, rows * i + nw, fixed.window), 0)
                region.constrain_equal(Cell(index, rows * i + 1, add.x_qr), Cell(index, rows * i, add.x_p))
                region.constrain_equal(Cell(index, rows * i + 1, add.y_qr), Cell(index, rows * i, add.y_p))
            return index
        return layouter.assign_region(name, assign)

    def _sum_trace(self, layouter, what: str, fixed_base: FixedBaseTables, cells, values, trace, launch, aux_width: int):
        """(columns, aux) of a running-sum bulk path as device tensors, or (None, None) without a witness.  cells: per input the
        AssignedCells the canonical limbs are read from where `values` has none; launch(FixedBase, *limbs) -> the trace"""
        import torch
        count, nw = len(cells[0]), fixed_base.num_windows
        if not layouter.cs.collect_advice or not count:
            return None, None
        if trace is None:
            if fixed_base.device is None:
                raise ValueError(f"{what}: the tables have no device copy to multiply over")
            values = list(values) if values is not None else [None] * len(cells)
            for j, group in enumerate(cells):
                if values[j] is None:
                    ints = [value_int(cell.value(), self.config.add.modulus) for cell in group]
                    if any(v is None for v in ints):
                        raise Synthesis(f"{what}: a witness is needed and there is none")
                    values[j] = fields.to_limbs(ints, FP, montgomery=False)
            trace = launch(fixed_base.device, *[v if torch.is_tensor(v) else _tensor(v).to(fields.current_device()) for v in values])
        columns, aux = (_tensor(t) for t in trace)
        if tuple(columns.shape) != (6, (nw + 1) * count, 4) or tuple(aux.shape) != (count, aux_width, 4):
            raise ValueError(f"{what}: the trace is ((6, {nw + 1} * count, 4), (count, {aux_width}, 4))")
        return columns, aux

    def mul_fixed_short_many(self, layouter, fixed_base: FixedBaseTables, magnitudes, signs, values=None, trace=None) -> MulFixedSumMany:
        """`count` multiplications [sign_i magnitude_i]B over the base's 22-window tables: ONE region of 23 * count rows whose advice
        columns 0 - 5 come from the device (`ecc.mul_fixed_short_trace`), the running sum of magnitude i in the `window` column of rows
        23 i .., then one region of 2 * count rows: the complete addition of multiplication i in row 2 i, and in row 2 i + 1 the short
        gate's cells -- the sign, z_21 and the signed y beside the sum.  Per multiplication the gates, cells and equality constraints
        of `mul_fixed_short`.

        magnitudes, signs: AssignedCells.  values: (magnitudes, signs), each (count, 4) CANONICAL limbs where the caller has them on
        the device already (else they are read from the cells); trace: (columns, aux) where the caller has them.  The copy of sign i
        in the gate's row is the one value no trace holds as a cell's: it is read from the sign's cell either way.  Without a witness
        (keygen) the same shape is laid out and nothing is launched."""
        import torch
        c, m = self.config, self.config.add.modulus
        if c.mul_fixed_short is None:
            raise ValueError("mul_fixed_short_many: the chip was configured without fixed_bases")
        count, nw = len(magnitudes), NUM_WINDOWS_SHORT
        if len(signs) != count or fixed_base.num_windows != nw:
            raise ValueError("mul_fixed_short_many: one sign per magnitude, over tables of 22 windows")
        columns, aux = self._sum_trace(layouter, "mul_fixed_short_many", fixed_base, (magnitudes, signs), values, trace,
                                       primitive.mul_fixed_short_trace, primitive.SHORT_AUX)
        add, fixed = c.add, c.mul_fixed
        result = MulFixedSumMany(c, count, nw, True)
        result.region_index = self._running_sum_many(layouter, "Short fixed-base mul (incomplete addition) many", fixed_base, magnitudes,
                                                     columns)
        second = None
        if aux is not None:
            sign_ints = [value_int(s.value(), m) for s in signs]
            if any(v is None for v in sign_ints):
                raise Synthesis("mul_fixed_short_many: a witness is needed and there is none")
            last = torch.from_numpy((nw + 1) * np.arange(count, dtype=np.int64) + nw - 1).to(columns.device)
            second = {fixed.window: _tensor(fields.to_limbs(sign_ints, FP)), fixed.u: columns[4][last], add.y_p: aux[:, 11]}

        def short_gate(region):
            index = region.region_index
            region.enable_selector_rows(c.mul_fixed_short.q_mul_fixed_short, 2 * np.arange(count, dtype=np.int64) + 1)
            for i in range(count):
                region.constrain_equal(Cell(index, 2 * i + 1, fixed.window), signs[i].cell())
                region.constrain_equal(Cell(index, 2 * i + 1, fixed.u), result.z(i, nw - 1))      # the last window, in a free cell of u
        result.add_region_index = self.additions_many(
            layouter, "Short fixed-base mul (most significant word) many", count, aux,
            lambda i: [Cell(result.region_index, (nw + 1) * i + nw - 1, column) for column in (add.x_p, add.y_p, add.x_qr, add.y_qr)],
            second=second, extra=short_gate)
        if aux is not None:
            result.outputs = torch.stack([aux[:, 9], aux[:, 11]], dim=1).contiguous()
        return result

    def mul_fixed_base_field_elem_many(self, layouter, fixed_base: FixedBaseTables, alphas, values=None, trace=None) -> MulFixedSumMany:
        """`count` multiplications [alpha_i]B for cells alpha_i of Fp read as integers, each with its canonicity check: ONE region of
        86 * count rows whose advice columns 0 - 5 come from the device (`ecc.mul_fixed_base_field_trace`), one region with the `count`
        complete additions, one `range_check_many` of the alpha_0' at 13 words, and one region of 3 * count rows with the gate
        "Canonicity checks".  Per multiplication the gates, cells and equality constraints of `mul_fixed_base_field_elem`.

        alphas: AssignedCells.  values: (count, 4) CANONICAL limbs where the caller has them on the device already (else they are read
        from the cells); trace: (columns, aux) where the caller has them.  Without a witness (keygen) the same shape is laid out and
        nothing is launched."""
        import torch
        c = self.config
        config = c.mul_fixed_base_field
        if config is None:
            raise ValueError("mul_fixed_base_field_elem_many: the chip was configured without fixed_bases")
        count, nw = len(alphas), NUM_WINDOWS
        if fixed_base.num_windows != nw:
            raise ValueError("mul_fixed_base_field_elem_many: tables of 85 windows")
        columns, aux = self._sum_trace(layouter, "mul_fixed_base_field_elem_many", fixed_base, (alphas,), None if values is None else (values,),
                                       trace, primitive.mul_fixed_base_field_trace, primitive.BASE_FIELD_AUX)
        add, fixed = c.add, c.mul_fixed
        result = MulFixedSumMany(c, count, nw, False)
        result.region_index = self._running_sum_many(layouter, "Base-field elem fixed-base mul (incomplete addition) many", fixed_base, alphas,
                                                     columns)
        result.add_region_index = self.additions_many(
            layouter, "Base-field elem fixed-base mul (complete addition) many", count, aux,
            lambda i: [Cell(result.region_index, (nw + 1) * i + nw - 1, column) for column in (add.x_p, add.y_p, add.x_qr, add.y_qr)])
        words = 13
        prime_rows = None
        if aux is not None:
            canonical = aux[:, 14].contiguous()
            prime_rows = range_primitive.decompose(canonical.to(fields.current_device()), words, field=FP)
            sums = config.lookup_config.range_check_many(layouter, [None] * count, words, False, values=canonical, trace=prime_rows)
            prime_rows = _tensor(prime_rows).reshape(count, words + 1, 4)
        else:
            sums = config.lookup_config.range_check_many(layouter, [None] * count, words, False)
        result.alpha_0_prime = sums
        canon = config.canon_advices

        def canonicity(region):
            index = region.region_index
            if aux is None:
                col0 = col1 = col2 = _blank(3 * count)
            else:
                dev_ = columns.device
                at = torch.from_numpy((nw + 1) * np.arange(count, dtype=np.int64)).to(dev_)
                z = columns[4]
                zero = torch.zeros_like(z[at])
                aux_d, prime_d = aux.to(dev_), prime_rows.to(dev_)
                col0 = torch.stack([z[at], aux_d[:, 11], prime_d[:, words]], dim=1).reshape(3 * count, 4)
                col1 = torch.stack([zero, aux_d[:, 12], z[at + 44]], dim=1).reshape(3 * count, 4)
                col2 = torch.stack([z[at + 84], aux_d[:, 13], z[at + 43]], dim=1).reshape(3 * count, 4)
            for column, values_ in zip(canon, (col0, col1, col2)):
                region.assign_advice_column(column, 0, values_)
            region.enable_selector_rows(config.q_mul_fixed_base_field, 3 * np.arange(count, dtype=np.int64) + 1)
            for i in range(count):
                region.constrain_equal(Cell(index, 3 * i, canon[0]), alphas[i].cell())
                region.constrain_equal(Cell(index, 3 * i, canon[2]), result.z(i, 84))
                region.constrain_equal(Cell(index, 3 * i + 1, canon[0]), sums[i][0])
                region.constrain_equal(Cell(index, 3 * i + 2, canon[0]), sums[i][words])
                region.constrain_equal(Cell(index, 3 * i + 2, canon[1]), result.z(i, 44))
                region.constrain_equal(Cell(index, 3 * i + 2, canon[2]), result.z(i, 43))
            return index
        result.canonicity_region_index = layouter.assign_region("Canonicity checks many", canonicity)
        if aux is not None:
            result.outputs = aux[:, 9:11].contiguous()
        return result

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

    @staticmethod
    def new_from_constant(chip: EccChip, layouter, value) -> "Point":       # ecc.rs:500-508
        return Point(chip, chip.witness_point_from_constant(layouter, value))

    def mul_sign(self, layouter, sign: AssignedCell) -> "Point":            # ecc.rs:441-451
        return Point(self.chip, self.chip.mul_sign(layouter, sign, self._inner))


class FixedPoint:
    """ecc.rs:577-607: a full-width fixed base"""

    def __init__(self, chip: EccChip, inner: FixedBaseTables):
        self.chip, self._inner = chip, inner

    @staticmethod
    def from_inner(chip: EccChip, inner: FixedBaseTables) -> "FixedPoint":
        return FixedPoint(chip, inner)

    def mul(self, layouter, by: ScalarFixed):
        """-> (Point, ScalarFixed)"""
        point, scalar = self.chip.mul_fixed(layouter, by, self._inner)
        return Point(self.chip, point), scalar


class FixedPointShort:
    """ecc.rs:640-672: a fixed base multiplied by short signed scalars, over its 22-window tables"""

    def __init__(self, chip: EccChip, inner: FixedBaseTables):
        self.chip, self._inner = chip, inner

    @staticmethod
    def from_inner(chip: EccChip, inner: FixedBaseTables) -> "FixedPointShort":
        return FixedPointShort(chip, inner)

    def mul(self, layouter, by: ScalarFixedShort):
        """-> (Point, ScalarFixedShort)"""
        point, scalar = self.chip.mul_fixed_short(layouter, by, self._inner)
        return Point(self.chip, point), scalar


class FixedPointBaseField:
    """ecc.rs:609-638: a fixed base multiplied by elements of the base field"""

    def __init__(self, chip: EccChip, inner: FixedBaseTables):
        self.chip, self._inner = chip, inner

    @staticmethod
    def from_inner(chip: EccChip, inner: FixedBaseTables) -> "FixedPointBaseField":
        return FixedPointBaseField(chip, inner)

    def mul(self, layouter, by: AssignedCell) -> "Point":
        return Point(self.chip, self.chip.mul_fixed_base_field_elem(layouter, by, self._inner))


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
