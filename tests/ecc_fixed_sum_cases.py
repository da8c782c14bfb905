"""Shared by test_ecc_fixed_sum_host.py and test_gpu_ecc_fixed_sum.py (a helper: nothing here is collected): the restatement, in Python
integers over `oracle.pasta`, of what the two fixed-base multiplications by a running sum assign (ecc/chip/mul_fixed/short.rs:108-243,
mul_fixed/base_field_elem.rs:165-378 over mul_fixed.rs:172-405 and utilities/decompose_running_sum.rs) in the layout of
h2_ecc_mul_fixed_short_trace_device and h2_ecc_mul_fixed_base_field_trace_device, the three gates they stand under evaluated on those
integers, the case list, the refusals, the stream-order cases and the circuits with their `many` arm."""
import ctypes as C
import functools
import random

import numpy as np

import ecc_cases as ec
import ecc_fixed_cases as fx
from ecc_cases import ORDER, P
from ecc_fixed_cases import GENERATOR, H, NUM_WINDOWS, NUM_WINDOWS_SHORT, U, WINDOW, X_P, X_QR, Y_P, Y_QR
from halo2_amd import _lib

FP = 0
SHORT, BASE_FIELD = "h2_ecc_mul_fixed_short_trace_device", "h2_ecc_mul_fixed_base_field_trace_device"
SHORT_AUX, BASE_FIELD_AUX = 12, 15
INV_H = pow(H, -1, P)
T_P = fx.T_P
MAX_MULS = 1 << 30

LAST_DOUBLING_SHORT = 0xB6DB6DB6DB6DB6DC                   # short.rs tests: the magnitude whose last addition is a doubling
SHORT_MAGNITUDES = [0, 1, (1 << 64) - 1, LAST_DOUBLING_SHORT]
SIGNS = [1, P - 1]
INVALID_MAGNITUDES = [1 << 64, (1 << 66) - 1, 1 << 66, P - 1]                  # short.rs tests: magnitude_error
INVALID_SIGNS = [0, 2, P - 2]                                                  # short.rs tests: sign_error
COUNTS = (1, 65)                                           # 64 lanes a workgroup: 65 is the first count with a second, partial one
CHUNKED = ((65, 64), (3, 1))                               # (count, lanes of scratch)


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
def running_sum(value, word_bits, num_windows):
    """RunningSumConfig._decompose on an element of Fp: the windows of the LOW word_bits bits and z_0 .. z_nw by the field's recurrence"""
    low = value & ((1 << word_bits) - 1)
    words = [low >> (3 * w) & 7 for w in range(num_windows)]
    zs = [value % P]
    for k in words:
        zs.append((zs[-1] - k) * INV_H % P)
    return words, zs


def sum_trace(table, us, value, word_bits):
    """-> (columns, record, result): columns[c][row] over nw + 1 rows, x_p y_p x_qr y_qr window u with the running sum in `window`
    and zeros where nothing is assigned; the 11 elements of the closing complete addition; the product"""
    nw = len(table)
    words, zs = running_sum(value, word_bits, nw)
    cols = [[0] * (nw + 1) for _ in range(6)]
    cols[WINDOW] = list(zs)
    acc = None
    for w, d in enumerate(words):
        cols[X_P][w], cols[Y_P][w] = point = table[w][d]
        cols[U][w] = us[w][d]
        if w == 0:
            acc = point
        else:
            cols[X_QR][w], cols[Y_QR][w] = acc
            if w < nw - 1:
                acc = ec.incomplete_add(point, acc)
                assert acc is not None
    result, witnesses = ec.complete_add(table[nw - 1][words[-1]], acc)
    return cols, list(table[nw - 1][words[-1]] + acc + witnesses + result), result


def short_trace(table, us, magnitude, sign):
    """-> (columns, aux of 12, (x, signed y))"""
    cols, record, (x, y) = sum_trace(table, us, magnitude, 64)
    signed = -y % P if sign == P - 1 else y                                    # short.rs:178-184
    return cols, record + [signed], (x, signed)


def alpha_cells(alpha):
    """base_field_elem.rs:212-260 -> alpha_0', alpha_1, alpha_2"""
    return (alpha - (alpha >> 252 << 252) + (1 << 130) - T_P) % P, alpha >> 252 & 3, alpha >> 254 & 1


def base_field_trace(table, us, alpha):
    """-> (columns, the 14 Montgomery elements of the aux, alpha_0' (its 15th, canonical), the product)"""
    cols, record, result = sum_trace(table, us, alpha, 255)
    prime, a_1, a_2 = alpha_cells(alpha)
    return cols, record + [prime, a_1, a_2], prime, result


def limbs(ints, montgomery=True):
    import stream_cases as stc
    return stc.limbs(ints, FP, montgomery)


def columns_bytes(per_item) -> bytes:
    return b"".join(limbs([v for cols in per_item for v in cols[c]]).tobytes() for c in range(6))


def short_bytes(table, us, pairs):
    want = [short_trace(table, us, m, s) for m, s in pairs]
    return columns_bytes([w[0] for w in want]), limbs([v for w in want for v in w[1]]).tobytes()


def base_field_bytes(table, us, alphas):
    want = [base_field_trace(table, us, a) for a in alphas]
    aux = b"".join(limbs(w[1]).tobytes() + limbs([w[2]], montgomery=False).tobytes() for w in want)
    return columns_bytes([w[0] for w in want]), aux


# ---- the gates, on integers -------------------------------------------------------------------------------------------------------------------
def coords_check(cols, coeffs, zs_fixed, nw):
    """"Running sum coordinates check" (mul_fixed.rs:115-169) on rows 0 .. nw-1 -> the nonzero (row, name)"""
    bad = []
    for w in range(nw):
        word = (cols[WINDOW][w] - cols[WINDOW][w + 1] * H) % P
        x, y, u = cols[X_P][w], cols[Y_P][w], cols[U][w]
        polys = {"check x": fx.evaluate(coeffs[w], word) - x, "check y": u * u - y - zs_fixed[w], "on-curve": y * y - x * x * x - 5}
        bad += [(w, name) for name, v in polys.items() if v % P]
    return bad


def range_checks(cols, nw):
    """the running sum's "range check" on rows 0 .. nw-1 -> the rows whose word is not in 0 .. 7"""
    return [w for w in range(nw) if (cols[WINDOW][w] - cols[WINDOW][w + 1] * H) % P >= H]


def short_gate(cols, aux, sign):
    """"Short fixed-base mul gate" (short.rs:32-75) on the second region's row 1 -> the nonzero names"""
    y_p, y_a, last_window = aux[11], aux[10], cols[WINDOW][21]
    polys = {"last_window_check": last_window * (1 - last_window), "sign_check": sign * sign - 1, "y_check": (y_p - y_a) * (y_p + y_a),
             "negation_check": sign * y_p - y_a}
    return [name for name, v in polys.items() if v % P]


def canonicity_gate(cols, aux, z_13_prime):
    """"Canonicity checks" (base_field_elem.rs:54-160) -> the nonzero names"""
    z = cols[WINDOW]
    alpha, z_84, z_44, z_43 = z[0], z[84], z[44], z[43]
    prime, a_1, a_2 = aux[11], aux[12], aux[13]
    alpha_0 = alpha - z_84 * (1 << 252)
    a_43 = z_43 - z_44 * H
    polys = {"MSB = 1 => alpha_1 = 0": a_2 * a_1, "MSB = 1 => alpha_0_hi_120 = 0": a_2 * (z_44 - z_84 * (1 << 120)),
             "MSB = 1 => a_43 = 0 or 1": a_2 * a_43 * (1 - a_43), "MSB = 1 => z_13_alpha_0_prime = 0": a_2 * z_13_prime,
             "alpha_1_range_check": a_1 * (1 - a_1) * (2 - a_1) * (3 - a_1), "alpha_2_range_check": a_2 * (1 - a_2),
             "z_84_alpha_check": z_84 - (a_1 + a_2 * 4), "alpha_0_prime check": prime - (alpha_0 + (1 << 130) - T_P)}
    return [name for name, v in polys.items() if v % P]


# ---- the case list ----------------------------------------------------------------------------------------------------------------------------
def short_edges():
    return [(m, s) for m in SHORT_MAGNITUDES for s in SIGNS]


def short_invalid():
    rnd = random.Random(0x5A01)
    return [(m, 1) for m in INVALID_MAGNITUDES] + [(rnd.getrandbits(64), s) for s in INVALID_SIGNS]


@functools.lru_cache(maxsize=None)
def short_pairs(count, valid_only=False):
    """the edges first, then the invalid inputs, then random pairs, cut to `count`"""
    rnd = random.Random(0x5A02)
    head = short_edges() + ([] if valid_only else short_invalid())
    return (head + [(rnd.getrandbits(64), rnd.choice(SIGNS)) for _ in range(count)])[:count]


def base_field_edges():
    return list(fx.EDGE_BASE_FIELD) + [fx.LAST_DOUBLING]


@functools.lru_cache(maxsize=None)
def base_field_alphas(count):
    rnd = random.Random(0x5A03)
    return (base_field_edges() + [rnd.randrange(P) for _ in range(count)])[:count]


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------------
def descriptor(num_windows, points=0x1000, u=0x2000, scratch=0x3000, scratch_elems=None, stream=0):
    elems = num_windows - 2 if scratch_elems is None else scratch_elems
    return _lib.EccFixedSum(num_windows, points, u, scratch, elems, stream)


def refusals(a=0x4000, b=0x5000, c=0x6000, d=0x7000, **table):
    """[(what, entry point, descriptor or None, the arguments after it)]: every one is H2_ERR_ARGS before anything touches the device.
    The pointers are never read, so without a device any nonzero value does.  table: the descriptor's pointers, where they are real."""
    rows = []
    for entry, nw, other, tail in ((SHORT, NUM_WINDOWS_SHORT, NUM_WINDOWS, (a, b, 1, c, d)), (BASE_FIELD, NUM_WINDOWS, NUM_WINDOWS_SHORT, (a, 1, c, d))):
        n_at = len(tail) - 3
        good = lambda **kw: descriptor(nw, **{**table, **kw})
        rows += [("a null descriptor", entry, None, tail), ("the other form's windows", entry, descriptor(other, **table), tail),
                 ("no windows", entry, descriptor(0, scratch_elems=64, **table), tail),
                 ("two windows", entry, descriptor(2, scratch_elems=64, **table), tail),
                 ("count over the limit", entry, good(scratch_elems=1 << 20), tail[:n_at] + (MAX_MULS + 1,) + tail[n_at + 1:]),
                 ("a null table", entry, good(points=None), tail), ("null roots", entry, good(u=None), tail),
                 ("a null scratch", entry, good(scratch=None), tail), ("scratch one element short", entry, good(scratch_elems=nw - 3), tail),
                 ("no scratch", entry, good(scratch_elems=0), tail)]
        rows += [(f"null argument {at}", entry, good(), tail[:at] + (None,) + tail[at + 1:]) for at in range(len(tail)) if at != n_at]
    return rows


def refuse(lib, row):
    _, entry, spec, tail = row
    return getattr(lib, entry)(None if spec is None else C.byref(spec), *tail)


# ---- stream order -----------------------------------------------------------------------------------------------------------------------------
STREAM_LANES = 65


@functools.lru_cache(maxsize=None)
def _stream_tables(num_windows):
    """a set-up object: the generator's tables and a scratch for every lane, built at the first call"""
    import torch

    from halo2_amd import ecc, fields
    base = ecc.FixedBase(fields.to_limbs(list(GENERATOR), FP).reshape(8), num_windows)
    return base, torch.empty((STREAM_LANES * (num_windows - 2), 4), dtype=torch.int64, device=fields.current_device())


def stream_cases():
    import stream_cases as stc
    n = STREAM_LANES

    def pairs(seed):
        rnd = random.Random(0x5B00 + seed)
        return (short_edges() if seed == stc.REAL else []) + [(rnd.getrandbits(64), rnd.choice(SIGNS)) for _ in range(n)]

    def alphas(seed):
        rnd = random.Random(0x5B10 + seed)
        return ((base_field_edges() if seed == stc.REAL else []) + [rnd.randrange(P) for _ in range(n)])[:n]

    def wanted(nw, make):
        table, _, _, us = fx.generator_tables(nw)
        return lambda seed: b"".join(make(table, us, seed))

    def call(entry, nw):
        def run(i, u, sp):
            base, scratch = _stream_tables(nw)
            d = _lib.EccFixedSum(nw, base.points.data_ptr(), base.us.data_ptr(), scratch.data_ptr(), scratch.shape[0], sp)
            args = [i[name].data_ptr() for name in i]
            stc.ok(getattr(stc._lib(), entry)(C.byref(d), *args, n, u["columns"].data_ptr(), u["aux"].data_ptr()))
        return run

    def roots(nw):                                         # the column u is compared as its squares: either root is a valid table
        return lambda name, raw: stc._square_roots_at(5 * (nw + 1) * n * 32, (nw + 1) * n)(name, raw) if name == "columns" else raw
    canonical = lambda ints: limbs(ints, montgomery=False)
    short_n, full_n = NUM_WINDOWS_SHORT, NUM_WINDOWS
    return {
        SHORT: stc.Case("ecc-mul-fixed-short-trace", SHORT, n,
                        lambda seed: {"magnitudes": canonical([m for m, _ in pairs(seed)[:n]]), "signs": canonical([s for _, s in pairs(seed)[:n]])},
                        lambda: {"columns": 6 * (short_n + 1) * n * 32, "aux": SHORT_AUX * n * 32}, call(SHORT, short_n),
                        wanted(short_n, lambda table, us, seed: short_bytes(table, us, pairs(seed)[:n])),
                        stc.fields_valid(FP, "magnitudes", "signs", montgomery=False), post=roots(short_n)),
        BASE_FIELD: stc.Case("ecc-mul-fixed-base-field-trace", BASE_FIELD, n, lambda seed: {"alphas": canonical(alphas(seed))},
                             lambda: {"columns": 6 * (full_n + 1) * n * 32, "aux": BASE_FIELD_AUX * n * 32}, call(BASE_FIELD, full_n),
                             wanted(full_n, lambda table, us, seed: base_field_bytes(table, us, alphas(seed))),
                             stc.fields_valid(FP, "alphas", montgomery=False), post=roots(full_n)),
    }


# ---- the circuits -----------------------------------------------------------------------------------------------------------------------------
from halo2_amd.circuit import Circuit                                         # noqa: E402
from halo2_amd.gadgets.ecc import EccChip, FixedPointBaseField, FixedPointShort, ScalarFixedShort      # noqa: E402
from halo2_amd.gadgets.utilities import load_private                          # noqa: E402


class _Traced:
    """passes the trace of the bulk call through `tamper(columns, aux)` before the gadget reads it"""

    def __init__(self, name, tamper):
        self.name, self.tamper = name, tamper

    def __enter__(self):
        from halo2_amd.gadgets import ecc as g
        self.g, self.original = g, getattr(g.primitive, self.name)
        if self.tamper is not None:
            def traced(*args, **kw):
                columns, aux = self.original(*args, **kw)
                self.tamper(columns, aux)
                return columns, aux
            setattr(g.primitive, self.name, traced)

    def __exit__(self, *exc):
        setattr(self.g.primitive, self.name, self.original)


class ShortManyCircuit(Circuit):
    """fx.ShortCircuit with a `many` arm: one `mul_fixed_short` per (magnitude, sign), or all of them through one
    `mul_fixed_short_many`; the inputs are loaded the same way on both arms, magnitude then sign, pair after pair.  tamper: see _Traced"""

    def __init__(self, pairs, tables, witness=True, many=False, tamper=None):
        self.pairs, self.tables, self.witness, self.many, self.tamper = pairs, tables, witness, many, tamper
        self.products, self.bulk, self.inputs = [], None, []

    def without_witnesses(self):
        return ShortManyCircuit(self.pairs, self.tables, witness=False, many=self.many)

    configure = staticmethod(fx.configure_fixed)

    def synthesize(self, config, layouter):
        self.config, self.layouter = config, layouter
        config.lookup_config.load_range_check_table(layouter)
        chip = EccChip(config)
        v = (lambda x: x) if self.witness else (lambda x: None)
        self.inputs = [(load_private(layouter, config.advices[0], v(m)), load_private(layouter, config.advices[0], v(s))) for m, s in self.pairs]
        if self.many:
            with _Traced("mul_fixed_short_trace", self.tamper):
                self.bulk = chip.mul_fixed_short_many(layouter, self.tables, [m for m, _ in self.inputs], [s for _, s in self.inputs])
            return
        base = FixedPointShort.from_inner(chip, self.tables)
        self.products = [base.mul(layouter, ScalarFixedShort.new(chip, layouter, cells)) for cells in self.inputs]


class BaseFieldManyCircuit(Circuit):
    """fx.BaseFieldCircuit with a `many` arm"""

    def __init__(self, alphas, tables, witness=True, many=False, tamper=None):
        self.alphas, self.tables, self.witness, self.many, self.tamper = alphas, tables, witness, many, tamper
        self.products, self.bulk, self.inputs = [], None, []

    def without_witnesses(self):
        return BaseFieldManyCircuit(self.alphas, self.tables, witness=False, many=self.many)

    configure = staticmethod(fx.configure_fixed)

    def synthesize(self, config, layouter):
        self.config, self.layouter = config, layouter
        config.lookup_config.load_range_check_table(layouter)
        chip = EccChip(config)
        self.inputs = [load_private(layouter, config.advices[0], a if self.witness else None) for a in self.alphas]
        if self.many:
            with _Traced("mul_fixed_base_field_trace", self.tamper):
                self.bulk = chip.mul_fixed_base_field_elem_many(layouter, self.tables, self.inputs)
            return
        base = FixedPointBaseField.from_inner(chip, self.tables)
        self.products = [base.mul(layouter, cell) for cell in self.inputs]


class AddManyCircuit(Circuit):
    """`add` of every pair of points, or all of them through one `add_many`; (0, 0) is the identity"""

    def __init__(self, pairs, witness=True, many=False):
        self.pairs, self.witness, self.many, self.sums, self.bulk = pairs, witness, many, [], None

    def without_witnesses(self):
        return AddManyCircuit(self.pairs, witness=False, many=self.many)

    configure = staticmethod(fx.configure_fixed)

    def synthesize(self, config, layouter):
        self.config, self.layouter = config, layouter
        config.lookup_config.load_range_check_table(layouter)
        chip = EccChip(config)
        v = (lambda x: x) if self.witness else (lambda x: None)
        points = [(chip.witness_point(layouter, v(p)), chip.witness_point(layouter, v(q))) for p, q in self.pairs]
        if self.many:
            self.bulk = chip.add_many(layouter, [p for p, _ in points], [q for _, q in points])
        else:
            self.sums = [chip.add(layouter, p, q) for p, q in points]


def add_pairs():
    """P + Q, P + P, P + (-P), the identity on either side and on both"""
    p, q = ec.random_bases(2, seed=0x5C)
    return [(p, q), (p, p), (p, (p[0], -p[1] % P)), ((0, 0), q), (p, (0, 0)), ((0, 0), (0, 0))]
