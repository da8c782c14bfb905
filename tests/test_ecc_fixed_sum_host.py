"""The bulk short and base-field fixed-base multiplications on the host: the integer model of tests/ecc_fixed_sum_cases.py against
`ec_mul`, the running sum's recurrence and the three gates its rows stand under, what each invalid input breaks, what the case list
reaches, the descriptor in the header and in ctypes, every refusal of the two entry points (they come before any device work), the
source scan for kept device memory, and the circuits without a witness: the keygen shape of as many single calls.  Nothing here needs
a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ecc_cases as ec
import ecc_fixed_cases as fx
import ecc_fixed_sum_cases as fs
from ecc_fixed_sum_cases import GENERATOR, NUM_WINDOWS, NUM_WINDOWS_SHORT, ORDER, P
from halo2_amd import _lib
from halo2_amd import circuit as front
from halo2_amd.gadgets.utilities import decompose_word

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "halo2_mi355x.h")
UNIT = os.path.join(ROOT, "halo2_amd", "csrc", "ecc_fixed_sum.hip")


def _short_tables():
    table, coeffs, zs, us = fx.generator_tables(NUM_WINDOWS_SHORT)
    return table, coeffs, zs, us


def _full_tables():
    return fx.generator_tables(NUM_WINDOWS)


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", fs.short_pairs(14, valid_only=True), ids=lambda p: f"{p[0]:#x}*{'+' if p[1] == 1 else '-'}")
def test_the_short_model_multiplies_by_the_signed_magnitude(pair):
    magnitude, sign = pair
    table, coeffs, zs_fixed, us = _short_tables()
    cols, aux, result = fs.short_trace(table, us, magnitude, sign)
    assert result == ec.ec_mul((magnitude if sign == 1 else -magnitude) % ORDER, GENERATOR)
    assert (aux[9], aux[11]) == result and aux[10] in (aux[11], -aux[11] % P)
    z = cols[fs.WINDOW]
    assert len(z) == 23 and z == [magnitude >> (3 * w) for w in range(23)] and z[22] == 0
    words = decompose_word(magnitude, 64, 3)
    assert [(a - 8 * b) % P for a, b in zip(z, z[1:])] == words and words[21] < 2
    assert not fs.range_checks(cols, 22) and not fs.coords_check(cols, coeffs, zs_fixed, 22) and not fs.short_gate(cols, aux, sign)
    assert all(cols[c][22] == 0 for c in range(6) if c != fs.WINDOW) and cols[fs.X_QR][0] == cols[fs.Y_QR][0] == 0
    assert (cols[fs.X_QR][1], cols[fs.Y_QR][1]) == (cols[fs.X_P][0], cols[fs.Y_P][0])


def test_the_short_doubling_string_ends_on_a_doubling():
    table, _, _, us = _short_tables()
    _, aux, _ = fs.short_trace(table, us, fs.LAST_DOUBLING_SHORT, 1)
    assert aux[0:2] == aux[2:4] and aux[5] == 0 and aux[8] != 0               # P + P: alpha = inv0(0), delta = 1 / 2y
    _, aux, result = fs.short_trace(table, us, 0, P - 1)
    assert result == (0, 0) and aux[11] == 0                                  # the identity's 0 stays 0 under the sign -1


@pytest.mark.parametrize("alpha", fs.base_field_alphas(10), ids=hex)
def test_the_base_field_model_multiplies_by_alpha(alpha):
    table, coeffs, zs_fixed, us = _full_tables()
    cols, aux, prime, result = fs.base_field_trace(table, us, alpha)
    assert result == ec.ec_mul(alpha % ORDER, GENERATOR) == (aux[9], aux[10])
    z = cols[fs.WINDOW]
    assert len(z) == 86 and z == [alpha >> (3 * w) for w in range(86)] and z[85] == 0
    assert [(a - 8 * b) % P for a, b in zip(z, z[1:])] == decompose_word(alpha, 255, 3)
    assert not fs.range_checks(cols, 85) and not fs.coords_check(cols, coeffs, zs_fixed, 85)
    assert prime == aux[11] < 1 << 253 and not fs.canonicity_gate(cols, aux, prime >> 130)
    assert (prime >> 130 == 0) or not aux[13]                                 # MSB = 1 leaves alpha_0' within 130 bits
    if alpha == fx.LAST_DOUBLING:
        assert aux[0:2] == aux[2:4]


@pytest.mark.parametrize("magnitude", fs.INVALID_MAGNITUDES, ids=hex)
def test_a_magnitude_of_65_bits_breaks_the_constant_and_nothing_else(magnitude):
    """the cells are RunningSumConfig._decompose's: the windows of the low 64 bits, the field's recurrence, z_22 != 0"""
    table, coeffs, zs_fixed, us = _short_tables()
    cols, aux, _ = fs.short_trace(table, us, magnitude, 1)
    z = cols[fs.WINDOW]
    inv = pow(8, -1, P)
    want = [magnitude]
    for word in decompose_word(magnitude, 64, 3)[:22]:
        want.append((want[-1] - word) * inv % P)
    assert z == want and z[22] != 0
    assert not fs.range_checks(cols, 22) and not fs.coords_check(cols, coeffs, zs_fixed, 22)
    bits_64_65 = magnitude >> 64 & 3
    assert z[22] == ((magnitude >> 66) + bits_64_65 * pow(4, -1, P)) % P      # what the kernel computes without a division
    assert ("last_window_check" in fs.short_gate(cols, aux, 1)) == (z[21] > 1)


@pytest.mark.parametrize("sign", fs.INVALID_SIGNS)
def test_a_bad_sign_breaks_the_sign_check(sign):
    table, _, _, us = _short_tables()
    magnitude = next(m for m, s in fs.short_invalid() if s == sign)
    cols, aux, result = fs.short_trace(table, us, magnitude, sign)
    assert aux[11] == aux[10] and cols[fs.WINDOW][22] == 0                    # every sign but -1 leaves y alone
    assert fs.short_gate(cols, aux, sign) == ["sign_check", "negation_check"]


def test_the_case_list_reaches_what_it_should():
    pairs = fs.short_pairs(65)
    assert len(pairs) == 65 and set(fs.short_edges()) <= set(pairs) and set(fs.short_invalid()) <= set(pairs)
    assert {m for m, _ in pairs} >= {0, 1, (1 << 64) - 1, 0xB6DB6DB6DB6DB6DC, 1 << 64, (1 << 66) - 1, 1 << 66, P - 1}
    assert {s for _, s in pairs} == {0, 1, 2, P - 2, P - 1}
    assert sum(1 for m, s in pairs if m < 1 << 64 and s in (1, P - 1)) > 40   # and random valid ones
    alphas = fs.base_field_alphas(65)
    assert len(alphas) == 65 and set(fx.EDGE_BASE_FIELD) | {fx.LAST_DOUBLING} <= set(alphas) and len(set(alphas)) == 65
    assert fs.COUNTS == (1, 65) and fs.CHUNKED == ((65, 64), (3, 1))
    assert all(0 <= v < P for m, s in pairs for v in (m, s)) and all(0 <= a < P for a in alphas)
    many = [fs.ShortManyCircuit, fs.BaseFieldManyCircuit]
    assert all("many" in c.__init__.__code__.co_varnames for c in many)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------------
def test_the_descriptor_is_the_same_in_the_header_and_in_ctypes():
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct h2_ecc_fixed_sum \{(.*?)\} h2_ecc_fixed_sum_t;", header, flags=re.S).group(1)
    names = ["num_windows", "d_points", "d_u", "d_scratch", "scratch_elems", "stream"]
    assert re.findall(r"([a-z_]+)\s*;", body) == [name for name, _ in _lib.EccFixedSum._fields_] == names
    assert C.sizeof(_lib.EccFixedSum) == 48 and _lib.EccFixedSum.scratch_elems.offset == 32
    protos = dict(re.findall(r"\bint\s+(h2_ecc_mul_fixed_(?:short|base_field)_trace_device)\s*\(([^()]*)\)\s*;", header))
    assert set(protos) == {fs.SHORT, fs.BASE_FIELD}
    for name, params in protos.items():
        assert re.match(r"\s*const\s+h2_ecc_fixed_sum_t\s*\*\s*d\b", params) and "stream" not in params
        assert len(_lib.SIGNATURES[name][0]) == params.count(",") + 1


@pytest.mark.parametrize("row", fs.refusals(), ids=lambda row: f"{row[1][17:-13]}: {row[0]}")
def test_refusals_come_before_the_device(row):
    import halo2_amd as h
    assert fs.refuse(h.lib(), row) == _lib.H2_ERR_ARGS


def test_the_refusal_list_is_complete():
    rows = fs.refusals()
    for entry, pointers in ((fs.SHORT, 4), (fs.BASE_FIELD, 3)):
        mine = [what for what, e, _, _ in rows if e == entry]
        assert len(mine) == 10 + pointers and len(set(mine)) == len(mine)


def test_the_argument_checks_come_before_the_device_check():
    """in the source: each entry point returns H2_ERR_ARGS before the one function that looks for a device is called"""
    code = re.sub(r"//[^\n]*", "", open(UNIT).read())
    bodies = re.findall(r'extern "C" int (h2_\w+)\([^)]*\)\s*\{(.*?)\n\}', code, flags=re.S)
    assert [name for name, _ in bodies] == [fs.SHORT, fs.BASE_FIELD]
    for _, body in bodies:
        assert "ensure_device" not in body and body.index("H2_ERR_ARGS") < body.index("sum_trace<")
    assert code.count("ensure_device()") == 1 and code.index("ensure_device()") > code.index("int sum_trace(")


def test_the_unit_owns_no_device_memory():
    code = re.sub(r"//[^\n]*", "", open(UNIT).read())
    assert "StreamContexts" not in code and "DevBuf" not in code and "hipMalloc" not in code and "g_" not in code


# ---- the circuits without a witness -------------------------------------------------------------------------------------------------------------
K = 11


def _keygen(circuit):
    _, assembly, _ = front.synthesize(circuit.without_witnesses(), K, fs.FP, fixed=True, advice=False, regions=True)
    return assembly


def copies(assembly):
    """the sizes of the permutation's cycles of more than one cell"""
    _, sizes = np.unique(assembly.permutation.aux, return_counts=True)
    return sorted(int(s) for s in sizes if s > 1)


def _circuits(form):
    if form == "short":
        tables = fx.host_tables(NUM_WINDOWS_SHORT)
        return [fs.ShortManyCircuit(fs.short_pairs(3), tables, many=many) for many in (True, False)]
    if form == "base_field":
        tables = fx.host_tables(NUM_WINDOWS)
        return [fs.BaseFieldManyCircuit(fs.base_field_alphas(3), tables, many=many) for many in (True, False)]
    return [fs.AddManyCircuit(fs.add_pairs()[:3], many=many) for many in (True, False)]


@pytest.mark.parametrize("form", ["short", "base_field", "add"])
def test_the_keygen_shape_is_that_of_as_many_single_calls(form):
    many_circuit, single_circuit = _circuits(form)
    cs_many, _, _ = front.synthesize(many_circuit.without_witnesses(), K, fs.FP, fixed=True, advice=False)
    cs_single, _, _ = front.synthesize(single_circuit.without_witnesses(), K, fs.FP, fixed=True, advice=False)
    assert cs_many.pinned() == cs_single.pinned()                             # the same constraint system
    many, single = _keygen(many_circuit), _keygen(single_circuit)
    assert many.selectors.sum(axis=1).tolist() == single.selectors.sum(axis=1).tolist() and many.selectors.sum() > 0
    assert copies(many) == copies(single) and sum(s - 1 for s in copies(many)) >= 3 * 4
    names = [r.name for r in many.regions]
    tail = {"short": ["Short fixed-base mul (incomplete addition) many", "Short fixed-base mul (most significant word) many"],
            "base_field": ["Base-field elem fixed-base mul (incomplete addition) many", "Base-field elem fixed-base mul (complete addition) many",
                           "13 words range check many", "Canonicity checks many"],
            "add": ["complete point addition many"]}[form]
    assert names[-len(tail):] == tail and len(names) < len([r.name for r in single.regions])
    # the fixed columns hold the same multiset: the tables row for row, and the constants the cells are constrained to
    for a, b in zip(many.host_columns(many.fixed), single.host_columns(single.fixed)):
        assert sorted(a) == sorted(b)
