"""Fixed-base multiplication on the host (no GPU): the restatement of tests/ecc_fixed_cases.py against `oracle.pasta.ec_mul`; the
order `EccChip.configure` creates the fixed-base configs in; the chip's full-width `mul_fixed`, `mul_fixed_short` with `mul_sign` and
`mul_fixed_base_field_elem` synthesized cell by cell over the restated tables and checked under tests/mock_prover_model.py, valid and
mutated; the fixed cells and selectors `mul_fixed_many` lays out; and the mirror of the reference's `MyEccCircuit` against the
constraint system of the reference's pinned key."""
import pytest

import ecc_cases as ec
import ecc_fixed_cases as fx
from ecc_fixed_cases import GENERATOR, NUM_WINDOWS, NUM_WINDOWS_SHORT, P, BaseFieldCircuit, MulFixedCircuit, ShortCircuit

K = 11
RANDOM = ec.random_scalars(3, seed=31)


def _named(failures, names):
    return [(f[0],) + (names[f[1]] if f[0] == "ConstraintNotSatisfied" else (f[1],)) + (f[2],) for f in failures]


# ---- 1: the restatement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_windows, scalars", [(NUM_WINDOWS, fx.EDGE_SCALARS + RANDOM), (NUM_WINDOWS_SHORT, fx.EDGE_SCALARS_SHORT)])
def test_the_restatement_multiplies(num_windows, scalars):
    """[k mod q]B for every edge scalar; no incomplete addition meets an exceptional pair; k = 0 ends on the identity and the two
    doubling strings on the doubling branch of complete addition"""
    table, _, _, us = fx.generator_tables(num_windows)
    for k in scalars:
        cols, aux, result = fx.mul_fixed_trace(table, us, k)
        assert result == ec.ec_mul(k, GENERATOR) == tuple(aux[9:11]), k
        assert (result == (0, 0)) == (k == 0)
        assert (aux[0:2] == aux[2:4]) == (k in (fx.LAST_DOUBLING, fx.LAST_DOUBLING_NON_CANONICAL))
        assert cols[fx.WINDOW] == fx.windows_of(k, num_windows) and cols[fx.X_QR][0] == cols[fx.Y_QR][0] == 0
        for w in range(num_windows):
            assert cols[fx.U][w] ** 2 % P == (cols[fx.Y_P][w] + fx.generator_tables(num_windows)[2][w]) % P


@pytest.mark.parametrize("num_windows", [NUM_WINDOWS_SHORT, NUM_WINDOWS])
def test_the_coefficients_interpolate_the_table(num_windows):
    table, coeffs, _, _ = fx.generator_tables(num_windows)
    for row, c in zip(table, coeffs):
        assert [fx.evaluate(c, k) for k in range(8)] == [pt[0] for pt in row]
    assert table[0][0] == ec.ec_mul(2, GENERATOR) and (0, 0) not in [pt for row in table for pt in row]


def test_the_last_window_takes_the_offsets_back():
    """constants.rs:61-79: sum_w scalars[w][k_w] = k mod q for any windows"""
    for nw in (2, NUM_WINDOWS_SHORT, NUM_WINDOWS):
        scalars = fx.window_scalars(nw)
        for k in (0, 1, (1 << (3 * nw)) - 1, 0o1234567 % (1 << (3 * nw))):
            assert sum(scalars[w][d] for w, d in enumerate(fx.windows_of(k, nw))) % fx.ORDER == k % fx.ORDER


# ---- 2: configure ----------------------------------------------------------------------------------------------------------------------------
def test_configure_appends_the_fixed_base_configs():
    """chip.rs:296-320: after the variable-base gates, mul_fixed (the running sum's gate, then the coordinates check), full_width,
    short and base_field_elem; q_running_sum, q_mul_fixed_full, q_mul_fixed_short and q_mul_fixed_base_field follow q_mul_lsb; fixed_z is the fixed column after the ten the circuit created (the table's, the eight
    Lagrange columns, the constants); advices 4
    (already equality-enabled by the hi half) and 5 are enabled"""
    cs, _, _ = ec.front.synthesize(MulFixedCircuit([], fx.host_tables()).without_witnesses(), K, ec.FP, fixed=True, advice=False)
    assert [g.name for g in cs.gates] == ["Short lookup bitshift"] + ec.GATE_NAMES + fx.GATE_NAMES_FIXED
    assert [c.index for c in cs.permutation_columns if c.kind == "advice"] == [9, 0, 1, 2, 3, 4, 6, 8, 7, 5]
    config = fx.configure_fixed(ec.front.ConstraintSystem(P))
    assert config.mul.q_mul_lsb.index == 15
    assert [config.mul_fixed.running_sum_config.q_range_check.index, config.mul_fixed_full.q_mul_fixed_full.index,
            config.mul_fixed_short.q_mul_fixed_short.index, config.mul_fixed_base_field.q_mul_fixed_base_field.index] == [16, 17, 18, 19]
    assert config.mul_fixed_base_field.canon_advices == config.advices[6:9]
    assert [c.index for c in config.lagrange_coeffs] == list(range(1, 9)) and config.mul_fixed.fixed_z.index == 10
    assert (config.mul_fixed.window, config.mul_fixed.u) == (config.advices[4], config.advices[5])
    names = [n for g in cs.gates[-4:] for n in g.constraint_names]
    assert names == ["check x", "check y", "on-curve"] * 2 + [
        "window range check", "last_window_check", "sign_check", "y_check", "negation_check", "MSB = 1 => alpha_1 = 0",
        "MSB = 1 => alpha_0_hi_120 = 0", "MSB = 1 => a_43 = 0 or 1", "MSB = 1 => z_13_alpha_0_prime = 0", "alpha_1_range_check",
        "alpha_2_range_check", "z_84_alpha_check", "alpha_0_prime check"]


def test_configure_without_fixed_bases_creates_nothing_more():
    config = ec.configure_ecc_chip(ec.front.ConstraintSystem(P))
    assert config.mul_fixed is None and config.mul_fixed_full is None and config.mul_fixed_short is None and config.fixed_bases is None


# ---- 3: mul_fixed, cell by cell --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mul_run():
    circuit = MulFixedCircuit(fx.EDGE_SCALARS + RANDOM[:1], fx.host_tables())
    failures, names, assembly, layouter, _ = ec.host_model(circuit, K)
    return circuit, failures, names, assembly, layouter


def test_mul_fixed_satisfies_every_constraint(mul_run):
    circuit, failures, names, _, _ = mul_run
    assert len(circuit.products) == 7 and _named(failures, names) == []


def test_mul_fixed_cells_are_the_restatements(mul_run):
    circuit, _, _, assembly, layouter = mul_run
    advice = assembly.host_columns(assembly.advice)
    fixed = assembly.host_columns(assembly.fixed)
    table, coeffs, zs, us = fx.generator_tables()
    for k, (product, scalar) in zip(circuit.scalars, circuit.products):
        cols, aux, result = fx.mul_fixed_trace(table, us, k)
        start = layouter.regions[scalar.windows[0].cell().region_index]
        assert [advice[c][start:start + NUM_WINDOWS] for c in range(6)] == cols
        assert [[fixed[c][start + w] for c in range(1, 9)] for w in range(NUM_WINDOWS)] == coeffs
        assert fixed[10][start:start + NUM_WINDOWS] == zs
        add_at = layouter.regions[product.inner().x().cell().region_index]
        assert [advice[c][add_at] for c in range(9)] == aux[:9] and [advice[2][add_at + 1], advice[3][add_at + 1]] == aux[9:]
        assert (product.inner().x().value().inner.evaluate(P), product.inner().y().value().inner.evaluate(P)) == result


@pytest.mark.parametrize("what, constraints", [("window", {"check x", "window range check"}), ("u", {"check y"})])
def test_a_mutated_cell_is_named(what, constraints):
    """window 40 of 2^255 - 1 is 7: 8 leaves the range and the interpolation, and nothing else reads it; a u off by one is no root"""
    circuit = MulFixedCircuit([(1 << 255) - 1], fx.host_tables(), mutate=(0, what))
    failures, names, _, _, _ = ec.host_model(circuit, K)
    named = _named(failures, names)
    assert named and all(f[0] == "ConstraintNotSatisfied" and f[1] == "Full-width fixed-base scalar mul" and f[3] == circuit.mutated_row
                         for f in named), named
    assert constraints == {f[2] for f in named}


def test_a_scalar_of_256_bits_is_refused():
    with pytest.raises(ValueError):
        ec.front.synthesize(MulFixedCircuit([1 << 255], fx.host_tables()), K, ec.FP, fixed=True, advice=True, instances=[])


# ---- 4: the short signed form and mul_sign ---------------------------------------------------------------------------------------------------
SHORT_PAIRS = [(m, s) for m in (0, 1, (1 << 64) - 1, 0x1234_5678_9abc_def0) for s in (1, P - 1)]


def _value(point):
    return (point.inner().x().value().inner.evaluate(P), point.inner().y().value().inner.evaluate(P))


def test_mul_fixed_short_and_mul_sign_satisfy_every_constraint():
    """short.rs tests: magnitudes 0, 1, 2^64 - 1 and a random one with both signs; mul_sign of a point, and of the identity, by both"""
    pt = ec.random_bases(1, seed=50)[0]
    signed = [(pt, 1), (pt, P - 1), ((0, 0), 1), ((0, 0), P - 1)]
    circuit = ShortCircuit(SHORT_PAIRS, fx.host_tables(NUM_WINDOWS_SHORT), signed)
    failures, names, _, _, _ = ec.host_model(circuit, K)
    assert _named(failures, names) == []
    assert [_value(p) for p in circuit.products] == [ec.ec_mul(m if s == 1 else -m, GENERATOR) for m, s in SHORT_PAIRS]
    assert [_value(p) for p in circuit.signed_points] == [pt, (pt[0], -pt[1] % P), (0, 0), (0, 0)]


@pytest.mark.parametrize("pair, constraints", [(((1 << 64), 1), {"last_window_check"}), ((1, 2), {"sign_check", "negation_check"})],
                         ids=["magnitude 2^64", "sign 2"])
def test_an_invalid_magnitude_or_sign_fails_where_the_reference_says(pair, constraints):
    """short.rs tests::invalid_magnitude_sign: 2^64 leaves z_21 = 2, no bit, and z_22 = 1/4 against its constant zero (a broken copy);
    a sign of 2 fails sign_check and, y_p being witnessed as y_a, negation_check"""
    circuit = ShortCircuit([pair], fx.host_tables(NUM_WINDOWS_SHORT))
    failures, names, _, _, _ = ec.host_model(circuit, K)
    named = _named(failures, names)
    gate = {f[2] for f in named if f[0] == "ConstraintNotSatisfied" and f[1] == "Short fixed-base mul gate"}
    assert gate == constraints and all(f[0] == "Permutation" or f[1] == "Short fixed-base mul gate" for f in named), named
    assert any(f[0] == "Permutation" for f in named) == (pair[0] == 1 << 64)


# ---- 5: the base-field form --------------------------------------------------------------------------------------------------------------------
def test_mul_fixed_base_field_elem_satisfies_every_constraint():
    circuit = BaseFieldCircuit(fx.EDGE_BASE_FIELD, fx.host_tables())
    failures, names, _, _, _ = ec.host_model(circuit, K)
    assert _named(failures, names) == []
    assert [_value(p) for p in circuit.products] == [ec.ec_mul(a, GENERATOR) for a in fx.EDGE_BASE_FIELD]


def test_a_mutated_canonicity_cell_is_named():
    """alpha = 2^254: alpha_1 = 0 under a set top bit; 1 in its place breaks the implication and the recomposition of z_84"""
    circuit = BaseFieldCircuit([1 << 254], fx.host_tables(), mutate=0)
    failures, names, _, _, _ = ec.host_model(circuit, K)
    named = _named(failures, names)
    assert named and all(f[0] == "ConstraintNotSatisfied" and f[1] == "Canonicity checks" and f[3] == circuit.mutated_row for f in named), named
    assert {f[2] for f in named} == {"MSB = 1 => alpha_1 = 0", "z_84_alpha_check"}


# ---- 6: the bulk path's shape (its advice needs the device: tests/test_gpu_ecc_fixed_circuit.py) ------------------------------------------------
def test_mul_fixed_many_lays_out_the_fixed_cells_of_mul_fixed():
    """keygen's view, no witness: the tables' fixed columns and every selector of the bulk region and of the bulk additions are those
    of three calls of `mul_fixed`, region by region"""
    sides = []
    for many in (False, True):
        circuit = MulFixedCircuit(fx.EDGE_SCALARS[:3], fx.host_tables(), many=many).without_witnesses()
        _, assembly, layouter = ec.front.synthesize(circuit, K, ec.FP, fixed=True, advice=False)
        sides.append((circuit, assembly.host_columns(assembly.fixed), assembly.selectors, layouter))
    (_, fa, sa, la), (bulk, fb, sb, lb) = sides
    nw = NUM_WINDOWS
    start, add_start = lb.regions[bulk.bulk.region_index], lb.regions[bulk.bulk.add_region_index]
    assert len(la.regions) == 6 and len(lb.regions) == 2
    for i in range(3):
        at, add_at = la.regions[2 * i], la.regions[2 * i + 1]
        for c in range(1, len(fa)):                                           # fixed column 0 is the range check's table
            assert fb[c][start + nw * i:start + nw * (i + 1)] == fa[c][at:at + nw], (i, c)
        assert (sb[:, start + nw * i:start + nw * (i + 1)] == sa[:, at:at + nw]).all()
        assert (sb[:, add_start + 2 * i:add_start + 2 * i + 2] == sa[:, add_at:add_at + 2]).all()


# ---- 7: the reference's test circuit ---------------------------------------------------------------------------------------------------------------
def test_the_mirror_of_the_references_circuit_has_its_constraint_system():
    """tests/golden/vk_ecc_chip.rdata.gz, the `cs:` section: after the selectors of the synthesized mirror are compressed, every gate,
    query, lookup and column of the reference's pinned key, text for text (the commitments need the device:
    tests/test_gpu_ecc_fixed_circuit.py)"""
    import numpy as np

    import sinsemilla_cases as sc
    circuit = fx.MyEccCircuit(fx.host_tables(NUM_WINDOWS), fx.host_tables(NUM_WINDOWS_SHORT)).without_witnesses()
    cs, assembly, layouter = ec.front.synthesize(circuit, K, ec.FP, fixed=True, advice=False)
    sel = assembly.selectors.astype(np.int64)
    conflicts = (sel @ sel.T) > 0
    np.fill_diagonal(conflicts, False)
    cs.compress_selectors(conflicts)
    assert cs.pinned() == sc.fixture_cs(sc.fixture_text("vk_ecc_chip.rdata.gz"))
    assert len(layouter.regions) == 138


def test_the_mirror_of_the_references_circuit_is_satisfied():
    circuit = fx.MyEccCircuit(fx.host_tables(NUM_WINDOWS), fx.host_tables(NUM_WINDOWS_SHORT), seed=3)
    failures, names, _, _, _ = ec.host_model(circuit, K)
    assert _named(failures, names) == []
