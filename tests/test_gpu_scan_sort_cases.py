"""The scan, reduction and sort kernels (halo2_amd/csrc/poly.hip, lookup.hip, through the C ABI) on the structured case list of
tests/scan_sort_cases.py: every launch kind of the bitonic sort on sorted, reversed, constant, two-valued and limb-by-limb inputs, both trip
counts of lk_scan_totals' chunk loop, the carry kernels at per = 1, 2, 3, zeros that empty a lane, a group or a tile of the batched inversion,
and the scalars 0, 1, p - 1.  Every output is compared bit for bit with the oracle (Python `sorted`, the numpy restatement of the reference's
walk, oracle/h2_oracle.c, Python integers), never with another device result.  tests/test_scan_sort_case_coverage.py proves on the CPU what
the list reaches.  Runs only on a real MI355X (`-m gpu`)."""
import numpy as np
import pytest
import torch

import halo2_amd as h
from halo2_amd import fields
from halo2_amd._lib import ConstraintSystemFailure
from halo2_amd.arithmetic import assigned_to_field, permute_expression_pair, sort_field
from oracle import c_oracle as co

import scan_sort_cases as sc

pytestmark = pytest.mark.gpu

FORMS = {sc.CANONICAL: h.FORM_CANONICAL, sc.MONTGOMERY: h.FORM_MONTGOMERY}
POISON = np.full((6, 4), 0xDEADBEEFDEADBEEF, dtype=np.uint64)          # not a field element: rows past `usable` are never read


def _up(limbs):
    return torch.from_numpy(np.ascontiguousarray(limbs, dtype=np.uint64).view(np.int64)).cuda()


def _dn(t):
    return t.cpu().numpy().view(np.uint64)


def _scalar(name, field):
    return fields.scalar_limbs(sc.scalar_value(name, field), field, True)


# ---- h2_sort_device --------------------------------------------------------------------------------------------------------------------
SORT_RUNS = {}
for _n, _pattern, _form, _field in sc.sort_cases():
    SORT_RUNS.setdefault((_n, _pattern), []).append((_form, _field))


@pytest.mark.parametrize("n,pattern", sorted(SORT_RUNS))
def test_sort_of_a_structured_input_is_python_sorted(n, pattern):
    for form, field in SORT_RUNS[(n, pattern)]:
        vals = sc.sort_values(n, pattern, field)
        t = _up(fields.to_limbs(vals, field, form == sc.MONTGOMERY))
        sort_field(t, field, FORMS[form])
        assert np.array_equal(_dn(t), fields.to_limbs(sorted(vals), field, form == sc.MONTGOMERY)), (form, field)


def test_sort_with_a_stride_of_2_20_keys():
    keys, want = sc.sort_large_limbs()
    assert ("global2", 21, 20) in sc.sort_schedule(len(keys))
    t = _up(keys)
    sort_field(t, h.FP, h.FORM_CANONICAL)
    assert np.array_equal(_dn(t), want)


# ---- h2_permute_expression_pair_device -------------------------------------------------------------------------------------------------
def _column_limbs(col, field, form, big):
    if big:
        assert form == sc.CANONICAL
        return sc.limbs_of_u64(col)
    return fields.to_limbs([int(v) for v in col], field, form == sc.MONTGOMERY)


def _runs(big):
    return [(h.FP, sc.CANONICAL)] if big else [(field, form) for field in (h.FP, h.FQ) for form in (sc.CANONICAL, sc.MONTGOMERY)]


def _permute_and_check(n, shape, field, form, big):
    a, t = sc.permute_columns(n, shape, field, big)
    want = sc.permute_model(a, t)
    assert want is not None
    in_limbs = np.concatenate([_column_limbs(a, field, form, big), POISON])
    tb_limbs = np.concatenate([_column_limbs(t, field, form, big), POISON[::-1]])
    d_in, d_tb = _up(in_limbs), _up(tb_limbs)
    got_a, got_s = permute_expression_pair(d_in, d_tb, n, field, FORMS[form])
    assert np.array_equal(_dn(got_a), _column_limbs(want[0], field, form, big)), ("A'", field, form)
    assert np.array_equal(_dn(got_s), _column_limbs(want[1], field, form, big)), ("S'", field, form)
    assert np.array_equal(_dn(d_in), in_limbs) and np.array_equal(_dn(d_tb), tb_limbs)        # the input columns are unchanged


@pytest.mark.parametrize("n,shape,big", sc.permute_cases())
def test_permute_expression_pair_on_a_structured_multiset(n, shape, big):
    for field, form in _runs(big):
        _permute_and_check(n, shape, field, form, big)


@pytest.mark.parametrize("n,shape,big", sc.permute_failure_cases())
def test_a_missing_value_is_a_constraint_system_failure_and_the_next_call_is_correct(n, shape, big):
    for field, form in _runs(big):
        a, t = sc.permute_columns(n, shape, field, big)
        assert sc.permute_model(a, t) is None
        d_in = _up(np.concatenate([_column_limbs(a, field, form, big), POISON]))
        d_tb = _up(np.concatenate([_column_limbs(t, field, form, big), POISON]))
        with pytest.raises(ConstraintSystemFailure):
            permute_expression_pair(d_in, d_tb, n, field, FORMS[form])
        _permute_and_check(1025, "input_is_table", field, form, False)


# ---- eval_polynomial, powers, compute_inner_product, scale_add ------------------------------------------------------------------------
@pytest.mark.parametrize("field", [h.FP, h.FQ])
@pytest.mark.parametrize("n", sc.POLY_LENGTHS)
def test_eval_powers_and_inner_product_at_the_extreme_points(field, n):
    assert {x for m, x in sc.eval_cases() if m == n} == set(sc.SCALARS)
    a, b = co.random_field(field, 1100 + n % 97, n), co.random_field(field, 1200 + n % 97, n)
    assert np.array_equal(h.compute_inner_product(a, b, field), co.inner_product(field, a, b))
    holes = a.copy()
    holes[::3] = 0
    assert np.array_equal(h.compute_inner_product(holes, b, field), co.inner_product(field, holes, b))
    for name in sc.SCALARS:
        x = _scalar(name, field)
        assert np.array_equal(h.eval_polynomial(a, x, field), co.eval_polynomial(field, a, x)), name
        assert np.array_equal(h.powers(x, n, field), co.powers(field, x, n)), name
        assert np.array_equal(h.compute_inner_product(a, co.powers(field, x, n), field), co.eval_polynomial(field, a, x)), name
        assert np.array_equal(h.scale_add(a, x, b, field), co.scale_add(field, a, x, b)), name


# ---- kate_division ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [h.FP, h.FQ])
@pytest.mark.parametrize("n", [n for n in sc.POLY_LENGTHS if n >= 2])
def test_kate_division_at_the_extreme_points_and_of_an_exact_multiple(field, n):
    m = fields.MODULUS[field]
    zero = np.zeros((1, 4), dtype=np.uint64)
    for name, kind in sorted({(b, k) for length, b, k in sc.kate_cases() if length == n}):
        b = _scalar(name, field)
        if kind == "random":
            a = co.random_field(field, 2100 + n % 97, n)
        else:                                                            # a = (X - b) q:  a_i = q_(i-1) - b q_i
            q = co.random_field(field, 2200 + n % 97, n - 1)
            minus_b = fields.scalar_limbs((m - sc.scalar_value(name, field)) % m, field, True)
            a = co.scale_add(field, np.concatenate([q, zero]), minus_b, np.concatenate([zero, q]))
        got = h.kate_division(a, b, field)
        assert np.array_equal(got, co.kate_division(field, a, b)), (name, kind)
        if kind == "multiple":
            assert np.array_equal(got, q), name


# ---- grand_product ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [h.FP, h.FQ])
@pytest.mark.parametrize("n", sc.PRODUCT_LENGTHS)
def test_grand_product_from_every_init_and_through_a_zero_factor(field, n):
    for init_name, where in [(i, w) for length, i, w in sc.product_cases() if length == n]:
        factors = co.random_field(field, 3100 + n % 97, n)               # the last one belongs to no z
        at = sc.zero_factor_index(where, n)
        if at is not None:
            factors[at] = 0
        init = _scalar(init_name, field)
        want = co.grand_product(field, factors, n, init)
        assert np.array_equal(h.grand_product(factors, n, init, field), want), (init_name, where)
        if at is not None and init_name != "zero":
            assert want[at].any() and not want[at + 1:].any()           # the case is what it says: zero from the factor on


@pytest.mark.parametrize("field", [h.FP, h.FQ])
@pytest.mark.parametrize("n", sc.POISON_LENGTHS)
def test_grand_product_ignores_the_factor_past_the_last(field, n):
    factors = co.random_field(field, 3200 + n, n)
    init = _scalar("full", field)
    want = co.grand_product(field, factors, n, init)
    factors[n - 1] = POISON[0]
    assert np.array_equal(_dn(h.grand_product(_up(factors), n, init, field)), want)
    can = lambda v: co.from_mont(field, v)
    poisoned = can(factors)
    poisoned[n - 1] = POISON[0]
    assert np.array_equal(_dn(h.grand_product(_up(poisoned), n, can(init), field, h.FORM_CANONICAL)), can(want))


# ---- batch_invert ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [h.FP, h.FQ])
@pytest.mark.parametrize("n,name", sc.invert_cases())
def test_batch_invert_with_zeros_placed(field, n, name):
    a = co.random_field(field, 4100 + n % 97, n)
    at = sc.placement(name, n)
    a[at] = 0
    want = co.batch_invert(field, a)
    assert not want[at].any() and (len(at) == n or want.any())
    assert np.array_equal(h.batch_invert(a, field), want)                                    # host arrays: a copy
    d = _up(a)
    assert h.batch_invert(d, field) is d and np.array_equal(_dn(d), want)                    # device tensor: in place
    can = co.from_mont(field, a)
    assert np.array_equal(h.batch_invert(can, field, h.FORM_CANONICAL), co.from_mont(field, want))
    d = _up(can)
    h.batch_invert(d, field, h.FORM_CANONICAL)
    assert np.array_equal(_dn(d), co.from_mont(field, want))


# ---- assigned_to_field -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [h.FP, h.FQ])
@pytest.mark.parametrize("n,name,fill", sc.assigned_cases())
def test_assigned_to_field_with_trivial_denominators_placed(field, n, name, fill):
    m = fields.MODULUS[field]
    num = fields.from_limbs(co.random_field(field, 5100 + n % 97, n), field, True)
    den = fields.from_limbs(co.random_field(field, 5200 + n % 97, n), field, True)
    idx, vals = sc.overlay_mask(n, name, fill)
    for i, v in zip(idx.tolist(), vals.tolist()):
        den[i] = v
    want = [a * pow(d, -1, m) % m if d else 0 for a, d in zip(num, den)]
    for form, mont in ((h.FORM_MONTGOMERY, True), (h.FORM_CANONICAL, False)):
        num_l, den_l, want_l = (fields.to_limbs(v, field, mont) for v in (num, den, want))
        d_num, d_den = _up(num_l), _up(den_l)
        out = torch.full_like(d_num, -1)
        assert assigned_to_field(d_num, d_den, field, form, out=out) is out                  # out=
        assert np.array_equal(_dn(out), want_l), (form, "out=")
        assert np.array_equal(_dn(d_num), num_l) and np.array_equal(_dn(d_den), den_l)
        assert assigned_to_field(d_num, d_den, field, form) is d_num                         # in place on the numerators
        assert np.array_equal(_dn(d_num), want_l), (form, "in place")
        assert np.array_equal(assigned_to_field(num_l, den_l, field, form), want_l), (form, "host")
