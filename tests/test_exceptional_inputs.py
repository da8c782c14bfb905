"""The input families of tests/exceptional_points.py against the C oracle (whose jac_add / jac_add_mixed are complete), and the property each
construction claims.  CPU only: the device runs of the same families are tests/test_gpu_exceptional_additions.py."""
import numpy as np
import pytest

import exceptional_points as xp
from halo2_amd import fields
from oracle import c_oracle as co
from oracle import pasta as o

CURVES = [0, 1]


def oracle_msm(inp, n=None):
    n = inp.n if n is None else n
    return co.jac_to_affine_ints(inp.curve, co.best_multiexp(inp.curve, inp.scalars[:n], inp.bases[:n]))


def families(curve, n):
    return [xp.palette(curve, n, 11 + curve), xp.heavy(curve, n, 12 + curve), xp.cancelling(curve, n, 13 + curve),
            xp.cancelling(curve, n, 14 + curve, shuffle=False),
            xp.uniform_buckets(curve, n, 10, 15 + curve), xp.uniform_buckets(curve, n, 8, 16 + curve, "alternating"),
            xp.uniform_buckets(curve, n, 10, 17 + curve, phi=True)]


@pytest.mark.parametrize("curve", CURVES)
def test_multiples_table(curve):
    m = o.CURVES[curve][0]
    t = xp.multiples(curve)
    assert co.affine_to_ints(curve, t[xp.CMAX]) is None
    for c in (-16, -1, 1, 2, 7, 16):
        p = co.affine_to_ints(curve, t[c + xp.CMAX])
        assert o.on_curve(p, m) and p == o.ec_mul(c % o.CURVES[curve][1], xp.generator(curve), m)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [1, 7, 600, 4096])
def test_closed_form_matches_the_oracle(curve, n):
    for inp in families(curve, n):
        assert inp.want() == oracle_msm(inp), (inp.name, n)
        if inp.name == "cancelling":
            assert inp.want() is None, n                         # the leftover rows carry scalar 0


@pytest.mark.parametrize("curve", CURVES)
def test_cancelling_groups_sum_to_the_identity(curve):
    sm = o.CURVES[curve][1]
    sf = fields.CURVE_FIELDS[curve][1]
    inp = xp.cancelling(curve, 7 * 300, 21 + curve, shuffle=False)
    c = inp.coeffs.reshape(-1, xp.GROUP)
    s = np.array(fields.from_limbs(inp.scalars, sf), dtype=object).reshape(-1, xp.GROUP)
    assert (c[:, 0] + c[:, 1] + c[:, 2] == 0).all() and (c[:, 3] + c[:, 4] == 0).all() and (c[:, 5] == c[:, 6]).all()
    assert all(s[g, 0] == s[g, 1] == s[g, 2] and s[g, 3] == s[g, 4] and (s[g, 5] + s[g, 6]) % sm == 0 for g in range(c.shape[0]))
    assert inp.want() is None and oracle_msm(inp) is None
    shuffled = xp.cancelling(curve, 7 * 300 + 3, 22 + curve)
    assert shuffled.want(7 * 300 + 3) == oracle_msm(shuffled)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("w,sign", [(8, "same"), (10, "alternating"), (13, "same")])
def test_uniform_buckets_sum_to_p(curve, w, sign):
    n = 1 << 12
    inp = xp.uniform_buckets(curve, n, w, 31 + curve, sign)
    used = min(n, 2 * ((1 << (w - 1)) - 1))
    sums = {}
    for b, c in zip(inp.bucket_of[:used], inp.coeffs[:used]):
        if b:
            sums[int(b)] = sums.get(int(b), 0) + int(c)
    assert sums and all(v == (5 if sign == "same" or j % 2 == 0 else -5) for j, v in sums.items()), sums
    assert len(sums) == min((1 << (w - 1)) - 1, used // 2)
    assert inp.want() == oracle_msm(inp)


@pytest.mark.parametrize("curve", CURVES)
def test_uniform_bucket_scalars_under_the_endomorphism_split(curve):
    """glv_split (the header's constants) of the scalars uniform_buckets uses: j < 2^15 splits as (j, 0), so the buckets of the plain
    variant are exactly the digits j; j lambda splits as (C1, C2 + j - 1) with (C1, C2) the split of lambda, so the phi variant's
    per-bucket digits sit in the phi half and its k1 half is one constant"""
    sm = o.CURVES[curve][1]
    lam = xp.LAMBDA[curve]
    c1, c2 = xp.glv_split(curve, lam)
    assert abs(c1) < 1 << 129 and abs(c2) < 1 << 129 and (c1 + c2 * lam - lam) % sm == 0
    inp = xp.uniform_buckets(curve, 1 << 16, 16, 51 + curve, phi=True)
    used = sorted({int(j) for j in inp.bucket_of if j})
    assert used[0] == 1 and used[-1] == (1 << 15) - 1
    sf = fields.CURVE_FIELDS[curve][1]
    phi_scalars = set(fields.from_limbs(inp.scalars[:inp.bucket_of.size][inp.bucket_of != 0], sf))
    assert phi_scalars == {j * lam % sm for j in used}
    for j in used:
        assert xp.glv_split(curve, j) == (j, 0), j
        assert xp.glv_split(curve, j * lam % sm) == (c1, c2 + j - 1), j


@pytest.mark.parametrize("curve", CURVES)
def test_cancelling_blind_commits_to_the_identity(curve):
    sf = fields.CURVE_FIELDS[curve][1]
    n = 1024
    inp = xp.palette(curve, n, 41 + curve)
    c_w = -3
    w = xp.point(curve, c_w)
    blind = xp.cancelling_blind(curve, inp, c_w)
    out = co.commit(curve, inp.bases, w, inp.scalars, fields.scalar_limbs(blind, sf, True))
    assert co.jac_to_affine_ints(curve, out) is None and inp.want(blind=blind, c_w=c_w) is None
    other = 123456789
    out = co.commit(curve, inp.bases, w, inp.scalars, fields.scalar_limbs(other, sf, True))
    assert co.jac_to_affine_ints(curve, out) == inp.want(blind=other, c_w=c_w)
