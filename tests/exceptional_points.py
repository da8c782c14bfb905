"""Multiexp inputs whose answers are known in closed form and that drive the point additions into their exceptional branches: P + P,
P - P and the identity.  Shared by tests/test_exceptional_inputs.py (the constructions against the C oracle) and
tests/test_gpu_exceptional_additions.py (every device entry point against the closed form).

Every base is c G for the oracle's generator G = (-1, 2) and a small integer c (0: the identity), so a multiexp, a commit or an opening has
the answer (sum_i s_i c_i + blind c_w mod q) G: one inner product over the scalar field and one scalar multiplication, O(n) whatever n is.
Random bases (co.generate_bases) meet two equal or opposite points in a bucket, a fold or a chain with probability about 2^-250; these
inputs meet them all the time:

  palette           c_i in [-8, 8]: bucket partial sums are small multiples of G (and of phi(G)), equal and opposite operands everywhere
  cancelling        triples (A, B, -(A + B)) and pairs (P, -P) under one scalar, and (s, P) with (q - s, P): the sum is the identity,
                    and in any order the last addition is X + (-X) against a projective accumulator
  uniform buckets   scalars below 2^(w-1) (one window of w bits, k2 = 0 in the endomorphism split): bucket j holds points that sum to
                    the same P (one base, or a pair X_j, P - X_j), or to +-P alternating, so the fold adds equal projective points that
                    arrived by different routes; the `phi` variant takes the scalars j lambda, which the split turns into
                    k1 = one constant and k2 = a constant + j - 1: the per-bucket digits move into the phi half (shifted by that
                    constant) and the k1 half becomes one heavy bucket per window
  heavy             one scalar for every palette base: a single heavy bucket per window
  cancelling blind  a palette column with blind = -sum_i s_i c_i / c_w: the commitment is exactly the identity
"""
from __future__ import annotations

import functools

import numpy as np

from glv_edge_scalars import LAMBDA
from halo2_amd import fields
from oracle import c_oracle as co
from oracle import pasta as o

CMAX = 16                                                  # |c| of every base below


def generator(curve):
    return (o.CURVES[curve][0] - 1, 2)


_tables = {}


def multiples(curve, cmax=CMAX):
    """(2 cmax + 1, 8) Montgomery affine limbs: row c + cmax is c G (row cmax is the identity, all zeros)."""
    if (curve, cmax) not in _tables:
        m = o.CURVES[curve][0]
        g = generator(curve)
        pts = [o.ec_mul(abs(c), g, m) if c >= 0 else o.ec_neg(o.ec_mul(-c, g, m), m) for c in range(-cmax, cmax + 1)]
        _tables[curve, cmax] = co.points_to_mont(curve, pts)
    return _tables[curve, cmax]


def point(curve, c):
    """c G as Montgomery affine limbs (8,)"""
    m = o.CURVES[curve][0]
    p = o.ec_mul(c % o.CURVES[curve][1], generator(curve), m)
    return co.points_to_mont(curve, [p])[0]


def closed_form_scalar(curve, scalars, coeffs, blind=0, c_w=0):
    """(sum_i s_i c_i + blind c_w) mod q for Montgomery scalars (n, 4) and small integer coefficients (numpy ints)"""
    sf, sm = fields.CURVE_FIELDS[curve][1], o.CURVES[curve][1]
    coeffs = np.asarray(coeffs, dtype=np.int64)
    k = 0
    if coeffs.size:
        lo = int(coeffs.min())
        row = fields.to_limbs([c % sm for c in range(lo, int(coeffs.max()) + 1)], sf, True)
        k = fields.from_limbs(co.inner_product(sf, np.ascontiguousarray(scalars), np.ascontiguousarray(row[coeffs - lo])), sf)[0]
    return (k + blind * c_w) % sm


def closed_form(curve, scalars, coeffs, blind=0, c_w=0):
    """the canonical affine (x, y) of the answer, or None for the identity (co.jac_to_affine_ints' convention)"""
    k = closed_form_scalar(curve, scalars, coeffs, blind, c_w)
    return o.ec_mul(k, generator(curve), o.CURVES[curve][0])


class Inputs:
    """scalars (n, 4) and bases (n, 8), Montgomery limbs; coeffs: the c_i of the bases; the answer in closed form"""

    def __init__(self, curve, name, scalars, coeffs, cmax=CMAX):
        self.curve, self.name = curve, name
        self.scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
        self.coeffs = np.asarray(coeffs, dtype=np.int64)
        assert int(np.abs(self.coeffs).max(initial=0)) <= cmax
        self.bases = np.ascontiguousarray(multiples(curve, cmax)[self.coeffs + cmax])
        self._want = {}

    @property
    def n(self):
        return self.scalars.shape[0]

    def want(self, n=None, blind=0, c_w=0):
        n = self.n if n is None else n
        if (n, blind, c_w) not in self._want:
            self._want[n, blind, c_w] = closed_form(self.curve, self.scalars[:n], self.coeffs[:n], blind, c_w)
        return self._want[n, blind, c_w]


def _sf(curve):
    return fields.CURVE_FIELDS[curve][1]


def _neg(curve, s):
    """-s for Montgomery scalars (n, 4)"""
    sf = _sf(curve)
    return co.scale_add(sf, s, fields.scalar_limbs(o.CURVES[curve][1] - 1, sf, True), np.zeros_like(s))      # s (-1) + 0


def palette(curve, n, seed):
    rng = np.random.default_rng(seed)
    return Inputs(curve, "palette", co.random_field(_sf(curve), seed, n), rng.integers(-8, 9, n))


def heavy(curve, n, seed):
    """one random scalar for every base; palette bases"""
    rng = np.random.default_rng(seed)
    s = np.ascontiguousarray(np.repeat(co.random_field(_sf(curve), seed, 1), n, axis=0))
    return Inputs(curve, "heavy", s, rng.integers(-8, 9, n))


# one group of the cancelling family: (A, B, -(A + B)) under s0, (C, -C) under s1, (D, D) under s2 and q - s2 -- seven bases
GROUP = 7


def cancelling(curve, n, seed, shuffle=True):
    """groups that each sum to the identity; the n % 7 leftover rows take scalar 0.  shuffle: the rows in a random order"""
    rng = np.random.default_rng(seed)
    g = n // GROUP
    a, b = rng.integers(-8, 9, g), rng.integers(-8, 9, g)
    c, d = rng.integers(-8, 9, g), rng.integers(-8, 9, g)
    coeffs = np.zeros(n, dtype=np.int64)
    coeffs[:g * GROUP] = np.stack([a, b, -(a + b), c, -c, d, d], axis=1).reshape(-1)
    coeffs[g * GROUP:] = rng.integers(-8, 9, n - g * GROUP)
    s3 = co.random_field(_sf(curve), seed, 3 * g).reshape(g, 3, 4)
    sc = np.zeros((n, 4), dtype=np.uint64)
    grp = sc[:g * GROUP].reshape(g, GROUP, 4)
    grp[:, 0:3] = s3[:, 0:1]
    grp[:, 3:5] = s3[:, 1:2]
    grp[:, 5] = s3[:, 2]
    grp[:, 6] = _neg(curve, np.ascontiguousarray(s3[:, 2]))
    if shuffle:
        perm = rng.permutation(n)
        sc, coeffs = sc[perm], coeffs[perm]
    return Inputs(curve, "cancelling", sc, coeffs)


def uniform_buckets(curve, n, w, seed, sign="same", phi=False):
    """scalars j in [1, 2^(w-1)) (one digit of a w-bit window, no carry); bucket j sums to P = 5 G (sign "same") or to (-1)^j P
    ("alternating"): a bucket j = 0 mod 3 holds P alone, every other one a pair (X_j, P - X_j).  Rows past the 2 (2^(w-1) - 1) that fill
    the buckets take scalar 0.  phi: scalars j lambda (see glv_split for where their digits land)."""
    rng = np.random.default_rng(seed)
    sm = o.CURVES[curve][1]
    nb = (1 << (w - 1)) - 1
    used = min(n, 2 * nb)
    j = 1 + np.arange(used) // 2                                # bucket of each used row
    second = (np.arange(used) % 2) == 1
    pc = 5 * (np.where(j % 2 == 1, -1, 1) if sign == "alternating" else np.ones(used, dtype=np.int64))
    x = rng.integers(-8, 9, nb + 1)[j]                          # X_j, one per bucket
    alone = j % 3 == 0
    coeffs = np.zeros(n, dtype=np.int64)
    coeffs[:used] = np.where(alone, np.where(second, x, pc), np.where(second, pc - x, x))
    coeffs[used:] = rng.integers(-8, 9, n - used)
    svals = np.where(alone & second, 0, j)                      # the partner row of a lone P carries nothing
    sval_list = [int(v) * (LAMBDA[curve] if phi else 1) % sm for v in range(nb + 1)]
    table = fields.to_limbs(sval_list, _sf(curve), True)
    sc = np.zeros((n, 4), dtype=np.uint64)
    sc[:used] = table[svals]
    inp = Inputs(curve, f"uniform buckets w={w} {sign}{' phi' if phi else ''}", sc, coeffs)
    inp.bucket_of, inp.bucket_sum = svals, pc                   # for the construction check
    return inp


def cancelling_blind(curve, inp, c_w=-3):
    """the blind that makes `inp`'s commitment with blind base c_w G exactly the identity"""
    sm = o.CURVES[curve][1]
    k = closed_form_scalar(curve, inp.scalars, inp.coeffs)
    return (-k * pow(c_w, -1, sm)) % sm


@functools.lru_cache(maxsize=None)
def _glv_constants(curve):
    from test_glv_constants import _array
    return tuple(_array(name, curve == 0) for name in ("a1", "b1", "a2", "b2", "g1", "g2"))       # Pallas scalars: FS == FQ


def glv_split(curve, k):
    """(k1, k2) of csrc/glv.cuh's glv_split for the canonical scalar k of `curve`, from the constants the header ships (parsed by
    tests/test_glv_constants.py): c_i = (k g_i) >> 256, k1 = k - c1 a1 - c2 a2, k2 = c1 |b1| - c2 b2"""
    a1, b1m, a2, b2, g1, g2 = _glv_constants(curve)
    c1, c2 = (k * g1) >> 256, (k * g2) >> 256
    return k - c1 * a1 - c2 * a2, c1 * b1m - c2 * b2
