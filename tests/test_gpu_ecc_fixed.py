"""Fixed-base multiplication on the device: the kernels of halo2_amd/csrc/ecc_fixed.hip against `oracle.pasta.ec_mul` and the restated
tables and witness of tests/ecc_fixed_cases.py.  Every comparison is bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

from halo2_amd import ecc, fields
from halo2_amd._lib import NotFound, lib

import ecc_cases as ec
import ecc_fixed_cases as fx
from ecc_fixed_cases import GENERATOR, NUM_WINDOWS, NUM_WINDOWS_SHORT, P

pytestmark = pytest.mark.gpu
FP = 0
OK, ERR_ARGS, ERR_NOTFOUND = 0, 1, 8


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(fields.current_device())


def _ints(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else t
    return fields.from_limbs(np.ascontiguousarray(a).view(np.uint64).reshape(-1, 4), FP, True)


def _points(t):
    v = _ints(t)
    return [(v[i], v[i + 1]) for i in range(0, len(v), 2)]


def _limbs(pt):
    return fields.to_limbs(list(pt), FP).reshape(8)


@functools.lru_cache(maxsize=None)
def generator_base(num_windows):
    return ecc.FixedBase(_limbs(GENERATOR), num_windows)


def _check_tables(base, point, num_windows):
    """the points, the coefficients at k = 0 .. 7, u^2 = y + z and z - y a non-residue; -> the table"""
    table = base.window_table()
    assert base.generator() == point
    assert table == fx.window_table(point, num_windows)
    coeffs, zs, us = base.lagrange_coeffs(), base.z(), base.u()
    assert len(coeffs) == len(zs) == len(us) == num_windows
    for w in range(num_windows):
        assert [fx.evaluate(coeffs[w], k) for k in range(8)] == [pt[0] for pt in table[w]], w
        for k, (_, y) in enumerate(table[w]):
            assert us[w][k] * us[w][k] % P == (y + zs[w]) % P and not fx.is_square(zs[w] - y), (w, k)
    assert coeffs == fx.lagrange_coeffs(table)
    return table


# ---- the tables -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_windows, want_z", [(NUM_WINDOWS_SHORT, fx.Z_GENERATOR_22), (NUM_WINDOWS, fx.Z_GENERATOR_85)])
def test_tables_of_the_generator(num_windows, want_z):
    base = generator_base(num_windows)
    table = _check_tables(base, GENERATOR, num_windows)
    assert base.z() == want_z
    if num_windows == NUM_WINDOWS:                                             # minimality, where the z is small enough to search the host
        for w in (42, 81, 10):
            assert fx.find_z([pt[1] for pt in table[w]], limit=want_z[w] + 1) == want_z[w], w


def test_z_limit():
    """window 42 has the smallest z of the 85, 1684: a bound of 1684 excludes it, one of 1685 still leaves the others without"""
    for limit in (1684, 1685):
        with pytest.raises(NotFound):
            ecc.FixedBase(_limbs(GENERATOR), NUM_WINDOWS, z_limit=limit)
    import torch
    dev = fields.current_device()
    points, lagrange, us = (torch.zeros((NUM_WINDOWS, 8, c), dtype=torch.int64, device=dev) for c in (8, 4, 4))
    zs = torch.zeros((NUM_WINDOWS,), dtype=torch.int64, device=dev)
    base = _limbs(GENERATOR)
    rc = lib().h2_ecc_fixed_tables_device(base.ctypes.data_as(C.POINTER(C.c_uint64)), NUM_WINDOWS, 1685, points.data_ptr(),
                                          lagrange.data_ptr(), zs.data_ptr(), us.data_ptr(), None)
    assert rc == ERR_NOTFOUND
    got = [int(v) for v in zs.cpu().numpy().view(np.uint64)]
    assert got[42] == 1684 and all(z == 2 ** 64 - 1 for w, z in enumerate(got) if w != 42)


def test_z_limit_just_above_the_largest_z_succeeds():
    """Two windows of the generator.  Window 0 is the first of every table, z = 43655; window 1 is then the LAST window, whose points
    are [8 k - 2]B and not the [(k + 2) 8]B behind the 109180 of the longer tables: its z is 5583, from the host search (re-derived
    here).  The bound is exclusive: 43656 admits both, 43655 leaves window 0 without."""
    two = ecc.FixedBase(_limbs(GENERATOR), 2, z_limit=fx.Z_GENERATOR_2[0] + 1)
    table = _check_tables(two, GENERATOR, 2)
    assert two.z() == fx.Z_GENERATOR_2 and fx.Z_GENERATOR_2[0] == fx.Z_GENERATOR_85[0]
    assert fx.find_z([pt[1] for pt in table[1]], limit=fx.Z_GENERATOR_2[1] + 1) == fx.Z_GENERATOR_2[1]
    with pytest.raises(NotFound):
        ecc.FixedBase(_limbs(GENERATOR), 2, z_limit=fx.Z_GENERATOR_2[0])


def test_tables_of_a_second_base():
    point = ec.random_bases(3)[2]
    _check_tables(ecc.FixedBase(_limbs(point), NUM_WINDOWS_SHORT), point, NUM_WINDOWS_SHORT)


# ---- mul_fixed --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scalar_pool(num_windows):
    """257 scalars, the edge ones in front, and their products"""
    if num_windows == NUM_WINDOWS:
        scalars = fx.EDGE_SCALARS + ec.random_scalars(257 - len(fx.EDGE_SCALARS), seed=21)
    else:
        scalars = fx.EDGE_SCALARS_SHORT + ec.random_scalars(257 - len(fx.EDGE_SCALARS_SHORT), bits=66, seed=22)
    return scalars, [ec.ec_mul(k, GENERATOR) for k in scalars]


@pytest.mark.parametrize("num_windows", [NUM_WINDOWS_SHORT, NUM_WINDOWS])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_mul_fixed_against_ec_mul(n, num_windows):
    scalars, want = scalar_pool(num_windows)
    k = fields.to_limbs(scalars[:n], FP, montgomery=False)
    pts = ecc.mul_fixed(generator_base(num_windows), _up(k))
    assert pts.shape == (n, 8) and _points(pts) == want[:n]
    assert scalars[0] == 0 and want[0] == (0, 0)
    if n == 65:                                                               # numpy in, numpy out
        host = ecc.mul_fixed(generator_base(num_windows), k)
        assert isinstance(host, np.ndarray) and (host.view(np.int64) == pts.cpu().numpy()).all()


def test_mul_fixed_short_negates():
    magnitudes = [0, 1, (1 << 64) - 1, 0, 1, (1 << 64) - 1, 12345]
    signs = [1, 1, 1, -1, -1, -1, -1]
    base = generator_base(NUM_WINDOWS_SHORT)
    pts = ecc.mul_fixed_short(base, _up(fields.to_limbs(magnitudes, FP, montgomery=False)), signs)
    assert _points(pts) == [ec.ec_mul(s * m, GENERATOR) for m, s in zip(magnitudes, signs)]
    with pytest.raises(ValueError):
        ecc.mul_fixed_short(base, fields.to_limbs([1], FP, montgomery=False), [2])


# ---- mul_fixed_trace --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_windows", [NUM_WINDOWS_SHORT, NUM_WINDOWS])
@pytest.mark.parametrize("count", [1, 65])
def test_trace_against_the_restated_witness(count, num_windows):
    """all six columns at every row and the 11 aux entries; row 0 of x_qr, y_qr is zero; the aux's last two are `mul_fixed`'s product"""
    base = generator_base(num_windows)
    scalars, products = scalar_pool(num_windows)
    first = 4 if count == 1 and num_windows == NUM_WINDOWS else 0             # count = 1 takes LAST_DOUBLING
    scalars, products = scalars[first:first + count], products[first:first + count]
    table, us, nw = base.window_table(), base.u(), num_windows
    k = _up(fields.to_limbs(scalars, FP, montgomery=False))
    cols, aux = ecc.mul_fixed_trace(base, k)
    assert cols.shape == (6, nw * count, 4) and aux.shape == (count, 11, 4)
    got, got_aux = [_ints(cols[c]) for c in range(6)], _ints(aux)
    for i, scalar in enumerate(scalars):
        w_cols, w_aux, result = fx.mul_fixed_trace(table, us, scalar)
        for c in range(6):
            assert got[c][i * nw:(i + 1) * nw] == w_cols[c], (i, c)
        assert got_aux[11 * i:11 * (i + 1)] == w_aux, i
        assert result == products[i] and got[fx.X_QR][i * nw] == got[fx.Y_QR][i * nw] == 0
        if scalar in (fx.LAST_DOUBLING, fx.LAST_DOUBLING_NON_CANONICAL):       # the doubling branch of add.rs: x_q = x_p, y_q = y_p
            assert w_aux[0:2] == w_aux[2:4] and w_aux[5] == 0 and w_aux[8] != 0 and result != (0, 0)
    assert _points(ecc.mul_fixed(base, k)) == products
    if count == 65:
        h_cols, h_aux = ecc.mul_fixed_trace(base, fields.to_limbs(scalars, FP, montgomery=False))
        assert isinstance(h_cols, np.ndarray) and (h_cols.view(np.int64) == cols.cpu().numpy()).all()
        assert (h_aux.view(np.int64) == aux.cpu().numpy()).all()


# ---- arguments --------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    import torch
    dev = fields.current_device()
    base = generator_base(NUM_WINDOWS_SHORT)
    buf = torch.zeros((4096, 4), dtype=torch.int64, device=dev)
    p = buf.data_ptr()
    for nw in (1, 86):
        assert lib().h2_ecc_mul_fixed_device(base.points.data_ptr(), nw, p, 1, p, None) == ERR_ARGS
        assert lib().h2_ecc_mul_fixed_trace_device(base.points.data_ptr(), base.us.data_ptr(), nw, p, 1, p, p, None) == ERR_ARGS
        with pytest.raises(ValueError):
            ecc.FixedBase(_limbs(GENERATOR), nw)
    assert lib().h2_ecc_mul_fixed_device(base.points.data_ptr(), 22, None, 1, p, None) == ERR_ARGS
    assert lib().h2_ecc_mul_fixed_device(base.points.data_ptr(), 22, p, 1, None, None) == ERR_ARGS
    assert lib().h2_ecc_mul_fixed_device(None, 22, p, 1, p, None) == ERR_ARGS
    assert lib().h2_ecc_mul_fixed_device(None, 22, None, 0, None, None) == OK
    assert lib().h2_ecc_mul_fixed_trace_device(base.points.data_ptr(), None, 22, p, 1, p, p, None) == ERR_ARGS
    assert lib().h2_ecc_mul_fixed_trace_device(base.points.data_ptr(), base.us.data_ptr(), 22, p, 1, None, p, None) == ERR_ARGS
    assert lib().h2_ecc_mul_fixed_trace_device(None, None, 22, None, 0, None, None, None) == OK
    off_curve = (GENERATOR[0], GENERATOR[1] + 1)
    for bad in (off_curve, (0, 0)):
        with pytest.raises(ValueError):
            ecc.FixedBase(_limbs(bad), NUM_WINDOWS_SHORT)
    g = _limbs(GENERATOR)
    assert lib().h2_ecc_fixed_tables_device(g.ctypes.data_as(C.POINTER(C.c_uint64)), 22, 0, None, p, p, p, None) == ERR_ARGS
