"""The opening argument's challenge recode (csrc/ipa_recode.h: the endomorphism split u = k1 + k2 lambda on 64-bit limbs and the
non-adjacent forms the collapse kernels walk) is plain C++ with no HIP in it: tests/native/ipa_recode_check.cpp compiles the header for
the CPU under the address and undefined-behaviour sanitizers -- the same text collapse_launch recodes with -- and its output is checked
here with big integers.  The device copy of the constants (glv.cuh) is what tests/test_glv_constants.py checks; this is the host copy."""
import os
import random
import subprocess

import pytest

from glv_edge_scalars import LAMBDA, endomorphism_edge_values, top_window_boundary_values
from oracle import pasta
from test_glv_constants import _array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = {0: "fq", 1: "fp"}      # curve -> its scalar field: Pallas scalars live in Fq, Vesta's in Fp


@pytest.fixture(scope="module")
def exe():
    path = os.path.join(ROOT, "build", "ipa_recode_check")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "ipa_recode_check.cpp"), "-o", path])
    return path


@pytest.fixture(scope="module")
def recoded(exe):
    """curve -> (exit code, stderr, [(u, top, digits of k1, digits of k2)]) over the edges of the split, the boundaries of the top
    window and 4000 random scalars: 4255 per field"""
    out = {}
    for curve, name in FIELDS.items():
        q = pasta.CURVES[curve][1]
        rng = random.Random(5)
        us = endomorphism_edge_values(curve) + top_window_boundary_values(curve, rng) + [rng.randrange(q) for _ in range(4000)]
        assert len(us) == 4255
        run = subprocess.run([exe, name], input="".join("%064x\n" % u for u in us), capture_output=True, text=True, timeout=120)
        rows = [[int(x) for x in ln.split()] for ln in run.stdout.splitlines()]
        assert len(rows) == len(us) and all(len(r) == 1 + 2 * 257 for r in rows), run.stderr[-2000:]
        out[curve] = (run.returncode, run.stderr, [(u, r[0], r[1:258], r[258:]) for u, r in zip(us, rows)])
    return out


@pytest.mark.parametrize("curve", [0, 1])
def test_host_constants_are_the_device_constants(exe, curve):
    """kGlv's row of the field, printed as integers, against what test_glv_constants parses out of glv.cuh"""
    run = subprocess.run([exe, FIELDS[curve], "constants"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr[-2000:]
    got = {k: int(v, 16) for k, v in (ln.split() for ln in run.stdout.splitlines())}
    want = {n: _array(d, curve == 0) for n, d in (("a1", "a1"), ("b1_abs", "b1"), ("a2", "a2"), ("b2", "b2"), ("g1", "g1"), ("g2", "g2"))}
    assert got == want


@pytest.mark.parametrize("curve", [0, 1])
def test_digits_are_non_adjacent_and_recombine(recoded, curve):
    """every digit in {-1, 0, 1}, no two neighbours both non-zero, and k1 + k2 lambda = u (mod q) for k_i = sum_j d_i[j] 2^j"""
    q, lam = pasta.CURVES[curve][1], LAMBDA[curve]
    for u, _, d1, d2 in recoded[curve][2]:
        for d in (d1, d2):
            assert set(d) <= {-1, 0, 1}, hex(u)
            assert not any(a and b for a, b in zip(d, d[1:])), hex(u)
        k1, k2 = (sum(v << j for j, v in enumerate(d)) for d in (d1, d2))
        assert (k1 + k2 * lam - u) % q == 0, hex(u)


@pytest.mark.parametrize("curve", [0, 1])
def test_top_is_the_highest_digit_used(recoded, curve):
    """`top` is where the kernels' walk starts: the highest index either row uses (-1 for u = 0), within the 130 bits of a half"""
    for u, top, d1, d2 in recoded[curve][2]:
        assert top == max([j for j in range(257) if d1[j] or d2[j]], default=-1), hex(u)
        assert top <= 129 and (top == -1) == (u == 0), hex(u)


@pytest.mark.parametrize("curve", [0, 1])
def test_sanitizers_are_silent(recoded, curve):
    """-fno-sanitize-recover=all: any report of either sanitizer ends the program with a non-zero status"""
    rc, err, _ = recoded[curve]
    assert rc == 0 and err == "", err[-2000:]
