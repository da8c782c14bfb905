"""The window digits of the bucket sort (csrc/msm_digits.h: the run-time and compile-time cutters, their dispatcher, the cutter of the
two halves of an endomorphism-split scalar, the 16- and 32-bit digit codes) are plain integer code with no HIP in it:
tests/native/msm_digits_check.cpp compiles the header for the CPU -- the same text the kernels cut with -- and prints the codes of the
values below at every width.  This module decodes them and holds them to a recode written here from the definition, in Python integers:
the digits of v at width c are the unique d_w in [-2^(c-1) + 1, 2^(c-1)] with sum d_w 2^(c w) = v."""
import hashlib
import os
import random
import re
import struct
import subprocess

import pytest

import commit_plans as cp
import glv_edge_scalars as ges
from oracle import pasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATIC_WIDTHS = (16, 17, 18, 19, 20, 13)      # the dispatcher's compile-time widths
ZERO16, ZERO32 = 0xFFFF, 0xFFFFFFFF
RANDOM = 2000


def recode(v, c, W):
    """the definition: d = v mod 2^c taken in (-2^(c-1), 2^(c-1)], then (v - d) / 2^c; v may be negative.  None if W digits do not reach v."""
    half, full, digits = 1 << (c - 1), 1 << c, []
    for _ in range(W):
        d = v % full
        if d > half:
            d -= full
        digits.append(d)
        v = (v - d) >> c
    return digits if v == 0 else None


def code16(d):
    return ZERO16 if d == 0 else (abs(d) - 1) | (0x8000 if d < 0 else 0)


def code32(d):
    return ZERO32 if d == 0 else (abs(d) - 1) | (0x80000000 if d < 0 else 0)


def decode(codes, bits):
    zero, sign = (ZERO16, 0x8000) if bits == 16 else (ZERO32, 0x80000000)
    return [0 if x == zero else -((x & (sign - 1)) + 1) if x & sign else (x & (sign - 1)) + 1 for x in codes]


def unpack(text, bits):
    raw = bytes.fromhex(text)
    return list(struct.unpack(">%d%s" % (len(raw) // (bits // 8), "H" if bits == 16 else "I"), raw))


def window_patterns(c, top):
    """every window that lies wholly below bit `top` set to 2^(c-1) (the largest positive digit: no carry), to 2^(c-1) + 1 (each digit
    negative, the carry runs all the way up) and to 2^c - 1"""
    n = top // c
    return [sum(p << (c * w) for w in range(n)) for p in (1 << (c - 1), (1 << (c - 1)) + 1, (1 << c) - 1)]


def scalars():
    """both fields: 0, 1, q - 1, the three window patterns at every width (below the modulus, and over all 256 bits reduced mod q), the
    values of tests/glv_edge_scalars.py, seeded random values"""
    out = []
    for curve in (0, 1):
        q = pasta.CURVES[curve][1]
        rng = random.Random(0x5ca1a5 + curve)
        vals = [0, 1, q - 1]
        for c in range(2, cp.MAX_C_SHARED + 1):
            vals += window_patterns(c, 254) + [v % q for v in window_patterns(c, 256)]
        vals += ges.endomorphism_edge_values(curve) + ges.top_window_boundary_values(curve, rng)
        vals += [rng.randrange(q) for _ in range(RANDOM)]
        assert all(0 <= v < q for v in vals)
        out += vals
    return out


def glv_halves():
    """(n0, n1, m0, m1): 0, 2^128, 2^129 - 1, the three window patterns at every width (below 2^129) and seeded random magnitudes below
    2^129, each in both positions and under each of the four sign pairs"""
    rng = random.Random(0x61b5)
    mags = [0, 1 << 128, (1 << 129) - 1]
    for c in range(2, cp.MAX_C + 1):
        mags += window_patterns(c, 129)
    mags += [rng.getrandbits(129) for _ in range(RANDOM)]
    assert all(0 <= m < 1 << 129 for m in mags)
    return [(n0, n1, m, mags[(i + 1) % len(mags)]) for i, m in enumerate(mags) for n0 in (0, 1) for n1 in (0, 1)]


def _build(exe, *flags):
    return subprocess.run(["g++", "-O2", "-std=c++17", *flags, os.path.join(ROOT, "tests", "native", "msm_digits_check.cpp"), "-o", exe], capture_output=True, text=True)


def _run(exe, values_file):
    """the driver's lines as they come, and afterwards its exit code and the digest of all it printed"""
    proc = subprocess.Popen([exe, values_file], stdout=subprocess.PIPE, text=True)
    digest = hashlib.sha256()

    def lines():
        for line in proc.stdout:
            digest.update(line.encode())
            yield line.rstrip("\n")
    return proc, lines(), digest


CHECKS = {
    "sum": "the run-time cutter's digits sum to the scalar (so the last carry is zero)",
    "range": "every digit lies in [-2^(c-1) + 1, 2^(c-1)]",
    "recode": "the digits are those of the recode from the definition",
    "runtime_codes": "the run-time cutter's 32-bit codes are those of the recode",
    "dispatcher_codes": "the dispatcher prints the same codes at every width",
    "static_codes": "the compile-time cutter prints the same codes at each width of the dispatcher's list, and is reached at no other",
    "narrow_codes": "up to kMaxC the narrowed 16-bit code of every digit has |d| - 1 < 2^15 and stands for the same digit as the 32-bit code",
    "glv_sum": "a half's digits sum to -mag when it is negative, else to mag",
    "glv_range": "a half's digits lie in the encodable set, |d| - 1 < 2^15 (a negative half is rounded so that no digit is -2^(c-1) after the flip)",
    "glv_recode": "a half's digits are those of the recode from the definition",
    "glv_code16": "a half's 16-bit codes are those of the recode",
    "glv_code32": "a half's 32-bit codes stand for the same digits as its 16-bit codes",
}


@pytest.fixture(scope="module")
def checked():
    """builds and runs the driver over every value and holds every line to every check above: `missed[check]` lists the (value, width) at
    which a check did not hold, `tally` what was seen.  Only a malformed line stops it."""
    S, G = scalars(), glv_halves()
    build = os.path.join(ROOT, "build")
    os.makedirs(build, exist_ok=True)
    values_file = os.path.join(build, "msm_digits_values.txt")
    with open(values_file, "w") as f:
        f.write("".join("S %x\n" % v for v in S) + "".join("G %d %d %x %x\n" % g for g in G))
    exe = os.path.join(build, "msm_digits_check")
    made = _build(exe)
    assert made.returncode == 0, made.stderr
    proc, lines, digest = _run(exe, values_file)
    m = re.fullmatch(r"constants: MAX_C (\d+) MAX_C_SHARED (\d+)", next(lines))
    max_c, max_c_shared = int(m.group(1)), int(m.group(2))
    assert (max_c, max_c_shared) == (cp.MAX_C, cp.MAX_C_SHARED)
    tally = dict(scalar_lines=0, glv_lines=0, static_lines=0, narrow_lines=0, digits=0, extreme=0, zero=0, carried_to_top=0)
    missed = {name: [] for name in CHECKS}

    def hold(name, ok, *where):
        if not ok:
            missed[name].append(where)

    for v in S:
        for c in range(2, max_c_shared + 1):
            kind, c_got, W, runtime, dispatcher, static, narrow = next(lines).split()
            assert (kind, int(c_got)) == ("S", c)
            W, half, at = int(W), 1 << (c - 1), (hex(v), c)
            want = recode(v, c, W)
            assert want is not None, (at, W, "the windows the plan gives do not reach the scalar")
            got = decode(unpack(runtime, 32), 32)
            hold("sum", sum(d << (c * w) for w, d in enumerate(got)) == v, *at)
            hold("range", all(-half + 1 <= d <= half for d in got), *at)
            hold("recode", got == want, *at)
            codes = [code32(d) for d in want]
            hold("runtime_codes", unpack(runtime, 32) == codes, *at)
            hold("dispatcher_codes", unpack(dispatcher, 32) == codes, *at)
            hold("static_codes", (static != "-") == (c in STATIC_WIDTHS) and (static == "-" or unpack(static, 32) == codes), *at)
            tally["static_lines"] += static != "-"
            hold("narrow_codes", (narrow != "-") == (c <= max_c), *at)
            if narrow != "-":
                n16 = unpack(narrow, 16)
                hold("narrow_codes", all(abs(d) - 1 < 1 << 15 for d in got if d) and n16 == [code16(d) for d in want] and decode(n16, 16) == got, *at)
                tally["narrow_lines"] += 1
            tally["scalar_lines"] += 1
            tally["digits"] += W
            tally["extreme"] += got.count(half)
            tally["zero"] += got.count(0)
            tally["carried_to_top"] += all(d < 0 for d in got[:254 // c])      # every whole window below the modulus carried
    for n0, n1, m0, m1 in G:
        for c in range(2, max_c + 1):
            kind, c_got, W, *parts = next(lines).split()
            assert (kind, int(c_got), len(parts)) == ("G", c, 4)
            W, half = int(W), 1 << (c - 1)
            for neg, mag, p16, p32 in ((n0, m0, parts[0], parts[1]), (n1, m1, parts[2], parts[3])):
                value, at = -mag if neg else mag, (hex(mag), neg, c)
                want = recode(value, c, W)
                assert want is not None, (at, W)
                got = decode(unpack(p16, 16), 16)
                hold("glv_sum", sum(d << (c * w) for w, d in enumerate(got)) == value, *at)
                hold("glv_range", all(-half + 1 <= d <= half for d in got) and all(abs(d) - 1 < 1 << 15 for d in got if d), *at)
                hold("glv_recode", got == want, *at)
                hold("glv_code16", unpack(p16, 16) == [code16(d) for d in want], *at)
                hold("glv_code32", unpack(p32, 32) == [code32(d) for d in want] and decode(unpack(p32, 32), 32) == got, *at)
                tally["digits"] += W
                tally["extreme"] += got.count(half)
            tally["glv_lines"] += 1
    assert next(lines, None) is None, "the driver printed more than it was asked"
    assert proc.wait(timeout=60) == 0
    return dict(tally=tally, missed=missed, values_file=values_file, digest=digest.hexdigest(), scalars=len(S), halves=len(G), max_c=max_c,
                max_c_shared=max_c_shared)


@pytest.mark.parametrize("check", list(CHECKS))
def test_digits_and_codes(checked, check):
    """One case per property of CHECKS, over every scalar of both fields at every width 2 .. kMaxCShared (the halves of a split scalar: every
    magnitude in both positions under the four sign pairs at 2 .. kMaxC), with the window count msm_plan.h gives for that width."""
    missed = checked["missed"][check]
    assert not missed, (CHECKS[check], len(missed), missed[:5])


def test_every_value_and_width_was_seen(checked):
    """a line per scalar and width, per pair of halves and width; the compile-time cutter at each of its widths; and the cases the values
    were made for occurred: the largest positive digit, digit zero, a carry through every whole window"""
    t = checked["tally"]
    assert t["scalar_lines"] == checked["scalars"] * (checked["max_c_shared"] - 1) and checked["scalars"] >= 2 * (RANDOM + 3)
    assert t["static_lines"] == checked["scalars"] * len(STATIC_WIDTHS)
    assert t["narrow_lines"] == checked["scalars"] * (checked["max_c"] - 1)
    assert t["glv_lines"] == checked["halves"] * (checked["max_c"] - 1) and checked["halves"] >= 4 * (RANDOM + 3)
    assert t["extreme"] > 0 and t["zero"] > 0 and t["carried_to_top"] > 0, t


def test_sanitized_build_prints_the_same(checked):
    """The cutters shift by computed amounts and pick limbs by computed indices: the same driver built with -fsanitize=address,undefined
    (errors fatal) runs over the same values and prints the same."""
    exe = os.path.join(ROOT, "build", "msm_digits_check_san")
    made = _build(exe, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    assert made.returncode == 0, made.stderr
    proc, lines, digest = _run(exe, checked["values_file"])
    count = sum(1 for _ in lines)
    assert proc.wait(timeout=60) == 0 and count > 1 and digest.hexdigest() == checked["digest"]
