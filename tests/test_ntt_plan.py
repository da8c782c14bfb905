"""The NTT's pass plan and its workgroup -> tile map (csrc/ntt_plan.h) are plain C++ with no HIP in them: tests/native/ntt_plan_check.cpp
compiles the header for the CPU -- the same text the library plans with and the kernel maps its workgroups with -- and checks it here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report():
    exe = os.path.join(ROOT, "build", "ntt_plan_check")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "native", "ntt_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "ntt_plans_parent.txt")], capture_output=True, text=True, timeout=120)
    return out.returncode, out.stdout + out.stderr


def test_every_plan_keeps_what_the_kernels_rely_on(report):
    """Every L in 1..32 x plan kind x in place / out of place x maxr in {4, 10, 11, 12} x logT in {0, 3, 5} (x both values of the
    nine-limb switch): the stages sum to L with each r in [1, maxr]; the 8 x 32 tile fits the LDS cap (64 KiB under plan 1) and the
    nine-limb tile 160 KiB; tiles x 2^(r + logT) = 2^L with tiles < 2^32; logT <= the pass's column bits; 64 <= threads <= 1024; for
    r >= 2 a quarter of the tile is at most `threads` -- the radix-4 rounds of both kernels are `if (tid < ngrp)` without a loop --
    and the nine-limb kernel is planned only up to 2^28 (its twiddle offsets are 32-bit)."""
    rc, text = report
    assert "invariants: 3072 plans, 0 violations" in text, text


def test_tile_map_is_a_permutation(report):
    """ntt_tile_of_block over b < tiles is a permutation of [0, tiles) for every pass after the first of every plan above with L <= 26:
    a workgroup that mapped onto another's tile would leave one tile of the vector untransformed."""
    rc, text = report
    assert "tile map: 873 passes, 0 not a permutation" in text, text


def test_plans_are_the_parent_commits(report):
    """tests/ntt_plans_parent.txt holds what the planning loop computed while it was still inline in ntt_run (printed by a copy of
    that loop, not by ntt_plan): r, logT, threads, tiles and the LDS bytes of both kernels for every pass, L = 1..32, both plan kinds,
    the knob grid above and five more settings (a first-pass width, 64 and 32 KiB caps, 7- and 1-stage passes).  Among its rows:
    2^20 = 10 + 10 at logT 2, 256 tiles of 1024 lanes and 131072 B; 2^21 = 8 + 6 + 7; 2^22 = 8 + 8 + 6; 2^18 = 10 + 8 with 256 tiles
    each; 2^10 one pass of 256 lanes; 2^20 under plan 1 = 8 + 6 + 6 with 65536, 32768 and 32768 B."""
    rc, text = report
    assert "parent plans: 1088 rows, 0 mismatches" in text and rc == 0, text
    rows = {tuple(ln.split()[:6]): ln.split()[6:] for ln in open(os.path.join(ROOT, "tests", "ntt_plans_parent.txt")) if not ln.startswith("#")}
    dflt = lambda L, kind: [int(x) for x in rows[(str(L), str(kind), "10", "3", "-1", "131072")]]
    # (passes, then r logT threads tiles lds lds9 per pass)
    assert dflt(20, 0) == [2, 10, 2, 1024, 256, 131072, 153648, 10, 2, 1024, 256, 131072, 153648]
    assert dflt(21, 0)[1::6] == [8, 6, 7] and dflt(22, 0)[1::6] == [8, 8, 6]
    assert dflt(18, 0)[1::6] == [10, 8] and dflt(18, 0)[4::6] == [256, 256]
    assert dflt(10, 0)[:4] == [1, 10, 0, 256]
    assert dflt(20, 1)[1::6] == [8, 6, 6] and dflt(20, 1)[5::6] == [65536, 32768, 32768]
