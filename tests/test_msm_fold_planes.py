"""The integer code of the fold (csrc/msm_plan.h: the k-th integer with a given bit set, which lines a bit plane of fold9_planes and
sub_planes holds, the launch geometry of the 8 x 32 fold) is plain code with no HIP in it: tests/native/msm_fold_check.cpp compiles the
header for the CPU -- the same text the kernels' index maps call -- and prints the maps over every plan of its sweep.  This module holds
what it prints to the definitions, written here in Python integers: a fold is right when every line's planes add up to the line's weight."""
import hashlib
import os
import re
import subprocess

import pytest

import commit_plans as cp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "msm_fold_check.cpp")


def _build(exe, *flags):
    return subprocess.run(["g++", "-O2", "-std=c++17", *flags, SRC, "-o", exe], capture_output=True, text=True)


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return out.returncode, out.stdout


def _ints(text):
    return [int(x) for x in text.split()]


@pytest.fixture(scope="module")
def printed():
    build = os.path.join(ROOT, "build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "msm_fold_check")
    made = _build(exe)
    assert made.returncode == 0, made.stderr
    rc, text = _run(exe)
    assert rc == 0
    lines = text.splitlines()
    m = re.fullmatch(r"constants: LDS_CAP (\d+) MAX_C (\d+) MAX_C_SHARED (\d+) TREE_LANES (\d+)", lines[0])
    assert lines[-1] == "done"
    got = dict(lds_cap=int(m.group(1)), max_c=int(m.group(2)), max_c_shared=int(m.group(3)), tree_lanes=int(m.group(4)), kth={}, sub={}, calls=[], shapes={},
               digest=hashlib.sha256(text.encode()).hexdigest())
    shape = None
    for line in lines[1:-1]:
        kind, rest = line.split(" ", 1)
        if kind == "K":
            head, vals = rest.split(":")
            got["kth"][tuple(_ints(head))] = _ints(vals)
        elif kind == "B":
            head, vals = rest.split(":")
            t, count = _ints(head)
            got["sub"][t] = (count, _ints(vals))
        elif kind == "C":
            call, fold = rest.split(" = ")
            got["calls"].append((call, fold.split()))
        elif kind == "P":
            c, S, NR, cb, planes = _ints(rest)
            shape = got["shapes"][(c, S, NR)] = dict(cb=cb, planes=planes, plane=[])
        elif kind == "p":
            head, vals = rest.split(":")
            t, ncol, nrow = _ints(head)
            assert t == len(shape["plane"])
            shape["plane"].append((ncol, nrow, _ints(vals)))
        else:
            raise AssertionError(line)
    assert (got["max_c"], got["max_c_shared"]) == (cp.MAX_C, cp.MAX_C_SHARED)
    return got


def test_kth_integer_with_bit_t_set(printed):
    """For every t in 0 .. 15 and width n in t + 1 .. 16: k -> the k-th integer with bit t set, over k < 2^(n-1), is strictly increasing and
    its image is exactly {v < 2^n : bit t of v}."""
    seen = 0
    for t in range(16):
        for n in range(t + 1, 17):
            vals = printed["kth"][(t, n)]
            assert len(vals) == 1 << (n - 1), (t, n)
            assert all(a < b for a, b in zip(vals, vals[1:])), (t, n)
            assert set(vals) == {v for v in range(1 << n) if v >> t & 1}, (t, n)
            seen += 1
    assert seen == len(printed["kth"]) == 136


def _weights(planes):
    """line -> sum of 2^t over the planes that hold it; each line at most once in a plane"""
    w = {}
    for t, lines in enumerate(planes):
        assert len(set(lines)) == len(lines), ("a line twice in plane", t)
        for line in lines:
            w[line] = w.get(line, 0) + (1 << t)
    return w


def test_fold9_planes_weights_add_up(printed):
    """Every (S, NR, cb) msm_plan and grouped_plan hand fold9_group over registered widths 8 .. 20 (plain, blinded, batched, paired) and the
    generic shapes: the planes number the c - 1 workgroups the launch has, each has the ncol + nrow summands it is launched for, column lo
    weighs lo + 1, row hi >= 1 weighs S hi, and row 0 is in no plane."""
    folds = [(call, f) for call, f in printed["calls"] if f[0] == "fold9"]
    widths = set()
    for call, f in folds:
        c, S, NR, cb = (int(x) for x in f[1:])
        assert (c, S, NR) in printed["shapes"] and printed["shapes"][(c, S, NR)]["cb"] == cb, call
        assert S * NR == 1 << (c - 1) and S == 1 << cb, call          # the matrix is the slice
        if call.startswith("table"):
            widths.add(c)
    assert widths == set(range(8, cp.MAX_C_SHARED + 1))
    assert any(call.startswith("generic") and "grouped" in call for call, _ in folds) and any(call.startswith("generic") and "grouped" not in call for call, _ in folds)
    for (c, S, NR), shape in printed["shapes"].items():
        assert shape["planes"] == c - 1 == len(shape["plane"]), (c, S, NR)
        for t, (ncol, nrow, lines) in enumerate(shape["plane"]):
            assert len(lines) == ncol + nrow and all(0 <= x < S + NR for x in lines), (c, t)
            assert all(x < S for x in lines[:ncol]) and all(x >= S for x in lines[ncol:]), (c, t)
        w = _weights([lines for _, _, lines in shape["plane"]])
        assert S not in w, "row 0 carries weight 0"
        want = {lo: lo + 1 for lo in range(S)}
        want.update({S + hi: S * hi for hi in range(1, NR)})
        assert w == want, (c, S, NR)


def test_sub_planes_weights_add_up(printed):
    """sub_planes' 128-bucket slices: 8 planes, plane 7 is bucket 127 alone, bucket b weighs b + 1."""
    assert sorted(printed["sub"]) == list(range(8))
    for t, (count, buckets) in printed["sub"].items():
        assert count == len(buckets)
    assert printed["sub"][7] == (1, [127])
    assert _weights([printed["sub"][t][1] for t in range(8)]) == {b: b + 1 for b in range(128)}


def test_r256_fold_geometry(printed):
    """Every plan of the sweep that folds on the 8 x 32 layer (registered widths below 8, fold-only calls, wide slices through their row /
    column sums, generic multiexps with a blind): the segments tile the points, the first tree level leaves at most 32 sums a slice and
    covers every partial, the second reads exactly what the first left, and a tree launch's LDS fits."""
    folds = [(call, [int(x) for x in f[1:]]) for call, f in printed["calls"] if f[0] == "r256"]
    assert len(folds) >= 50 and any(f[1] == 2 and call.startswith("table") and int(call.split()[1]) > cp.MAX_C for call, f in folds), "a wide slice"
    two_level = 0
    for call, f in folds:
        nb, slices, c, seg, segs, levels = f[:6]
        lv = [tuple(f[6 + 3 * i:9 + 3 * i]) for i in range(levels)]
        lds = f[6 + 3 * levels]
        assert len(f) == 7 + 3 * levels and levels in (1, 2), call
        assert seg in (4, 8) and nb % seg == 0 and segs * seg == slices * nb, call
        bps, per_slice, share = lv[0]
        assert per_slice * slices == segs, call
        assert 1 <= bps <= 32 and bps * share >= per_slice and (bps - 1) * share < per_slice, call      # (no workgroup of the first level is idle)
        assert (levels == 2) == (bps > 1), call
        if levels == 2:
            assert lv[1] == (1, bps, bps), call
            two_level += 1
        assert lv[-1][0] == 1, call
        assert lds == printed["tree_lanes"] // 4 * 128 <= printed["lds_cap"], call
    assert two_level > 0


def test_sanitized_build_prints_the_same(printed):
    """The maps shift by computed amounts: the same driver built with -fsanitize=address,undefined (errors fatal) prints the same.  Skipped
    only where the toolchain has no sanitizer runtime to link."""
    exe = os.path.join(ROOT, "build", "msm_fold_check_san")
    made = _build(exe, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    if made.returncode != 0 and re.search(r"cannot find -l?(asan|ubsan)|libasan|libubsan", made.stderr):
        pytest.skip("no sanitizer runtime to link")
    assert made.returncode == 0, made.stderr
    rc, text = _run(exe)
    assert rc == 0 and hashlib.sha256(text.encode()).hexdigest() == printed["digest"]
