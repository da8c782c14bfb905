"""The divstep inversion (csrc/field_inv.cuh) on the whole inversion list of tests/field_edge_cases.py -- 2^k, 2^k +- 1 and p - 2^k for every
k in 0 .. 254, p - 1, p - 2, (p +- 1) / 2, single limbs, about 1 100 values per field -- compiled for the host with the undefined-behaviour
and address sanitizers: tests/native/modinv_edge_check.cpp, a stand-alone program that is run directly.  The limb arithmetic is signed 32-
and 64-bit; a signed overflow would be undefined behaviour that hipcc may compile differently from g++.  No GPU."""
import os
import subprocess

import pytest

import field_edge_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-std=c++17", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"]


def host_program(sanitized=True):
    """build/modinv_edge_check (with the sanitizers) or build/modinv_edge_check_plain (the same source without them, for the comparison the
    GPU test makes: sanitizer runs stay on this side), built when missing or older than its sources.  No compiler is a failure, not a skip."""
    exe = os.path.join(ROOT, "build", "modinv_edge_check" if sanitized else "modinv_edge_check_plain")
    srcs = [os.path.join(ROOT, "tests", "native", "modinv_edge_check.cpp"), os.path.join(ROOT, "halo2_amd", "csrc", "field_inv.cuh")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++"] + (FLAGS if sanitized else ["-O1", "-std=c++17"]) + [srcs[0], "-o", exe])
    return exe


def run_host(exe, tmp_path, field, values):
    """[(modinv30(x), the same by the spelled-out loop, sign of the final f, batches until g = 0)], one process"""
    src, dst = tmp_path / f"modinv_{field}.in", tmp_path / f"modinv_{field}.out"
    src.write_bytes(b"".join(int(v).to_bytes(32, "little") for v in values))
    done = subprocess.run([exe, ec.FIELD_ARG[field], str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, (field, done.returncode, done.stdout, done.stderr[-3000:])      # a sanitizer report ends the program
    raw = dst.read_bytes()
    assert len(raw) == 72 * len(values)
    rec = lambda i: raw[72 * i:72 * i + 72]
    return [(int.from_bytes(rec(i)[:32], "little"), int.from_bytes(rec(i)[32:64], "little"),
             int.from_bytes(rec(i)[64:68], "little", signed=True), int.from_bytes(rec(i)[68:72], "little", signed=True)) for i in range(len(values))]


@pytest.mark.parametrize("field", ec.FIELDS)
def test_modinv30_on_the_whole_inversion_list_under_the_sanitizers(tmp_path, field):
    """Every inverse == pow(x, -1, p) (0 for 0), below p, the same from modinv30 and from its loop spelled out batch by batch; both signs
    of the final f occur; g is zero after at most 20 batches of 30 divsteps -- the "590 divsteps, 20 batches" claim of field_inv.cuh.
    Largest batch index observed on these inputs: 18 in both fields (540 divsteps: two batches of margin)."""
    p, values = ec.P[field], ec.inversion_values(field)
    assert all(0 <= x < p for x in values) and 0 in values and p - 1 in values          # field_inv.cuh: `x < p`
    got = run_host(host_program(), tmp_path, field, values)
    assert run_host(host_program(sanitized=False), tmp_path, field, values) == got      # the build the GPU test compares the device with
    for x, (inv, traced, sign, batches) in zip(values, got):
        assert inv == ec.plain_inv(x, field) and traced == inv and sign in (1, -1), (hex(x), hex(inv), sign)
        assert 0 <= batches <= 20 and (batches == 0) == (x == 0), (hex(x), batches)
    assert {s for _, _, s, _ in got} == {1, -1}
    largest = max(b for _, _, _, b in got)
    print(f"field {field}: largest batch index {largest}, final f = -1 on {sum(s < 0 for _, _, s, _ in got)} of {len(got)} inputs")
    assert largest <= 20
