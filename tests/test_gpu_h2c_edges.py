"""The square root (csrc/field_sqrt.cuh), the simplified SWU map, the affine sum and the isogeny (csrc/h2c_map.cuh), the point decoder
(csrc/points.hip) and BLAKE2b (csrc/h2c.hip) on the crafted inputs of tests/h2c_edge_cases.py: every 2-adic order of a^T, a = 0,
u = 0, equal and opposite mapped points, the kernel point of the isogeny, hash inputs on and next to a multiple of 128 bytes.
build/h2c_edge_driver (tests/native/h2c_edge_driver.hip) applies the device functions; every comparison here is equality of integers
with `oracle.pasta` / `oracle.hash_to_curve`."""
import glob
import os
import subprocess

import pytest

import h2c_edge_cases as ec
import halo2_amd as h
from oracle import c_oracle as co
from oracle import hash_to_curve as oh
from oracle import pasta as o

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVE = {"pallas": h.PALLAS, "vesta": h.VESTA}
FIELD_ARG = {"pallas": "fp", "vesta": "fq"}                      # the base field of the curve
WORDS_OUT = {"sqrt": 2, "swu": 2, "add": 3, "iso": 2, "pair": 2}


@pytest.fixture(scope="module")
def driver():
    """build/h2c_edge_driver, built here when it is missing or older than its sources (build() makes it).  No compiler and no binary
    is a failure, not a skip."""
    exe = os.path.join(ROOT, "build", "h2c_edge_driver")
    csrc = os.path.join(ROOT, "halo2_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "native", "h2c_edge_driver.hip")] + glob.glob(os.path.join(csrc, "*.cuh")) + glob.glob(os.path.join(csrc, "*.inc"))
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", srcs[0], "-o", exe])
    return exe


def run_driver(exe, tmp_path, mode, cid, cases):
    """cases: tuples of canonical integers -> tuples of canonical integers, one driver process"""
    src, dst = tmp_path / f"{mode}_{cid}.in", tmp_path / f"{mode}_{cid}.out"
    src.write_bytes(b"".join(int(v).to_bytes(32, "little") for case in cases for v in case))
    done = subprocess.run([exe, mode, FIELD_ARG[cid], str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, (mode, cid, done.returncode, done.stdout, done.stderr)
    raw, k = dst.read_bytes(), WORDS_OUT[mode]
    assert len(raw) == 32 * k * len(cases)
    words = [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]
    return [tuple(words[k * i:k * i + k]) for i in range(len(cases))]


@pytest.mark.parametrize("cid", ec.FIELDS)
def test_sqrt_at_every_two_adic_order(driver, tmp_path, cid):
    """fe_sqrt's flag and root == sqrt_mod for four elements of each order 2^0 .. 2^32 of a^T (`b == 1` on entry, every
    `v - k - 1` that can occur -- 0 .. 30, k being at least 1 inside the loop -- and the `++k == v` exit), 0, 1, 4, p - 1, p - 4, 5,
    2^256 mod p and 256 random elements: 395 lanes whose neighbours need different numbers of rounds, 8448 lanes in waves of one
    order each, and p - 1 alone.  Roots are below p, and the same a gives the same root in both orderings."""
    m, runs = ec.modulus(cid), ec.sqrt_runs(cid)
    roots = {}
    for name in ("interleaved", "grouped", "single"):
        got = run_driver(driver, tmp_path, "sqrt", cid, [(a,) for a in runs[name]])
        for a, (flag, root) in zip(runs[name], got):
            want_flag, want_root = ec.sqrt_expected(a, m)
            assert flag == want_flag and root < m, (name, a, flag, root)
            assert root == (want_root if want_flag else 0), (name, ec.two_adic_order(a, m) if a else None, a, root, want_root)
            assert roots.setdefault(a, root) == root, (name, a)
    assert roots[0] == 0 and set(runs["grouped"]) <= set(runs["interleaved"])


@pytest.mark.parametrize("cid", ec.FIELDS)
def test_swu_at_the_edges_of_u(driver, tmp_path, cid):
    """map_to_curve_simple_swu == the oracle's at u = 0 (the only u with tv == 0), 1, 2, p - 1, p - 2, (p +- 1) / 2 (sgn0 at the
    extremes), 16 u whose g(x1) is a square and 16 whose is not, the negatives of those 32, and 128 random u: 199 lanes."""
    us = ec.swu_inputs(cid)
    got = run_driver(driver, tmp_path, "swu", cid, [(u,) for u in us])
    assert got == [ec.swu(u, cid) for u in us]


@pytest.mark.parametrize("cid", ec.FIELDS)
def test_pairs_through_tangent_identity_and_zero(driver, tmp_path, cid):
    """What h2c_kernel computes after hashing == iso_map(Q0 + Q1): (u, u) and same-x equal-y pairs take the tangent branch, (u, p - u)
    and same-x opposite-y pairs give the identity (0, 0), u = 0 on either side or both; plus 128 random pairs.  1, 63 and 210 lanes."""
    for name, run in ec.pair_runs(cid).items():
        got = run_driver(driver, tmp_path, "pair", cid, [p for _, p in run])
        for (kind, (u0, u1)), r in zip(run, got):
            assert r == ec.pair_expected(u0, u1, cid), (name, kind, u0, u1, r)


@pytest.mark.parametrize("cid", ec.FIELDS)
def test_add_and_isogeny_on_their_own(driver, tmp_path, cid):
    """The affine sum: P + P at y = 0 and P + (-P) are the identity, P + P elsewhere the tangent, distinct x the chord.  The isogeny:
    x = x0 (`d == 0`, not reachable from a point of the curve) gives (0, 0), x0 +- 1 and 32 points of the iso curve the oracle's image."""
    adds = ec.add_inputs(cid)
    assert run_driver(driver, tmp_path, "add", cid, adds) == [ec.add_expected(*a, cid) for a in adds]
    isos = ec.iso_inputs(cid)
    assert run_driver(driver, tmp_path, "iso", cid, isos) == [ec.iso_expected(x, y, cid) for x, y in isos]


def canonical_ints(row):
    v = [int(x) for x in row]
    return (v[0] | v[1] << 64 | v[2] << 128 | v[3] << 192, v[4] | v[5] << 64 | v[6] << 128 | v[7] << 192)


@pytest.mark.parametrize("cid", ec.FIELDS)
def test_decoder_at_every_two_adic_order(cid):
    """h.points_from_bytes (the production kernel) on x whose x^3 + 5 has order 2^j, j = 0 .. 31, both sign bits: the oracle's point in
    both forms and the bytes back; j = 32 raises; one bad encoding at index 256 or 299 of 300 fails the batch."""
    curve, m, xs = CURVE[cid], ec.modulus(cid), ec.decoder_xs(cid)
    good = [ec.encode_x(xs[j], sign) for j in range(32) for sign in (0, 1)]
    want = [o.point_from_bytes(b, m) for b in good]
    mont = h.points_from_bytes(b"".join(good), curve)
    assert [co.affine_to_ints(curve, p) for p in mont] == want
    assert [canonical_ints(p) for p in h.points_from_bytes(b"".join(good), curve, h.FORM_CANONICAL)] == want
    assert h.points_to_bytes(mont, curve) == b"".join(good)
    for b in good:                                                       # and one at a time
        assert co.affine_to_ints(curve, h.points_from_bytes(b, curve)[0]) == o.point_from_bytes(b, m)
    for sign in (0, 1):
        with pytest.raises(ValueError):
            h.points_from_bytes(ec.encode_x(xs[32], sign), curve)
    batch = (good * 5)[:300]
    assert len(batch) == 300
    for at in (256, 299):
        broken = list(batch)
        broken[at] = ec.encode_x(xs[32], at & 1)
        with pytest.raises(ValueError):
            h.points_from_bytes(b"".join(broken), curve)
    assert [co.affine_to_ints(curve, p) for p in h.points_from_bytes(b"".join(batch), curve)] == (want * 5)[:300]


@pytest.mark.parametrize("cid", ec.FIELDS)
def test_blake2b_block_boundaries(cid):
    """h.hash_to_curve == the oracle for every prefix length 0 .. 64 at message lengths 0 and 64 (b1 and b2 hash 127, 128 and 129
    bytes at three of them) and for b0 inputs of 255, 256 and 257 bytes at six prefix / message splits each; bytes differ by position."""
    curve = CURVE[cid]
    cases, _ = ec.blake_cases(cid)
    assert {127, 128, 129} <= {ec.b1_len(cid, p) for p, _ in cases} and {255, 256, 257} <= {ec.b0_len(cid, p, msg) for p, msg in cases}
    for prefix, msg in cases:
        got = co.affine_to_ints(curve, h.hash_to_curve(curve, prefix, [msg])[0])
        assert got == oh.hash_to_curve(cid, prefix)(msg), (prefix, len(msg), ec.b0_len(cid, prefix, msg), ec.b1_len(cid, prefix))
