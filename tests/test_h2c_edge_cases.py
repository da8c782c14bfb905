"""The crafted inputs of tests/h2c_edge_cases.py are what they claim to be: every class is present in full, every element has the
2-adic order / the branch it was built for, and the expectations satisfy the curve equations.  No GPU: this is the condition that
keeps tests/test_gpu_h2c_edges.py from silently covering less."""
import pytest

import h2c_edge_cases as ec
from oracle import hash_to_curve as oh
from oracle import pasta as o

CIDS = ec.FIELDS


@pytest.mark.parametrize("cid", CIDS)
def test_sqrt_classes_are_complete_and_have_their_orders(cid):
    m, c = ec.modulus(cid), ec.sqrt_classes(cid)
    assert sorted(c["orders"]) == list(range(33))
    for j, elems in c["orders"].items():
        assert len(elems) == 4 and len(set(elems)) == 4
        for a in elems:
            assert 0 < a < m and ec.two_adic_order(a, m) == j
            flag, root = ec.sqrt_expected(a, m)
            assert flag == (1 if j <= 31 else 0)
            if flag:
                assert 0 <= root < m and root * root % m == a
    assert c["fixed"] == [0, 1, 4, m - 1, m - 4, 5, (1 << 256) % m] and ec.sqrt_expected(0, m) == (1, 0)
    assert ec.two_adic_order(m - 1, m) == 1 and ec.two_adic_order(1, m) == 0
    assert len(c["random"]) == 256 and len(set(c["random"])) == 256
    for a in c["fixed"] + c["random"]:
        flag, root = ec.sqrt_expected(a, m)
        assert flag == 0 or root * root % m == a
    runs = ec.sqrt_runs(cid)
    inter = runs["interleaved"]
    assert len(inter) == 132 + 7 + 256
    for w in range(0, 132, 33):                               # lanes cycle through the 33 orders: every wave of 64 holds many
        assert [ec.two_adic_order(a, m) for a in inter[w:w + 33]] == list(range(33))
    assert len(runs["grouped"]) == 132 * 64 and set(runs["grouped"]) == set(inter[:132])
    for w in range(0, 132 * 64, 64):                          # whole waves share one element
        assert len(set(runs["grouped"][w:w + 64])) == 1
    assert runs["single"] == [m - 1]


@pytest.mark.parametrize("cid", CIDS)
def test_swu_classes_and_their_expected_points(cid):
    m, c = ec.modulus(cid), ec.swu_classes(cid)
    assert c["fixed"] == [0, 1, 2, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2]
    assert len(c["square"]) == 16 and all(ec.gx1_is_square(u, cid) for u in c["square"])
    assert len(c["nonsquare"]) == 16 and not any(ec.gx1_is_square(u, cid) for u in c["nonsquare"])
    assert c["negated"] == [m - u for u in c["square"] + c["nonsquare"]] and len(c["negated"]) == 32
    assert len(c["random"]) == 128
    us = ec.swu_inputs(cid)
    assert len(us) == 7 + 16 + 16 + 32 + 128
    for u in us:
        x, y = ec.swu(u, cid)
        assert 0 <= x < m and 0 <= y < m and y * y % m == ec.iso_rhs(x, cid) and (y & 1) == (u & 1)
    # u = 0 is the only generated u with tv == 0 (1 / 13 is a non-residue, so Z u^2 = -1 has no solution)
    assert o.sqrt_mod(pow(13, -1, m), m) is None
    every_u = us + [u for run in ec.pair_runs(cid).values() for _, p in run for u in p]
    assert [u for u in every_u if ec.swu_tv(u, m) == 0] == [0] * every_u.count(0) and every_u.count(0) >= 1


@pytest.mark.parametrize("cid", CIDS)
def test_pair_classes_reach_the_branches_they_name(cid):
    m, c = ec.modulus(cid), ec.pair_classes(cid)
    assert len(c["tangent"]) == 8 and all(a == b != 0 for a, b in c["tangent"])
    assert len(c["opposite"]) == 8 and all((a + b) % m == 0 and a for a, b in c["opposite"])
    assert len(c["zero"]) == 9 and c["zero"][0] == (0, 0) and sum(a == 0 for a, _ in c["zero"]) == 5 and sum(b == 0 for _, b in c["zero"]) == 5
    assert len(c["same_x_equal_y"]) == 8 and len(c["same_x_opposite_y"]) == 8 and len(c["random"]) == 128
    z = oh.SWU_Z % m
    for kind in ("same_x_equal_y", "same_x_opposite_y"):
        for u0, u1 in c[kind]:
            q0, q1 = ec.swu(u0, cid), ec.swu(u1, cid)
            assert u1 not in (u0, m - u0) and (z * u1 * u1 + 1 + z * u0 * u0) % m == 0
            assert q0[0] == q1[0] and q0[1] != 0 and (q0[1] == q1[1]) == (kind == "same_x_equal_y")
            assert (q0[1] + q1[1]) % m == 0 or q0[1] == q1[1]
    runs = ec.pair_runs(cid)
    assert [len(runs[k]) for k in ("single", "wave63", "all")] == [1, 63, 210]
    for name in ("wave63", "all"):
        kinds = {k for k, _ in runs[name]}
        assert kinds == {"tangent", "opposite", "zero", "same_x_equal_y", "same_x_opposite_y", "random"}
    for run in runs.values():
        for kind, (u0, u1) in run:
            r = ec.pair_expected(u0, u1, cid)
            # the identity appears exactly for the opposite-y constructions
            assert (r == (0, 0)) == (kind in ec.IDENTITY_PAIR_CLASSES)
            if r != (0, 0):
                assert o.on_curve(r, m)


@pytest.mark.parametrize("cid", CIDS)
def test_add_and_iso_classes(cid):
    m, c = ec.modulus(cid), ec.add_classes(cid)
    assert len(c["self_y0"]) == 4 and len(c["opposite"]) == 8 and len(c["double"]) == 8 and len(c["distinct"]) == 23
    for case in c["self_y0"] + c["opposite"]:
        assert ec.add_expected(*case, cid) == (0, 0, 1)
    for case in c["double"] + c["distinct"]:
        assert ec.add_expected(*case, cid)[2] == 0
    assert all(x0 != x1 for x0, _, x1, _ in c["distinct"])
    for x0, y0, x1, y1 in c["distinct"][16:] + c["double"][4:]:        # the ones on the iso curve stay on it
        x3, y3, _ = ec.add_expected(x0, y0, x1, y1, cid)
        assert y3 * y3 % m == ec.iso_rhs(x3, cid)
    ic, x0 = ec.iso_classes(cid), ec.isogeny(cid)[0]
    assert len(ic["kernel"]) == 3 and all(x == x0 and ec.iso_expected(x, y, cid) == (0, 0) for x, y in ic["kernel"])
    assert [x for x, _ in ic["next_to_kernel"]] == [(x0 + 1) % m, (x0 - 1) % m]
    assert all(ec.iso_expected(x, y, cid) != (0, 0) for x, y in ic["next_to_kernel"])
    assert len(ic["on_curve"]) == 32
    for x, y in ic["on_curve"]:
        assert y * y % m == ec.iso_rhs(x, cid) and o.on_curve(ec.iso_expected(x, y, cid), m)
    # the kernel point has no rational y: d == 0 cannot be reached from a point of the iso curve
    assert o.sqrt_mod(ec.iso_rhs(x0, cid), m) is None


@pytest.mark.parametrize("cid", CIDS)
def test_decoder_xs_have_their_orders(cid):
    m, xs = ec.modulus(cid), ec.decoder_xs(cid)
    assert sorted(xs) == list(range(33))
    for j, x in xs.items():
        assert 0 < x < m and ec.two_adic_order((x * x * x + o.CURVE_B) % m, m) == j
        for sign in (0, 1):
            if j == 32:
                with pytest.raises(ValueError):
                    o.point_from_bytes(ec.encode_x(x, sign), m)
            else:
                pt = o.point_from_bytes(ec.encode_x(x, sign), m)
                assert o.on_curve(pt, m) and pt[0] == x and (pt[1] & 1) == sign


@pytest.mark.parametrize("cid", CIDS)
def test_blake_cases_sit_on_the_block_boundaries(cid):
    cases, splits = ec.blake_cases(cid)
    dl0 = 29 if cid == "pallas" else 28
    assert ec.dst_len(cid, 0) == dl0
    sweep = cases[:130]
    assert [(len(p), len(msg)) for p, msg in sweep] == [(lp, ml) for lp in range(65) for ml in (0, 64)]
    assert {127, 128, 129} <= {ec.b1_len(cid, p) for p, _ in sweep}
    first = 33 if cid == "pallas" else 34
    assert [ec.b1_len(cid, "x" * lp) for lp in (first, first + 1, first + 2)] == [127, 128, 129]
    for total, want in ((124, 255), (125, 256), (126, 257)):
        sp = splits[total]
        assert len(sp) == 6 and len({len(msg) for _, msg in sp}) == 6
        assert all(ec.b0_len(cid, p, msg) == want and len(p) <= 64 and len(msg) <= 64 for p, msg in sp)
        lens = [len(msg) for _, msg in sp]
        assert 64 in lens and min(lens) == total - dl0 - 64      # the shortest message that fits: the prefix is at its 64 bytes
    for p, msg in cases:                                       # bytes differ by position
        assert len(set(p)) == len(p) and len(set(msg)) == len(msg) and "\0" not in p
