"""The crafted operands of tests/field_edge_cases.py reach what they claim.  A step-by-step integer replica of the plain C++ of csrc/field.cuh
and csrc/field9.cuh (word by word, with the carries and selects the sources spell) reports the events a lane goes through; the lists must
reach every one, the replica must agree with plain big integers on every case, and six deliberately wrong replicas must each be caught by
a crafted case.  The constants the case module mirrors are read from the headers.  No GPU: this keeps tests/test_gpu_field_edges.py from
silently covering less."""
import os
import re

import pytest

import field_edge_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo2_amd", "csrc")
M29, M32 = ec.M29, ec.M32


class Replica:
    """field.cuh / field9.cuh on Python integers, one statement of the source per statement here.  `mutant` names one deliberate defect."""

    def __init__(self, field, mutant=None):
        self.field, self.mutant, self.ev = field, mutant, set()
        self.p, self.p2 = ec.words8(ec.P[field]), ec.words8(2 * ec.P[field])
        self.pk = [ec.limbs9(ec.P[field] << sh) for sh in range(5)]
        self.p16 = ec.limbs9(16 * ec.P[field])

    # ---- 8 x 32 ----
    def _sub(self, a, b, tag):
        d, br, run = [], 0, 0
        for i in range(8):
            t = a[i] - b[i] - br
            d.append(t & M32)
            br = 1 if t < 0 else 0
            if br:
                self.ev.add((tag, "borrow", i))
                run += 1
        if run == 8:
            self.ev.add((tag, "one borrow through all eight limbs"))
        return d, br

    def _add(self, a, b, tag):
        s, c, run = [], 0, 0
        for i in range(8):
            t = a[i] + b[i] + c
            s.append(t & M32)
            c = t >> 32
            if c:
                self.ev.add((tag, "carry", i))
                run += i < 7
        if run == 7:
            self.ev.add((tag, "one carry out of limbs 0 .. 6"))
        return s, c

    def reduce_once(self, a, tag="reduce_once"):
        d, br = self._sub(a, self.p, tag + ".sub")
        if self.mutant == "reduce_once_gt" and not any(d):
            br = 1                                                   # `>` in place of `>=`
        v = sum(w << (32 * i) for i, w in enumerate(a)) - ec.P[self.field]
        self.ev.add((tag, "kept" if br else "subtracted"))
        if v in (0, -1):
            self.ev.add((tag, "at p" if v == 0 else "at p - 1"))
        if v == ec.P[self.field] - 1:
            self.ev.add((tag, "at 2p - 1"))
        return a if br else d

    def add(self, a, b):
        s, _ = self._add(a, b, "add")
        return self.reduce_once(s, "add.reduce")

    def sub(self, a, b):
        d, br = self._sub(a, b, "sub")
        self.ev.add(("sub", "borrowed" if br else "clean"))
        if d == [0] * 8 or d == [M32] * 8:
            self.ev.add(("sub", "difference 0" if not br else "difference -1"))
        r, _ = self._add(d, [w if br else 0 for w in self.p], "sub.addback")
        return r

    def redc(self, a):
        t = list(a)
        nonzero_so_far = True
        for step in range(8):
            m = (-t[0]) & M32
            if t[0] == 0 and nonzero_so_far:
                self.ev.add(("redc", "zero low word first at step", step))
            nonzero_so_far = nonzero_so_far and t[0] != 0
            acc = 0 if self.mutant == "redc_no_carry" else 1 if self.mutant == "redc_carry_always" else int(t[0] != 0)
            acc += t[1] + m * self.p[1]; t[0] = acc & M32; acc >>= 32
            acc += t[2] + m * self.p[2]; t[1] = acc & M32; acc >>= 32
            acc += t[3] + m * self.p[3]; t[2] = acc & M32; acc >>= 32
            acc += t[4]; t[3] = acc & M32; acc >>= 32
            acc += t[5]; t[4] = acc & M32; acc >>= 32
            acc += t[6]; t[5] = acc & M32; acc >>= 32
            acc += t[7] + (m << 30); t[6] = acc & M32
            t[7] = (acc >> 32) & M32
            assert acc >> 64 == 0
        return self.reduce_once(t, "redc.reduce")

    def mul_c(self, a, b):
        t = [0] * 9
        for i in range(8):
            c = 0
            for j in range(8):
                c = a[j] * b[i] + t[j] + (c >> 32)
                assert c >> 64 == 0
                t[j] = c & M32
            t[8] = c >> 32
            m = (-t[0]) & M32
            k = int(t[0] != 0)
            if not k:
                self.ev.add(("mul_c", "zero low word at row", i))
                if any(t):
                    self.ev.add(("mul_c", "zero low word under a nonzero value at row", i))
            c = m * self.p[1] + t[1] + k; t[0] = c & M32
            c = m * self.p[2] + t[2] + (c >> 32); t[1] = c & M32
            c = m * self.p[3] + t[3] + (c >> 32); t[2] = c & M32
            c = t[4] + (c >> 32); t[3] = c & M32
            c = t[5] + (c >> 32); t[4] = c & M32
            c = t[6] + (c >> 32); t[5] = c & M32
            c = (m << 30) + t[7] + (c >> 32); t[6] = c & M32
            c = t[8] + (c >> 32); t[7] = c & M32
            assert c >> 32 == 0
        return self.reduce_once(t[:8], "mul_c.reduce")

    def sub_lazy(self, a, b_in):
        b, rounds = list(b_in), 0
        while b[7] >> 31 and self.mutant != "sub_lazy_no_loop":
            b = self.reduce_once(b, "sub_lazy.loop")
            rounds += 1
        self.ev.add(("sub_lazy", "loop rounds", rounds))
        d, br = self._sub(a, b, "sub_lazy")
        self.ev.add(("sub_lazy", "borrowed" if br else "clean"))
        r, _ = self._add(d, [w if br else 0 for w in self.p2], "sub_lazy.addback")
        return r

    def add_lazy(self, a, b):
        s, c = self._add(a, b, "add_lazy")
        d, br = self._sub(s, self.p2, "add_lazy.sub")
        if c:
            self.ev.add(("add_lazy", "carry out of limb 7"))
        take = br == 0 if self.mutant == "add_lazy_no_carry" else (c != 0 or br == 0)
        v = sum(w << (32 * i) for i, w in enumerate(s)) + (c << 256) - 2 * ec.P[self.field]
        self.ev.add(("add_lazy", "subtracted" if take else "kept"))
        if v in (0, -1):
            self.ev.add(("add_lazy", "at 2p" if v == 0 else "at 2p - 1"))
        return d if take else s

    def is_zero_lazy(self, a):
        z = e1 = e2 = 0
        for i in range(8):
            z |= a[i]
            e1 |= a[i] ^ self.p[i]
            e2 |= a[i] ^ self.p2[i]
        self.ev.add(("is_zero_lazy", "0" if z == 0 else "p" if e1 == 0 else "2p" if e2 == 0 else "no"))
        return int(z == 0 or e1 == 0 or e2 == 0)

    # ---- 9 x 29 ----
    def norm9(self, a, tag="norm9"):
        r, c = [], 0
        for i in range(8):
            t = a[i] + c
            assert -(1 << 31) <= t < (1 << 31), "int32 overflow in the carry pass"
            r.append(t & M29)
            c = t >> 29
            if c:
                self.ev.add((tag, "carry" if c > 0 else "borrow", i))
        assert -(1 << 31) <= a[8] + c < (1 << 31)
        return r + [a[8] + c]

    def quadruple_norm9(self, a):
        r, c = [], 0
        for i in range(8):
            t = (((a[i] & M32) << 2) & M32) + c
            assert t <= M32
            r.append(t & M29)
            c = t >> 29
        return r + [a[8] * 4 + c]

    def unpack9(self, a):
        r = []
        for i in range(9):
            bit = 29 * i
            w, s = bit >> 5, bit & 31
            lo = a[w] >> s
            if s > 3 and w + 1 < 8:
                lo |= (a[w + 1] << (32 - s)) & M32
                self.ev.add(("unpack9", "straddles words", w))
            r.append(lo & M29)
        return r

    def pack9(self, a):
        r = []
        for w in range(8):
            x = 0
            for i in range(9):
                lo = 29 * i - 32 * w
                if -29 < lo < 32:
                    u = a[i] & M32
                    x |= (u << lo) & M32 if lo >= 0 else u >> (-lo)
            r.append(x)
        return r

    def canonical9(self, a):
        t = self.norm9([x + y for x, y in zip(a, self.p16)], "canonical9.norm")
        for sh in range(4, -1, -1):
            d = self.norm9([x - y for x, y in zip(t, self.pk[sh])], "canonical9.sub")
            gap = ec.value9(t) - (ec.P[self.field] << sh)
            self.ev.add(("canonical9", sh, "subtracted" if d[8] >= 0 else "kept"))
            if gap in (0, -1):
                self.ev.add(("canonical9", sh, "at the boundary" if gap == 0 else "one below"))
            if d[8] >= 0:
                t = d
        return self.pack9(t)

    def canonical_small9(self, a):
        t = self.norm9([x + y for x, y in zip(a, self.pk[0])], "small9.norm")
        for rep in range(1 if self.mutant == "small9_one_subtraction" else 2):
            d = self.norm9([x - y for x, y in zip(t, self.pk[0])], "small9.sub")
            gap = ec.value9(t) - ec.P[self.field]
            self.ev.add(("canonical_small9", rep, "subtracted" if d[8] >= 0 else "kept"))
            if gap in (0, -1):
                self.ev.add(("canonical_small9", rep, "at the boundary" if gap == 0 else "one below"))
            if d[8] >= 0:
                t = d
        return self.pack9(t)

    # ---- one driver mode on one case; None for the modes the generated statements or field_inv.cuh carry ----
    def apply(self, mode, case):
        w = [ec.words8(x) if isinstance(x, int) else x for x in case]
        val = lambda words: sum(x << (32 * i) for i, x in enumerate(words))
        if mode == "reduce_once":
            return val(self.reduce_once(w[0]))
        if mode == "add":
            return val(self.add(w[0], w[1]))
        if mode == "dbl":
            return val(self.add(w[0], w[0]))
        if mode == "sub":
            return val(self.sub(w[0], w[1]))
        if mode == "neg":
            return val(self.sub([0] * 8, w[0]))
        if mode == "redc":
            return val(self.redc(w[0]))
        if mode == "mul_c":
            return val(self.mul_c(w[0], w[1]))
        if mode == "sub_lazy":
            return val(self.sub_lazy(w[0], w[1]))
        if mode == "add_lazy":
            return val(self.add_lazy(w[0], w[1]))
        if mode == "reduce_lazy":
            return val(self.reduce_once(self.reduce_once(w[0], "reduce_lazy.1"), "reduce_lazy.2"))
        if mode == "is_zero_lazy":
            return self.is_zero_lazy(w[0])
        if mode == "norm9":
            return self.norm9(w[0])
        if mode == "quadruple_norm9":
            return self.quadruple_norm9(w[0])
        if mode == "unpack9":
            return self.unpack9(w[0])
        if mode == "pack9":
            return val(self.pack9(w[0]))
        if mode == "canonical9":
            return val(self.canonical9(w[0]))
        if mode == "canonical_small9":
            return val(self.canonical_small9(w[0]))
        if mode == "is_zero9":
            near = ((w[0][0] + 16) & M29) <= 32
            return int(near and val(self.canonical9(w[0])) == 0)
        return None


REPLICA_MODES = ("reduce_once", "add", "dbl", "sub", "neg", "redc", "mul_c", "sub_lazy", "add_lazy", "reduce_lazy", "is_zero_lazy", "norm9",
                 "quadruple_norm9", "unpack9", "pack9", "canonical9", "canonical_small9", "is_zero9")
# mutant -> the mode whose crafted list has to catch it.  REDC "without the (t[0] != 0) carry" is read both ways: the carry never added
# (wrong on every word with a nonzero low word) and the carry always added (wrong only where a low word is zero)
MUTANTS = {"redc_no_carry": "redc", "redc_carry_always": "redc", "reduce_once_gt": "reduce_once", "add_lazy_no_carry": "add_lazy", "sub_lazy_no_loop": "sub_lazy",
           "small9_one_subtraction": "canonical_small9"}


def crafted(mode, field):
    """the crafted cases of a mode: what the grouped order repeats, one of each"""
    return ec.runs(mode, field)["grouped"][::ec.WAVE]


@pytest.fixture(scope="module", params=ec.FIELDS)
def replayed(request):
    """the replica over every case of every mode it covers, once per field: (field, events)"""
    field = request.param
    rep = Replica(field)
    for mode in REPLICA_MODES:
        for case in ec.runs(mode, field)["interleaved"]:
            got = rep.apply(mode, case)
            assert ec.judge(mode, field, case, got) is None, (mode, case, got, ec.judge(mode, field, case, got))
    return field, rep.ev


def test_the_replica_equals_big_integer_truth_and_the_orders_hold_the_same_cases(replayed):
    """(the fixture asserts the first half.)  Every grouped lane is an interleaved case too, in whole waves of one case."""
    field, _ = replayed
    for mode in ec.MODES:
        run = ec.runs(mode, field)
        inter = {ec._key(c) for c in run["interleaved"]}
        assert len(run["grouped"]) % ec.WAVE == 0 and run["grouped"]
        for i in range(0, len(run["grouped"]), ec.WAVE):
            wave = run["grouped"][i:i + ec.WAVE]
            assert all(c == wave[0] for c in wave) and ec._key(wave[0]) in inter


def test_every_reduction_step_meets_a_zero_low_word(replayed):
    _, ev = replayed
    for s in range(8):
        assert ("redc", "zero low word first at step", s) in ev             # nonzero at every earlier step
        assert ("mul_c", "zero low word under a nonzero value at row", s) in ev


def test_every_conditional_subtraction_goes_both_ways_at_its_boundary(replayed):
    _, ev = replayed
    for tag in ("reduce_once", "add.reduce", "redc.reduce", "mul_c.reduce", "reduce_lazy.1", "reduce_lazy.2"):
        assert (tag, "kept") in ev and (tag, "subtracted") in ev, tag
    # exactly p and p - 1 where the operation can produce them: a product of canonical operands never equals p before its subtraction
    # (p would divide a b), so mul_c only has the two sides
    for tag in ("reduce_once", "add.reduce", "redc.reduce", "reduce_lazy.2"):
        assert (tag, "at p") in ev and (tag, "at p - 1") in ev, tag
    assert ("reduce_once", "at 2p - 1") in ev
    assert {("sub", "borrowed"), ("sub", "clean"), ("sub", "difference 0"), ("sub", "difference -1")} <= ev
    assert {("add_lazy", "kept"), ("add_lazy", "subtracted"), ("add_lazy", "at 2p"), ("add_lazy", "at 2p - 1"), ("add_lazy", "carry out of limb 7")} <= ev
    assert {("sub_lazy", "borrowed"), ("sub_lazy", "clean"), ("sub_lazy", "loop rounds", 0), ("sub_lazy", "loop rounds", 1)} <= ev
    assert {("is_zero_lazy", k) for k in ("0", "p", "2p", "no")} <= ev
    for sh in range(5):
        assert {("canonical9", sh, k) for k in ("subtracted", "kept", "at the boundary", "one below")} <= ev, sh
    for rep in range(2):
        assert {("canonical_small9", rep, k) for k in ("subtracted", "kept", "at the boundary", "one below")} <= ev, rep


def test_a_carry_and_a_borrow_cross_every_limb_boundary(replayed):
    _, ev = replayed
    for i in range(7):
        assert ("add", "carry", i) in ev and ("sub", "borrow", i) in ev and ("add_lazy", "carry", i) in ev and ("sub_lazy", "borrow", i) in ev, i
        assert ("norm9", "carry", i) in ev and ("norm9", "borrow", i) in ev, i
    assert {("sub", "one borrow through all eight limbs"), ("sub_lazy", "one borrow through all eight limbs"), ("add", "one carry out of limbs 0 .. 6"),
            ("add_lazy", "one carry out of limbs 0 .. 6")} <= ev
    assert ("sub", "borrow", 7) in ev and ("norm9", "carry", 7) in ev and ("norm9", "borrow", 7) in ev
    for w in range(7):
        assert ("unpack9", "straddles words", w) in ev


def run_mutant(field, mutant, mode, cases):
    """the number of cases on which the mutated replica differs from big-integer truth"""
    rep = Replica(field, mutant)
    return sum(ec.judge(mode, field, case, rep.apply(mode, case)) is not None for case in cases)


@pytest.mark.parametrize("field", ec.FIELDS)
@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_each_mutant_is_caught_by_a_crafted_case(field, mutant):
    mode = MUTANTS[mutant]
    assert run_mutant(field, mutant, mode, crafted(mode, field)) > 0
    assert run_mutant(field, None, mode, crafted(mode, field)) == 0


def test_what_the_random_operands_of_field_check_catch(capsys):
    """Documents the gap, whichever way it comes out: the same mutants over the 2^14 random pairs (and five edges) tests/native/field_check.hip
    runs per field, as operands of the same functions.  Printed, not asserted."""
    from oracle import c_oracle as co
    lines = []
    for field in ec.FIELDS:
        p, n = ec.P[field], 1 << 14
        ints = lambda rows: [int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192 for r in rows]
        a, b = ints(co.random_field(field, 11 + field, n)), ints(co.random_field(field, 23 + field, n))
        a[0], a[1], a[2], b[2], a[3], a[4], b[4] = 0, 1, p - 1, p - 1, b[3], 1, p - 1
        pairs = list(zip(a, b))
        for mutant, mode in sorted(MUTANTS.items()):
            if mode == "canonical_small9":                           # field_check reaches it through fe9_to_r256: a product by 2^256 mod p
                k, pinv = ec.R % p, pow(p, -1, ec.R9)
                cases = [(ec.limbs9((x * k + (-x * k * pinv) % ec.R9 * p) >> 261),) for x in a[:4096]]
            elif len(ec.MODES[mode][0]) == 1:
                cases = [(x,) for x in a]
            else:
                cases = pairs
            lines.append(f"field {field} mutant {mutant}: {run_mutant(field, mutant, mode, cases)} of {len(cases)} random cases differ")
    with capsys.disabled():
        print("\n" + "\n".join(lines))


# ---- the constants this module mirrors, read from the headers ------------------------------------------------------------------------
def _source(name):
    return open(os.path.join(CSRC, name)).read()


def _braces(text, anchor, field, count):
    """the `count` integers of the initialiser for `field` after `anchor` (FP first, FQ second)"""
    at = text.index(anchor)
    lists = re.findall(r"\{\{?([0-9a-fA-Fxu, ]+)\}\}?", text[at:at + 1200])
    lists = [[int(x.strip().rstrip("u"), 0) for x in body.split(",")] for body in lists if body.count(",") == count - 1]
    return lists[field]


@pytest.mark.parametrize("field", ec.FIELDS)
def test_constants_match_the_headers(field):
    p = ec.P[field]
    src, consts = _source("field.cuh"), _source("field9_consts.inc")
    name = ("FP", "FQ")[field]
    limbs = dict(re.findall(r"(P[123]) = (0x[0-9a-f]+)u", re.search(rf"struct Mod<{name}> \{{(.*?)\}};", src, re.S).group(1)))
    p7 = int(re.search(r"P7 = (0x[0-9a-f]+)u", src).group(1), 16)
    assert ec.words8(p) == [1, int(limbs["P1"], 16), int(limbs["P2"], 16), int(limbs["P3"], 16), 0, 0, 0, p7]
    assert _braces(src, "fe fe_one()", field, 8) == ec.words8(ec.R % p)
    assert _braces(src, "fe fe_r2()", field, 8) == ec.words8(ec.R * ec.R % p)
    assert _braces(src, "u32 mod2_limb(int i)", field, 8) == ec.words8(2 * p)
    mod9 = dict(re.findall(r"(P[1234]) = (0x[0-9a-f]+)", re.search(rf"struct Mod9<{name}> \{{(.*?)\}};", consts, re.S).group(1)))
    assert re.search(r"P9_8 = 1 << 22;", _source("field9.cuh"))
    assert ec.limbs9(p) == [1] + [int(mod9[k], 16) for k in ("P1", "P2", "P3", "P4")] + [0, 0, 0, 1 << 22]
    assert _braces(consts, "fe9 fe9_k_in()", field, 9) == ec.limbs9((1 << 266) % p)
    assert _braces(consts, "fe9 fe9_k_out()", field, 9) == ec.limbs9(ec.R % p)
    assert _braces(consts, "fe9 fe9_one()", field, 9) == ec.limbs9(ec.R9 % p)
    assert _braces(consts, "fe9 fe9_p16()", field, 9) == ec.limbs9(16 * p)
    for sh in range(5):
        anchor = f"if (sh == {sh})" if sh else "if (sh == 1)"
        got = _braces(consts[consts.index(anchor):], "return", field + (2 if sh == 0 else 0), 9)
        assert got == ec.limbs9(p << sh), sh


def test_every_mode_has_a_list_inside_its_contract():
    for field in ec.FIELDS:
        p = ec.P[field]
        for mode, (kinds, _) in ec.MODES.items():
            run = ec.runs(mode, field)
            assert run["interleaved"] and all(len(c) == len(kinds) for c in run["interleaved"]), mode
            assert len(ec.encode(mode, run["interleaved"])) == len(run["interleaved"]) * 4 * sum(ec.KIND_WORDS[k] for k in kinds)
        for mode in ("mul", "mul_c", "add", "sub", "sqr", "to_mont", "neg", "dbl", "inv", "modinv30"):
            assert all(0 <= x < p for c in ec.runs(mode, field)["interleaved"] for x in c), mode
        assert len(ec.pair_palette(field)) >= 120 and 1000 <= len(ec.inversion_values(field)) <= 1300
        for k in range(255):
            assert {1 << k, (1 << k) - 1, (1 << k) + 1, p - (1 << k)} <= set(ec.inversion_values(field))
