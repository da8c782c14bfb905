"""Sinsemilla commitments and hashing from a private point on the host (no GPU): the restatement of tests/sinsemilla_commit_cases.py
checks itself; the four entries of sinsemilla_commit.hip are declared, bound and refuse bad arguments before any device work; the
`CommitDomain` gadget and the chip with `allow_init_from_private_point` are synthesized cell by cell over a CPU generator table and
host-built tables of R, evaluated with Python integers, and their constraint system is the reference's pinned one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from halo2_amd import _lib
from halo2_amd.gadgets import sinsemilla as g
from oracle import pasta as o

import ecc_cases as ec
import sinsemilla_cases as sc
import sinsemilla_commit_cases as cc
from sinsemilla_cases import P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 11
NEW_ENTRIES = ["h2_sinsemilla_hash_from_device", "h2_sinsemilla_commit_device", "h2_sinsemilla_trace_from_device", "h2_ecc_add_trace_device"]


def _on_curve(pt):
    return (pt[1] * pt[1] - pt[0] ** 3 - 5) % P == 0


# ---- 1: the restatement ----------------------------------------------------------------------------------------------------------------------
def test_the_domains_points_are_on_the_curve():
    q, r = cc.q_of(cc.PERSONALIZATION), cc.r_of(cc.PERSONALIZATION)
    assert _on_curve(q) and _on_curve(r) and q != r
    assert q == sc.q_of(sc.TEST_DOMAIN)                                       # the Q the Merkle tests already use


def test_the_crafted_qs_reach_their_targets_with_every_round_clean():
    t = cc.blind(cc.CRAFT_R)
    crafted = cc.crafted_cases()
    assert sc.hash_to_point(crafted["doubling"], cc.CRAFT_WORDS) == t
    assert sc.hash_to_point(crafted["identity"], cc.CRAFT_WORDS) == o.ec_neg(t, P)
    assert cc.commit(crafted["doubling"], cc.CRAFT_WORDS, cc.CRAFT_R) == o.ec_add(t, t, P)
    assert cc.commit(crafted["identity"], cc.CRAFT_WORDS, cc.CRAFT_R) == (0, 0)
    assert cc.commit(crafted["identity"], cc.CRAFT_WORDS, 0) == o.ec_neg(t, P)                # r = 0 leaves the hash
    _, q, m = sc.exceptional_cases()[3]
    assert cc.commit(q, m, cc.CRAFT_R) is None                                # only the hash can be bottom


def test_the_restated_witness_of_a_private_start_opens_with_y_q():
    q = cc.private_qs()[2]
    cols = cc.trace_from(q, [12345], [5])
    assert [col[0] for col in cols] == [0, q[1], 0, 0, 0] and [col[1:] for col in cols] == sc.trace(q, [12345], [5])
    assert all(len(col) == 7 for col in cols)


def test_the_restated_addition_covers_every_branch():
    rows = [cc.add_row(p, q) for p, q in cc.add_pairs(6)]
    assert [tuple(row[9:]) for row in rows] == [cc.group_add(p, q) for p, q in cc.add_pairs(6)]
    assert rows[2][9:] == [0, 0] and rows[5][4:] == [0] * 7
    assert rows[0][8] == 0 and rows[1][8] != 0 and rows[2][8] == 0          # delta only where x_q = x_p and y_q != -y_p: the doubling
    assert rows[1][9:] == list(ec.ec_mul(2, cc.add_pairs(6)[1][0]))


# ---- 2: the ABI ----------------------------------------------------------------------------------------------------------------------------
def test_the_entries_are_declared_with_the_bound_signatures():
    text = open(os.path.join(ROOT, "include", "halo2_mi355x.h")).read()
    kinds = {"const void *": C.c_void_p, "void *": C.c_void_p, "size_t": C.c_size_t, "const uint64_t *": _lib.u64p,
             "const uint32_t *": C.POINTER(C.c_uint32)}
    for name in NEW_ENTRIES:
        found = re.search(r"\bint " + name + r"\(([^)]*)\);", text)
        assert found, name
        params = [re.sub(r"\s*\w+$", "", " ".join(p.split())) for p in found.group(1).split(",")]      # the type without the name
        args, res = _lib.SIGNATURES[name]
        assert res is C.c_int and [kinds[p] for p in params] == args, (name, params)
    units = open(os.path.join(ROOT, "halo2_amd", "csrc", "Makefile")).read()
    assert "sinsemilla_commit.hip" in units.split("SRCS :=")[1].split("\n")[0]


def test_argument_validation_without_gpu():
    lib = _lib.lib()
    q = np.zeros(8, np.uint64)
    nw = (C.c_uint32 * 2)(25, 25)
    one = 0x1000                                                              # never read: every call below is refused first
    p = q.ctypes.data_as(_lib.u64p)
    commit = lib.h2_sinsemilla_commit_device
    assert commit(one, 1, 5, p, one, one, one, one, one, one, None) == _lib.H2_ERR_ARGS       # both forms of Q
    assert commit(one, 1, 5, None, None, one, one, one, one, one, None) == _lib.H2_ERR_ARGS   # neither
    assert commit(one, 1, 254, p, None, one, one, one, one, one, None) == _lib.H2_ERR_ARGS    # more than C words
    assert commit(one, (1 << 30) + 1, 5, p, None, one, one, one, one, one, None) == _lib.H2_ERR_ARGS
    assert commit(None, 1, 5, p, None, one, one, one, one, one, None) == _lib.H2_ERR_ARGS     # words without a message
    assert commit(one, 1, 5, p, None, one, None, one, one, one, None) == _lib.H2_ERR_ARGS     # no table of R
    hash_from = lib.h2_sinsemilla_hash_from_device
    assert hash_from(one, 1, 254, one, one, one, one, None) == _lib.H2_ERR_ARGS
    assert hash_from(one, 1, 5, None, one, one, one, None) == _lib.H2_ERR_ARGS                # no Q
    assert hash_from(one, (1 << 30) + 1, 5, one, one, one, one, None) == _lib.H2_ERR_ARGS
    trace = lib.h2_sinsemilla_trace_from_device
    assert trace(one, 1, None, 2, one, one, one, one, None) == _lib.H2_ERR_ARGS
    assert trace(one, 1, nw, 0, one, one, one, one, None) == _lib.H2_ERR_ARGS
    assert trace(one, 1, (C.c_uint32 * 2)(25, 26), 2, one, one, one, one, None) == _lib.H2_ERR_ARGS      # a piece of 26 words
    assert trace(one, 1, (C.c_uint32 * 11)(*[25] * 11), 11, one, one, one, one, None) == _lib.H2_ERR_ARGS      # 275 words
    assert trace(one, 1, nw, 2, None, one, one, one, None) == _lib.H2_ERR_ARGS                # no Q
    assert trace(one, (1 << 30) + 1, nw, 2, one, one, one, one, None) == _lib.H2_ERR_ARGS
    add = lib.h2_ecc_add_trace_device
    assert add(one, None, 1, one, None) == _lib.H2_ERR_ARGS and add(one, one, (1 << 30) + 1, one, None) == _lib.H2_ERR_ARGS
    if lib.h2_device_count() == 0:                                            # good arguments get as far as the missing device
        assert add(one, one, 1, one, None) == _lib.H2_ERR_NODEV
        assert commit(one, 1, 5, p, None, one, one, one, one, one, None) == _lib.H2_ERR_NODEV


# ---- 3: messages ---------------------------------------------------------------------------------------------------------------------------
class _Pieces:
    """a chip that only records what it is asked to witness"""

    def __init__(self):
        self.seen = []

    def witness_message_piece(self, layouter, field_elem, num_words):
        self.seen.append((field_elem, num_words))
        return g.MessagePiece(None, num_words)


def test_message_from_bitstring_cuts_pieces_of_25_words():
    chip = _Pieces()
    value = (1 << 499) | (0x2AB << 250) | 0x155
    message = g.Message.from_bitstring(chip, None, cc.bits_of(value, 500))
    assert [p.num_words for p in message] == [25, 25] and isinstance(message, list)
    assert chip.seen == [(value & ((1 << 250) - 1), 25), (value >> 250, 25)]
    chip = _Pieces()
    assert [p.num_words for p in g.Message.from_bitstring(chip, None, [True] * 520)] == [25, 25, 2] and chip.seen[2] == ((1 << 20) - 1, 2)
    chip = _Pieces()
    pieces = [g.MessagePiece.from_bitstring(chip, None, cc.bits_of(v, n)) for v, n in ((0, 10), (5, 250), (7, 250))]
    assert [p.num_words for p in g.Message.from_pieces(chip, pieces)] == [1, 25, 25] and chip.seen == [(0, 1), (5, 25), (7, 25)]
    assert g.MessagePiece.from_bitstring(chip, None, [None] * 20).num_words == 2 and chip.seen[-1] == (None, 2)
    with pytest.raises(AssertionError):
        g.Message.from_bitstring(chip, None, [True] * 505)                   # not whole words
    with pytest.raises(AssertionError):
        g.MessagePiece.from_bitstring(chip, None, [True] * 260)              # 26 words in one piece


# ---- 4: the gadgets ------------------------------------------------------------------------------------------------------------------------
def _mirror(**kwargs):
    return cc.MySinsemillaCircuit(cc.host_domain(), table=sc.table(), **kwargs)


def test_the_constraint_system_is_the_references():
    """every gate, lookup, query, permutation column and constant of the reference's pinned vk_sinsemilla_chip"""
    cs = sc.host_keygen_cs(_mirror(), K)
    assert cs.pinned() == sc.fixture_cs(sc.fixture_text("vk_sinsemilla_chip.rdata.gz"))
    proof = open(os.path.join(sc.GOLDEN, "proof_sinsemilla_chip.bin"), "rb").read()
    assert len(proof) == 4576


def test_with_the_flag_initial_y_q_reads_x_p_one_row_up():
    plain, flagged = sc.host_keygen_cs(_mirror(), K), sc.host_keygen_cs(_mirror(private=True), K)
    assert [gate.name for gate in plain.gates] == [gate.name for gate in flagged.gates]
    a, b = plain.pinned(), flagged.pinned()
    assert a != b and len(plain.gates) == len(flagged.gates)
    # chip 1's y_Q column, lagrange_coeffs[0], is still queried by the fixed-base gates; the flag only moves the gate's y_Q
    config = cc.configure_chips(ec.front.ConstraintSystem(P), sc.table(), True)
    assert config[1].allow_init_from_private_point and config[2].allow_init_from_private_point
    assert not cc.configure_chips(ec.front.ConstraintSystem(P), sc.table(), False)[1].allow_init_from_private_point


@pytest.mark.parametrize("private", [False, True], ids=["public-q", "private-init"])
def test_the_mirror_is_satisfied_on_the_host(private):
    """the reference's circuit with a seeded witness, both ways of configuring the chips: every gate, lookup and copy holds"""
    failures, _, _ = sc.host_failures(_mirror(seed=5, private=private), K)
    assert failures == []


def test_a_mutated_y_q_breaks_initial_y_q_and_its_copy():
    circuit = _mirror(seed=5, private=True, mutate=True)
    failures, _, _ = sc.host_failures(circuit, K)
    gates = [f for f in failures if f[0] == "gate"]
    assert gates == [("gate", "Initial y_Q", "init_y_q_check", circuit.mutated_row + 1)]
    assert [f for f in failures if f[0] != "gate"] and all(f[0] == "copy" for f in failures if f[0] != "gate")


def test_private_init_on_a_chip_without_the_flag_is_refused():
    with pytest.raises(g.IllegalHashFromPrivatePoint):
        sc.host_failures(_mirror(seed=5, private=True, flag=False), K)


def test_commit_gadget_computes_the_restatement():
    messages, scalars = [(1 << 500) - 1, 0x1234 << 300 | 99], [cc.CRAFT_R, 1]
    circuit = cc.CommitCircuit(messages, scalars, cc.host_domain(), table=sc.table())
    failures, _, _ = sc.host_failures(circuit, K)
    assert failures == []
    got = [(pt.inner().x().value().inner.evaluate(P), pt.inner().y().value().inner.evaluate(P)) for pt, _ in circuit.results]
    assert got == [cc.commit(cc.q_of(cc.PERSONALIZATION), sc.words_of([m], [50]), k) for m, k in zip(messages, scalars)]
    short = g.CommitDomain(None, None, cc.host_domain())
    assert short.q_init() == cc.q_of(cc.PERSONALIZATION)


def test_commit_many_lays_out_the_shape_of_keygen_on_the_host():
    """without a witness nothing is launched: the bulk circuit's constraint system and fixed cells come out on a machine with no GPU,
    and its three bulk regions take the rows of the per-call regions"""
    messages, scalars = [5, 6, 7], [1, 2, 3]
    bulk = cc.CommitCircuit(messages, scalars, cc.host_domain(), table=sc.table(), many=True)
    one = cc.CommitCircuit(messages, scalars, cc.host_domain(), table=sc.table())
    assert sc.host_keygen_cs(bulk, 12).pinned() == sc.host_keygen_cs(one, 12).pinned()
    sides = []
    for circuit in (one, bulk):
        _, assembly, layouter = ec.front.synthesize(circuit.without_witnesses(), 12, 0, fixed=True, advice=False)
        sides.append((assembly.host_columns(assembly.fixed), assembly.selectors, layouter))
    (fa, sa, la), (fb, sb, lb) = sides
    assert sorted(int(v) for v in sa.sum(axis=1)) == sorted(int(v) for v in sb.sum(axis=1))   # every selector on as many rows
    assert [sum(1 for v in col if v) for col in fa] == [sum(1 for v in col if v) for col in fb]


@pytest.mark.parametrize("private", [False, True], ids=["public-q", "private-q"])
def test_bulk_hashes_on_a_flagged_chip_lay_out_the_shape_of_the_calls(private):
    """keygen's view, which launches nothing: `hash_to_point_many` on a chip with the flag -- a public Q under its extra row, or one
    witnessed Q per hash -- gives the selectors, the fixed cells, the copies and the constraint system of the calls one after the other"""
    nw = sc.STRUCTURES["merkle"]
    msgs = cc.random_messages(nw, 3, seed=2)
    start = list(cc.private_qs()[:3]) if private else cc.q_of(cc.PERSONALIZATION)
    sides = []
    for bulk in (False, True):
        circuit = cc.FlaggedHashCircuit(nw, msgs, start, table=sc.table(), bulk=bulk)
        cs, assembly, _ = ec.front.synthesize(circuit.without_witnesses(), K, 0, fixed=True, advice=False)
        sides.append((assembly.selectors.copy(), assembly.host_columns(assembly.fixed), assembly.permutation.flat().copy(), cs.pinned()))
    a, b = sides
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3] == b[3]
    assert a[0].sum() >= 3 * 53                                               # q_sinsemilla1 on 52 rows and q_sinsemilla4 on one, per hash
    failures, _, _ = sc.host_failures(cc.FlaggedHashCircuit(nw, msgs, start, table=sc.table()), K)
    assert failures == []
