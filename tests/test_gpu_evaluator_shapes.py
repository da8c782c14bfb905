"""The evaluation kernel `ev_run` (h2_evaluate_device) and the MockProver's copy of its stack, `mp_check` (h2_check_expressions_device), on
every case of tests/evaluator_cases.py: every opcode at every stack depth, rotations that wrap at len/2, len - step, len and across
workgroup boundaries, the field's extreme values, LINEAR at every length and under two roots of unity, late constants, launches back to
back and on two streams, and everything the C ABI refuses.  All 2^log_len outputs are compared as limbs with the integer interpreter of
tests/evaluator_model.py -- field arithmetic is exact, so there is no sampling and no tolerance.  tests/test_evaluator_case_coverage.py
proves on the CPU what these runs reach.  Runs only on a real MI355X (`-m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import evaluator_cases as ec
import evaluator_model as em
import halo2_amd as h
from halo2_amd import _lib, fields
from halo2_amd.evaluator import EXTENDED, LAGRANGE, LateConstant, new_evaluator

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELD_IDS = {h.FP: "fp", h.FQ: "fq"}
fields_param = pytest.mark.parametrize("field", ec.FIELDS, ids=lambda f: FIELD_IDS[f])
MARKER = 0x5A5A5A5A5A5A5A5A


def _upload(ints, field):
    return torch.from_numpy(fields.to_limbs(ints, field, True).view(np.int64)).cuda()


def _same(tensor, ints, field):
    """The device vector holds exactly these integers (compared as Montgomery limbs)."""
    return np.array_equal(tensor.cpu().numpy().view(np.uint64), fields.to_limbs(ints, field, True))


def _first_difference(tensor, ints, field):
    got = fields.from_limbs(tensor.cpu().numpy().view(np.uint64), field, True)
    bad = [i for i, (g, w) in enumerate(zip(got, ints)) if g != w]
    return f"{len(bad)} of {len(ints)} elements differ, first at {bad[:8]}"


def _launch(field, basis, words, consts, tensors, log_len, omega, out, stream=None, keep=None, n_words=None, null_poly=None):
    """h2_evaluate_device on integers: returns the status.  Nothing synchronises; `keep` receives the host arrays, which the caller holds
    on to until it has synchronised."""
    limb_field = field if field in fields.MODULUS else h.FP                 # a refused field still needs well-formed arrays
    m = fields.MODULUS[limb_field]
    prog = (C.c_uint32 * len(words))(*words)
    cst = np.ascontiguousarray(fields.to_limbs([c % m for c in consts] or [0], limb_field, True))
    ptrs = (C.c_void_p * max(1, len(tensors)))(*[None if i == null_poly else t.data_ptr() for i, t in enumerate(tensors)])
    om = fields.scalar_limbs(omega, limb_field, True) if omega is not None else None
    st = C.c_void_p((stream if stream is not None else torch.cuda.current_stream()).cuda_stream)
    if keep is not None:
        keep += [prog, cst, ptrs, om]
    return h.lib().h2_evaluate_device(field, basis, prog, len(words) if n_words is None else n_words, cst.ctypes.data_as(_lib.u64p), len(consts), ptrs,
                                      len(tensors), log_len, om.ctypes.data_as(_lib.u64p) if om is not None else None, out.data_ptr(), st)


def _launch_case(mat, tensors, out, stream=None, keep=None):
    return _launch(mat.field, mat.case.basis, mat.words, mat.consts, tensors, mat.case.log_len, mat.omega, out, stream, keep)


@fields_param
@pytest.mark.parametrize("case", ec.CASES, ids=repr)
def test_case_matches_the_integer_model(case, field):
    mat = ec.materialize(case, field)
    tensors = [_upload(p, field) for p in mat.polys]
    if case.is_ast:                                        # through EvaluationDomain / Evaluator: compile and run as create_proof does
        ev = new_evaluator(case.basis)
        leaves = [ev.register_poly(t) for t in tensors]
        out = ev.evaluate(case.build(leaves)[0], mat.dom)
    else:
        out = torch.empty_like(tensors[0])
        keep = []
        assert _launch_case(mat, tensors, out, keep=keep) == _lib.H2_OK
        torch.cuda.synchronize()
    assert out.shape == (mat.n, 4)
    assert _same(out, mat.values, field), _first_difference(out, mat.values, field)


@fields_param
@pytest.mark.parametrize("basis", [LAGRANGE, EXTENDED], ids=lambda b: ec.BASIS_NAME[b])
def test_two_roots_of_unity_back_to_back(basis, field):
    """omega, omega^3 and omega again at one length on one stream with nothing between the launches: the twiddle cache is keyed by the root,
    so each result follows its own."""
    a, b = (ec.materialize(ec.BY_NAME[f"roots-{ec.BASIS_NAME[basis]}-L9-w{p}"], field) for p in (1, 3))
    tensors = {id(mat): [_upload(p, field) for p in mat.polys] for mat in (a, b)}
    outs = [torch.empty((a.n, 4), dtype=torch.int64, device="cuda") for _ in range(3)]
    keep = []
    for mat, out in zip((a, b, a), outs):
        assert _launch_case(mat, tensors[id(mat)], out, keep=keep) == _lib.H2_OK
    torch.cuda.synchronize()
    for mat, out in zip((a, b, a), outs):
        assert _same(out, mat.values, field), (mat.case, _first_difference(out, mat.values, field))


@fields_param
@pytest.mark.parametrize("name", [c[0] for c in ec.LATE_CASES])
def test_late_constants_follow_their_own_run(name, field):
    """Evaluator.compile once with a LateConstant base, Evaluator.run twice with two values and no synchronisation between the launches:
    the constant table is staged in stream order, so each output belongs to its own y.  An empty expression list folds to 0 whatever y is."""
    late = ec.materialize_late(name, field)
    ev = new_evaluator(late.basis)
    leaves = [ev.register_poly(_upload(p, field)) for p in late.polys]
    slot = LateConstant()
    compiled = ev.compile(late.build(leaves, slot)[0], late.dom)
    assert (slot.index is not None) == late.slot_used
    outs = [ev.run(compiled, late.dom, {slot: y}) for y in ec.LATE_YS]
    torch.cuda.synchronize()
    for out, want in zip(outs, late.values):
        assert _same(out, want, field), _first_difference(out, want, field)


@fields_param
def test_two_programs_back_to_back_and_on_two_streams(field):
    a, b = (ec.materialize(ec.BY_NAME[name], field) for name in ec.BACK_TO_BACK)
    ta, tb = [_upload(p, field) for p in a.polys], [_upload(p, field) for p in b.polys]
    outs = [torch.empty_like(ta[0]) for _ in range(8)]
    torch.cuda.synchronize()                               # the uploads and allocations are done before another stream reads them
    keep = []
    order = [(a, ta), (b, tb), (b, tb), (a, ta)]
    for (mat, tensors), out in zip(order, outs[:4]):       # one stream: the staging buffers of the stream's context are reused at once
        assert _launch_case(mat, tensors, out, keep=keep) == _lib.H2_OK
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for (mat, tensors), out, stream in zip(order, outs[4:], (s1, s2, s1, s2)):     # two streams: a context each
        assert _launch_case(mat, tensors, out, stream=stream, keep=keep) == _lib.H2_OK
    torch.cuda.synchronize()
    for (mat, _), out in zip(order + order, outs):
        assert _same(out, mat.values, field), (mat.case, _first_difference(out, mat.values, field))


@pytest.mark.parametrize("name", [name for name, _ in ec.REFUSALS])
def test_refused_calls_touch_nothing(name):
    """H2_ERR_ARGS, and the output vector still holds its marker after a synchronise: nothing was launched."""
    a = dict(ec.REFUSAL_BASE, **dict(ec.REFUSALS)[name])
    n = 1 << a["log_len"]
    words = a["words"]
    if words == "2^20+1":
        words = [ec.word(ec.CONST, 0)] + [ec.word(ec.SCALE, 0)] * (1 << 20)
        assert len(words) == (1 << 20) + 1
    field_ok = a["field"] if a["field"] in ec.FIELDS else h.FP
    tensors = [_upload(list(range(1, n + 1)), field_ok), _upload(list(range(n, 2 * n)), field_ok)]
    out = torch.full((n, 4), MARKER, dtype=torch.int64, device="cuda")
    keep = []
    rc = _launch(a["field"], a["basis"], words, [5], tensors, a["log_len"], 1 if a["omega"] else None, out, keep=keep,
                 n_words=a["n_words"], null_poly=a["null_poly"])
    assert rc == _lib.H2_ERR_ARGS
    torch.cuda.synchronize()
    assert bool((out == MARKER).all())


def test_the_ten_slot_tree_stays_refused_and_the_nine_slot_tree_runs():
    field = h.FP
    dom = h.EvaluationDomain(3, 6, field)
    m, n = dom.m, dom.n
    polys = [ec.poly_values(("random", i), n, m, "full") for i in range(4)]
    ev = new_evaluator(LAGRANGE)
    leaves = [ev.register_poly(_upload(p, field)) for p in polys]
    count = [0]

    def full(depth):                                       # a complete binary tree needs depth + 1 slots; every leaf another (polynomial, rotation)
        if depth == 0:
            count[0] += 1
            i, rot = count[0] % 4, count[0] // 4 % n
            return ec.Ast.of(leaves[i].with_rotation(rot)), polys[i][rot:] + polys[i][:rot]
        (a, va), (b, vb) = full(depth - 1), full(depth - 1)
        return (a + b, [(x + y) % m for x, y in zip(va, vb)]) if depth % 2 else (a * b, [x * y % m for x, y in zip(va, vb)])
    with pytest.raises(ValueError):
        ev.evaluate(full(9)[0], dom)
    count[0] = 0
    ast, want = full(8)
    out = ev.evaluate(ast, dom)
    assert _same(out, want, field), _first_difference(out, want, field)


def _planes(tensor, n):
    """(programs, n) array of bits from (programs, n / 64) words: row r is bit r % 64 of word r / 64."""
    words = tensor.cpu().numpy().view(np.uint64)
    return np.array([[(int(w[r >> 6]) >> (r & 63)) & 1 for r in range(n)] for w in words], dtype=np.uint8)


def _check_expressions(field, programs, offsets, consts, tensors, advice, log_len, usable):
    n, n_programs, vp = 1 << log_len, len(offsets) - 1, C.c_void_p
    nz = torch.full((n_programs, n // 64), -1, dtype=torch.int64, device="cuda")
    po = torch.full((n_programs, n // 64), -1, dtype=torch.int64, device="cuda")
    counts = torch.full((2 * n_programs,), -1, dtype=torch.int32, device="cuda")
    values = torch.full((n_programs, n, 4), MARKER, dtype=torch.int64, device="cuda")
    cst = np.ascontiguousarray(fields.to_limbs(consts, field, True))
    rc = h.lib().h2_check_expressions_device(field, (C.c_uint32 * len(programs))(*programs), (C.c_size_t * len(offsets))(*offsets), n_programs,
                                             cst.ctypes.data_as(_lib.u64p), len(consts), (vp * len(tensors))(*[t.data_ptr() for t in tensors]),
                                             (C.c_uint8 * len(tensors))(*[1 if i in advice else 0 for i in range(len(tensors))]), len(tensors),
                                             log_len, usable, nz.data_ptr(), po.data_ptr(), counts.data_ptr(),
                                             (vp * n_programs)(*[values[p].data_ptr() for p in range(n_programs)]), None)
    assert rc == _lib.H2_OK
    torch.cuda.synchronize()
    return _planes(nz, n), _planes(po, n), counts.cpu().tolist(), values


@fields_param
def test_mock_prover_takes_a_rotation_by_the_whole_length(field):
    """|shift| == len is the identity in `mp_check` as in `ev_run`, for the value and for the row the poison rule looks at."""
    log_len, n, m = ec.MOCK_LOG_LEN, 1 << ec.MOCK_LOG_LEN, fields.MODULUS[field]
    polys = [ec.poly_values(("random", i), n, m, "whole-length") for i in range(2)]
    program = [ec.word(ec.POLY, 0), ec.u32(n), ec.word(ec.POLY, 1), ec.u32(-n), ec.word(ec.MUL), ec.word(ec.POLY, 0), ec.u32(1 - n), ec.word(ec.ADD)]
    usable = n - ec.MOCK_UNUSABLE
    want, _ = em.interpret(program, [], polys, LAGRANGE, n, m, None, advice={0}, usable=usable)
    assert want == [None if r >= usable - 1 else (polys[0][r] * polys[1][r] + polys[0][r + 1]) % m for r in range(n)]
    nz, po, counts, values = _check_expressions(field, program, [0, len(program)], [], [_upload(p, field) for p in polys], {0}, log_len, usable)
    assert po[0].tolist() == [1 if v is em.POISON else 0 for v in want] and nz[0].tolist() == [1 if v else 0 for v in want]
    assert counts == [sum(1 for v in want if v), ec.MOCK_UNUSABLE + 1]
    assert _same(values[0], [v or 0 for v in want], field)


@fields_param
@pytest.mark.parametrize("poisoned", [False, True], ids=["plain", "poisoned"])
def test_mock_prover_stack_matches_the_evaluator_and_the_poison_model(field, poisoned):
    """The deep-stack programs without LINEAR, three in one launch of `mp_check` in storing mode at 2^9.  With no advice column the stored
    values are the evaluator's output bit for bit, the non-zero plane is `value != 0` and the counts are the planes' popcounts; with
    two advice columns and 37 unusable rows, planes, counts and values (0 where poisoned) are those of the poison-carrying model, whose
    runs put Poison into every spilled level (tests/test_evaluator_case_coverage.py)."""
    programs, offsets, consts, polys = ec.mock_programs(field)
    log_len, n = ec.MOCK_LOG_LEN, 1 << ec.MOCK_LOG_LEN
    tensors = [_upload(p, field) for p in polys]
    model = ec.mock_model(field, poisoned)
    advice, usable = (set(ec.MOCK_ADVICE), n - ec.MOCK_UNUSABLE) if poisoned else (set(), n)
    nz, po, counts, values = _check_expressions(field, programs, offsets, consts, tensors, advice, log_len, usable)
    for p, (want, _) in enumerate(model):
        want_po = [1 if v is em.POISON else 0 for v in want]
        want_nz = [1 if v is not em.POISON and v != 0 else 0 for v in want]
        stored = [0 if v is em.POISON else v for v in want]
        assert po[p].tolist() == want_po and nz[p].tolist() == want_nz, p
        assert counts[2 * p:2 * p + 2] == [sum(want_nz), sum(want_po)] == [int(nz[p].sum()), int(po[p].sum())]
        assert _same(values[p], stored, field), (p, _first_difference(values[p], stored, field))
        if poisoned:
            assert sum(want_po) >= ec.MOCK_UNUSABLE
        else:                                              # the same words through the evaluator kernel
            out = torch.empty_like(tensors[0])
            keep = []
            assert _launch(field, LAGRANGE, programs[offsets[p]:offsets[p + 1]], consts, tensors, log_len, None, out, keep=keep) == _lib.H2_OK
            torch.cuda.synchronize()
            assert torch.equal(out, values[p]) and sum(want_po) == 0
