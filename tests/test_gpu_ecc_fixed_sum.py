"""The bulk short and base-field fixed-base multiplications on the device: both traces bit for bit against the integer model of
tests/ecc_fixed_sum_cases.py over its case list, at both counts and through a scratch that holds fewer lanes than the call has; every
refusal; stream order; `EccChip.mul_fixed_short_many`, `mul_fixed_base_field_elem_many` and `add_many` against a loop of the single
calls, cell for cell; the invalid inputs and four tampered witnesses, which must fail where the single call fails; proofs; the example."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import halo2_amd as h
from halo2_amd import _lib, dev, ecc, fields
from halo2_amd import circuit as front
from halo2_amd import verifier as hv
from halo2_amd.gadgets.ecc import FixedBaseTables
from halo2_amd.transcript import Blake2bWrite
from oracle import c_oracle as co

import ecc_cases as ec
import ecc_fixed_cases as fx
import ecc_fixed_sum_cases as fs
from ecc_fixed_sum_cases import GENERATOR, NUM_WINDOWS, NUM_WINDOWS_SHORT, ORDER, P

pytestmark = pytest.mark.gpu
FP = 0
VESTA = h.VESTA
MARKER = 0xA5
K = 11                                                     # the 1024-row range-check table needs k = 11


def _ints(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else t
    return fields.from_limbs(np.ascontiguousarray(a).view(np.uint64).reshape(-1, 4), FP, True)


def _rng(seed):
    sf = co.field_of_curve(VESTA, "scalar")
    ctr = [seed]

    def rng(count):
        ctr[0] += 1
        return co.random_field(sf, ctr[0], count)
    return rng


@functools.lru_cache(maxsize=None)
def base(nw):
    return ecc.FixedBase(fields.to_limbs(list(GENERATOR), FP).reshape(8), nw)


@functools.lru_cache(maxsize=None)
def tables(nw):
    return FixedBaseTables.of(base(nw))


def model_tables(nw):
    """the host's window table (checked against the device's here) and the DEVICE's roots: the reference does not pin their sign"""
    t = tables(nw)
    assert t.window_table == fx.generator_tables(nw)[0]
    return t.window_table, t.u


def _canonical(ints):
    return torch.from_numpy(fields.to_limbs(list(ints), FP, montgomery=False).view(np.int64)).to("cuda:0")


def _run(entry, nw, inputs, count, aux_width, lanes=None):
    """the C ABI on the default stream over outputs filled with a pattern -> (columns bytes, aux bytes)"""
    ins = [_canonical(v) for v in inputs]
    columns = torch.full((6 * (nw + 1) * count * 32 + 64,), MARKER, dtype=torch.uint8, device="cuda:0")
    aux = torch.full((aux_width * count * 32 + 64,), MARKER, dtype=torch.uint8, device="cuda:0")
    scratch = torch.empty(((count if lanes is None else lanes) * (nw - 2), 4), dtype=torch.int64, device="cuda:0")
    d = _lib.EccFixedSum(nw, base(nw).points.data_ptr(), base(nw).us.data_ptr(), scratch.data_ptr(), scratch.shape[0], 0)
    rc = getattr(h.lib(), entry)(C.byref(d), *[t.data_ptr() for t in ins], count, columns.data_ptr(), aux.data_ptr())
    assert rc == 0, h.lib().h2_last_error()
    torch.cuda.synchronize()
    got = [t.cpu().numpy().tobytes() for t in (columns, aux)]
    assert all(raw[-64:] == bytes([MARKER]) * 64 for raw in got)              # nothing past the end
    return got[0][:-64], got[1][:-64]


def _short(pairs, lanes=None):
    return _run(fs.SHORT, NUM_WINDOWS_SHORT, ([m for m, _ in pairs], [s for _, s in pairs]), len(pairs), fs.SHORT_AUX, lanes)


def _base_field(alphas, lanes=None):
    return _run(fs.BASE_FIELD, NUM_WINDOWS, (list(alphas),), len(alphas), fs.BASE_FIELD_AUX, lanes)


def _same(got, want, what):
    assert len(got) == len(want), what
    bad = [i // 32 for i in range(0, len(want), 32) if got[i:i + 32] != want[i:i + 32]]
    assert not bad, f"{what}: {len(bad)} of {len(want) // 32} elements differ, first {bad[:6]}"


# ---- the traces against the model -------------------------------------------------------------------------------------------------------------
def test_the_short_trace_is_the_models_at_65():
    pairs = fs.short_pairs(65)
    (columns, aux), (want_columns, want_aux) = _short(pairs), fs.short_bytes(*model_tables(NUM_WINDOWS_SHORT), pairs)
    _same(columns, want_columns, "columns")
    _same(aux, want_aux, "aux")


def test_the_short_trace_is_the_models_one_at_a_time():
    for pair in fs.short_edges() + fs.short_invalid():
        (columns, aux), (want_columns, want_aux) = _short([pair]), fs.short_bytes(*model_tables(NUM_WINDOWS_SHORT), [pair])
        _same(columns, want_columns, f"columns of {pair}")
        _same(aux, want_aux, f"aux of {pair}")


def test_the_base_field_trace_is_the_models_at_65():
    alphas = fs.base_field_alphas(65)
    (columns, aux), (want_columns, want_aux) = _base_field(alphas), fs.base_field_bytes(*model_tables(NUM_WINDOWS), alphas)
    _same(columns, want_columns, "columns")
    _same(aux, want_aux, "aux")


def test_the_base_field_trace_is_the_models_one_at_a_time():
    for alpha in fs.base_field_edges():
        (columns, aux), (want_columns, want_aux) = _base_field([alpha]), fs.base_field_bytes(*model_tables(NUM_WINDOWS), [alpha])
        _same(columns, want_columns, f"columns of {alpha:#x}")
        _same(aux, want_aux, f"aux of {alpha:#x}")


@pytest.mark.parametrize("count, lanes", fs.CHUNKED)
def test_a_scratch_of_fewer_lanes_gives_the_same_bytes(count, lanes):
    pairs, alphas = fs.short_pairs(count), fs.base_field_alphas(count)
    assert _short(pairs, lanes) == _short(pairs)
    assert _base_field(alphas, lanes) == _base_field(alphas)


def test_the_python_primitives(monkeypatch):
    """host arrays in, host arrays out; device tensors in, device tensors out; the scratch's bound cuts the call into chunks"""
    pairs, alphas = fs.short_pairs(5), fs.base_field_alphas(5)
    m, s, a = (fields.to_limbs(v, FP, montgomery=False) for v in ([m for m, _ in pairs], [s for _, s in pairs], alphas))
    columns, aux = ecc.mul_fixed_short_trace(base(NUM_WINDOWS_SHORT), m, s)
    assert isinstance(columns, np.ndarray) and columns.shape == (6, 23 * 5, 4) and aux.shape == (5, 12, 4)
    assert (columns.tobytes(), aux.tobytes()) == _short(pairs)
    d_columns, d_aux = ecc.mul_fixed_base_field_trace(base(NUM_WINDOWS), _canonical(alphas))
    assert torch.is_tensor(d_columns) and d_columns.is_cuda and d_columns.shape == (6, 86 * 5, 4) and d_aux.shape == (5, 15, 4)
    assert (d_columns.cpu().numpy().tobytes(), d_aux.cpu().numpy().tobytes()) == _base_field(alphas)
    monkeypatch.setattr(ecc, "SUM_SCRATCH_LANES", 2)
    chunked = ecc.mul_fixed_base_field_trace(base(NUM_WINDOWS), a)
    assert (chunked[0].tobytes(), chunked[1].tobytes()) == _base_field(alphas)
    chunked = ecc.mul_fixed_short_trace(base(NUM_WINDOWS_SHORT), m, s)
    assert (chunked[0].tobytes(), chunked[1].tobytes()) == _short(pairs)
    with pytest.raises(ValueError):
        ecc.mul_fixed_short_trace(base(NUM_WINDOWS), m, s)
    with pytest.raises(ValueError):
        ecc.mul_fixed_short_trace(base(NUM_WINDOWS_SHORT), m, _canonical([1] * 5))
    empty = ecc.mul_fixed_base_field_trace(base(NUM_WINDOWS), np.zeros((0, 4), dtype=np.uint64))
    assert empty[0].shape == (6, 0, 4) and empty[1].shape == (0, 15, 4)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_and_the_empty_call():
    lib = h.lib()
    assert lib.h2_init(0) == 0
    memory = torch.full((1 << 16,), MARKER, dtype=torch.uint8, device="cuda:0")
    at = memory.data_ptr()
    rows = fs.refusals(at, at + 4096, at + 8192, at + 12288, points=at + 16384, u=at + 20480, scratch=at + 24576)
    assert len(rows) == 27
    for row in rows:
        assert fs.refuse(lib, row) == _lib.H2_ERR_ARGS, row[:2]
    short, full = fs.descriptor(NUM_WINDOWS_SHORT, None, None, None, 0), fs.descriptor(NUM_WINDOWS, None, None, None, 0)
    assert lib.h2_ecc_mul_fixed_short_trace_device(C.byref(short), None, None, 0, None, None) == 0
    assert lib.h2_ecc_mul_fixed_base_field_trace_device(C.byref(full), None, 0, None, None) == 0
    short = fs.descriptor(NUM_WINDOWS_SHORT, at + 16384, at + 20480, at + 24576)
    assert lib.h2_ecc_mul_fixed_short_trace_device(C.byref(short), at, at, 0, at, at) == 0
    torch.cuda.synchronize()
    assert bool((memory == MARKER).all())


# ---- stream order -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig():
    """The harness of tests/test_gpu_stream_order.py for the two cases of tests/ecc_fixed_sum_cases.py: a delay of four warm call times
    on `s`, and a stream `w` shown to overtake it."""
    import test_gpu_stream_order as so
    assert h.lib().h2_init(0) == 0, h.lib().h2_last_error()
    r = so.Rig()
    r.so = so
    r.null = torch.cuda.default_stream()
    r.pool = [torch.cuda.Stream() for _ in range(so.POOL_STREAMS)]
    r.cases = fs.stream_cases()
    r.warm_ms = {name: so._warm(case) for name, case in r.cases.items()}
    r.delay = so.Delay(r.pool[0])
    r.delay.size(max(20.0, so.DELAY_FACTOR * max(r.warm_ms.values())))
    r.s = r.w = None
    for s in r.pool:
        for w in [r.null] + [p for p in r.pool if p is not s]:
            if so._overtakes(r.delay, s, w):
                r.s, r.w = s, w
                break
        if r.s is not None:
            break
    if r.s is None:
        pytest.fail("no pair of streams overtakes: a misplaced launch cannot be told from an ordered one on this device")
    assert r.delay.measured_ms >= 2 * max(r.warm_ms.values()), (r.delay.ms, r.delay.measured_ms, r.warm_ms)
    return r


@pytest.mark.parametrize("entry", [fs.SHORT, fs.BASE_FIELD])
def test_stream_order_late_producer_early_overwrite(entry, rig):
    """The inputs are produced late by work queued on the descriptor's stream, a non-default one, and overwritten on that stream right
    after the call; the result is the oracle's."""
    so, case = rig.so, rig.cases[entry]
    assert rig.s.cuda_stream != 0
    want = so._wanted(case, so.sc.REAL)
    clones, host, _ = so._ordered_run(case, rig.s, rig.s, rig.delay)
    rig.s.synchronize()
    got = so._collect(case, clones, host)
    torch.cuda.synchronize()
    assert got == want, f"{case} on a held-back stream: {so._first_difference(got, want)}"


# ---- the bulk forms against the single calls ----------------------------------------------------------------------------------------------------
def _synthesized(circuit):
    cs, assembly, layouter = front.synthesize(circuit, K, FP, fixed=True, advice=True, instances=[])
    advice = [_ints(c) for c in assembly.columns_to_field(assembly.advice)]
    fixed = [_ints(c) for c in assembly.columns_to_field(assembly.fixed)]
    return cs, assembly, layouter, advice, fixed


def _rows_equal(a, b, columns, at_a, at_b, rows, what):
    for c in columns:
        assert a[c][at_a:at_a + rows] == b[c][at_b:at_b + rows], (what, c)


def _selectors_equal(sa, sb, selectors, at_a, at_b, rows, what):
    for q in selectors:
        assert (sa[q.index, at_a:at_a + rows] == sb[q.index, at_b:at_b + rows]).all(), (what, q.index)
        assert sa[q.index, at_a:at_a + rows].any(), (what, q.index)


def _fixed_columns(config):
    return [c.index for c in config.mul_fixed.lagrange_coeffs] + [config.mul_fixed.fixed_z.index]


def test_mul_fixed_short_many_lays_the_cells_of_mul_fixed_short():
    pairs = fs.short_edges() + [p for p in fs.short_pairs(20, valid_only=True)[8:12]]
    t = tables(NUM_WINDOWS_SHORT)
    one, bulk = fs.ShortManyCircuit(pairs, t), fs.ShortManyCircuit(pairs, t, many=True)
    (cs, aa, la, a, fa), (_, ab, lb, b, fb) = _synthesized(one), _synthesized(bulk)
    config = one.config
    fixed, short, add, inc = config.mul_fixed, config.mul_fixed_short, config.add, config.add_incomplete
    start, add_start = lb.regions[bulk.bulk.region_index], lb.regions[bulk.bulk.add_region_index]
    for i, (product, scalar) in enumerate(one.products):
        at = la.regions[scalar.running_sum[1].cell().region_index]
        last = la.regions[product.inner().x().cell().region_index]
        _rows_equal(a, b, range(6), at, start + 23 * i, 23, ("incomplete", i))
        _rows_equal(fa, fb, _fixed_columns(config), at, start + 23 * i, 23, ("tables", i))
        _selectors_equal(aa.selectors, ab.selectors, [fixed.running_sum_config.q_range_check, inc.q_add_incomplete], at, start + 23 * i, 23, i)
        _rows_equal(a, b, range(9), last, add_start + 2 * i, 2, ("most significant word", i))
        _selectors_equal(aa.selectors, ab.selectors, [add.q_add, short.q_mul_fixed_short], last, add_start + 2 * i, 2, i)
    got = _ints(bulk.bulk.outputs)
    want = [ec.ec_mul((m if s == 1 else -m) % ORDER, GENERATOR) for m, s in pairs]
    single = [(p.inner().x().value().inner.evaluate(P), p.inner().y().value().inner.evaluate(P)) for p, _ in one.products]
    assert [(got[2 * i], got[2 * i + 1]) for i in range(len(pairs))] == want == single
    assert bulk.bulk.z(1, 22).row_offset == 23 + 22 and bulk.bulk.result_y(2).column == add.y_p
    dev.MockProver.run_circuit(K, fs.ShortManyCircuit(pairs, t, many=True), [], FP).assert_satisfied()


def test_mul_fixed_base_field_elem_many_lays_the_cells_of_the_single_call():
    alphas = fs.base_field_alphas(8)
    assert set(fs.base_field_edges()) <= set(alphas)
    t = tables(NUM_WINDOWS)
    one, bulk = fs.BaseFieldManyCircuit(alphas, t), fs.BaseFieldManyCircuit(alphas, t, many=True)
    (cs, aa, la, a, fa), (_, ab, lb, b, fb) = _synthesized(one), _synthesized(bulk)
    config = one.config
    fixed, add, inc, lookup = config.mul_fixed, config.add, config.add_incomplete, config.lookup_config
    res = bulk.bulk
    start, add_start, canon_start = (lb.regions[r] for r in (res.region_index, res.add_region_index, res.canonicity_region_index))
    check_start = lb.regions[res.alpha_0_prime[0][0].region_index]
    for i, product in enumerate(one.products):
        r = product.inner().x().cell().region_index                          # the complete addition; its neighbours are the call's
        at, add_at, check_at, canon_at = (la.regions[r + d] for d in (-1, 0, 1, 2))
        _rows_equal(a, b, range(6), at, start + 86 * i, 86, ("incomplete", i))
        _rows_equal(fa, fb, _fixed_columns(config), at, start + 86 * i, 86, ("tables", i))
        _selectors_equal(aa.selectors, ab.selectors, [fixed.running_sum_config.q_range_check, inc.q_add_incomplete], at, start + 86 * i, 86, i)
        _rows_equal(a, b, range(9), add_at, add_start + 2 * i, 2, ("complete addition", i))
        _selectors_equal(aa.selectors, ab.selectors, [add.q_add], add_at, add_start + 2 * i, 2, i)
        _rows_equal(a, b, [9], check_at, check_start + 14 * i, 14, ("alpha_0' range check", i))
        _selectors_equal(aa.selectors, ab.selectors, [lookup.q_lookup, lookup.q_running], check_at, check_start + 14 * i, 14, i)
        _rows_equal(a, b, [6, 7, 8], canon_at, canon_start + 3 * i, 3, ("canonicity", i))
        _selectors_equal(aa.selectors, ab.selectors, [config.mul_fixed_base_field.q_mul_fixed_base_field], canon_at, canon_start + 3 * i, 3, i)
    got = _ints(res.outputs)
    want = [ec.ec_mul(alpha % ORDER, GENERATOR) for alpha in alphas]
    single = [(p.inner().x().value().inner.evaluate(P), p.inner().y().value().inner.evaluate(P)) for p in one.products]
    assert [(got[2 * i], got[2 * i + 1]) for i in range(len(alphas))] == want == single
    dev.MockProver.run_circuit(K, fs.BaseFieldManyCircuit(alphas, t, many=True), [], FP).assert_satisfied()


def test_add_many_lays_the_cells_of_add():
    pairs = fs.add_pairs()
    one, bulk = fs.AddManyCircuit(pairs), fs.AddManyCircuit(pairs, many=True)
    (cs, aa, la, a, fa), (_, ab, lb, b, fb) = _synthesized(one), _synthesized(bulk)
    start = lb.regions[bulk.bulk.region_index]
    for i, total in enumerate(one.sums):
        at = la.regions[total.x().cell().region_index]
        _rows_equal(a, b, range(9), at, start + 2 * i, 2, i)
        _selectors_equal(aa.selectors, ab.selectors, [one.config.add.q_add], at, start + 2 * i, 2, i)
    got = _ints(bulk.bulk.outputs)
    want = [ec.complete_add(p, q)[0] for p, q in pairs]
    assert [(got[2 * i], got[2 * i + 1]) for i in range(len(pairs))] == want
    assert want[1] == ec.ec_mul(2, pairs[1][0]) and want[2] == (0, 0) and want[3] == pairs[3][1] and want[4] == pairs[4][0]
    dev.MockProver.run_circuit(K, fs.AddManyCircuit(pairs, many=True), [], FP).assert_satisfied()
    # bare cells carry no value: the trace comes from the caller
    with pytest.raises(front.Synthesis):
        front.synthesize(_BareCells(pairs), K, FP, fixed=True, advice=True, instances=[])


class _BareCells(fs.AddManyCircuit):
    def synthesize(self, config, layouter):
        from halo2_amd.gadgets.ecc import EccChip
        chip = EccChip(config)
        points = [(chip.witness_point(layouter, p), chip.witness_point(layouter, q)) for p, q in self.pairs]
        chip.add_many(layouter, [(p.x().cell(), p.y().cell()) for p, _ in points], [q for _, q in points])


# ---- invalid inputs and tampered witnesses ------------------------------------------------------------------------------------------------------
def _gate_names(circuit):
    cs, _, _ = front.synthesize(circuit.without_witnesses(), K, FP, fixed=True, advice=False)
    return [(g.name, n) for g in cs.gates for n in g.constraint_names]


def _failures(circuit, spans):
    """the failures of a circuit as a sorted list of (kind, what, where): `where` is (label, row offset) within the spans
    [(label, start, rows)] of the item under test, or None outside them (the constants' fixed column)"""
    names = _gate_names(circuit)

    def where(row):
        return next(((label, row - start) for label, start, rows in spans() if start <= row < start + rows), None)
    out = []
    for f in dev.MockProver.run_circuit(K, circuit, [], FP).verify():
        if isinstance(f, dev.ConstraintNotSatisfied):
            out.append(("gate", names[f.gate_index], where(f.row)))
        elif isinstance(f, dev.Permutation):
            out.append(("copy", f.column, where(f.row) if f.column[0] == "advice" else None))
        else:
            out.append((type(f).__name__, None, where(f.row)))
    return sorted(out, key=repr)


def _short_spans(circuit, i):
    def spans():
        layouter = circuit.layouter
        if circuit.many:
            r = circuit.bulk
            return [("incomplete", layouter.regions[r.region_index] + 23 * i, 23), ("last", layouter.regions[r.add_region_index] + 2 * i, 2)]
        product, scalar = circuit.products[i]
        return [("incomplete", layouter.regions[scalar.running_sum[1].cell().region_index], 23),
                ("last", layouter.regions[product.inner().x().cell().region_index], 2)]
    return spans


@pytest.mark.parametrize("pair", fs.short_invalid(), ids=lambda p: f"{p[0]:#x}*{p[1]:#x}")
def test_an_invalid_input_fails_in_bulk_where_the_single_call_fails(pair):
    pairs = [(5, 1), pair, (7, P - 1)]
    t = tables(NUM_WINDOWS_SHORT)
    one, bulk = fs.ShortManyCircuit(pairs, t), fs.ShortManyCircuit(pairs, t, many=True)
    want, got = _failures(one, _short_spans(one, 1)), _failures(bulk, _short_spans(bulk, 1))
    assert want and got == want
    assert all(w is not None or kind == "copy" for kind, _, w in want)         # every gate failure lies in the invalid item
    if pair[0] >> 64:
        assert any(kind == "copy" and w == ("incomplete", 22) for kind, _, w in want)      # z_22 against the constant 0
    else:
        assert {what for kind, what, _ in want if kind == "gate"} == {("Short fixed-base mul gate", "sign_check"),
                                                                       ("Short fixed-base mul gate", "negation_check")}


def _replace(t, index, source):
    t[index] = t[source].clone()


def test_a_tampered_signed_y_fails_the_short_gate_alone():
    pairs = [(5, 1), (0x1234567, P - 1), (7, 1)]
    bulk = fs.ShortManyCircuit(pairs, tables(NUM_WINDOWS_SHORT), many=True, tamper=lambda columns, aux: _replace(aux, (1, 11), (1, 9)))
    got = _failures(bulk, _short_spans(bulk, 1))
    assert got == [("gate", ("Short fixed-base mul gate", name), ("last", 1)) for name in ("negation_check", "y_check")]


def test_a_tampered_running_sum_fails_its_two_gates_alone():
    pairs = [(5, 1), (0x123456789ABCDEF, P - 1), (7, 1)]
    row = 23 + 10
    bulk = fs.ShortManyCircuit(pairs, tables(NUM_WINDOWS_SHORT), many=True, tamper=lambda columns, aux: _replace(columns, (4, row), (4, row + 1)))
    got = _failures(bulk, _short_spans(bulk, 1))
    assert got and all(kind == "gate" and what[0] in ("range check", "Running sum coordinates check") and where in (("incomplete", 9), ("incomplete", 10))
                       for kind, what, where in got)
    assert {what[0] for _, what, _ in got} == {"range check", "Running sum coordinates check"}


def test_a_tampered_u_fails_check_y_alone():
    alphas = fs.base_field_alphas(3)
    row = 86 + 17
    bulk = fs.BaseFieldManyCircuit(alphas, tables(NUM_WINDOWS), many=True, tamper=lambda columns, aux: _replace(columns, (5, row), (5, row + 1)))
    failures = dev.MockProver.run_circuit(K, bulk, [], FP).verify()
    names = _gate_names(bulk)
    start = bulk.layouter.regions[bulk.bulk.region_index]
    assert [(names[f.gate_index], f.row - start) for f in failures] == [(("Running sum coordinates check", "check y"), row)]


def test_a_tampered_alpha_1_fails_the_canonicity_gate_alone():
    alphas = [3, (1 << 252) + 12345, 9]                                       # alpha_1 = 1, alpha_2 = 0
    bulk = fs.BaseFieldManyCircuit(alphas, tables(NUM_WINDOWS), many=True, tamper=lambda columns, aux: _replace(aux, (1, 12), (1, 13)))
    failures = dev.MockProver.run_circuit(K, bulk, [], FP).verify()
    names = _gate_names(bulk)
    start = bulk.layouter.regions[bulk.bulk.canonicity_region_index]
    assert [(names[f.gate_index], f.row - start) for f in failures] == [(("Canonicity checks", "z_84_alpha_check"), 3 + 1)]


# ---- proofs ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["short", "base_field"])
def test_a_proof_of_eight_multiplications(form):
    """keygen, create_proof and verify_proof of the `many` circuit at k = 11, the smallest that holds the range check's table"""
    if form == "short":
        circuit = fs.ShortManyCircuit(fs.short_pairs(8, valid_only=True), tables(NUM_WINDOWS_SHORT), many=True)
    else:
        circuit = fs.BaseFieldManyCircuit(fs.base_field_alphas(8), tables(NUM_WINDOWS), many=True)
    with pytest.raises(front.NotEnoughRowsAvailable):
        front.synthesize(circuit.without_witnesses(), K - 1, FP, fixed=True, advice=False)
    params = h.Params.new(VESTA, K)
    try:
        pk = h.keygen_pk(params, circuit)
        tr = Blake2bWrite(VESTA)
        h.create_proof(params, pk, [circuit], [[]], _rng(23), tr)
        proof = tr.finalize()
        assert hv.verify_proof(params, pk.vk, [], proof)
        bad = bytearray(proof)
        bad[len(proof) // 2] ^= 1
        assert not hv.verify_proof(params, pk.vk, [], bytes(bad))
    finally:
        params.close()


def test_the_example_commits_to_64_values():
    """examples/value_commitment.py end to end: mock-proved, proved, verified, and rejected against one wrong commitment"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "value_commitment.py")
    spec = importlib.util.spec_from_file_location("value_commitment", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.main([]) is True
