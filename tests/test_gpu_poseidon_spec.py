"""Poseidon for any Spec on the device: the three kernels of halo2_amd/csrc/poseidon_spec.hip bit for bit against the Python-integer
model of tests/poseidon_model.py (see its docstring and tests/test_poseidon_spec_host.py for what stands behind the model: reference
values exist for width 3 only), against the existing P128Pow5T3 kernels byte for byte, every refusal with the outputs untouched, and
the stream order of each entry point, whose stream travels in the descriptor: the first two modes of tests/test_gpu_stream_order.py
and a producer on another stream joined by an event."""
import ctypes as C
import functools

import numpy as np
import pytest

import halo2_amd as h
import poseidon_model as pm
import poseidon_spec_cases as psc
from halo2_amd import _lib, fields, poseidon
from halo2_amd.poseidon_spec import Spec
from poseidon_spec_cases import FP, FQ

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MARKER = 0xA5


def _up(limbs):
    return torch.from_numpy(np.ascontiguousarray(limbs).view(np.int64)).to(fields.current_device())


def _ints(t, field):
    return psc.ints_of(t, field)


def _limbs(ints, field, *shape):
    return psc.limbs_of(ints, field).reshape(*shape, 4)


# ---- the grid ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pool(field, key):
    """257 random states of the spec with their permutations, and 257 messages of `rate` words with their digests: computed once"""
    model = pm.model(field, *key)
    states = pm.random_states(257, model.width, field, 0x900 + 16 * model.width + field)
    messages = [s[:model.rate] for s in pm.random_states(257, model.width, field, 0xA00 + 16 * model.width + field)]
    return states, [model.permute(s) for s in states], messages, [model.hash(msg) for msg in messages]


@pytest.mark.parametrize("field", [FP, FQ])
@pytest.mark.parametrize("key", psc.GRID, ids=str)
def test_permute_and_hash_over_the_grid(field, key):
    spec = Spec(field, *key)
    states, permuted, messages, digests = _pool(field, key)
    for n in psc.COUNTS:
        first = 257 - n                                                       # another slice per count
        d_states = _up(_limbs([w for s in states[first:first + n] for w in s], field, n, spec.width))
        before = d_states.clone()
        out = spec.permute(d_states)
        assert out.shape == (n, spec.width, 4) and _ints(out, field) == [w for s in permuted[first:first + n] for w in s], (key, n)
        assert (d_states == before).all()
        got = spec.hash(_up(_limbs([w for msg in messages[first:first + n] for w in msg], field, n, spec.rate)))
        assert got.shape == (n, 4) and _ints(got, field) == digests[first:first + n], (key, n)


@pytest.mark.parametrize("field", [FP, FQ])
@pytest.mark.parametrize("key", psc.GRID, ids=str)
def test_crafted_states_lengths_and_in_place(field, key):
    spec, model, m = Spec(field, *key), pm.model(field, *key), pm.MOD[field]
    width, rate = model.width, model.rate
    states = [[0] * width, [m - 1] * width] + pm.random_states(2, width, field, 0xB00 + width)
    want = [w for s in states for w in model.permute(s)]
    d_states = _up(_limbs([w for s in states for w in s], field, len(states), width))
    assert _ints(spec.permute(d_states), field) == want
    assert spec.permute(d_states, out=d_states) is d_states and _ints(d_states, field) == want          # in place
    host = spec.permute(_limbs([w for s in states for w in s], field, len(states), width))                # numpy in, numpy out
    assert isinstance(host, np.ndarray) and host.dtype == np.uint64 and _ints(host, field) == want
    for length in (1, rate, rate + 1, 2 * rate):
        messages = [[0] * length, [m - 1] * length] + pm.random_states(2, length, field, 0xC00 + length)
        messages[2][-1], messages[3][0] = 0, m - 1
        got = spec.hash(_up(_limbs([w for msg in messages for w in msg], field, len(messages), length)))
        assert _ints(got, field) == [model.hash(msg) for msg in messages], (key, length)
    assert spec.permute(_up(np.zeros((0, width, 4), dtype=np.uint64))).shape == (0, width, 4)
    with pytest.raises(ValueError):
        spec.permute(np.zeros((2, width + 1, 4), dtype=np.uint64))
    with pytest.raises(ValueError):
        spec.hash(np.zeros((3, 0, 4), dtype=np.uint64))


@pytest.mark.parametrize("field", [FP, FQ])
def test_merkle_root_by_arity(field):
    for key, arity, n_leaves in (((9, 8, 8, 56), None, 64), ((3, 2, 8, 56), None, 8), ((5, 4, 8, 57), 2, 4)):
        spec, model = Spec(field, *key), pm.model(field, *key)
        leaves = [s[0] for s in pm.random_states(n_leaves, 1, field, 0xD00 + n_leaves)]
        root = spec.merkle_root(_up(_limbs(leaves, field, n_leaves)), arity)
        assert root.shape == (4,) and root.is_cuda and _ints(root, field) == [model.merkle_root(leaves, arity)]
        with pytest.raises(ValueError):
            spec.merkle_root(np.zeros((n_leaves + 1, 4), dtype=np.uint64), arity)


# ---- the existing kernels --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [FP, FQ])
def test_the_t3_spec_gives_the_bytes_of_the_existing_kernels(field):
    spec = Spec.p128pow5t3(field)
    states, _, _, _ = _pool(field, (3, 2, 8, 56))
    d_states = _up(_limbs([w for s in states for w in s], field, 257, 3))
    assert torch.equal(spec.permute(d_states), poseidon.permute(d_states, field))
    assert torch.equal(spec.trace(d_states[:65]), poseidon.trace(d_states[:65], field))
    words = torch.cat([d_states, poseidon.permute(d_states, field)]).reshape(-1, 4)                     # 1542 elements
    for length in (1, 2, 5):
        messages = words[:257 * length].reshape(257, length, 4).contiguous()
        assert torch.equal(spec.hash(messages), poseidon.hash(messages, field))
    leaves = d_states[:64, 0].contiguous()
    assert torch.equal(spec.merkle_root(leaves), poseidon.merkle_root(leaves, field))


# ---- trace -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [FP, FQ])
@pytest.mark.parametrize("key", psc.TRACE_GRID, ids=str)
def test_trace_every_cell(field, key):
    spec, model, m = Spec(field, *key), pm.model(field, *key), pm.MOD[field]
    width, rows, half = model.width, model.rows, model.full // 2
    pool = [[m - 1] * width, [0] * width] + pm.random_states(63, width, field, 0xE00 + width)
    want_all = model.trace_limbs(pool)
    for count in (1, 65):
        got = spec.trace(_up(model.states_limbs(pool[:count])))
        assert got.shape == (width + 1, rows * count, 4)
        got = got.cpu().numpy().view(np.uint64)
        for column in range(width + 1):
            assert np.array_equal(got[column], want_all[column][:rows * count]), f"{key} count {count} column {column}"
        sbox = np.array([v != 0 for v in _ints(got[width], field)]).reshape(count, rows)
        assert not sbox[:, :half].any() and not sbox[:, half + model.partial // 2:].any()
        assert sbox[:, half:half + model.partial // 2].all()                  # (a zero S-box output has probability 2^-254)
    with pytest.raises(ValueError):
        Spec(field, 5, 4, 8, 57).trace(np.zeros((1, 5, 4), dtype=np.uint64))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_outputs_untouched():
    lib = h.lib()
    assert lib.h2_init(0) == 0, lib.h2_last_error()
    d_in = torch.full((4096,), MARKER, dtype=torch.uint8, device="cuda:0")
    d_out = torch.full((1 << 16,), MARKER, dtype=torch.uint8, device="cuda:0")
    table = poseidon.spec_constants(Spec.p128pow5t3(FP), "cuda:0")
    before = table.clone()
    rows = psc.refusals(d_in.data_ptr(), d_out.data_ptr(), table.data_ptr())
    for row in rows:
        assert psc.refuse(lib, row) == _lib.H2_ERR_ARGS, row[:2]
    torch.cuda.synchronize()
    assert bool((d_out == MARKER).all()) and bool((d_in == MARKER).all()) and torch.equal(table, before)
    # a count of 0 launches nothing and needs no buffer
    d = psc.descriptor(constants=None)
    assert lib.h2_poseidon_spec_permute_device(C.byref(d), None, 0, None) == 0
    assert lib.h2_poseidon_spec_hash_device(C.byref(d), None, 0, 3, None) == 0
    assert lib.h2_poseidon_spec_trace_device(C.byref(d), None, 0, None) == 0
    torch.cuda.synchronize()
    assert bool((d_out == MARKER).all())


# ---- stream order ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig():
    """The harness of tests/test_gpu_stream_order.py for the three cases of tests/poseidon_spec_cases.py: a delay of four warm call times
    on `s`, and a stream `w` shown to overtake it."""
    import test_gpu_stream_order as so
    assert h.lib().h2_init(0) == 0, h.lib().h2_last_error()
    r = so.Rig()
    r.so = so
    r.null = torch.cuda.default_stream()
    r.pool = [torch.cuda.Stream() for _ in range(so.POOL_STREAMS)]
    cases = psc.stream_cases()
    r.warm_ms = {name: so._warm(case) for name, case in cases.items()}
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
    print(f"\nposeidon spec stream order: warm calls {r.warm_ms}; delay asked for {r.delay.ms:.2f} ms, measured {r.delay.measured_ms:.2f} ms")
    return r


@pytest.mark.parametrize("entry", psc.STREAM_ENTRIES)
def test_stream_mode_a_late_producer_early_overwrite(entry, rig):
    """The input is produced late by work queued on spec.stream, and overwritten on that stream right after the call."""
    so, case = rig.so, psc.stream_cases()[entry]
    assert rig.s.cuda_stream != 0                                             # a non-default stream
    want = so._wanted(case, so.sc.REAL)
    clones, host, _ = so._ordered_run(case, rig.s, rig.s, rig.delay)
    rig.s.synchronize()                                                       # and nothing wider
    got = so._collect(case, clones, host)
    torch.cuda.synchronize()
    assert got == want, f"{case} on a held-back stream: {so._first_difference(got, want)}"


@pytest.mark.parametrize("entry", psc.STREAM_ENTRIES)
def test_stream_mode_b_a_misplaced_stream_is_seen(entry, rig):
    """The harness can fail: with the descriptor's stream another one than the producer's, and no event, the answer is not REAL's."""
    so, case = rig.so, psc.stream_cases()[entry]
    want = so._wanted(case, so.sc.REAL)
    streams = [rig.null] + rig.pool
    pairs = [(rig.s, rig.w)] + [(s, w) for s in rig.pool for w in streams if w is not s and (s, w) != (rig.s, rig.w)]
    serialised = []
    for s, w in pairs:
        clones, host, overtook = so._ordered_run(case, s, w, rig.delay)
        torch.cuda.synchronize()
        got = so._collect(case, clones, host)
        assert len(got) == len(want)
        if got != want:
            return
        assert not overtook, f"{case}: the call ran ahead of its inputs on another stream and the answer is REAL's all the same"
        serialised.append((streams.index(s), streams.index(w)))
    pytest.fail(f"{case}: on every pair of streams the call waited for the delay on the other: {serialised}")


@pytest.mark.parametrize("entry", psc.STREAM_ENTRIES)
def test_stream_producer_on_another_stream_with_an_event_wait(entry, rig):
    """The producer runs on `p`, held back; spec.stream `s` waits for the producer's event and for nothing else."""
    so, case = rig.so, psc.stream_cases()[entry]
    sc = so.sc
    p, s = rig.s, next(x for x in rig.pool if x is not rig.s)
    want = so._wanted(case, sc.REAL)
    real = {name: so._dev(a) for name, a in case.inputs(sc.REAL).items()}
    decoy = {name: so._dev(a) for name, a in case.inputs(sc.DECOY).items()}
    ins, outs = so._buffers(case, sc.DECOY)
    produced = torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(p):
        rig.delay.on(p)
        for name in ins:
            ins[name].copy_(real[name], non_blocking=True)
        for t in outs.values():
            t.fill_(so.MARKER)
        produced.record(p)
    with torch.cuda.stream(s):
        s.wait_event(produced)
        host = case.call(ins, outs, s.cuda_stream)
        clones = [(name, t.clone()) for name, t in so._result_views(case, ins, outs)]
        for name in ins:
            ins[name].copy_(decoy[name], non_blocking=True)
    s.synchronize()
    got = so._collect(case, clones, host)
    torch.cuda.synchronize()
    assert got == want, f"{case} behind an event of another stream: {so._first_difference(got, want)}"
