"""Every `*_device` entry point is ordered by its stream alone (tests/stream_cases.py is the table, tests/test_stream_case_coverage.py
holds it to the header).  The header promises "asynchronous on `stream`", and for the entry points that fork onto the library's own
streams "joined on `stream`"; nearly every other GPU test runs on the null stream with a device-wide synchronise around the call,
where a kernel on the wrong stream or a side stream never joined back is ordered anyway.  Here the caller's stream `s` is held back
by a delay kernel and nothing but `s` is ever waited for:

  Mode A  late producer, early overwrite.  The input buffers hold DECOY data.  On `s` only: the delay, device copies of the REAL
          inputs over them (and the marker over every output buffer once more), the one library call with stream = s, a clone of every
          output, DECOY copied back over every input.  Then s.synchronize() and nothing wider: the clones are the oracle's bytes of
          REAL.  Work launched on another stream reads DECOY and is wiped by the marker; a side stream not joined before the call
          returns leaves a marker or a partial result in the clone, or reads the DECOY written back; a host read-back that forgot to
          wait for `s` carries DECOY's answer.
  Mode B  the harness can fail: the same with the library call on `w`, a stream that demonstrably overtakes the delay.  The clones must
          DIFFER from the oracle's bytes -- a wrong answer from valid data and nothing more.  (The hardware queues are shared among
          all streams of the process, the library's own included: a case whose call on `w` waited for the delay on `s` takes another
          pair of the four streams.)
  Mode C  two streams, cold shared caches: after h2_trim and with the Python-level Sinsemilla table zeroed and dropped, the call on
          REAL data goes on `s` behind the delay and at once the same call on THIRD data on `w`; each stream is synchronised on its
          own and both results are the oracle's.  Both calls use the same root of unity / generator table, so the second is a hit on a cache
          whose build is still held behind the delay: the twiddle cache's `ready` event, the per-stream scratch contexts and the event
          halo2_amd.sinsemilla.generator_table records.

The delay is torch.cuda._sleep, sized from one timed unit and then measured whole with events; its length is four times the slowest case's warm, device-synchronised wall
time (twice that time already lets all misplaced work finish on DECOY data; four for run-to-run spread).  Acceptance is Mode B passing
for every case, not a figure.  Measured on one MI355X: the slowest warm case (ecc-fixed-tables, whose search reads its minima
back round by round) takes 169.9 ms; the delay asked for is 679.6 ms (1.63e9 cycles of torch.cuda._sleep at 4.17e-7 ms a cycle) and
the whole delay, timed between two events on the stream it holds back, is 678.9 ms (the fixture asserts that the two agree within a
fifth); `w` is the null stream.

At most four streams: torch's default (null) stream and three of its pool.  No environment variable or queue setting is changed.
Runs only on a real MI355X (`-m gpu`)."""
import time

import numpy as np
import pytest

import call_sequences as cs
import halo2_amd as h
import stream_cases as sc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MARKER = 0xA5
POOL_STREAMS = 3                                                  # and the null stream: four in all
DELAY_FACTOR = 4
CALIBRATION_CYCLES = 20_000_000
CHAIN_ELEMENTS = 1 << 26                                          # the fallback delay: element-wise passes over 256 MiB


def _dev(a):
    """a host array as a flat uint8 tensor on the device"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def _bytes(t) -> bytes:
    return t.cpu().numpy().tobytes()


def _first_difference(got, want):
    if len(got) != len(want):
        return f"{len(got)} bytes, expected {len(want)}"
    bad = [i for i in range(0, len(want), 32) if got[i:i + 32] != want[i:i + 32]]
    return f"{len(bad)} of {(len(want) + 31) // 32} 32-byte pieces differ, first at {bad[:4]}; a marker there: {[got[i:i + 32] == bytes([MARKER]) * 32 for i in bad[:4]]}"


class Delay:
    """A kernel that keeps a stream busy for a wanted time: torch.cuda._sleep(cycles), or without it a fixed chain of element-wise
    passes over a large tensor.  One unit of either is timed once with events."""

    def __init__(self, stream):
        self.sleep = getattr(torch.cuda, "_sleep", None)
        self.scratch = None if self.sleep else torch.zeros(CHAIN_ELEMENTS, dtype=torch.float32, device="cuda:0")
        self.unit = CALIBRATION_CYCLES if self.sleep else 8
        self._issue(stream, self.unit)                            # once unmeasured: the kernel is loaded
        stream.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record()
            self._issue(stream, self.unit)
            b.record()
        stream.synchronize()
        self.unit_ms = a.elapsed_time(b)
        assert self.unit_ms > 0
        self.ms = self.measured_ms = None

    def _issue(self, stream, units):
        with torch.cuda.stream(stream):
            if self.sleep:
                self.sleep(int(units))
            else:
                for _ in range(int(units)):
                    self.scratch.mul_(1.0001).add_(1.0)

    def size(self, ms):
        self.ms = ms
        self.units = max(1, int(ms / self.unit_ms * self.unit + 0.5))

    def on(self, stream):
        self._issue(stream, self.units)


class Rig:
    pass


def _overtakes(delay, s, w):
    """a trivial copy on w finishes while the delay queued before it on s still runs"""
    src, dst = torch.zeros(64, dtype=torch.uint8, device="cuda:0"), torch.ones(64, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    e0, e_s, e_w = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    with torch.cuda.stream(s):
        e0.record()
        delay.on(s)
        e_s.record()
    with torch.cuda.stream(w):
        dst.copy_(src, non_blocking=True)
        e_w.record()
    e_w.synchronize()
    still_running = not e_s.query()
    s.synchronize()
    torch.cuda.synchronize()
    delay.measured_ms = e0.elapsed_time(e_s)                      # the whole delay between two events on s
    return still_running and e0.elapsed_time(e_w) < 0.5 * delay.measured_ms


def _buffers(case, seed):
    """the case's input buffers filled with the seed's data, and its fresh output buffers filled with the marker"""
    ins = {name: _dev(a) for name, a in case.inputs(seed).items()}
    outs = {name: torch.full((spec,), MARKER, dtype=torch.uint8, device="cuda:0") for name, spec in case.outputs().items() if isinstance(spec, int)}
    return ins, outs


def _result_views(case, ins, outs):
    """the device bytes the case compares: a fresh buffer, or the prefix of the input a call works in place on"""
    return [(name, outs[name] if isinstance(spec, int) else ins[spec[1]][:spec[2]]) for name, spec in case.outputs().items()]


def _collect(case, clones, host) -> bytes:
    return b"".join(case.post(name, _bytes(t)) for name, t in clones) + (host or b"")


def _wanted(case, seed) -> bytes:
    want = case.expected(seed)
    at, out = 0, b""
    for name, size in case.output_bytes():
        out += case.post(name, want[at:at + size])
        at += size
    return out + want[at:]


def _warm(case):
    """The call on REAL data on the default stream with a device-wide synchronise: allocation, hipFuncSetAttribute, the set-up objects and
    the cache builds are out of the way.  -> the wall time of a second, warm call (device-synchronised)."""
    for _ in range(2):
        ins, outs = _buffers(case, sc.REAL)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = case.call(ins, outs, 0)
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
    got = _collect(case, _result_views(case, ins, outs), host)
    want = _wanted(case, sc.REAL)
    assert got == want, f"{case}: wrong on the default stream, before any stream is held back: {_first_difference(got, want)}"
    return 1e3 * elapsed


@pytest.fixture(scope="module")
def rig():
    assert h.lib().h2_init(0) == 0, h.lib().h2_last_error()
    r = Rig()
    r.null = torch.cuda.default_stream()
    r.pool = [torch.cuda.Stream() for _ in range(POOL_STREAMS)]
    assert r.null.cuda_stream == 0 and len({s.cuda_stream for s in r.pool} | {0}) == POOL_STREAMS + 1 <= 4
    r.warm_ms = {case.name: _warm(case) for case in sc.ALL_CASES}
    r.slowest = max(r.warm_ms, key=r.warm_ms.get)
    r.delay = Delay(r.pool[0])
    r.delay.size(DELAY_FACTOR * r.warm_ms[r.slowest])
    # the pair: s is held back, work on w overtakes it.  Four hardware queues are shared among all streams, so two streams may serialise
    r.s = r.w = None
    for s in r.pool:
        for w in [r.null] + [p for p in r.pool if p is not s]:
            if _overtakes(r.delay, s, w):
                r.s, r.w = s, w
                break
        if r.s is not None:
            break
    # the delay itself, measured with events on the stream it held back: what was asked for within a fifth, and at least the two warm
    # times after which all misplaced work has run on DECOY data
    assert 0.8 * r.delay.ms <= r.delay.measured_ms <= 1.25 * r.delay.ms and r.delay.measured_ms >= 2 * r.warm_ms[r.slowest], (r.delay.ms, r.delay.measured_ms)
    print(f"\nstream order: slowest warm case {r.slowest} {r.warm_ms[r.slowest]:.2f} ms; delay asked for {r.delay.ms:.2f} ms, measured {r.delay.measured_ms:.2f} ms "
          f"({'torch.cuda._sleep' if r.delay.sleep else 'element-wise chain'}, {r.delay.units} units of {r.delay.unit_ms / r.delay.unit:.3e} ms); "
          f"w is {'the null stream' if r.w is r.null else 'a pool stream'}")
    if r.s is None:
        pytest.fail("no pair of streams overtakes: work on every candidate stream waited for a delay queued on another, so a misplaced "
                    "launch cannot be told from an ordered one on this device")
    return r


def _ordered_run(case, s, library_stream, delay):
    """Mode A's sequence on `s` with the library call on `library_stream` -> the clones, the call's host bytes, and whether the call's
    work had finished while the delay on `s` was still running (always False for a call on `s` itself)"""
    real = {name: _dev(a) for name, a in case.inputs(sc.REAL).items()}
    decoy = {name: _dev(a) for name, a in case.inputs(sc.DECOY).items()}
    ins, outs = _buffers(case, sc.DECOY)
    delayed, called = torch.cuda.Event(), torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay.on(s)
        delayed.record()
        for name in ins:
            ins[name].copy_(real[name], non_blocking=True)
        for t in outs.values():
            t.fill_(MARKER)
        host = case.call(ins, outs, library_stream.cuda_stream)
        called.record(library_stream)
        clones = [(name, t.clone()) for name, t in _result_views(case, ins, outs)]
        for name in ins:
            ins[name].copy_(decoy[name], non_blocking=True)
    overtook = False
    if library_stream is not s:
        called.synchronize()
        overtook = not delayed.query()
    return clones, host, overtook


def test_the_opening_cases_are_the_argument_the_call_sequences_restate(rig):
    want = cs.opening_proof_wanted(sc.IPA_CURVE, sc.IPA_SMALL_K, sc.OPEN_SEED)
    assert sc.BY_NAME["open-device"].expected(sc.REAL) == sc.BY_NAME["open-device-host-s"].expected(sc.REAL) == want


@pytest.mark.parametrize("case", sc.ALL_CASES, ids=repr)
def test_mode_a_late_producer_early_overwrite(case, rig):
    want = _wanted(case, sc.REAL)
    clones, host, _ = _ordered_run(case, rig.s, rig.s, rig.delay)
    rig.s.synchronize()                                           # and nothing wider
    got = _collect(case, clones, host)
    torch.cuda.synchronize()
    assert got == want, f"{case} on a held-back stream: {_first_difference(got, want)}"


@pytest.mark.parametrize("case", sc.ALL_CASES, ids=repr)
def test_mode_b_a_misplaced_stream_is_seen(case, rig):
    """The module's pair (s, w) is proved with a trivial copy.  A call that forks onto the library's own streams brings streams of its own,
    and the hardware queues are shared among all streams of the process: where one of them waits behind the delay on `s`, the
    misplaced call is ordered by the hardware and no test could tell.  So a REAL answer counts against the library only where the call
    on `w` is seen to have finished while the delay on `s` still ran; where it waited for the delay, the other pairs of the four streams
    are tried in turn, and the case fails if none of them lets the call run ahead."""
    want = _wanted(case, sc.REAL)
    streams = [rig.null] + rig.pool
    pairs = [(rig.s, rig.w)] + [(s, w) for s in rig.pool for w in streams if w is not s and (s, w) != (rig.s, rig.w)]
    serialised = []
    for s, w in pairs:
        clones, host, overtook = _ordered_run(case, s, w, rig.delay)
        torch.cuda.synchronize()
        got = _collect(case, clones, host)
        assert len(got) == len(want)
        if got != want:
            if (s, w) != (rig.s, rig.w):
                print(f"\nmode B, {case}: held back stream {streams.index(s)}, called on stream {streams.index(w)} (0 is the null stream) "
                      f"after the call waited for the delay on {serialised}")
            return
        assert not overtook, (f"{case}: the call ran on another stream than its inputs, had finished while they were still held back, and the "
                              f"answer is REAL's all the same (delay {rig.delay.ms:.1f} ms, warm call {rig.warm_ms[case.name]:.2f} ms)")
        serialised.append((streams.index(s), streams.index(w)))
    pytest.fail(f"{case}: on every pair of the four streams the call on one waited for the delay of {rig.delay.ms:.1f} ms on the other and "
                f"gave REAL's answer (warm call {rig.warm_ms[case.name]:.2f} ms): (held back, called on) = {serialised}")


@pytest.mark.parametrize("case", sc.MODE_C, ids=repr)
def test_mode_c_two_streams_cold_shared_caches(case, rig):
    from halo2_amd import sinsemilla
    wants = _wanted(case, sc.REAL), _wanted(case, sc.THIRD)
    first, second = _buffers(case, sc.REAL), _buffers(case, sc.THIRD)
    torch.cuda.synchronize()
    assert h.lib().h2_trim() == 0, h.lib().h2_last_error()
    # the table that is dropped goes back to torch's allocator, and the rebuild may be handed the same block: it must not find the old,
    # complete table there.  Identity points are valid input that gives another answer
    for cached in sinsemilla._tables.values():
        (cached[0] if isinstance(cached, tuple) else cached).zero_()
    torch.cuda.synchronize()
    sinsemilla._tables.clear()
    before = cs.counters()
    results = []
    for stream, (ins, outs), held in ((rig.s, first, True), (rig.w, second, False)):
        with torch.cuda.stream(stream):
            if held:
                rig.delay.on(stream)
            host = case.call(ins, outs, stream.cuda_stream)
            results.append(([(name, t.clone()) for name, t in _result_views(case, ins, outs)], host))
    rig.s.synchronize()
    got_first = _collect(case, *results[0])
    rig.w.synchronize()
    got_second = _collect(case, *results[1])
    torch.cuda.synchronize()
    moved = cs.delta(before, cs.counters())
    if case.entry.startswith(("h2_ntt", "h2_ifft", "h2_coeff_to", "h2_extended_to", "h2_lagrange")):
        assert moved.get("twiddle_built", 0) >= 1 and moved.get("twiddle_hits", 0) >= 1, f"the second call was no hit on the first one's table: {moved}"
    assert got_first == wants[0], f"{case} behind the delay: {_first_difference(got_first, wants[0])}"
    assert got_second == wants[1], f"{case} on the second stream: {_first_difference(got_second, wants[1])}"
