"""What the library keeps between calls, driven through sequences of calls: every unit's grow-only workspace through small / large /
small on two streams around an h2_trim (the probes of tests/call_sequences.py), the captured launch graphs of the host-slice multiexp
across a reallocation, another shape, a trim and the profiler, the opening argument's kept table of collapsed generators through
refills and frees, and the twiddle cache under two roots of one order.  Every result is held to the oracle; which arm a call took is
read back through h2_debug_counters, so a sequence cannot pass by reaching another state than the one it names.  Every test starts
from an h2_trim: what earlier tests of the process left behind decides nothing.  Runs only on a real MI355X (`-m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import call_sequences as cs
import halo2_amd as h
from call_sequences import LARGE, SMALL, counters, delta
from halo2_amd import _lib, fields
from oracle import c_oracle as co
from oracle import pasta as o

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _trim():
    """h2_trim as the existing trim test asserts it: status 0, and no less free device memory than just before."""
    free0 = torch.cuda.mem_get_info()[0]
    assert h.lib().h2_trim() == 0, h.lib().h2_last_error()
    assert torch.cuda.mem_get_info()[0] >= free0


@pytest.fixture(scope="module")
def side_stream():
    return torch.cuda.Stream()


def _first_difference(got, want):
    if len(got) != len(want):
        return f"{len(got)} bytes, expected {len(want)}"
    bad = [i for i in range(0, len(want), 32) if got[i:i + 32] != want[i:i + 32]]
    return f"{len(bad)} of {len(want) // 32} 32-byte elements differ, first at element {bad[:4]}"


# ---- a. regrowth and trim, per unit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("probe", cs.PROBES, ids=repr)
def test_regrowth_and_trim(probe, side_stream):
    """small, large, small on torch's current stream, small on a second one, h2_trim, then small on the first and large, small on the
    second: every result is the oracle's.  The workspaces only grow, so a small call behind small and large ones allocates nothing; the trim
    releases what the calls allocated (the DevBuf epoch rises across it), registered bases stay, and the call after it allocates
    again exactly where the first one did."""
    s0, s1 = torch.cuda.current_stream(), side_stream
    want = {size: probe.expected(size) for size in cs.SIZES}
    torch.cuda.synchronize()
    _trim()                                                # every workspace of the device starts empty
    allocations = []

    def step(size, stream):
        before = counters()["devbuf_epoch"]
        got = probe.run(size, stream)
        allocations.append(counters()["devbuf_epoch"] - before)
        assert got == want[size], f"step {len(allocations)} ({size}): {_first_difference(got, want[size])}"

    for size, stream in ((SMALL, s0), (LARGE, s0), (SMALL, s0), (SMALL, s1)):
        step(size, stream)
    assert allocations[2] == 0, f"a small call behind a large one on the same stream reallocated: {allocations}"
    held = sum(allocations) > 0
    assert held, "the unit owns cached device memory: the probe's calls must have allocated some"
    tables = [cs.commit_table_state(n) for n, _ in cs.COMMIT_SHAPES] if probe.name.startswith("registered-commit") else None
    torch.cuda.synchronize()
    epoch = counters()["devbuf_epoch"]
    _trim()
    assert counters()["devbuf_epoch"] > epoch, "h2_trim released nothing of a unit that held a buffer"
    if tables is not None:                                 # "Registered bases stay" (include/halo2_mi355x.h)
        assert [cs.commit_table_state(n) for n, _ in cs.COMMIT_SHAPES] == tables
        assert all(t[0] == _lib.H2_OK and t[4] == 1 for t in tables), tables
    for size, stream in ((SMALL, s0), (LARGE, s1), (SMALL, s1)):
        step(size, stream)
    assert (allocations[4] > 0) == (allocations[0] > 0), f"the first call after the trim did not rebuild what the first call built: {allocations}"
    # (the second stream ran large first this time: its last small call may still allocate a buffer the large form never uses)
    torch.cuda.synchronize()
    _trim()


# ---- b. the host-slice multiexp's captured launch graphs ------------------------------------------------------------------------------------
HOST_N = (1 << 19) + 4097                                  # the smallest size class with ranges (host_msm_chunks), ragged over three
HOST_CURVE = h.PALLAS


class HostSliceMultiexp:
    """h2_msm from host slices at HOST_N, call by call: fresh scalars every time, the result held to the oracle, the counters' movement
    held to what a call can do -- exactly one of plain / replayed, a capture only with a replay, and a replay only while the DevBuf
    epoch is the one the graphs were captured under."""
    _bases = None

    def __init__(self):
        if HostSliceMultiexp._bases is None:
            bf = co.field_of_curve(HOST_CURVE, "base")
            mont = co.generate_bases(HOST_CURVE, 4343, HOST_N)
            HostSliceMultiexp._bases = (mont, np.ascontiguousarray(co.from_mont(bf, mont.reshape(2 * HOST_N, 4)).reshape(HOST_N, 8)))
        self.calls, self.capture_epoch, self.graphs = 0, None, False

    def forget(self):
        """after an h2_trim: the graphs are gone"""
        self.capture_epoch, self.graphs = None, False

    def call(self, shape):
        """shape "A": Montgomery in, Jacobian out; "B": canonical in, affine out.  -> ("plain" | "capture" | "replay", graph sets dropped)"""
        sf, bf = co.field_of_curve(HOST_CURVE, "scalar"), co.field_of_curve(HOST_CURVE, "base")
        canonical = shape == "B"
        self.calls += 1
        scal = co.random_field(sf, 9900 + self.calls, HOST_N)
        if self.calls % 5 == 3:
            scal[: HOST_N // 2] = 0                        # half the scalars zero: empty digits everywhere in the first ranges
        before = counters()
        got = np.ascontiguousarray(h.best_multiexp(co.from_mont(sf, scal) if canonical else scal, self._bases[1 if canonical else 0], HOST_CURVE,
                                                   form=h.FORM_CANONICAL if canonical else h.FORM_MONTGOMERY, affine=canonical), dtype=np.uint64)
        after = counters()
        if canonical:                                      # canonical coordinates out: back to Montgomery limbs for the oracle's reader
            got = co.to_mont(bf, got.reshape(-1, 4)).reshape(-1)
        got_xy = co.affine_to_ints(HOST_CURVE, got) if canonical else co.jac_to_affine_ints(HOST_CURVE, got)
        d = delta(before, after)
        plain, captured, replayed = (d.get(k, 0) for k in ("host_msm_plain", "host_msm_captured", "host_msm_replayed"))
        dropped = d.get("host_msm_graphs_dropped", 0)
        assert plain + replayed == 1 and captured <= replayed, (self.calls, d)
        kind = "plain" if plain else "capture" if captured else "replay"
        # the result first: a wrong point is the finding, whatever the counters say
        assert got_xy == co.jac_to_affine_ints(HOST_CURVE, co.best_multiexp(HOST_CURVE, scal, self._bases[0])), (self.calls, shape, kind, d)
        if kind == "capture":
            assert after["devbuf_epoch"] == before["devbuf_epoch"], (self.calls, d)          # a capture that had to allocate is not replayable
            self.capture_epoch, self.graphs = after["devbuf_epoch"], True
        elif kind == "replay":
            assert self.graphs and before["devbuf_epoch"] == after["devbuf_epoch"] == self.capture_epoch, \
                (self.calls, d, before["devbuf_epoch"], self.capture_epoch, "replayed although a buffer was (re)allocated or released since the capture")
        if dropped:
            assert dropped == 1 and self.graphs and kind == "plain", (self.calls, d)
            self.graphs = False
        return kind, dropped

    def settle(self, shape, calls=3):
        """`calls` calls of one shape from a state without graphs for it: the first runs plain launches, a later one captures, the last
        replays.  (The call that captures is the first whose DevBuf epoch at entry is the one the call before it left: the second, or
        the third when the first call's own allocations moved the epoch.)"""
        kinds = [self.call(shape)[0] for _ in range(calls)]
        assert kinds[0] == "plain" and kinds.count("capture") == 1 and kinds[-1] in ("capture", "replay"), kinds
        assert all(k == "replay" for k in kinds[kinds.index("capture") + 1:]), kinds
        return kinds


@pytest.fixture
def host_msm():
    torch.cuda.synchronize()
    _trim()
    yield HostSliceMultiexp()
    torch.cuda.synchronize()
    _trim()


def test_host_slice_multiexp_graphs(host_msm):
    """Plain launches, the capture, replays; then another unit's workspace grows (the DevBuf epoch rises): the next call must not
    replay -- one set of graphs dropped, the result still the oracle's -- and the shape is captured and replayed again."""
    kinds = host_msm.settle("A", calls=4)
    assert kinds[-1] == "replay", kinds                    # a replay of graphs captured by an EARLIER call
    epoch = counters()["devbuf_epoch"]
    poly = cs.BY_NAME["kate-division"]
    assert poly.run(LARGE, torch.cuda.current_stream()) == poly.expected(LARGE)
    assert counters()["devbuf_epoch"] > epoch              # (the poly workspace was empty: the fixture's trim)
    assert host_msm.call("A") == ("plain", 1)
    assert [host_msm.call("A")[0] for _ in range(2)] in (["capture", "replay"], ["plain", "capture"])


def test_host_slice_multiexp_graphs_across_shapes(host_msm):
    """The graphs belong to ONE shape: canonical data and an affine result at the same size drop them and are captured in their turn;
    going back drops those."""
    host_msm.settle("A")
    first = host_msm.call("B")
    assert first == ("plain", 1), first
    kinds = [host_msm.call("B")[0] for _ in range(2)]
    assert kinds in (["capture", "replay"], ["plain", "capture"]), kinds
    assert host_msm.call("A") == ("plain", 1)


def test_host_slice_multiexp_graphs_across_trim_and_profiler(host_msm):
    """h2_trim between two replays drops the graphs with the workspaces they name: plain launches, capture and replay follow.  While
    the event profiler is on no call replays; afterwards the shape replays again, or is captured afresh if the profiled call allocated."""
    host_msm.settle("A")
    torch.cuda.synchronize()
    dropped = counters()["host_msm_graphs_dropped"]
    _trim()
    assert counters()["host_msm_graphs_dropped"] == dropped + 1
    host_msm.forget()
    host_msm.settle("A")
    assert h.lib().h2_profile_enable(1) == 0
    try:
        kind, _ = host_msm.call("A")
    finally:
        assert h.lib().h2_profile_enable(0) == 0
        ms, launches = C.c_double(0), C.c_uint64(0)
        for slot in range(4):                              # drains the profiler's pending events
            assert h.lib().h2_profile_read(slot, C.byref(ms), C.byref(launches)) == 0
    assert kind == "plain"
    kinds = [host_msm.call("A")[0] for _ in range(2)]
    assert kinds in (["replay", "replay"], ["plain", "capture"], ["capture", "replay"]), kinds


# ---- c. the opening argument's kept table ---------------------------------------------------------------------------------------------------
def _table_shape(curve, k):
    """(curve, points) of the table of collapsed generators an opening at 2^k leaves, from the library's own switch rule."""
    rounds = int(h.lib().h2_ipa_default_switch_rounds(k, 1))
    assert 0 < rounds < k
    kept = 1 << (k - rounds)
    return curve, kept + (4 if h.lib().h2_commit_pair_supported(kept + 4) else 2)


def test_opening_keeps_and_refills_its_table():
    """opening.create_proof with the default schedule on one stream, proof bytes against the C restatement at every step: the table of
    collapsed generators is registered, refilled in place for other generators and from another k that leaves the same shape, freed and
    registered again for another curve and back, freed by h2_trim and registered again.  The second set of generators collapses to the
    identity in three columns (call_sequences.IDENTITY_COLUMNS): their rows of the refilled table must be the zeros of a fresh one."""
    v, p = h.VESTA, h.PALLAS
    steps = [(v, 16, 0x2600), (v, 16, 0x2700), (v, 17, 0x2800), (p, 16, 0x2900), (v, 16, 0x2600), "trim", (v, 16, 0x2600)]
    assert set(cs.IDENTITY_COLUMNS) == {steps[1][2]} and _table_shape(v, 16)[1] == (1 << 14) + 4       # (the columns are residues modulo the table's 2^14)
    assert _table_shape(v, 16) == _table_shape(v, 17) and _table_shape(v, 16)[1] <= (1 << 17) + 4      # one shape from two sizes, and it is kept
    names = ("ipa_table_registered", "ipa_table_refilled", "ipa_table_freed")
    torch.cuda.synchronize()
    _trim()
    kept, arms = None, []
    try:
        for i, step in enumerate(steps):
            before = counters()
            if step == "trim":
                torch.cuda.synchronize()
                _trim()
                want, kept = ((0, 0, 1) if kept else (0, 0, 0)), None
            else:
                curve, k, seed = step
                assert cs.opening_proof(curve, k, seed) == cs.opening_proof_wanted(curve, k, seed), f"step {i}: the proof is not the restatement's"
                shape = _table_shape(curve, k)
                want = (1, 0, 0) if kept is None else (0, 1, 0) if kept == shape else (1, 0, 1)
                kept = shape
            d = delta(before, counters())
            got = tuple(d.get(name, 0) for name in names)
            assert got == want, f"step {i} {step}: (registered, refilled, freed) moved by {got}, expected {want}"
            arms.append(want)
        assert arms == [(1, 0, 0), (0, 1, 0), (0, 1, 0), (1, 0, 1), (1, 0, 1), (0, 0, 1), (1, 0, 0)]     # the sequence reached every arm it names
    finally:
        for key in [key for key in cs._params if key[1] >= 16]:
            cs._params.pop(key)[0].close()
        torch.cuda.synchronize()
        _trim()


# ---- d. the twiddle cache ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [h.FP, h.FQ], ids=["fp", "fq"])
def test_twiddle_cache_follows_the_root(field):
    """Two primitive roots of order 2^11 alternate at one size: a table is built for each, the first is found again; the curve-point FFT
    of lagrange_basis takes its table (the inverse root's) from the same cache; h2_trim clears it.  Every output is the oracle's."""
    L = 11
    m = fields.MODULUS[field]
    omega = o.omega_for(m, L)
    roots = [omega, pow(omega, 3, m)]
    assert all(pow(w, 1 << (L - 1), m) == m - 1 for w in roots) and roots[0] != roots[1]
    curve = next(c for c in (h.PALLAS, h.VESTA) if fields.CURVE_FIELDS[c][1] == field)
    a = co.random_field(field, 6100 + field, 1 << L)
    g = co.generate_bases(curve, 6200, 1 << L)
    torch.cuda.synchronize()
    _trim()

    def fft(w, built, hits):
        limbs = fields.scalar_limbs(w, field, True)
        before = counters()
        got = h.best_fft(a.copy(), limbs, L, field)
        d = delta(before, counters())
        assert np.array_equal(got, co.best_fft(field, a, limbs, L)), hex(w)
        assert (d.get("twiddle_built", 0), d.get("twiddle_hits", 0)) == (built, hits), (hex(w), d)

    fft(roots[0], 1, 0)
    fft(roots[1], 1, 0)
    fft(roots[0], 0, 1)
    before = counters()
    assert np.array_equal(h.lagrange_basis(g, curve, L), co.lagrange_basis(curve, g, L))
    d = delta(before, counters())
    assert (d.get("twiddle_built", 0), d.get("twiddle_hits", 0)) == (1, 0), d        # omega^-1 is neither omega nor omega^3
    fft(roots[1], 0, 1)
    torch.cuda.synchronize()
    _trim()
    fft(roots[0], 1, 0)
    _trim()
