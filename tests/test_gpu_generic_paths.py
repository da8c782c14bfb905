"""Every form of the generic multiexp (h2_msm_device without a registered basis; best_multiexp, arithmetic.rs:143-180) against the C oracle at
the edges of its dispatch, with the form each call took read back through h2_msm_last_path:

  ONE_PASS            below 65536 scalars (window bits 10 up to 2048 scalars, 13 above)
  TWO_PASS            65536 .. 2^18 scalars; every size from 65536 under h2_profile_enable (and H2_TIMELINE=1)
  GROUPED_LATENCY     a lone call from 2^18 + 1 scalars (16-bit windows, 5 + 2 + 2 slices) while its layout fits: group_geometry
  GROUPED_THROUGHPUT  another stream's call in flight, below 2^22 scalars, while the one-group layout fits
  SLICE_SPLIT         the sizes the grouped form declines (round 5's split of the window slices)

The size limits of the grouped form come from a host replica of group_geometry (csrc/msm_plan.h; the replica is tests/generic_plans.py); the device's answer at each limit
checks the replica.  Bases repeat with an odd period (BASE_PERIOD) so that 5 M-point inputs cost one 2^20-point generation per curve; a
column index that lost its high bits would still pick another base."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import halo2_amd as h
from halo2_amd import _lib, fields
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = {k: int(v) for k, v in re.findall(r"#define H2_MSM_PATH_([A-Z_]+) (\d+)", open(os.path.join(ROOT, "include", "halo2_mi355x.h")).read())}
ONE_PASS, TWO_PASS, SLICE_SPLIT = PATH["ONE_PASS"], PATH["TWO_PASS"], PATH["SLICE_SPLIT"]
LATENCY, THROUGHPUT = PATH["GROUPED_LATENCY"], PATH["GROUPED_THROUGHPUT"]

from generic_plans import LATENCY_MAX, LOWB_6, LOWB_7, THROUGHPUT_MAX, _low      # the host replica of group_geometry and the limits it gives


def test_replica_limits_match_the_documented_ones():
    assert (LATENCY_MAX, THROUGHPUT_MAX) == (5120255, 2560127)
    assert (LOWB_7, LOWB_6) == (1280064, 2560128)
    assert _low(LOWB_7 - 1) == 8 and _low(LOWB_6 - 1) == 7


# ---- inputs: prefixes of one long column per curve, oracle results cached per (curve, n)
BASE_PERIOD = (1 << 20) + 7
MAX_N = LATENCY_MAX + 1
_cache = {}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def bases(curve):
    if ("b", curve) not in _cache:
        period = co.generate_bases(curve, 7100 + curve, BASE_PERIOD)
        full = np.ascontiguousarray(np.resize(period, (MAX_N, 8)))
        _cache["b", curve] = (full, _dev(full))
    return _cache["b", curve]


def scalars(curve):
    if ("s", curve) not in _cache:
        full = co.random_field(fields.CURVE_FIELDS[curve][1], 7200 + curve, MAX_N)
        _cache["s", curve] = (full, _dev(full))
    return _cache["s", curve]


def want(curve, n):
    if ("w", curve, n) not in _cache:
        _cache["w", curve, n] = co.jac_to_affine_ints(curve, co.best_multiexp(curve, scalars(curve)[0][:n], bases(curve)[0][:n]))
    return _cache["w", curve, n]


def enqueue(curve, n):
    """h2_msm_device on torch's current stream over the first n scalars / bases; returns the device output and the form it took"""
    out = h.best_multiexp(scalars(curve)[1][:n], bases(curve)[1][:n], curve)
    return out, last_path()


def got_of(curve, out):
    return co.jac_to_affine_ints(curve, np.ascontiguousarray(out.cpu().numpy().view(np.uint64)))


def last_path(stream=None):
    import torch
    s = (stream or torch.cuda.current_stream()).cuda_stream
    p, g, t, c = C.c_int(), C.c_int(), C.c_uint(), C.c_int()
    rc = h.lib().h2_msm_last_path(C.c_void_p(s), C.byref(p), C.byref(g), C.byref(t), C.byref(c))
    assert rc == 0, f"h2_msm_last_path: {rc}"
    return p.value, g.value, t.value, c.value


def device_lanes():
    """resident lanes of the M9 accumulate, as msm_launch.hip sizes them: CUs x H2_ACC9_WAVES (2) workgroups of 256 lanes"""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 2 * 256


def lone(curve, n):
    """one call with nothing else of the library in flight; checked against the oracle; returns its form"""
    import torch
    torch.cuda.synchronize()
    out, path = enqueue(curve, n)
    torch.cuda.synchronize()
    assert got_of(curve, out) == want(curve, n), (curve, n, path)
    return path


# (n, form, window bits, groups) at both sides of every threshold of the dispatch
SWEEP = [
    (1024, ONE_PASS, 10, 1), (1025, ONE_PASS, 10, 1),
    (2048, ONE_PASS, 10, 1), (2049, ONE_PASS, 13, 1),                  # choose_c: 10 bits up to 2048 scalars
    (65535, ONE_PASS, 13, 1), (65536, TWO_PASS, 13, 1),
    (131072, TWO_PASS, 13, 1), (131073, TWO_PASS, 13, 1),
    (1 << 18, TWO_PASS, 13, 1), ((1 << 18) + 1, LATENCY, 16, 3),      # 16 bits and the grouped form from 2^18 + 1
    (LOWB_7 - 1, LATENCY, 16, 3), (LOWB_7, LATENCY, 16, 3),
    (LOWB_6 - 1, LATENCY, 16, 3), (LOWB_6, LATENCY, 16, 3),
    (1 << 22, LATENCY, 16, 3),
    (LATENCY_MAX, LATENCY, 16, 3), (LATENCY_MAX + 1, SLICE_SPLIT, 16, 2),
]


def test_last_path_before_any_call_is_refused():
    import torch
    # torch hands streams out round-robin from a pool of 32 per priority: a default-priority stream may be one that an earlier test
    # already ran a multiexp on; no test uses the high-priority pool, so this one is fresh
    s = torch.cuda.Stream(priority=-1)
    assert h.lib().h2_msm_last_path(C.c_void_p(s.cuda_stream), None, None, None, None) == _lib.H2_ERR_ARGS


def test_boundary_sweep_lone_calls():
    """Lone calls on one stream, the curves alternating: the form, the window bits and the group count on each side of every threshold."""
    import torch
    lanes = device_lanes()
    with torch.cuda.stream(torch.cuda.Stream()):
        assert h.lib().h2_msm_window_bits(2048) == 10 and h.lib().h2_msm_window_bits(2049) == 13
        for i, (n, form, c, groups) in enumerate(SWEEP):
            curve = (h.PALLAS, h.VESTA)[i % 2]
            path, g, acc, bits = lone(curve, n)
            assert (path, bits, g) == (form, c, groups), (n, curve, path, g, acc, bits)
            assert bits == h.lib().h2_msm_window_bits(n)
            assert 0 < acc <= lanes and acc % 256 == 0, (n, acc)


def test_throughput_form_at_its_sizes():
    """A fresh stream Y enqueues while a 2^22 latency-form call is in flight on X: the throughput form (one group) up to the one-group
    layout's limit, round 5's slice split from there to 2^22 - 1 (the documented fallback), and the latency form again at 2^22."""
    import torch
    curve = h.PALLAS
    x = torch.cuda.Stream()
    with torch.cuda.stream(x):                                           # warm-up: X's workspaces and side streams exist
        enqueue(curve, 1 << 22)
    torch.cuda.synchronize()
    cases = [((1 << 20) + 1, THROUGHPUT, 1), ((1 << 21) + 3, THROUGHPUT, 1), (THROUGHPUT_MAX, THROUGHPUT, 1),
             (THROUGHPUT_MAX + 1, SLICE_SPLIT, 2), ((1 << 22) - 1, SLICE_SPLIT, 2), (1 << 22, LATENCY, 3)]
    for n, form, groups in cases:
        y = torch.cuda.Stream()
        with torch.cuda.stream(x):
            out_x, path_x = enqueue(curve, 1 << 22)
        with torch.cuda.stream(y):
            out_y, path_y = enqueue(curve, n)
        torch.cuda.synchronize()
        assert path_x[:2] == (LATENCY, 3), (n, path_x)
        assert path_y[:2] == (form, groups) and path_y[3] == 16, (n, path_y)
        assert got_of(curve, out_x) == want(curve, 1 << 22), n
        assert got_of(curve, out_y) == want(curve, n), (n, path_y)


def _drain_profile():
    tot, cnt = C.c_double(), C.c_uint64()
    for slot in range(4):
        h.lib().h2_profile_read(slot, C.byref(tot), C.byref(cnt))


@pytest.mark.parametrize("curve", [h.PALLAS, h.VESTA])
def test_profiling_takes_the_two_pass_path(curve):
    """Under h2_profile_enable every generic call from 65536 scalars takes the plain two-pass sort with the endomorphism split inside it:
    across its bin-bit steps (2^19, 2^20), and with the split's edge scalars and the top window's boundary scalars at 2^19."""
    import torch
    from glv_edge_scalars import endomorphism_edge_values, top_window_boundary_values
    sf = fields.CURVE_FIELDS[curve][1]
    n19 = 1 << 19
    edge = endomorphism_edge_values(curve)
    edge_sc = fields.to_limbs((edge * (n19 // len(edge) + 1))[:n19], sf, True)
    rng = random.Random(7300 + curve)
    crafted = top_window_boundary_values(curve, rng)
    top_sc = co.random_field(sf, 7310 + curve, n19)
    idx = rng.sample(range(n19), len(crafted))
    top_sc[idx] = fields.to_limbs(crafted, sf, True)
    b = bases(curve)
    torch.cuda.synchronize()
    assert h.lib().h2_profile_enable(1) == 0
    try:
        with torch.cuda.stream(torch.cuda.Stream()):
            for n in ((1 << 18) + 1, (1 << 19) + 1, (1 << 20) + 1, (1 << 21) + 3):
                path = lone(curve, n)
                assert path[:2] == (TWO_PASS, 1) and path[3] == 16, (n, path)
            for name, sc in (("edge", edge_sc), ("top window", top_sc)):
                out = h.best_multiexp(_dev(sc), b[1][:n19], curve)
                path = last_path()
                torch.cuda.synchronize()
                assert path[:2] == (TWO_PASS, 1), (name, path)
                assert got_of(curve, out) == co.jac_to_affine_ints(curve, co.best_multiexp(curve, sc, b[0][:n19])), name
    finally:
        torch.cuda.synchronize()
        _drain_profile()
        h.lib().h2_profile_enable(0)
    with torch.cuda.stream(torch.cuda.Stream()):                         # and back to the grouped form once profiling is off
        assert lone(curve, (1 << 19) + 1)[0] == LATENCY


def test_lane_fraction_in_the_grouped_form():
    """msm_lane_fraction narrows the grouped form's accumulate (minus the CUs left to the chain links, never below 512 lanes) and never
    changes its result.  The option takes (0.05, 1]: smaller fractions are refused and leave the setting as it was."""
    import torch
    curve, n = h.PALLAS, (1 << 20) + 1
    lanes = device_lanes()
    spare = max(1, lanes // 512 // 32)
    lib = h.lib()
    try:
        with torch.cuda.stream(torch.cuda.Stream()):
            for f in (1.0, 0.5, 0.2, 0.06):
                assert lib.h2_set_option(b"msm_lane_fraction", f) == 0
                path, g, acc, _ = lone(curve, n)
                assert (path, g) == (LATENCY, 3), (f, path, g)
                bound = max(512, int(lanes * f) // 512 * 512)
                assert 512 <= acc <= bound, f"fraction {f}: accumulate of {acc} lanes, at most {bound} allowed ({lanes} resident)"
                assert acc == max(512, int(lanes * f) // 512 * 512 - 512 * min(spare, 64)), (f, acc)
            for f in (0.05, 0.02, 0.01, 0.0):
                assert lib.h2_set_option(b"msm_lane_fraction", f) == _lib.H2_ERR_ARGS, f
            assert lone(curve, n)[2] == max(512, int(lanes * 0.06) // 512 * 512 - 512 * min(spare, 64))
    finally:
        lib.h2_set_option(b"msm_lane_fraction", 1.0)


def test_lane_fraction_below_the_spare_cus():
    """The same bound where the CUs kept from the accumulate outnumber the fraction's share (laboratory build, H2_GG_SPARE=64: 32768
    lanes kept back; at fraction 0.2 of an MI355X's 131072 that is more than the share): the accumulate must shrink to 512 lanes, not
    wrap round to every lane there is."""
    if not os.environ.get("H2_AB_CHILD"):
        from conftest import run_test_in_ab_child
        run_test_in_ab_child(__file__, "test_lane_fraction_below_the_spare_cus", H2_GG_SPARE="64")
        return
    import torch
    curve, n = h.VESTA, (1 << 20) + 1
    lanes = device_lanes()
    try:
        with torch.cuda.stream(torch.cuda.Stream()):
            for f in (1.0, 0.2, 0.06):
                assert h.lib().h2_set_option(b"msm_lane_fraction", f) == 0
                path, g, acc, _ = lone(curve, n)
                assert (path, g) == (LATENCY, 3)
                assert 512 <= acc <= max(512, int(lanes * f) // 512 * 512), f"fraction {f}: accumulate of {acc} lanes ({lanes} resident)"
                assert acc == max(512, int(lanes * f) // 512 * 512 - 512 * 64), (f, acc)
    finally:
        h.lib().h2_set_option(b"msm_lane_fraction", 1.0)


@pytest.mark.parametrize("order", [(h.VESTA, h.PALLAS), (h.PALLAS, h.VESTA)])
def test_both_curves_on_one_fresh_stream(order):
    """The latency form of both curves on ONE fresh stream (one context), in both orders: the second curve's chain links must run with
    the LDS they ask for even though the context set its attributes for the first."""
    import torch
    with torch.cuda.stream(torch.cuda.Stream()):
        for curve in order + order:
            path = lone(curve, (1 << 18) + 1)
            assert path[:2] == (LATENCY, 3), (curve, path)
