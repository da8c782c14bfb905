"""The grouped generic multiexp's size limits, replicated on the host (a helper: nothing here is collected): group_geometry follows
csrc/msm_plan.h's, and the limits are found from it by bisection.  tests/test_gpu_generic_paths.py checks the replica against the device's
answer at each limit, tests/test_msm_plan.py against the C++ itself."""

# ---- host replica of group_geometry and its constants (csrc/msm_plan.h)
LDS_CAP = 160 * 1024 - 512          # kLdsCap
NB16 = 1 << 15                      # buckets per window slice at 16-bit windows
LATENCY_SLICES = (5, 2, 2)          # a lone call: nine slices, upper first
THROUGHPUT_SLICES = (9,)


def group_geometry(cols, ns, nb=NB16):
    """(lowb, nh, S) of a group of `ns` window slices over `cols` digit columns, or None where the library's group_geometry fails."""
    lb = (cols - 1).bit_length()
    tb, emax = ns * nb, ns * cols
    for lowb in range(12, 0, -1):
        if lowb + lb > 31:
            continue
        nbk = 1 << lowb
        nh = (tb + nbk - 1) >> lowb
        if nh > 4096:
            break
        avg = emax // nh
        cap_max = (LDS_CAP - nbk * 8) // 4 if nbk * 8 + 64 < LDS_CAP else 0
        cap = min(cap_max, max(4096, avg * 5 // 4 + 1024))
        if avg > 20000 or avg > cap * 9 // 10:
            continue
        S = 4096
        while S > 512 and (nh * 3 + 1 + S * ns) * 4 > LDS_CAP // 2:
            S //= 2
        if S == 4096 and cols // 8192 >= 512 and (nh * 3 + 1 + 8192 * ns) * 4 <= LDS_CAP:
            S = 8192
        if (nh * 3 + 1 + S * ns) * 4 > LDS_CAP:
            continue
        return lowb, nh, S
    return None


def layout(n, slices):
    g = [group_geometry(2 * n, ns) for ns in slices]
    return None if None in g else g


def _first(pred, lo, hi):
    """smallest n in (lo, hi] with pred(n), pred monotone and false at lo"""
    assert not pred(lo) and pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if pred(mid) else (mid, hi)
    return hi


LATENCY_MAX = _first(lambda n: layout(n, LATENCY_SLICES) is None, 1 << 20, 1 << 24) - 1
THROUGHPUT_MAX = _first(lambda n: layout(n, THROUGHPUT_SLICES) is None, 1 << 19, 1 << 23) - 1
_low = lambda n: layout(n, LATENCY_SLICES)[0][0]                       # pass-1 low key bits of the latency layout's first group
LOWB_7 = _first(lambda n: _low(n) <= 7, (1 << 18) + 1, LATENCY_MAX)     # 8 -> 7
LOWB_6 = _first(lambda n: _low(n) <= 6, LOWB_7, LATENCY_MAX)            # 7 -> 6
