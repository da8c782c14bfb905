"""What a commit over a registered basis decides before it launches anything, replicated on the host (a helper: nothing here is collected).

`plan()` follows msm_plan (csrc/msm_plan.h) for calls with a table; `expected()` wraps it in the caller forms of h2_commit,
h2_commit_device, h2_commit_range_device, h2_commit_batch_device and h2_commit_pair_device and returns, field by field, what
h2_commit_last_plan must answer.  The lanes of the accumulate kernel the device holds at once are an input (the GPU test takes them from the
device's first answer); LANES_MI355X is what the CPU coverage test enumerates with.

SWEEP lists the cases tests/test_gpu_commit_plans.py runs; EXCLUDED the plan shapes it leaves out, each with the smallest table that
reaches it -- only shapes whose smallest table has more than 2^19 points may stand there.  tests/test_commit_plan_coverage.py holds
SWEEP and EXCLUDED to `enumerate_projections()`, every shape the replica can produce within BOUNDS."""
from collections import namedtuple

LDS_CAP = 160 * 1024 - 512          # kLdsCap
MAX_C, MAX_C_SHARED = 16, 20        # kMaxC, kMaxCShared
S1_SCALARS = 2048                   # kS1Scalars
MAX_BIG = 32                        # kMaxBig
MAX_COLS = 8                        # kMaxCols
PIPE_CHUNK, PIPE_MAX_CHUNKS = 1 << 18, 16          # kPipeChunk, kPipeMaxChunks (csrc/msm_host.hip)
SUBDIGIT_MAX = (1 << 16) + 4        # pair_subdigit_max (csrc/msm_table.hip)
LANES_MI355X = 256 * 2 * 256        # CUs x H2_ACC9_WAVES workgroups x 256 lanes
MAX_TABLE = 1 << 19                 # the largest table the sweep registers

DIRECT, HOST_RANGE, HOST_PIPELINED, BATCH_COLUMNS, BATCH_FORK, PAIR_TWO_PASS, PAIR_SUBDIGIT = 1, 2, 3, 4, 5, 6, 7      # H2_COMMIT_CALLER_*
ERR_ARGS, ERR_BATCH_SHAPE = "H2_ERR_ARGS", "H2_ERR_BATCH_SHAPE"

FIELDS = ("caller", "caller_count", "cols_first", "cols_last", "empty", "lanes", "c", "W", "m", "K", "T", "lane_div",
          "use_sort2", "s2_lowb", "s2_nh", "s2_side", "s2_s1_scalars", "s2_bins_form", "max_big", "zero_in_sort",
          "fold9", "wide_reduce", "pair", "joined", "add_only", "fold_only")


# ---------------------------------------------------------------------------------------------------- geometry
def windows(c):
    return 255 // c + 1


def sort2_geometry(stride, c, want_s1=False):
    """(lowb, lb, side, s1) or None: sort2_geometry of csrc/msm_plan.h; want_s1 = the caller passes s1_out (msm_plan does, the
    registration check does not)"""
    W, bucket_bits = windows(c), c - 1
    top = W * stride - 1
    if top >= 1 << 31:
        return None
    lb = top.bit_length()
    lowb, side = min(31 - lb, bucket_bits - 9), 0
    if bucket_bits - lowb > 10 and bucket_bits - 9 <= 14 and W <= 64:
        lowb, side = bucket_bits - 9, 1
    if lowb < 1 or bucket_bits - lowb > 12:
        return None
    nh = 1 << (bucket_bits - lowb)
    s1 = S1_SCALARS
    if want_s1 and (nh * 3 + 1 + s1 * W) * 4 > LDS_CAP:
        s1 = 1024
    if (nh * 3 + 1 + s1 * W) * 4 > LDS_CAP:
        return None
    return lowb, lb, side, s1


def pair_geometry(m, c, stride):
    """(lowb, lb, nh, s1) or None"""
    if c > MAX_C or c < 2 or m < 8192:
        return None
    W, tb = windows(c), 2 << (c - 1)
    top = W * stride - 1
    if top >= 1 << 31:
        return None
    lb, kb = top.bit_length(), (tb - 1).bit_length()
    lowb = min(31 - lb, max(1, kb - 9))
    if lowb < 1:
        return None
    nh = (tb + (1 << lowb) - 1) >> lowb
    if nh > 4096:
        return None
    s1 = S1_SCALARS
    while s1 >= 1024 and (nh * 3 + 1 + s1 * W) * 4 > LDS_CAP:
        s1 //= 2
    if s1 < 1024:
        return None
    return lowb, lb, nh, s1


def choose_c(n, shared):
    """window bits of h2_bases_register (shared) / of a generic multiexp"""
    n = n or 1
    if shared:
        return 8 if n <= 384 else 13 if n <= 6144 else 16
    return 10 if n <= 2048 else 13 if n <= 262144 else 16


def make_shape(m, c):
    """(W, NB, items) of a registered commit over m digit columns"""
    return windows(c), 1 << (c - 1), windows(c) * m


def h2_commit_column_window_bits(n):
    c = choose_c(n, True)
    return 17 if c == 16 and n >= 1 << 18 and n + 1 < 1 << 31 and sort2_geometry(n + 1, 17) else c


def table_bits(points, bits):
    """the width h2_bases_register_ex(points, bits) builds, or None where it refuses"""
    if not bits:
        return choose_c(points, True)
    if bits < 4 or bits > MAX_C_SHARED or (bits > MAX_C and not sort2_geometry(points + 1, bits)):
        return None
    return bits


def pair_supported(n):
    return int(8 <= n <= 1 << 26 and pair_geometry(n, choose_c(n, True), n + 1) is not None)


# ---------------------------------------------------------------------------------------------------- msm_plan with a table
def plan(lanes, points, c, n_used, blind, K=1, pair=False, add_into=False, fold_only=False, fraction=1.0):
    """The summary of one msm_launch over the table of `points` points and c-bit windows (caller fields: DIRECT), or the error it
    answers before launching anything."""
    stride = points + 1
    m = n_used + (1 if blind else 0)
    r = dict.fromkeys(FIELDS, 0)
    r.update(caller=DIRECT, caller_count=1, c=c)
    if m == 0 and not fold_only:
        r.update(empty=2 if add_into else 1, add_only=int(add_into))
        return r
    if fold_only and m < 1:
        m = 1
    W, NB, all_items = make_shape(m, c)
    if K > 1 and (K > MAX_COLS or pair or add_into or fold_only or n_used == 0):
        return ERR_BATCH_SHAPE
    slices = 2 if pair else 1
    tb = slices * NB
    if all_items >= 1 << 31:
        return ERR_ARGS
    usable = max(256, int(lanes * fraction) // 256 * 256)
    lane_div = 8 if all_items < 1 << 20 else 16
    joined = K > 1
    T = min(usable, max(256, ((K if joined else 1) * all_items // lane_div + 255) // 256 * 256))
    use_sort2, lowb, nh, side, s1 = False, 0, 0, 0, 0
    if pair:
        g = pair_geometry(m, c, stride)
        if g is None:
            return ERR_ARGS
        use_sort2, (lowb, _, nh, s1) = True, g
    elif c > MAX_C or (NB >= 4096 and (m >= 8192 or K > 1)):
        g = sort2_geometry(stride, c, True)
        if g is not None:
            use_sort2, (lowb, _, side, s1) = True, g
            nh = NB >> lowb
    if c > MAX_C and not use_sort2:
        return ERR_ARGS
    if K > 1 and not use_sort2:
        return ERR_BATCH_SHAPE
    fold9 = NB >= 128 and not add_into and not fold_only
    if K > 1 and not fold9:
        return ERR_BATCH_SHAPE
    bins_form = False
    if use_sort2:
        nbk = 1 << lowb
        cap_max = (LDS_CAP - nbk * 8) // 4 if nbk * 8 + 64 < LDS_CAP else 0
        cap = min(cap_max, max(4096, all_items // nh * 5 // 4 + 1024))
        bins_form = lowb <= 12 and (tb + nbk - 1) >> lowb == nh and cap > 0 and all_items // nh <= cap * 9 // 10
    if K > 1 and not bins_form:
        return ERR_BATCH_SHAPE
    r.update(lanes=lanes, W=W, m=m, K=K, T=T, lane_div=lane_div, use_sort2=int(use_sort2), s2_lowb=lowb, s2_nh=nh, s2_side=side,
             s2_s1_scalars=s1, s2_bins_form=int(bins_form), max_big=MAX_BIG if all_items >= 3 << 20 else 0,
             zero_in_sort=int(use_sort2 and bins_form and not fold_only), fold9=int(fold9), wide_reduce=int(NB > 32768), pair=int(pair),
             joined=int(joined), add_only=int(add_into and not fold_only), fold_only=int(fold_only))
    return r


# ---------------------------------------------------------------------------------------------------- the callers
# points: table size; bits: what h2_bases_register_ex is asked for (0: the library's choice); entry: device / range / host / batch / pair;
# first: h2_commit_range_device's first column; K: h2_commit_batch_device's count; chunk: host_commit_chunk (0: the default)
Case = namedtuple("Case", "points bits entry n_used blind K pair_shift first chunk note", defaults=(1, -1, 0, 0, ""))


def host_ranges(n, chunk_option):
    """(ranges, scalars of the last one) of commit_host_pipelined_locked"""
    chunk = chunk_option or PIPE_CHUNK
    if n < 2 * chunk:
        chunk = max(n, 1)
    chunk = max(chunk, (n + PIPE_MAX_CHUNKS - 1) // PIPE_MAX_CHUNKS)
    chunks = max(1, (n + chunk - 1) // chunk)
    return chunks, n - (chunks - 1) * chunk


def expected(case, lanes):
    """What h2_commit_last_plan answers behind the case's call (on the caller's stream; stream NULL for the host entry), or the error of
    the call itself."""
    c = table_bits(case.points, case.bits)
    if c is None:
        return ERR_ARGS
    W = windows(c)
    if case.entry in ("device", "range"):
        return plan(lanes, case.points, c, case.n_used, case.blind)
    if case.entry == "host":
        chunks, last = host_ranges(case.n_used, case.chunk)
        r = plan(lanes, case.points, c, last, case.blind, add_into=True)
        if isinstance(r, str):
            return r
        r.update(caller=HOST_PIPELINED if chunks > 1 else HOST_RANGE, caller_count=chunks, fold_only=1)
        return r
    if case.entry == "pair":
        n = case.points
        assert case.n_used == n and not case.blind
        if n < 8:
            return ERR_ARGS
        if c == 16 and W == 16 and n <= SUBDIGIT_MAX:
            r = dict.fromkeys(FIELDS, 0)
            r.update(caller=PAIR_SUBDIGIT, caller_count=1, lanes=lanes, c=c, W=W, m=n, K=1, lane_div=8, pair=1,
                     T=min(lanes, max(256, (n * 32 // 8 + 255) // 256 * 256)))
            return r
        r = plan(lanes, n, c, n, False, pair=True)
        if not isinstance(r, str):
            r.update(caller=PAIR_TWO_PASS)
        return r
    assert case.entry == "batch"
    count, n = case.K, case.n_used
    if count >= 2 and n > 0 and not (n >= 1 << 19 and count > 3):
        groups = (count + MAX_COLS - 1) // MAX_COLS
        r = plan(lanes, case.points, c, n, case.blind, K=count // groups)       # the LAST group's (groups are balanced, larger ones first)
        if r == ERR_ARGS:
            return r
        if r != ERR_BATCH_SHAPE:
            r.update(caller=BATCH_COLUMNS, caller_count=groups, cols_first=count // groups + (1 if count % groups else 0), cols_last=count // groups)
            return r
    r = plan(lanes, case.points, c, n, case.blind)
    if not isinstance(r, str):
        r.update(caller=BATCH_FORK, caller_count=count)
    return r


# ---------------------------------------------------------------------------------------------------- projection and enumeration
def projection(r):
    """The discrete fields of a summary: what selects kernels, LDS sizes and strides."""
    if r["empty"]:
        return ("empty", r["empty"], r["caller"])
    usable = max(256, r["lanes"] // 256 * 256)
    raw = ((r["K"] if r["joined"] else 1) * r["W"] * r["m"] // r["lane_div"] + 255) // 256 * 256
    if r["caller"] == PAIR_SUBDIGIT:
        raw = (r["m"] * 32 // 8 + 255) // 256 * 256
    clamp = "low" if raw <= 256 else "high" if raw >= usable else "free"
    return (r["caller"], r["c"], r["lane_div"], r["use_sort2"], r["s2_side"], r["s2_bins_form"], int(r["max_big"] != 0), r["zero_in_sort"],
            r["fold9"], r["wide_reduce"], r["pair"], r["joined"], r["add_only"], r["fold_only"], clamp)


BOUNDS = dict(max_points=1 << 20, widths=range(4, 21), counts=range(1, 10), chunks=(0, 1 << 17))
STANDARD_TABLES = ((1 << 13) + 3, (1 << 16) + 3, (1 << 18) + 3, 1 << 19)      # what the enumerated cases register where one of them gives the shape


def _tables_for(c, max_points):
    """Table sizes that can change a summary at width c: both sides of every size at which the table index gains a bit, of the
    library's own width edges, of the pair and batch and host thresholds -- and the largest table."""
    W = windows(c)
    out = {8, 384, 385, 6144, 6145, 8191, 8192, SUBDIGIT_MAX, SUBDIGIT_MAX + 1, 1 << 18, (1 << 18) + 1, (1 << 19) - 1, 1 << 19, (1 << 19) + 1, max_points}
    for bit in range(8, 32):
        n = (1 << bit) // W - 1       # the largest table whose last index W * (n + 1) - 1 stays below 2^bit
        out |= {n, n + 1}
    return sorted(n for n in out if 8 <= n <= max_points and table_bits(n, c) == c)


def _walk(f, lo, hi, flo=None, fhi=None):
    """f at every step of [lo, hi], f a tuple of functions monotone in their argument: bisect wherever the ends differ"""
    flo = f(lo) if flo is None else flo
    fhi = f(hi) if fhi is None else fhi
    if flo == fhi or hi - lo <= 1:
        return
    mid = (lo + hi) // 2
    fmid = f(mid)
    _walk(f, lo, mid, flo, fmid)
    _walk(f, mid, hi, fmid, fhi)


def enumerate_projections(lanes=LANES_MI355X, bounds=BOUNDS):
    """{projection: smallest witness Case found} over every table, width, entry point, column count and column length within bounds.
    For a fixed table and entry every field of a summary is monotone in the column length, so the lengths are walked by bisection (the
    last range of a host commit: between the teeth of its sawtooth).  A table enters a summary through its two-pass geometry alone, so
    of the tables that share one only the largest is walked; the paired commit, whose column IS the table, is walked over the table
    sizes between two neighbours of _tables_for, where its geometry is fixed."""
    found = {}

    def note(case):
        r = expected(case, lanes)
        if isinstance(r, str):
            return r
        p = projection(r)
        old = found.get(p)
        if old is None or (case.points, case.n_used + case.blind, case.blind) < (old.points, old.n_used + old.blind, old.blind):
            found[p] = case
        return p

    for c in bounds["widths"]:
        tables = _tables_for(c, bounds["max_points"])
        largest = {}
        for points in tables:
            g = sort2_geometry(points + 1, c, True)
            largest[g and (g[0], g[2], g[3])] = points
        for points in sorted(largest.values()):
            variants = [dict(entry="device", blind=0)] + [dict(entry="host", blind=0, chunk=ch) for ch in bounds["chunks"]]
            variants += [dict(entry="batch", blind=0, K=k) for k in bounds["counts"]]
            for v in variants:
                segments = [(0, points)]
                if v["entry"] == "host":
                    chunk = v["chunk"] or PIPE_CHUNK
                    segments = [(0, 2 * chunk - 1), (2 * chunk, 2 * chunk)] + [(k * chunk + 1, (k + 1) * chunk) for k in range(2, PIPE_MAX_CHUNKS)]
                for lo, hi in segments:
                    if lo <= points:
                        _walk(lambda n: note(Case(points, c, n_used=n, **v)), lo, min(hi, points))
                for n_used in (0, points):                      # a blind adds one digit column: the identity's neighbour and the widest call
                    note(Case(points, c, n_used=n_used, **dict(v, blind=1)))
        for lo, hi in zip([7] + tables, tables):
            _walk(lambda n: note(Case(n, c, "pair", n, 0, pair_shift=0)), lo + 1, hi)
    return found


def smallest_table(case, lanes=LANES_MI355X, bounds=BOUNDS):
    """the case over the smallest table that gives its projection: the column's own length, or the first size above it at which the
    geometry changes (a paired commit's column is its table, and the enumeration already walked it down)"""
    want = projection(expected(case, lanes))
    if case.entry == "pair":
        return case
    floor = max(case.n_used, 8)
    for points in sorted({floor} | {t for t in _tables_for(case.bits, bounds["max_points"]) if floor <= t < case.points}):
        r = expected(case._replace(points=points), lanes)
        if not isinstance(r, str) and projection(r) == want:
            return case._replace(points=points)
    return case


def shrink(case, lanes=LANES_MI355X):
    """the same projection from the smallest standard table that gives it (so that the sweep registers few tables), else from the
    smallest table there is"""
    want = projection(expected(case, lanes))
    small = smallest_table(case, lanes)
    if case.entry != "pair":
        for points in STANDARD_TABLES:
            if points >= small.points:
                r = expected(case._replace(points=points), lanes)
                if not isinstance(r, str) and projection(r) == want:
                    return case._replace(points=points)
    return small


# ---------------------------------------------------------------------------------------------------- the sweep
def _first(pred, lo, hi):
    """smallest n in (lo, hi] with pred(n), pred monotone and false at lo"""
    assert not pred(lo) and pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if pred(mid) else (mid, hi)
    return hi


SMALL = (1 << 13) + 3                                                             # one small table for every width
SIDE_EDGE = _first(lambda n: sort2_geometry(n + 1, 20, True)[2] == 1, 1 << 18, 1 << 19)      # smallest 20-bit table with the side array


def _chunked_pass2():
    """(points, bits, n_used) of the smallest table at or below 2^20 points whose full column, committed alone, takes the chunked pass 2, or
    None.  (A PAIRED commit over 7- to 9-bit windows has 64 to 256 pass-1 bins and takes it from 63561 points: the enumeration finds those.)"""
    best = None
    for c in range(13, 21):
        ok_ = lambda n: (lambda r: not isinstance(r, str) and r["use_sort2"] == 1 and r["s2_bins_form"] == 0)(plan(LANES_MI355X, n, c, n, 0))
        if table_bits(1 << 20, c) == c and ok_(1 << 20):
            n = _first(ok_, 8192, 1 << 20)
            if best is None or n < best[0]:
                best = (n, c, n)
    return best


CHUNKED = _chunked_pass2()


def _threshold_cases():
    """max_big off / on at W * m either side of 3 * 2^20 and lane_div 8 / 16 either side of 2^20, at 4-bit windows (W = 64)"""
    W = windows(4)
    big, div = (3 << 20) // W, (1 << 20) // W
    return [Case(big, 4, "device", big - 1, 0, note="max_big off"), Case(big, 4, "device", big, 0, note="max_big on"),
            Case(big, 4, "device", div - 1, 0, note="lane_div 8"), Case(big, 4, "device", div, 0, note="lane_div 16")]


def _explicit_sweep():
    s = []
    for bits in range(4, 21):                                                     # every width over one small table
        for n_used, blind in ((SMALL, 0), (SMALL - 1, 1), (8192, 0), (8191, 0), (2, 0), (1, 1), (0, 0), (0, 1)):
            s.append(Case(SMALL, bits, "device", n_used, blind, note="width sweep"))
    for points in (384, 385, 6144, 6145):                                         # the library's own width edges
        s.append(Case(points, 0, "device", points, 1, note="width edge"))
    s.append(Case(SIDE_EDGE, 20, "device", SIDE_EDGE, 1, note="side array"))
    s.append(Case(SIDE_EDGE - 1, 20, "device", SIDE_EDGE - 1, 1, note="side array off"))
    if CHUNKED and CHUNKED[0] <= MAX_TABLE:
        s.append(Case(CHUNKED[0], CHUNKED[1], "device", CHUNKED[2], 0, note="chunked pass 2"))
        s.append(Case(CHUNKED[0], CHUNKED[1], "device", CHUNKED[2] - 1, 0, note="chunked pass 2 off"))
    s += _threshold_cases()
    for points, bits in ((8191, 0), (8192, 0), (8192, 13), (SUBDIGIT_MAX, 0), (SUBDIGIT_MAX + 1, 0)):      # the paired commit
        for shift in (0, 1, (points - 1).bit_length() - 1):
            s.append(Case(points, bits, "pair", points, 0, pair_shift=shift, note="pair"))
    for points, bits in ((1 << 11, 13), (1 << 13, 16)):                           # joined groups
        for K in (1, 2, 8, 9):
            s.append(Case(points, bits, "batch", points, 1, K=K, note="batch"))
        s.append(Case(points, bits, "batch", points - 5, 0, K=3, note="batch, short columns"))
    s.append(Case(1 << 19, 0, "batch", 1 << 19, 0, K=4, note="batch, fork per column"))
    s.append(Case(384, 0, "batch", 384, 1, K=3, note="batch, narrow windows fork"))
    s.append(Case(1 << 18, 17, "host", 1 << 18, 1, chunk=1 << 17, note="host, two ranges"))
    s.append(Case(1 << 18, 17, "host", 1 << 18, 1, note="host, one range"))
    s.append(Case(SMALL, 0, "host", SMALL, 0, note="host, one range"))
    for first, n_used in ((0, SMALL), (1, SMALL - 1), (SMALL - 1, 1), (5, 0)):       # h2_commit_range_device
        s.append(Case(SMALL, 0, "range", n_used, 0, first=first, note="range"))
    s.append(Case(SMALL, 0, "range", 0, 1, first=SMALL, note="range"))
    return s


def _build_sweep():
    explicit = _explicit_sweep()
    have = set()
    for case in explicit:
        r = expected(case, LANES_MI355X)
        if not isinstance(r, str):
            have.add(projection(r))
    extra, excluded = [], []
    for p, case in sorted(enumerate_projections().items(), key=lambda kv: (kv[1].points, kv[1].bits, kv[1].n_used, str(kv[0]))):
        if p in have:
            continue
        case = shrink(case)
        if case.points > MAX_TABLE:
            excluded.append((p, case.points, f"the smallest table reaching it has {case.points} points, more than 2^19"))
        else:
            extra.append(case._replace(note="enumerated"))
    return explicit + extra, excluded


SWEEP, EXCLUDED = _build_sweep()
