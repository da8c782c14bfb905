"""Both multiexp plans (csrc/msm_plan.h: msm_plan for registered and plain generic calls, grouped_plan for the grouped generic form) are
plain C++ with no HIP in them: tests/native/msm_plan_check.cpp compiles the header for the CPU -- the same text the library plans with --
and this module holds it against the Python replicas the plan-coverage tests rest on (tests/commit_plans.py, tests/generic_plans.py),
against what the kernels assume of a plan, and against the plans of the commit before the header existed (tests/msm_plans_parent.txt)."""
import os
import re
import subprocess

import pytest

import commit_plans as cp
import generic_plans as gp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES = (cp.LANES_MI355X, 256 * 3 * 256, 304 * 2 * 256, 1024)
ERR_ARGS = int(re.search(r"#define H2_ERR_ARGS \(?(-?\d+)\)?", open(os.path.join(ROOT, "include", "halo2_mi355x.h")).read()).group(1))


def plan_calls(case, lanes):
    """The msm_plan calls behind a case, as arguments of cp.plan(), mapped the way cp.expected() maps them: the device or range call; the
    last range of a host commit (add_into) and the fold the ranges share; the paired call where the sub-digit form does not take it; a
    batch's first and last group and the commit per column it falls back to where the batched form refuses (or is not asked)."""
    c = cp.table_bits(case.points, case.bits)
    if c is None:
        return []
    call = lambda n_used, blind, **kw: (lanes, case.points, c, n_used, int(blind), kw.get("K", 1), int(kw.get("pair", False)),
                                        int(kw.get("add_into", False)), int(kw.get("fold_only", False)))
    if case.entry in ("device", "range"):
        return [call(case.n_used, case.blind)]
    if case.entry == "host":
        return [call(cp.host_ranges(case.n_used, case.chunk)[1], case.blind, add_into=True), call(0, 0, fold_only=True)]
    if case.entry == "pair":
        if case.points < 8 or (c == 16 and cp.windows(c) == 16 and case.points <= cp.SUBDIGIT_MAX):
            return []
        return [call(case.points, 0, pair=True)]
    assert case.entry == "batch"
    calls = []
    if case.K >= 2 and case.n_used > 0 and not (case.n_used >= 1 << 19 and case.K > 3):
        groups = (case.K + cp.MAX_COLS - 1) // cp.MAX_COLS                                          # balanced groups, larger ones first
        calls += [call(case.n_used, case.blind, K=case.K // groups + (1 if case.K % groups else 0)), call(case.n_used, case.blind, K=case.K // groups)]
    return calls + [call(case.n_used, case.blind)]


def replica(call):
    lanes, points, c, n_used, blind, K, pair, add_into, fold_only = call
    return cp.plan(lanes, points, c, n_used, blind, K=K, pair=bool(pair), add_into=bool(add_into), fold_only=bool(fold_only))


# generic calls: (lanes, scalars, instrumented, another stream's multiexp in flight)
L0 = cp.LANES_MI355X
GENERIC = [(L0, n, 0, 0) for n in (1, 2048, 2049, 65535, 65536, 1 << 18, (1 << 18) + 1, 1 << 19, 1 << 20, gp.LOWB_7 - 1, gp.LOWB_7, gp.LOWB_6 - 1, gp.LOWB_6,
                                   gp.LATENCY_MAX, gp.LATENCY_MAX + 1, 1 << 22)]
GENERIC += [(L0, n, 0, 1) for n in ((1 << 18) + 1, 1 << 20, gp.THROUGHPUT_MAX, gp.THROUGHPUT_MAX + 1, (1 << 22) - 1, 1 << 22)]
GENERIC += [(L0, n, 1, f) for n in (65536, (1 << 18) + 1, 1 << 20, gp.LATENCY_MAX + 1) for f in (0, 1)]
GEOMETRY = [(2 * n, ns) for n in ((1 << 18) + 1, gp.LOWB_7 - 1, gp.LOWB_7, gp.LOWB_6 - 1, gp.LOWB_6, gp.THROUGHPUT_MAX, gp.THROUGHPUT_MAX + 1, gp.LATENCY_MAX,
                                  gp.LATENCY_MAX + 1) for ns in (5, 2, 9)]
WIDTHS = [("C", n, s) for s, edges in ((1, (384, 385, 6144, 6145)), (0, (2048, 2049, 262144, 262145))) for n in edges]
WIDTHS += [("W", (1 << 18) - 1), ("W", 1 << 18), ("S", 8191), ("S", 8192)]
WIDTHS += [("R", points, bits) for points in (cp.SMALL, cp.SIDE_EDGE - 1, cp.SIDE_EDGE) for bits in range(4, 22)]


def _build(exe, *flags):
    return subprocess.run(["g++", "-O2", "-std=c++17", *flags, os.path.join(ROOT, "tests", "native", "msm_plan_check.cpp"), "-o", exe], capture_output=True, text=True)


@pytest.fixture(scope="module")
def report():
    """the driver's answers to every call above, one line per call in the order asked, and its summary lines"""
    cases = list(cp.SWEEP) + list(cp.enumerate_projections().values())
    table = list(dict.fromkeys(call for lanes in LANES for case in cases for call in plan_calls(case, lanes)))
    lines = ["P " + " ".join(map(str, call)) for call in table] + ["G " + " ".join(map(str, g)) for g in GENERIC]
    lines += [f"Q {cols} {ns} {gp.NB16}" for cols, ns in GEOMETRY] + [" ".join(map(str, w)) for w in WIDTHS]
    build = os.path.join(ROOT, "build")
    os.makedirs(build, exist_ok=True)
    calls_file = os.path.join(build, "msm_plan_calls.txt")
    open(calls_file, "w").write("\n".join(lines) + "\n")
    exe = os.path.join(build, "msm_plan_check")
    made = _build(exe)
    assert made.returncode == 0, made.stderr
    argv = [calls_file, os.path.join(ROOT, "tests", "msm_plans_parent.txt")]
    out = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=300)
    text = out.stdout.splitlines()
    assert len(text) >= 2 + len(lines), out.stdout[-2000:] + out.stderr[-2000:]
    answers = text[2:2 + len(lines)]
    n_t, n_g, n_q = len(table), len(GENERIC), len(GEOMETRY)
    return dict(rc=out.returncode, stdout=out.stdout, argv=argv, constants=text[0], limits=text[1], tail="\n".join(text[2 + len(lines):]), table=table,
                table_answers=answers[:n_t], generic=answers[n_t:n_t + n_g], geometry=answers[n_t + n_g:n_t + n_g + n_q], widths=answers[n_t + n_g + n_q:])


def test_replica_of_the_registered_plan_is_held_to_the_code(report):
    """Every msm_plan call behind commit_plans.SWEEP and behind every witness of enumerate_projections() -- the shapes EXCLUDED from the GPU
    sweep among them -- at four lane counts: each field of h2_commit_plan_t that the replica fills equals what msm_plan + plan_summary give,
    and a refusal carries the same code."""
    code = {cp.ERR_ARGS: ERR_ARGS, cp.ERR_BATCH_SHAPE: int(re.search(r"ERR_BATCH_SHAPE (-?\d+)", report["constants"]).group(1))}
    wrong = []
    for call, answer in zip(report["table"], report["table_answers"]):
        want = replica(call)
        if isinstance(want, str):
            same = answer == f"ERR {code[want]}"
        else:
            got = dict(zip(cp.FIELDS, map(int, answer.split()))) if not answer.startswith("ERR") else {}
            same = len(answer.split()) == len(cp.FIELDS) and all(got[f] == want[f] for f in cp.FIELDS)
        if not same:
            wrong.append((call, answer, want))
    assert not wrong, (len(wrong), wrong[:5])
    assert len(report["table_answers"]) == len(report["table"]) > 4000, len(report["table"])
    refused = [c for c in report["table"] if isinstance(replica(c), str)]
    assert refused, "the calls include refusals"


def test_constants_of_the_replicas_are_the_headers(report):
    want = f"LDS_CAP {cp.LDS_CAP} MAX_C {cp.MAX_C} MAX_C_SHARED {cp.MAX_C_SHARED} S1_SCALARS {cp.S1_SCALARS} MAX_BIG {cp.MAX_BIG} MAX_COLS {cp.MAX_COLS} "
    assert report["constants"].startswith("constants: " + want), report["constants"]
    assert gp.LDS_CAP == cp.LDS_CAP


def test_window_widths_and_small_deciders_agree_with_the_replica(report):
    """Both sides of every edge: choose_c for tables at 384 / 385 and 6144 / 6145, for generic calls at 2048 / 2049 and 2^18 / 2^18 + 1; the
    column tables' width at 2^18 - 1 / 2^18; h2_commit_pair_supported at 8191 / 8192; the widths 4 .. 21 h2_bases_register_ex accepts for
    a small table and either side of the smallest 20-bit table with the side array."""
    want = []
    for w in WIDTHS:
        if w[0] == "C":
            want.append(cp.choose_c(w[1], bool(w[2])))
        elif w[0] == "W":
            want.append(cp.h2_commit_column_window_bits(w[1]))
        elif w[0] == "S":
            want.append(cp.pair_supported(w[1]))
        else:
            want.append(int(cp.table_bits(w[1], w[2]) is not None))
    assert list(map(int, report["widths"])) == want
    assert want[:8] == [8, 13, 13, 16, 10, 13, 13, 16] and want[8:12] == [16, 17, 0, 1]


def test_every_plan_keeps_what_the_kernels_rely_on(report):
    """Of every plan above (registered and generic, and every group of a grouped plan): each dynamic LDS size the stages ask for -- from the
    functions the launches use -- is at most kLdsCap, the one-pass sort's NB * 4 at most 131072; the five areas of cx.plan do not overlap and
    end within plan_words (the chunked pass 2's histograms, or the one-launch form's list of oversized bins); lowb + lb <= 31 unless the
    side array carries the low bits; T is a multiple of 256, at most max(256, lanes / 256 * 256); a batched plan (K > 1) has the two-pass
    sort in its one-launch form and the carry-free fold."""
    m = re.search(r"invariants: (\d+) plans of (\d+) calls, (\d+) violations", report["tail"])
    assert m, report["tail"]
    assert int(m.group(3)) == 0 and int(m.group(1)) > 4000, report["tail"]


def test_generic_arm_and_the_grouped_plan(report):
    """The form a call takes: one pass below 65536 scalars, two pass up to 2^18, grouped from 2^18 + 1, never for an instrumented call.  The grouped plan: 5 + 2 + 2 slices for a lone call, one group of 9 with another call in flight (below 2^22), declined
    beyond each form's limit.  The limits and the pass-1 geometry at them, from the real group_geometry, are the replica's."""
    ans = dict(zip(GENERIC, report["generic"]))
    cls = lambda g: ans[g].split()[2]
    assert [cls((L0, n, 0, 0)) for n in (1, 2048, 2049, 65535)] == ["one_pass"] * 4
    assert [ans[(L0, n, 0, 0)].split()[1] for n in (2048, 2049, 1 << 18, (1 << 18) + 1)] == ["10", "13", "13", "16"]
    assert cls((L0, 65536, 0, 0)) == cls((L0, 1 << 18, 0, 0)) == "two_pass"
    assert all(cls(g) == "two_pass" and "try_grouped 0" in ans[g] for g in GENERIC if g[2]), "an instrumented call is never grouped"
    slices = lambda g: [int(x) for x in re.findall(r"\((\d+) ", ans[g])]
    for n in ((1 << 18) + 1, 1 << 20, gp.LATENCY_MAX, 1 << 22):
        assert cls((L0, n, 0, 0)) == "grouped_latency" and " G 3 " in ans[(L0, n, 0, 0)] and slices((L0, n, 0, 0)) == [5, 2, 2], ans[(L0, n, 0, 0)]
    for n in ((1 << 18) + 1, 1 << 20, gp.THROUGHPUT_MAX):
        assert cls((L0, n, 0, 1)) == "grouped_throughput" and " G 1 " in ans[(L0, n, 0, 1)] and slices((L0, n, 0, 1)) == [9], ans[(L0, n, 0, 1)]
    assert cls((L0, 1 << 22, 0, 1)) == "grouped_latency", "from 2^22 scalars a call does not ask who else is in flight"
    for g in ((L0, gp.LATENCY_MAX + 1, 0, 0), (L0, gp.THROUGHPUT_MAX + 1, 0, 1), (L0, (1 << 22) - 1, 0, 1)):
        assert cls(g) == "slice_split" and "split_k 3 try_grouped 1" in ans[g], ans[g]
    assert report["limits"] == "limits: LATENCY_MAX 5120255 THROUGHPUT_MAX 2560127 LOWB_7 1280064 LOWB_6 2560128"
    assert (gp.LATENCY_MAX, gp.THROUGHPUT_MAX, gp.LOWB_7, gp.LOWB_6) == (5120255, 2560127, 1280064, 2560128)
    for (cols, ns), answer in zip(GEOMETRY, report["geometry"]):
        want = gp.group_geometry(cols, ns)
        assert answer == ("NONE" if want is None else "%d %d %d" % want), (cols, ns, answer, want)
    first = lambda n: gp.group_geometry(2 * n, 5)[0]
    assert (first(gp.LOWB_7 - 1), first(gp.LOWB_7), first(gp.LOWB_6 - 1), first(gp.LOWB_6)) == (8, 7, 7, 6)


def test_plans_are_the_parent_commits(report):
    """tests/msm_plans_parent.txt holds every word of the plans the commit before the header computed (printed by a stand-alone copy of that
    commit's text of the functions, not by the header): registered calls over widths 4 to 20 at the table sizes where a summary can
    change (from 13-bit windows, where the two-pass sort's geometry follows the table; a few tables per width below), with a blind, and
    at six widths batched, paired, as a host range, as the shared fold and short on a small device; generic calls either side of every size at which
    the path, the window width or a grouped layout changes, alone and beside another, instrumented or not.  It is the one check of
    split_k, head_slots, plan_words, s2_cap_entries and the ColStride words, which the replicas do not model.  Words that only copy an
    argument or another word are not in the table: the driver checks those copies on every plan of the tests above.  424 rows: none may go missing."""
    m = re.search(r"parent plans: (\d+) rows, (\d+) mismatches", report["tail"])
    assert m and int(m.group(1)) == 424 and int(m.group(2)) == 0 and report["rc"] == 0, report["tail"]


def test_sanitized_build_answers_the_same(report):
    """The planning is full of shifts by computed amounts: the same driver built with -fsanitize=address,undefined (errors fatal) runs over
    the same calls and prints the same."""
    exe = os.path.join(ROOT, "build", "msm_plan_check_san")
    made = _build(exe, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    if made.returncode != 0 and re.search(r"cannot find .*(asan|ubsan)", made.stderr):
        pytest.skip("this toolchain has no sanitizer runtimes to link")
    assert made.returncode == 0, made.stderr
    out = subprocess.run([exe] + report["argv"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout == report["stdout"], out.stderr[-3000:]
