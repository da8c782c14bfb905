// best_multiexp(coeffs, bases) without a registered table (halo2_proofs/src/arithmetic.rs:143-180, benches/msm.rs:14-22), large sizes:
// the GROUPED form.
//
// The generic multiexp splits every scalar k = k1 + k2 lambda (glv.cuh) into two half-length digit columns -- 2n columns over nine window
// slices of 2^15 buckets at 16-bit windows -- converts the caller's bases once per call to M9 form (+ phi(P)), and runs the same
// accumulate and fold kernels as a registered commit, followed by a Horner step over the window slices (128 dependent doublings).
// Round 5 ran ONE sort over all slices in front of the first addition (0.25 ms at 2^20, 0.59 / 1.37 ms at 2^21 / 2^22, where its bins
// outgrew LDS) with the endomorphism split done in both of its passes, and everything behind the last addition -- the lower slices'
// fold and the end of the chain -- serial.  Here:
//
//   * the split happens ONCE (msm_glv_digits): one row of 16-bit digit codes per window slice;
//   * the window slices are cut into GROUPS, upper slices first (a lone call: 5 + 2 + 2 of nine).  Each group has its own two-pass sort (pass 1
//     reads the group's digit rows, 2 bytes per entry; pass 2 a workgroup per bin in LDS at every size), its own sorted list and
//     boundary array, its own accumulate launch, its own fold;
//   * only the FIRST group's sort stands in front of the first addition: the others are sorted beside the first accumulate (the sort
//     kernels are light now: 8-24 registers, no field arithmetic), and every group but the last is folded beside the next group's accumulate;
//   * the Horner chain is cut at the group boundaries: group g's link A_g = R_g + D_(g-1), D_g = 2^(c ns_(g+1)) A_g runs behind that
//     group's fold, so behind the last addition stand only the last (smallest) group's fold, its c (ns - 1) doublings and one addition;
//   * TWO FORMS.  Latency form (a lone call): three groups on three streams of the library's own, created back to back -- accumulates on one,
//     everything beside them on the other two -- because HIP multiplexes streams onto four hardware queues and a side stream sharing the
//     CALLER's queue would run behind the accumulate it was meant to run beside; the caller's stream only waits for the result.  8 CUs are left
//     without an accumulate workgroup and the chain links are fenced onto them by LDS requests (a chain link is one wave holding a SIMD).
//     Throughput form (another stream's generic multiexp is in flight, below 2^22 points): ONE group, everything on the caller's stream.
//   * SIZE LIMITS: group_geometry decides them (a pass-1 bin must hold ~16 K entries at most, and at most 4096 bins per group).  The latency
//     form takes 2^18 + 1 .. 5 120 255 scalars, the throughput form's single group up to 2 560 127.  Beyond that this returns
//     H2_ERR_BATCH_SHAPE and msm_launch runs round 5's slice split: a lone call from 5 120 256 scalars, a call that finds another in flight
//     from 2 560 128 to 2^22 - 1.  (h2_profile_enable and H2_TIMELINE=1 never come here: msm_launch keeps their calls on the plain two-pass
//     sort.)  h2_msm_last_path reports the form a call took.
//
// Measured against round 5's form on one box (profiles/r06_generic_grouped.txt): 2^20 one call 1.50-1.58 against 1.55-1.62 ms, three streams
// 1.16-1.20 against 1.33-1.43; 2^21 2.59-2.62 against 2.84-2.87; 2^22 4.98-5.13 against 5.68-5.74 ms.  DESIGN.md section 4.4 has the reasons.
//
// Results are the same group element as every other form (the order of additions inside a bucket is free: SURVEY.md appendix A.1);
// parity (bit-exact canonical affine coordinates against the C restatement of the reference): tests/test_gpu_generic_grouped.py, tests/test_gpu_parity.py, build/h2bench msm / parity.
#include <cassert>

#include "msm_internal.cuh"

namespace h2 {

namespace {

// every workspace, attribute, stream and event of the call before anything is enqueued (a reservation that grows frees and synchronises)
int grouped_reserve(MsmContext &cx, const GroupedPlan &gp, u32 m, u32 W, u32 NB, hipStream_t st) {
    const int G = gp.G;
    const u32 cols = 2 * m, tb = W * NB, row = (cols + 7) & ~7u;
    int rc;
    if ((rc = cx.digits.reserve((size_t)W * row * 2 + 64)) != H2_OK) return rc;
    if ((rc = cx.hist.reserve(gp.hist_words * 4)) != H2_OK) return rc;
    if ((rc = cx.tagged.reserve(gp.tagged_words * 4)) != H2_OK) return rc;
    if ((rc = cx.plan.reserve(gp.plan_words * 4)) != H2_OK) return rc;
    if ((rc = cx.starts.reserve(((size_t)tb + 2 * G) * 4)) != H2_OK) return rc;
    if ((rc = cx.entries.reserve((size_t)W * cols * 4)) != H2_OK) return rc;
    if ((rc = cx.heavy.reserve((size_t)G * (kMaxHeavy + 2) * 4)) != H2_OK) return rc;
    if ((rc = cx.hscratch.reserve((size_t)G * kMaxHeavy * kHeavyBlocks * 144)) != H2_OK) return rc;
    if ((rc = cx.partial.reserve((size_t)W * (gp.wideS + gp.wideNR + 32) * 144)) != H2_OK) return rc;
    if ((rc = cx.ssums.reserve((size_t)(W + G + 1) * 128)) != H2_OK) return rc;
    if ((rc = cx.seg9.reserve((gp.head_slots + (size_t)tb) * 144)) != H2_OK) return rc;
    if ((rc = cx.bases9.reserve((size_t)m * 128 + 64)) != H2_OK) return rc;
    if (cx.fold_ctr.cap < (size_t)kMaxCols * 64) {      // fold9_planes' arrival counters: zero once, every launch leaves them at zero
        if ((rc = cx.fold_ctr.reserve((size_t)kMaxCols * 64)) != H2_OK) return rc;
        H2_HIP(hipMemsetAsync(cx.fold_ctr.ptr, 0, (size_t)kMaxCols * 64, st));
    }
    if (!cx.attr_grouped_set) {       // (one flag per context: both curves' chain links, whichever curve comes first)
        H2_HIP(hipFuncSetAttribute((const void *)msm_d1_scatter, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512));
        H2_HIP(hipFuncSetAttribute((const void *)msm_s2_bins, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512));
        if ((rc = msm_combine_allow_lds(128 * 1024)) != H2_OK) return rc;
        cx.attr_grouped_set = true;
    }
    // Hardware queues.  HIP multiplexes streams onto a handful of hardware queues (four per priority level), and every packet of a queue waits
    // for the one before it: a side stream that happens to share the CALLER's queue runs its kernels behind the accumulate they were meant to run
    // beside (measured inside bench.py, a dozen streams open: the second group's fold landed on the caller's queue, 1.85 ms per call against 1.55
    // from the native driver with the same library).  High-priority streams have queues of their own but cost every other stream of the process
    // (independent calls 1.19 -> 1.32 ms with one such stream merely open: profiles/r06_generic_grouped.txt).  So the latency form runs on THREE
    // streams of its own, created back to back (the runtime hands a new stream the least-used queue: three in a row get different ones): one
    // carries the accumulates and what is serial with them, two side streams the rest (the conversion, the later groups' sorts and the even groups'
    // folds and chain links on one, the odd groups' on the other: a group's fold must not queue behind the previous group's chain link); the caller's stream waits for `ms` at the end and does
    // nothing in between, so it does not matter whose queue it shares.  The throughput form (one group) has nothing beside its accumulate and
    // stays on the caller's stream.
    if (G > 1 && !cx.gstream[0])
        for (int i = 0; i < 3; ++i) H2_HIP(hipStreamCreateWithFlags(&cx.gstream[i], hipStreamNonBlocking));
    for (int i = 0; i < 4 + 3 * G; ++i)
        if (!cx.gev[i]) H2_HIP(hipEventCreateWithFlags(&cx.gev[i], hipEventDisableTiming));
    return H2_OK;
}

}  // namespace

template <int FB, int FS>
int msm_generic_grouped(MsmContext &cx, const MsmArgs &a, const MsmShape &sh, size_t scalars_n, u32 lanes, hipStream_t st) {
    // the plan (msm_plan.h).  Whether another stream's generic multiexp is in flight is asked for the calls whose form it decides, and for no
    // other: the query takes host time and clears the pending flag of every context it finds completed.
    const MsmKnobs kn = msm_knobs(a.lane_fraction);
    if (!grouped_takes(sh, scalars_n, kn)) return H2_ERR_BATCH_SHAPE;
    const bool other_in_flight = grouped_asks_in_flight(scalars_n, kn) && msm_other_generic_in_flight(&cx);
    GroupedPlan gp;
    int rc;
    if ((rc = grouped_plan(sh, scalars_n, lanes, other_in_flight, kn, gp)) != H2_OK) return rc;
    const int G = gp.G;
    const Group *grp = gp.grp;
    const u32 m = (u32)scalars_n, cols = 2 * m, W = (u32)sh.W, NB = sh.NB, c = (u32)sh.c, row = (cols + 7) & ~7u;
    const u32 wideS = gp.wideS, wideNR = gp.wideNR;
    cx.last.path = gp.throughput ? H2_MSM_PATH_GROUPED_THROUGHPUT : H2_MSM_PATH_GROUPED_LATENCY;       // h2_msm_last_path
    cx.last.groups = G;
    cx.last.acc_lanes = 0;
    for (int g = 0; g < G; ++g) cx.last.acc_lanes = std::max(cx.last.acc_lanes, grp[g].T);
    cx.last.c = (int)c;
    if ((rc = grouped_reserve(cx, gp, m, W, NB, st)) != H2_OK) return rc;
    hipStream_t const caller = st;
    if (G > 1) {
        assert(cx.gstream[0] && cx.gstream[1] && cx.gstream[2]);
        st = cx.gstream[1];
    }
    hipStream_t const sort_s = G > 1 ? cx.gstream[0] : nullptr;      // (one group: no side stream -- a context that never ran the latency form has none)
    hipEvent_t ev_fork = cx.gev[0], ev_conv = cx.gev[1];
    auto ev_sorted = [&](int g) { return cx.gev[2 + 3 * g]; };
    auto ev_acc = [&](int g) { return cx.gev[3 + 3 * g]; };
    auto ev_chain = [&](int g) { return cx.gev[4 + 3 * g]; };
    auto fold_s = [&](int g) { return g == G - 1 ? st : cx.gstream[(g & 1) ? 2 : 0]; };          // the last group folds behind its accumulate

    ColStride cs;
    memset(&cs, 0, sizeof cs);
    const bool mont = a.form == H2_FORM_MONTGOMERY;
    uint16_t *digits = cx.digits.as<uint16_t>();
    u32 *hist1 = cx.hist.as<u32>(), *tagged = cx.tagged.as<u32>();
    u32 *heads_all = cx.seg9.as<u32>(), *buckets_all = heads_all + 36 * gp.head_slots;
    u32 *lines9 = cx.partial.as<u32>(), *planes9 = lines9 + 36 * (size_t)W * (wideS + wideNR), *ssums = cx.ssums.as<u32>();
    const u32 *pts = cx.bases9.as<u32>();

    if (st != caller) {               // everything below waits for what the caller's stream holds now
        H2_HIP(hipEventRecord(cx.gev[2 + 3 * G], caller));
        H2_HIP(hipStreamWaitEvent(st, cx.gev[2 + 3 * G], 0));
    }
    // ---- the bases' conversion (it reads nothing the sorts write) beside the recode and the first sort
    H2_HIP(hipEventRecord(ev_fork, st));
    H2_HIP(hipStreamWaitEvent(fold_s(0), ev_fork, 0));
    hipLaunchKernelGGL((msm_bases_to_m9_glv<FB>), dim3((m + 255) / 256), dim3(256), 0, fold_s(0), (const u32 *)a.d_bases, cx.bases9.as<u32>(), m);
    H2_HIP(hipEventRecord(ev_conv, fold_s(0)));
    // ---- the endomorphism split, once
    hipLaunchKernelGGL((msm_glv_digits<FS>), dim3((m + 255) / 256), dim3(256), 0, st, (const u32 *)a.d_scalars, digits, m, row, (int)c, (int)W, mont ? 1 : 0);

    size_t heads_off = 0;
    u32 *heads_of[MsmContext::kMaxGroups];
    for (int g = 0; g < G; ++g) {
        heads_of[g] = heads_all + 36 * heads_off;
        heads_off += grp[g].T;
    }
    auto sort_group = [&](int g, hipStream_t s_) {
        const Group &q = grp[g];
        u32 *bin_count = cx.plan.as<u32>(), *bin_start = bin_count + q.gs.nh, *big = bin_count + group_big_offset(q.gs.nh);
        u32 *starts = cx.starts.as<u32>() + q.starts_off, *entries = cx.entries.as<u32>() + q.ent_off, *heavy = cx.heavy.as<u32>() + (size_t)g * (kMaxHeavy + 2);
        hipLaunchKernelGGL(msm_d1_count, dim3(q.B1), dim3(512), q.gs.nh * 4, s_, (const uint16_t *)digits, q.gs, hist1);
        hipLaunchKernelGGL(msm_s1_prefix, dim3((q.gs.nh + 15) / 16), dim3(1024), 0, s_, hist1, bin_count, q.B1, q.gs.nh, heavy, big, starts + q.tb + 1, cs);
        hipLaunchKernelGGL(msm_d1_scatter, dim3(q.B1), dim3(512), d1_stage_bytes(q.gs.nh, q.gs.S, q.ns), s_, (const uint16_t *)digits, q.gs,
                           (const u32 *)hist1, (const u32 *)bin_count, bin_start, tagged);
        // pass 2: a workgroup per bin; it also clears the group's raw bucket slots.  A bin beyond its stage (the carry slice of the split
        // is ONE bucket; columns of repeated scalars) goes to the chunked msm_s2_big_* kernels, which return at once when the list is empty
        sort2_pass2_bins(s_, tagged, (const uint16_t *)nullptr, bin_start, q.p2, q.tb, q.cap, starts, entries, big, kMaxBig, buckets_all + 36 * q.bucket_off, 1u, cs);
    };
    // a group's fold down to its slice sums: finish (range heads into their buckets), the heavy buckets, line sums, planes
    auto fold_group = [&](int g, hipStream_t s_) {
        const Group &q = grp[g];
        Fold9Group f;
        f.heads9 = heads_of[g];
        f.starts = cx.starts.as<u32>() + q.starts_off;
        f.buckets9 = buckets_all + 36 * q.bucket_off;
        f.heavy = cx.heavy.as<u32>() + (size_t)g * (kMaxHeavy + 2);
        f.hscratch = cx.hscratch.as<u32>() + (size_t)g * kMaxHeavy * kHeavyBlocks * 36;
        f.lines9 = lines9;
        f.planes9 = planes9;
        f.ctr = cx.fold_ctr.as<u32>();
        f.out = ssums;
        f.out_mont = mont;
        f.tb = q.tb;
        f.T = q.T;
        f.lane_div = kLaneDiv;
        f.c = (int)c;
        f.wideS = wideS;
        f.wideNR = wideNR;
        f.slice0 = q.w0;
        f.nslices = q.ns;
        fold9_group(FB, s_, f);      // (one column, no strides; slice sums out)
    };

    // ---- sorts: the first group on the caller's stream, the others on the side stream behind it (they share hist / tagged / plan)
    sort_group(0, st);
    if (G > 1) {
        H2_HIP(hipEventRecord(ev_sorted(0), st));
        H2_HIP(hipStreamWaitEvent(sort_s, ev_sorted(0), 0));
    }
    for (int g = 1; g < G; ++g) {
        sort_group(g, sort_s);
        H2_HIP(hipEventRecord(ev_sorted(g), sort_s));
    }
    // ---- accumulates back to back on the caller's stream; every group's fold and its link of the chain beside the next accumulate
    H2_HIP(hipStreamWaitEvent(st, ev_conv, 0));
    for (int g = 0; g < G; ++g) {
        const Group &q = grp[g];
        if (g) H2_HIP(hipStreamWaitEvent(st, ev_sorted(g), 0));
        hipLaunchKernelGGL((msm_accumulate<FB, false, true, 512>), dim3(q.T / 512), dim3(512), gp.lds_fence ? 65536 : 0, st, pts, (const u32 *)nullptr, 0xFFFFFFFFu,
                           (const u32 *)(cx.entries.as<u32>() + q.ent_off), (const u32 *)(cx.starts.as<u32>() + q.starts_off), heads_of[g],
                           buckets_all + 36 * q.bucket_off, q.tb, q.T, kLaneDiv, cs);
        if (g < G - 1) {
            hipStream_t fs = fold_s(g);
            H2_HIP(hipEventRecord(ev_acc(g), st));
            H2_HIP(hipStreamWaitEvent(fs, ev_acc(g), 0));
            fold_group(g, fs);
            if (g) H2_HIP(hipStreamWaitEvent(fs, ev_chain(g - 1), 0));
            // A_g = Horner(group g) + D_(g-1);  D_g = 2^(c ns_(g+1)) A_g, an XYZZ point behind the slice sums
            msm_combine_launch(FB, fs, gp.lds_fence ? 100 * 1024 : 0, 1, ssums + 32 * (size_t)q.w0, (int)q.ns, (int)c, ssums + 32 * (size_t)(W + g), kOutSliceSum, true,
                               (int)(c * grp[g + 1].ns), g ? ssums + 32 * (size_t)(W + g - 1) : nullptr, true);
            H2_HIP(hipEventRecord(ev_chain(g), fs));
        }
    }
    fold_group(G - 1, st);
    if (G > 1) H2_HIP(hipStreamWaitEvent(st, ev_chain(G - 2), 0));
    msm_combine_launch(FB, st, 0, 1, ssums + 32 * (size_t)grp[G - 1].w0, (int)grp[G - 1].ns, (int)c, (u32 *)a.d_out, a.out_kind, mont, 0,
                       G > 1 ? ssums + 32 * (size_t)(W + G - 2) : nullptr, true);
    H2_HIP(hipGetLastError());
    if (st != caller) {               // ... and the caller's stream for the result
        H2_HIP(hipEventRecord(cx.gev[3 + 3 * G], st));
        H2_HIP(hipStreamWaitEvent(caller, cx.gev[3 + 3 * G], 0));
        st = caller;
    }
    if (!cx.gdone) H2_HIP(hipEventCreateWithFlags(&cx.gdone, hipEventDisableTiming));
    H2_HIP(hipEventRecord(cx.gdone, st));
    cx.gpending = true;
    return H2_OK;
}

template int msm_generic_grouped<FP, FQ>(MsmContext &cx, const MsmArgs &a, const MsmShape &sh, size_t scalars_n, u32 lanes, hipStream_t st);
template int msm_generic_grouped<FQ, FP>(MsmContext &cx, const MsmArgs &a, const MsmShape &sh, size_t scalars_n, u32 lanes, hipStream_t st);

}  // namespace h2
