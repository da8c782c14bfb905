// Pippenger multi-scalar multiplication for Pallas / Vesta on gfx950.
//
// Replaces the body of `best_multiexp` (halo2_proofs/src/arithmetic.rs:143-180) and `Buckets::sum`
// (:74-93), and -- for bases registered once per `Params` -- `Params::commit` / `commit_lagrange`
// (poly/commitment.rs:119-150).  The reference runs one CPU task per c-bit window, each re-streaming
// all n (scalar, base) pairs; the result is a group element, so window width, digit encoding and
// summation order are free.  Organised for the GPU instead:
//
//   recode      one lane per scalar: Montgomery -> canonical once (the reference redoes `to_repr` per
//               window, :77), W signed c-bit digits -> u16 codes, window-major                 [HBM]
//   count       per (slice, chunk) workgroup: 2^(c-1)-bin histogram in LDS (128 KiB at c = 16; global
//               atomics measured 20x slower), written out as per-chunk slices                   [LDS]
//   scan        chunk prefixes, then a three-kernel exclusive scan giving every bucket its entry
//               offset and the offsets of its fixed-size work parts
//   scatter     same workgroups: offsets in LDS, LDS atomics hand out slots; base index | sign
//               lands in the bucket-sorted entry list                                           [LDS]
//   accumulate  the hot kernel: the sorted entry list is cut into T EQUAL ranges, T = the lanes the chip
//               keeps resident; each lane gathers 64-B affine bases and does XYZZ mixed additions in
//               registers, flushing a segment whenever its range crosses a bucket boundary.  Every lane
//               does the same work whatever the digit distribution (repeated or tiny scalars)      [VALU]
//   finish      bucket = its own segment + the heads of the ranges that begin inside it
//   reduce      running-sum fold (:86-92) restructured as 8-bucket segments + a small scalar
//               multiple per segment, then a tree sum per slice
//   combine     Horner over windows (:169-178) on one lane; emits Jacobian or affine
//
// Two shapes share these kernels:
//   generic     (h2_msm) W slices of 2^(c-1) buckets, one per window; combine does the c*i doublings.
//   registered  (h2_bases_register / h2_commit) the table [W][n+1] of 2^(c*w) * P_i is precomputed in
//               HBM (1 GiB at k = 20 -- nothing next to 288 GB), so all windows share ONE slice of
//               buckets: 16x fewer buckets to reduce and no doubling chain at all.  Column n holds the
//               blind's base `w` (poly/commitment.rs:127).
//
// No MFMA anywhere: this is modular-integer arithmetic.  Bound by VALU integer-multiply issue, not
// HBM: algorithmic traffic is 96 B per (scalar, base) pair against ~1.8e2 modular multiplies.
#include "msm_internal.cuh"

namespace h2 {

std::atomic<double> g_lane_fraction{1.0};
std::atomic<size_t> g_pipe_chunk{0};   // h2_set_option("host_commit_chunk"): sweeps only

// The laboratory's switches of the plans (msm_plan.h), read once per process (ab_env: a constant null in the product, where the defaults
// hold) -- except H2_MSM_C, read at every call as it always was: a test sets it around one registration.
static MsmKnobs msm_read_switches() {
    MsmKnobs k;
    if (const char *e = ab_env("H2_MSM_DIV")) { const int v = atoi(e); k.lane_div = (u32)(v >= 1 && v <= 64 ? v : 0); }
    if (const char *e = ab_env("H2_BATCH_JOIN")) k.batch_join = e[0] != '0';
    if (const char *e = ab_env("H2_GENERIC_SPLIT")) k.generic_split = atoi(e);
    if (const char *e = ab_env("H2_GENERIC_GROUPED")) k.grouped = atoi(e) != 0;         // 0: round 5's slice split (A/B)
    if (const char *e = ab_env("H2_GG_FORM")) k.gg_form = atoi(e);                      // 1: latency form always, 2: throughput form always (A/B)
    if (const char *e = ab_env("H2_GG_SPARE")) k.gg_spare = atoi(e);                    // CUs left without an accumulate workgroup
    if (const char *e = ab_env("H2_GENERIC_GROUPS"))                                    // "a,b,c"
        for (const char *p = e; *p;) {
            if (k.ngroups < kMaxGroups) k.groups[k.ngroups] = atoi(p);
            ++k.ngroups;
            while (*p && *p != ',') ++p;
            if (*p == ',') ++p;
        }
    return k;
}
MsmKnobs msm_knobs(double lane_fraction) {
    static const MsmKnobs read = msm_read_switches();
    MsmKnobs k = read;
    if (const char *e = ab_env("H2_MSM_C")) k.force_c = atoi(e);
    k.lane_fraction = lane_fraction > 0.0 ? lane_fraction : g_lane_fraction.load();
    return k;
}

// ---- small helpers -----------------------------------------------------------------------------
// canonical -> Montgomery for n field elements / affine coordinates (in place)
template <int F> __global__ void __launch_bounds__(256) k_to_mont(u32 *a, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe_store(a + 8 * i, fe_to_mont<F>(fe_load(a + 8 * i)));
}

// sum of Jacobian points (host helper for the multi-GPU partial sum): Jacobian -> XYZZ is
// (X, Y, Z^2, Z^3)
template <int FB>
__global__ void k_points_sum(const u32 *__restrict__ pts, u32 count, u32 *__restrict__ out, bool in_mont = true, int out_kind = H2_OUT_JACOBIAN,
                             bool out_mont = true) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    xyzz<FB> r = xyzz_identity<FB>();
    for (u32 i = 0; i < count; ++i) {
        const u32 *p = pts + 24 * (size_t)i;
        fe Z = fe_load(p + 16);
        if (fe_is_zero(Z)) continue;
        xyzz<FB> q;
        q.x = fe_load(p);
        q.y = fe_load(p + 8);
        if (!in_mont) { q.x = fe_to_mont<FB>(q.x); q.y = fe_to_mont<FB>(q.y); Z = fe_to_mont<FB>(Z); }
        q.zz = fe_sqr<FB>(Z);
        q.zzz = fe_mulx<FB>(q.zz, Z);
        xyzz_add<FB>(r, q);
    }
    point_out_store<FB>(out, r, out_kind, out_mont);
}

// ---- debug timeline (H2_TIMELINE=1): one-lane stamp kernels between the stages of a commit record the device wall
// clock; h2_debug_timeline drains them.  Used to see how commits on different streams interleave on the chip.
__global__ void msm_stamp(unsigned long long *buf, u32 *count, u32 tag, u32 cap) {
    u32 i = atomicAdd(count, 1u);
    if (i < cap) {
        buf[2 * i] = wall_clock64();
        buf[2 * i + 1] = tag;
    }
}
static unsigned long long *g_tl_buf = nullptr;
static u32 *g_tl_count = nullptr;
static const u32 kTlCap = 1 << 16;
bool timeline_on() {
    static int on = -1;
    if (on < 0) {
        const char *e = getenv("H2_TIMELINE");
        on = e && atoi(e) ? 1 : 0;
        if (on) {
            if (hipMalloc(&g_tl_buf, kTlCap * 16) != hipSuccess || hipMalloc(&g_tl_count, 4) != hipSuccess) on = 0;
            else (void)hipMemset(g_tl_count, 0, 4);
        }
    }
    return on == 1;
}
#define TL_STAMP(tag) do { if (timeline_on()) hipLaunchKernelGGL(msm_stamp, dim3(1), dim3(1), 0, st, g_tl_buf, g_tl_count, (u32)(tag), kTlCap); } while (0)

// One workspace per (device, stream): calls enqueued on different streams never share scratch.
static std::mutex g_ctx_mu;
static std::map<std::pair<int, hipStream_t>, std::unique_ptr<MsmContext>> g_ctxs;
MsmContext &msm_ctx(hipStream_t st) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    auto &slot = g_ctxs[std::make_pair(dev, st)];
    if (!slot) slot.reset(new MsmContext());
    return *slot;
}
// Is a grouped generic multiexp (msm_generic.hip) of ANOTHER stream of this device still in flight?  hipEventQuery on the event each context
// records behind its last one: a few microseconds, no synchronisation.
bool msm_other_generic_in_flight(const MsmContext *self) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    for (auto &kv : g_ctxs) {
        MsmContext *c = kv.second.get();
        if (kv.first.first != dev || c == self || !c->gpending.load()) continue;
        if (c->gdone && hipEventQuery(c->gdone) == hipErrorNotReady) return true;
        c->gpending = false;
    }
    return false;
}
// h2_msm_last_path: the context of (current device, st) if one exists -- the query must not create one
static MsmContext *msm_ctx_find(hipStream_t st) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    auto it = g_ctxs.find(std::make_pair(dev, st));
    return it == g_ctxs.end() ? nullptr : it->second.get();
}
void msm_hand_last_plan(hipStream_t from, hipStream_t to, u32 caller, u32 count, u32 cols_first, u32 cols_last) {
    h2_commit_plan_t r;
    {
        MsmContext &src = msm_ctx(from);
        std::lock_guard<std::mutex> cl(src.mu);
        r = src.last_plan;
    }
    if (!r.caller) return;
    r.caller = caller; r.caller_count = count; r.cols_first = cols_first; r.cols_last = cols_last;
    MsmContext &dst = msm_ctx(to);
    std::lock_guard<std::mutex> cl(dst.mu);
    dst.last_plan = r;
}
// h2_trim: the per-(device, stream) scratch of this device goes back to the allocator (the device is idle by then)
void msm_release_workspaces() {
    msm_release_host_pipe();
    msm_release_host_msm_pipe();
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    for (auto &kv : g_ctxs) {
        if (kv.first.first != dev) continue;
        std::lock_guard<std::mutex> cl(kv.second->mu);
        kv.second->release_all();
    }
}

// ---- context set-up: the LDS attributes of the sort kernels, once per (device, stream) context (the attribute is per device), and how many
// lanes of this call's accumulate kernel the chip holds at once
template <int FB> static int msm_context_setup(MsmContext &cx, bool m9, u32 *lanes_out) {
    if (!cx.attr_set) {
        H2_HIP(hipFuncSetAttribute((const void *)msm_count, hipFuncAttributeMaxDynamicSharedMemorySize, 131072));
        H2_HIP(hipFuncSetAttribute((const void *)msm_scatter, hipFuncAttributeMaxDynamicSharedMemorySize, 131072));
        for (const void *k : {(const void *)msm_s2_count, (const void *)msm_s2_scatter, (const void *)msm_s2_bins, (const void *)msm_s1_scatter<FP, false>,
                              (const void *)msm_s1_scatter<FQ, false>, (const void *)msm_s1_scatter<FP, true>, (const void *)msm_s1_scatter<FQ, true>})
            H2_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512));
        cx.attr_set = true;
    }
    u32 &lanes = cx.lanes[FB][m9 ? 1 : 0];
    if (!lanes) {
        int dev = 0, cus = 0, per_cu = 0;
        H2_HIP(hipGetDevice(&dev));
        H2_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        if (m9) H2_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)msm_accumulate<FB, false, true>, 256, 0));
        else H2_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)msm_accumulate<FB, false>, 256, 0));
        // the M9 accumulate is sized for H2_ACC9_WAVES workgroups per CU even where its register count would let a third one in:
        // the wave slots and registers left over are what the sort / fold kernels of commits on OTHER streams run in
        // (H2_ACC_WAVES: sweeps only)
        static const int acc_waves = [] { const char *e = ab_env("H2_ACC_WAVES"); int v = e ? atoi(e) : 0; return v >= 1 && v <= 4 ? v : H2_ACC9_WAVES; }();
        if (m9) per_cu = std::min(per_cu, acc_waves);
        lanes = (u32)cus * (u32)std::max(per_cu, 1) * 256u;
    }
    *lanes_out = lanes;
    return H2_OK;
}
// Every workspace of the call, in front of its first launch: a reservation that grows frees and synchronises (and invalidates the graphs
// msm_host.hip captured).  The sizes follow from the plan alone, so a phase-2 / 3 / 4 call finds what its phase-1 call reserved.
static int msm_reserve(MsmContext &cx, const MsmPlan &p, hipStream_t st) {
    const MsmShape &sh = p.sh;
    const Sort2 &S2 = p.S2;
    const u32 K = p.K, tb = p.tb;
    const size_t groups = p.split_k ? 2 : K;                 // heavy-bucket lists: one per column, or one per group of a slice split
    int rc;
    if (p.use_sort2) {
        if ((rc = cx.hist.reserve((size_t)K * S2.B1 * S2.nh * 4)) != H2_OK) return rc;
        if ((rc = cx.tagged.reserve((size_t)K * p.all_items * 4)) != H2_OK) return rc;
        if (S2.side && (rc = cx.tagged_low.reserve((size_t)K * p.all_items * 2 + 64)) != H2_OK) return rc;
        if ((rc = cx.plan.reserve((size_t)K * p.plan_words * 4)) != H2_OK) return rc;
    } else {
        if ((rc = cx.digits.reserve(p.all_items * 2)) != H2_OK) return rc;
        if ((rc = cx.hist.reserve((size_t)sh.slices * sh.B * sh.NB * 4)) != H2_OK) return rc;
    }
    if ((rc = cx.counts.reserve((size_t)tb * 4)) != H2_OK) return rc;
    if ((rc = cx.starts.reserve((size_t)K * (tb + 2) * 4)) != H2_OK) return rc;
    if ((rc = cx.bsums.reserve((size_t)(p.nblocks + 4) * 4)) != H2_OK) return rc;
    if ((rc = cx.entries.reserve((size_t)K * p.all_items * 4)) != H2_OK) return rc;
    if ((rc = cx.heads.reserve((size_t)std::max<size_t>(p.T, (size_t)sh.slices * 32) * 128)) != H2_OK) return rc;
    if ((rc = cx.heavy.reserve(groups * (kMaxHeavy + 2) * 4)) != H2_OK) return rc;
    if ((rc = cx.hscratch.reserve(groups * kMaxHeavy * kHeavyBlocks * 144)) != H2_OK) return rc;
    if ((rc = cx.buckets.reserve((size_t)tb * 128)) != H2_OK) return rc;
    if ((rc = cx.partial.reserve(std::max(p.wide_reduce ? ((size_t)2 * p.wideNR / kSeg + 2 * p.wideNR) * 128 : (size_t)(tb / kSeg) * 128,
                                          p.fold9 ? (size_t)K * sh.slices * (p.wideS + p.wideNR + 32) * 144 : (size_t)0))) != H2_OK) return rc;
    if (p.fold9 && cx.fold_ctr.cap < (size_t)K * 64) {      // fold9_planes' arrival counters (16 words per column): zero once, every launch leaves them at zero
        if ((rc = cx.fold_ctr.reserve((size_t)kMaxCols * 64)) != H2_OK) return rc;
        H2_HIP(hipMemsetAsync(cx.fold_ctr.ptr, 0, (size_t)kMaxCols * 64, st));
    }
    if ((rc = cx.ssums.reserve((size_t)(std::max<u32>(sh.slices, 2) + 1) * 128)) != H2_OK) return rc;      // (+ 1: the upper group's weighted sum of a slice split)
    if (p.m9 && !p.fold_only) {
        if (p.glv && (rc = cx.bases9.reserve((size_t)p.scalars_n * 128 + 64)) != H2_OK) return rc;
        // raw M9 segments: the heads of the T ranges of every column, then the bucket slots of every column
        if ((rc = cx.seg9.reserve((p.head_slots + (size_t)K * tb) * 144)) != H2_OK) return rc;
    }
    if (p.split_k && !cx.side) {
        H2_HIP(hipStreamCreateWithFlags(&cx.side, hipStreamNonBlocking));
        for (hipEvent_t *e : {&cx.ev_fork, &cx.ev_conv, &cx.ev_acc_a, &cx.ev_join}) H2_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    return H2_OK;
}
// ---- the stages.  Each enqueues on `st` what the plan says; msm_launch decides which of them a call (or a phase of one) runs.
// nothing to sum: the identity in the form the caller asked for
template <int FB> static int msm_empty(MsmContext &cx, const MsmArgs &a, hipStream_t st) {
    int rc;
    if ((rc = cx.ssums.reserve(128)) != H2_OK) return rc;
    H2_HIP(hipMemsetAsync(cx.ssums.ptr, 0, 128, st));
    msm_combine_launch(FB, st, 0, 1, cx.ssums.as<u32>(), 1, 0, (u32 *)a.d_out, a.out_kind, a.form == H2_FORM_MONTGOMERY);
    H2_HIP(hipGetLastError());
    return H2_OK;
}
// where the two-pass sort keeps its tables inside cx.plan (sort2_layout, msm_plan.h)
struct Sort2Areas { u32 *bin_count, *bin_start, *hlo, *woff, *hist2; };
static Sort2Areas sort2_areas(MsmContext &cx, const Sort2 &S2) {
    const Sort2Layout l = sort2_layout(S2.nh, S2.B2, S2.lowb);
    u32 *plan = cx.plan.as<u32>();
    return {plan + l.bin_count, plan + l.bin_start, plan + l.hlo, plan + l.woff, plan + l.hist2};
}
// bucket counts (cx.counts) -> bucket starts (cx.starts): the three-kernel exclusive scan both sorts end their counting with
static void scan_bucket_starts(MsmContext &cx, const MsmPlan &p, hipStream_t st) {
    const u32 tb = p.tb, nblocks = p.nblocks;
    u32 *grand = cx.bsums.as<u32>() + nblocks;
    hipLaunchKernelGGL(msm_scan_blocksums, dim3(nblocks), dim3(kScanBlock), 0, st, cx.counts.as<u32>(), cx.bsums.as<u32>(), tb);
    hipLaunchKernelGGL(msm_scan_top, dim3(1), dim3(kScanBlock), 0, st, cx.bsums.as<u32>(), nblocks, grand);
    hipLaunchKernelGGL(msm_scan_apply, dim3(nblocks), dim3(kScanBlock), 0, st, cx.counts.as<u32>(), cx.bsums.as<u32>(), grand, cx.starts.as<u32>(), tb);
}
// two-pass sort, pass 1: partition by the top bucket bits into the tagged list (generic: the endomorphism split on the fly; registered / batched:
// a launch set over the K columns)
template <int FS> static void sort2_pass1(MsmContext &cx, const MsmPlan &p, const MsmArgs &a, hipStream_t st) {
    const Sort2 &S2 = p.S2;
    const u32 K = p.K, tb = p.tb;
    const Sort2Areas w = sort2_areas(cx, S2);
    u32 *hist1 = cx.hist.as<u32>();
    const size_t lds1 = s1_stage_bytes(S2.nh, S2.s1_scalars, (size_t)(p.glv ? 2 : 1) * p.sh.W);
    // 512 lanes per pass-1 workgroup: msm_s1_scatter takes 72 registers a lane, and 16 waves of it do not fit beside the two
    // msm_accumulate waves a SIMD already holds (2 x 168 of 512 registers) -- with 1024 lanes the sort of the NEXT commit on
    // another stream sat out the whole accumulate (416 us on average in a 3-stream trace against 57 us alone); LDS is free
    // there, the accumulate uses none.
    const u32 s1_threads = 512;
    if (p.glv) {
        hipLaunchKernelGGL((msm_s1_count<FS, true>), dim3(S2.B1), dim3(s1_threads), S2.nh * 4, st, (const u32 *)a.d_scalars, (const u32 *)nullptr, S2, hist1, p.ci, p.cs);
        hipLaunchKernelGGL(msm_s1_prefix, dim3((S2.nh + 15) / 16), dim3(1024), 0, st, hist1, w.bin_count, S2.B1, S2.nh, cx.heavy.as<u32>(), w.hist2, cx.starts.as<u32>() + tb + 1, p.cs);
        hipLaunchKernelGGL((msm_s1_scatter<FS, true>), dim3(S2.B1), dim3(s1_threads), lds1, st, (const u32 *)a.d_scalars,
                           (const u32 *)nullptr, S2, hist1, w.bin_count, w.bin_start, cx.tagged.as<u32>(), (uint16_t *)nullptr, p.ci, p.cs);
    } else {
        hipLaunchKernelGGL((msm_s1_count<FS, false>), dim3(S2.B1, 1, K), dim3(s1_threads), S2.nh * 4, st, (const u32 *)a.d_scalars,
                           (const u32 *)a.d_extra_scalar, S2, hist1, p.ci, p.cs);
        ColStride cs1 = p.cs;                 // joined columns: one heavy-bucket list and one sentinel, behind the K x tb boundaries
        if (p.joined) cs1.heavy = cs1.starts = 0;
        hipLaunchKernelGGL(msm_s1_prefix, dim3((S2.nh + 15) / 16, 1, K), dim3(1024), 0, st, hist1, w.bin_count, S2.B1, S2.nh, cx.heavy.as<u32>(), w.hist2,
                           cx.starts.as<u32>() + (p.joined ? (size_t)K * tb : (size_t)tb) + 1, cs1);
        hipLaunchKernelGGL((msm_s1_scatter<FS, false>), dim3(S2.B1, 1, K), dim3(s1_threads), lds1, st, (const u32 *)a.d_scalars,
                           (const u32 *)a.d_extra_scalar, S2, hist1, w.bin_count, w.bin_start, cx.tagged.as<u32>(), cx.tagged_low.as<uint16_t>(), p.ci, p.cs);
    }
}
// two-pass sort, pass 2 in its chunked form: chunks of 16 K tagged entries, counting sort inside the one or two bins a chunk spans
static int sort2_pass2_chunked(MsmContext &cx, const MsmPlan &p, hipStream_t st) {
    const Sort2 &S2 = p.S2;
    const u32 tb = p.tb;
    const Sort2Areas w = sort2_areas(cx, S2);
    const u32 *tagged = cx.tagged.as<u32>();
    const uint16_t *tagged_low = cx.tagged_low.as<uint16_t>();
    hipLaunchKernelGGL(msm_s2_plan, dim3(1), dim3(kScanBlock), 0, st, w.bin_start, S2, w.hlo, w.woff);
    const size_t hist2_words = sort2_layout(S2.nh, S2.B2, S2.lowb).hist2_words;
    if (tb > S2.lds_window) H2_HIP(hipMemsetAsync(w.hist2, 0, hist2_words * 4, st));   // the HBM-counted windows start from zero
    const size_t lds2 = s2_count_bytes(S2.lds_window, S2.nh);
    hipLaunchKernelGGL(msm_s2_count, dim3(S2.B2), dim3(1024), lds2, st, tagged, tagged_low, w.bin_start, w.hlo, w.woff, S2, w.hist2);
    hipLaunchKernelGGL(msm_s2_prefix, dim3((tb + 255) / 256), dim3(256), 0, st, w.hist2, w.bin_start, w.hlo, w.woff, S2, cx.counts.as<u32>(), tb);
    scan_bucket_starts(cx, p, st);
    const size_t lds2s = s2_scatter_bytes(S2.lds_window, S2.nh);
    hipLaunchKernelGGL(msm_s2_scatter, dim3(S2.B2), dim3(1024), lds2s, st, tagged, tagged_low, w.bin_start, w.hlo, w.woff, S2, w.hist2,
                       cx.starts.as<u32>(), cx.entries.as<u32>());
    return H2_OK;
}
// the two-pass sort.  Pass 2: one launch, a workgroup per bin, when an average bin fits LDS with room to spare (registered tables; the
// 9-slice generic sort from 2^21 scalars has bins of ~64 K entries and keeps the chunked form)
template <int FS> static int sort_two_pass(MsmContext &cx, const MsmPlan &p, const MsmArgs &a, hipStream_t st) {
    sort2_pass1<FS>(cx, p, a, st);
    if (!p.s2_bins_form) return sort2_pass2_chunked(cx, p, st);
    const Sort2Areas w = sort2_areas(cx, p.S2);
    // (the chunked form's histogram area is free here: it holds the list of oversized bins; msm_s1_prefix zeroed its head)
    sort2_pass2_bins(st, cx.tagged.as<u32>(), cx.tagged_low.as<uint16_t>(), w.bin_start, p.S2, p.tb, p.s2_cap_entries, cx.starts.as<u32>(), cx.entries.as<u32>(),
                     w.hist2, p.max_big, p.zero_in_sort ? cx.seg9.as<u32>() + 36 * p.head_slots : (u32 *)nullptr, p.K, p.cs);
    return H2_OK;
}
// the one-pass sort: 16-bit digit codes, per-chunk histograms in LDS, one scatter
template <int FS> static void sort_one_pass(MsmContext &cx, const MsmPlan &p, const MsmArgs &a, hipStream_t st) {
    const MsmShape &sh = p.sh;
    const u32 tb = p.tb, m32 = (u32)p.m;
    const u32 extra_col = a.d_extra_scalar ? (a.table ? a.extra_col : (u32)a.n_used) : 0xFFFFFFFFu;
    if (p.glv)
        hipLaunchKernelGGL((msm_recode_glv<FS>), dim3(((u32)p.scalars_n + 255) / 256), dim3(256), 0, st, (const u32 *)a.d_scalars,
                           cx.digits.as<uint16_t>(), (u32)p.scalars_n, sh.c, sh.W, a.form == H2_FORM_MONTGOMERY);
    else
        hipLaunchKernelGGL((msm_recode<FS>), dim3((m32 + 255) / 256), dim3(256), 0, st, (const u32 *)a.d_scalars,
                           (const u32 *)a.d_extra_scalar, cx.digits.as<uint16_t>(), m32, sh.c, sh.W,
                           a.form == H2_FORM_MONTGOMERY);
    hipLaunchKernelGGL(msm_count, dim3(sh.B, sh.slices), dim3(1024), sh.NB * 4, st, cx.digits.as<uint16_t>(), cx.hist.as<u32>(), sh.items, sh.chunk, sh.NB);
    hipLaunchKernelGGL(msm_chunk_prefix, dim3((tb + 255) / 256), dim3(256), 0, st, cx.hist.as<u32>(), cx.counts.as<u32>(), sh.NB, sh.B, tb);
    scan_bucket_starts(cx, p, st);
    hipLaunchKernelGGL(msm_scatter, dim3(sh.B, sh.slices), dim3(1024), sh.NB * 4, st, cx.digits.as<uint16_t>(),
                       cx.hist.as<u32>(), cx.starts.as<u32>(), cx.entries.as<u32>(), sh.items, sh.chunk, sh.NB, m32,
                       a.table ? a.stride : 0u, extra_col, a.table ? 1 : 0, a.table ? a.col0 : 0u);
}
// what the accumulate adds into starts from zero: the bucket slots (unless the sort cleared them) and the heavy-bucket list
static int clear_buckets(MsmContext &cx, const MsmPlan &p, hipStream_t st) {
    if (p.m9) {
        // the bucket slots of every column, zeroed in one go
        if (!p.zero_in_sort) H2_HIP(hipMemsetAsync(cx.seg9.as<u32>() + 36 * p.head_slots, 0, (size_t)p.K * p.tb * 144, st));
    } else {
        H2_HIP(hipMemsetAsync(cx.buckets.ptr, 0, (size_t)p.tb * 128, st));
    }
    if (!p.use_sort2) H2_HIP(hipMemsetAsync(cx.heavy.ptr, 0, 8, st));          // (the two-pass sort's msm_s1_prefix zeroed it)
    return H2_OK;
}
// the accumulate: registered tables on the carry-free layer (one launch over the joined columns of a batch, or a column per grid z), the
// generic path likewise after converting its bases (+ phi(P)) to M9 form, and a generic call with a blind term on the 8 x 32 layer
template <int FB> static void accumulate(MsmContext &cx, const MsmPlan &p, const MsmArgs &a, hipStream_t st) {
    const u32 K = p.K, tb = p.tb, T = p.T;
    if (p.m9) {
        const u32 *pts = (const u32 *)a.d_bases;
        if (p.glv) {
            hipLaunchKernelGGL((msm_bases_to_m9_glv<FB>), dim3(((u32)p.scalars_n + 255) / 256), dim3(256), 0, st, (const u32 *)a.d_bases,
                               cx.bases9.as<u32>(), (u32)p.scalars_n);
            pts = cx.bases9.as<u32>();
        }
        hipLaunchKernelGGL((msm_accumulate<FB, false, true>), dim3(T / 256, 1, p.joined ? 1 : K), dim3(256), 0, st, pts,
                           (const u32 *)nullptr, 0xFFFFFFFFu, cx.entries.as<u32>(), cx.starts.as<u32>(), cx.seg9.as<u32>(),
                           cx.seg9.as<u32>() + 36 * p.head_slots, p.joined ? K * tb : tb, T, p.lane_div, p.cs);
        if (!p.fold9)
            hipLaunchKernelGGL((msm_segments_to_r256<FB>), dim3((T + tb + 255) / 256), dim3(256), 0, st, cx.seg9.as<u32>(), cx.heads.as<u32>(), cx.buckets.as<u32>(), T, tb);
    } else {
        hipLaunchKernelGGL((msm_accumulate<FB, false>), dim3(T / 256), dim3(256), 0, st, (const u32 *)a.d_bases,
                           (const u32 *)a.d_extra_base, (!a.table && a.d_extra_base) ? (u32)a.n_used : 0xFFFFFFFFu,
                           cx.entries.as<u32>(), cx.starts.as<u32>(), cx.heads.as<u32>(), cx.buckets.as<u32>(), tb, T, p.lane_div, p.cs);
    }
}
// what the carry-free folds of a call share: the lines, planes (behind every slice's lines in cx.partial) and arrival counters, and the shape
static Fold9Group fold9_shared(MsmContext &cx, const MsmPlan &p) {
    Fold9Group g;
    g.lines9 = cx.partial.as<u32>();
    g.planes9 = g.lines9 + 36 * (size_t)p.K * p.sh.slices * (p.wideS + p.wideNR);
    g.ctr = cx.fold_ctr.as<u32>();
    g.T = p.T;
    g.lane_div = p.lane_div;
    g.c = p.sh.c;
    g.wideS = p.wideS;
    g.wideNR = p.wideNR;
    g.co = p.co;
    g.cs = p.cs;
    return g;
}
// the carry-free fold: finish on the raw M9 segments, one lane per bucket; the buckets stay in cx.seg9.  Window slices (generic path) meet in
// msm_combine's Horner step, unless the caller wants the slice sums (slice_sums_only)
template <int FB> static void fold_carry_free(MsmContext &cx, const MsmPlan &p, const MsmArgs &a, hipStream_t st) {
    const MsmShape &sh = p.sh;
    const bool mont = a.form == H2_FORM_MONTGOMERY, windows = p.glv;
    Fold9Group g = fold9_shared(cx, p);
    g.heads9 = cx.seg9.as<u32>();
    g.starts = cx.starts.as<u32>();
    g.buckets9 = cx.seg9.as<u32>() + 36 * p.head_slots;
    g.heavy = cx.heavy.as<u32>();
    g.hscratch = cx.hscratch.as<u32>();
    g.out = windows ? cx.ssums.as<u32>() : (u32 *)a.d_out;
    g.out_kind = windows ? kOutSliceSum : a.out_kind;
    g.out_mont = mont;
    g.tb = p.tb;
    g.slice0 = 0;
    g.nslices = sh.slices;
    g.cols = p.K;
    fold9_group(FB, st, g);
    if (windows && !a.slice_sums_only) msm_combine_launch(FB, st, 0, 1, cx.ssums.as<u32>(), (int)sh.slices, sh.c, (u32 *)a.d_out, a.out_kind, mont);
}
// the slice split, in front of the sort: the bases' conversion (it reads nothing the sort writes) on the side stream, beside the sort
template <int FB> static int slice_split_convert(MsmContext &cx, const MsmPlan &p, const MsmArgs &a, hipStream_t st) {
    H2_HIP(hipEventRecord(cx.ev_fork, st));
    H2_HIP(hipStreamWaitEvent(cx.side, cx.ev_fork, 0));
    hipLaunchKernelGGL((msm_bases_to_m9_glv<FB>), dim3(((u32)p.scalars_n + 255) / 256), dim3(256), 0, cx.side, (const u32 *)a.d_bases, cx.bases9.as<u32>(), (u32)p.scalars_n);
    H2_HIP(hipEventRecord(cx.ev_conv, cx.side));
    return H2_OK;
}
// the slice split, behind the sort: both groups' accumulates on `st`, the upper group's fold and Horner chain on the side stream
template <int FB> static int slice_split_accumulate_fold(MsmContext &cx, const MsmPlan &p, const MsmArgs &a, hipStream_t st) {
    const MsmShape &sh = p.sh;
    const u32 tb = p.tb, T = p.T, split_k = (u32)p.split_k;
    u32 *heads_b = cx.seg9.as<u32>(), *heads_a = heads_b + 36 * (size_t)T, *buckets9 = cx.seg9.as<u32>() + 36 * p.head_slots;
    if (!p.zero_in_sort) H2_HIP(hipMemsetAsync(buckets9, 0, (size_t)tb * 144, st));
    const u32 kb = split_k * sh.NB, tb_a = tb - kb, ns_a = sh.slices - split_k;       // buckets of the lower group; buckets / slices of the upper one
    u32 *heavy_b = cx.heavy.as<u32>(), *heavy_a = heavy_b + (kMaxHeavy + 2);
    u32 *hscr_b = cx.hscratch.as<u32>(), *hscr_a = hscr_b + (size_t)kMaxHeavy * kHeavyBlocks * 36;
    if (!p.use_sort2) H2_HIP(hipMemsetAsync(heavy_b, 0, 8, st));
    H2_HIP(hipMemsetAsync(heavy_a, 0, 8, st));
    H2_HIP(hipStreamWaitEvent(st, cx.ev_conv, 0));
    const u32 *pts = cx.bases9.as<u32>(), *starts = cx.starts.as<u32>();
    u32 *ssums = cx.ssums.as<u32>();
    const bool mont = a.form == H2_FORM_MONTGOMERY;
    Fold9Group upper = fold9_shared(cx, p);      // both groups leave slice sums (kOutSliceSum) in ssums
    upper.out = ssums;
    upper.out_mont = mont;
    Fold9Group lower = upper;
    upper.heads9 = heads_a; upper.starts = starts + kb; upper.buckets9 = buckets9 + 36 * (size_t)kb; upper.heavy = heavy_a; upper.hscratch = hscr_a;
    upper.tb = tb_a; upper.slice0 = split_k; upper.nslices = ns_a;
    lower.heads9 = heads_b; lower.starts = starts; lower.buckets9 = buckets9; lower.heavy = heavy_b; lower.hscratch = hscr_b;
    lower.tb = kb; lower.slice0 = 0; lower.nslices = split_k;
    // the upper slices first, then the lower ones
    hipLaunchKernelGGL((msm_accumulate<FB, false, true>), dim3(T / 256), dim3(256), 0, st, pts, (const u32 *)nullptr, 0xFFFFFFFFu, cx.entries.as<u32>(),
                       starts + kb, heads_a, buckets9 + 36 * (size_t)kb, tb_a, T, p.lane_div, p.cs);
    H2_HIP(hipEventRecord(cx.ev_acc_a, st));
    hipLaunchKernelGGL((msm_accumulate<FB, false, true>), dim3(T / 256), dim3(256), 0, st, pts, (const u32 *)nullptr, 0xFFFFFFFFu, cx.entries.as<u32>(),
                       starts, heads_b, buckets9, kb, T, p.lane_div, p.cs);
    // upper group on the side stream: fold, Horner over its slices, split_k c more doublings -> one weighted point behind the slice sums
    H2_HIP(hipStreamWaitEvent(cx.side, cx.ev_acc_a, 0));
    fold9_group(FB, cx.side, upper);
    msm_combine_launch(FB, cx.side, 0, 1, ssums + 32 * (size_t)split_k, (int)ns_a, sh.c, ssums + 32 * (size_t)sh.slices, kOutSliceSum, true, p.split_k * sh.c);
    H2_HIP(hipEventRecord(cx.ev_join, cx.side));
    // lower group behind its accumulate, then the two halves meet
    fold9_group(FB, st, lower);
    H2_HIP(hipStreamWaitEvent(st, cx.ev_join, 0));
    msm_combine_launch(FB, st, 0, 1, ssums, p.split_k, sh.c, (u32 *)a.d_out, a.out_kind, mont, 0, ssums + 32 * (size_t)sh.slices);
    return H2_OK;
}
// One multiexp, or one phase of it (MsmArgs::phase): 1 = the sort; 2 = accumulate + fold behind a phase-1 sort; 3 = the accumulate; 4 = the fold.
// The fold-only call (fold_from) is the 8 x 32 fold alone.
template <int FB, int FS> static int msm_launch(MsmContext &cx, const MsmArgs &a, hipStream_t st) {
    const bool empty = a.n_used + (a.d_extra_scalar ? 1 : 0) == 0;
    if (empty && a.table && !a.fold_from) cx.last_plan = empty_summary(a, a.add_into ? 2u : 1u);      // (h2_commit_last_plan; the caller holds cx.mu)
    if (empty && a.add_into) return H2_OK;           // an empty range adds nothing
    if (empty && !a.fold_from) return msm_empty<FB>(cx, a, st);
    int rc;
    u32 lanes = 0;
    if ((rc = msm_context_setup<FB>(cx, msm_m9(a), &lanes)) != H2_OK) return rc;
    MsmPlan p;
    if ((rc = msm_plan(a, lanes, prof_enabled() || timeline_on(), msm_knobs(a.lane_fraction), &p)) != H2_OK) return rc;
    if (p.try_grouped) {
        rc = msm_generic_grouped<FB, FS>(cx, a, p.sh, p.scalars_n, lanes, st);
        if (rc != H2_ERR_BATCH_SHAPE) return rc;
    }
    if (!a.table && a.phase == 0 && !p.fold_only && !a.add_into && !a.slice_sums_only) {      // a whole generic multiexp (h2_msm_last_path)
        cx.last.path = p.split_k ? H2_MSM_PATH_SLICE_SPLIT : p.use_sort2 ? H2_MSM_PATH_TWO_PASS : H2_MSM_PATH_ONE_PASS;
        cx.last.groups = p.split_k ? 2 : 1;
        cx.last.acc_lanes = p.T;
        cx.last.c = p.sh.c;
    }
    if (a.table) cx.last_plan = plan_summary(p, lanes);        // (h2_commit_last_plan)
    if ((rc = msm_reserve(cx, p, st)) != H2_OK) return rc;
    // which stages this call runs (phases >= 2 resume behind a sort the phase-1 call enqueued and timed)
    const bool sorts = !p.fold_only && a.phase < 2, accumulates = !p.fold_only && a.phase != 1 && a.phase != 4, folds = a.phase != 1 && a.phase != 3;
    const u32 tl_id = (u32)(((uintptr_t)st >> 4) & 0xFFFF) << 8;
    if (!p.fold_only) TL_STAMP(tl_id | 1);
    if (p.split_k && (rc = slice_split_convert<FB>(cx, p, a, st)) != H2_OK) return rc;
    if (sorts) {
        prof_begin(PROF_MSM_SORT, st);
        if (!p.use_sort2) sort_one_pass<FS>(cx, p, a, st);
        else if ((rc = sort_two_pass<FS>(cx, p, a, st)) != H2_OK) return rc;
    }
    if (p.split_k) {
        if ((rc = slice_split_accumulate_fold<FB>(cx, p, a, st)) != H2_OK) return rc;
        H2_HIP(hipGetLastError());
        return H2_OK;
    }
    if (accumulates && (rc = clear_buckets(cx, p, st)) != H2_OK) return rc;
    if (sorts) prof_end(PROF_MSM_SORT, st);
    if (accumulates) {
        TL_STAMP(tl_id | 2);
        prof_begin(PROF_MSM_ACCUMULATE, st);
        accumulate<FB>(cx, p, a, st);
        prof_end(PROF_MSM_ACCUMULATE, st);
        TL_STAMP(tl_id | 3);
    }
    if (folds) {
        prof_begin(PROF_MSM_REDUCE, st);
        if (p.fold9) fold_carry_free<FB>(cx, p, a, st);
        else if ((rc = fold_r256(FB, cx, p, a, st)) != H2_OK) return rc;
        prof_end(PROF_MSM_REDUCE, st);
        if (!p.add_only) TL_STAMP(tl_id | 4);
    }
    H2_HIP(hipGetLastError());
    return H2_OK;
}

int msm_dispatch(MsmContext &cx, int curve, const MsmArgs &a, hipStream_t st) {
    if (curve == H2_PALLAS) return msm_launch<FP, FQ>(cx, a, st);
    return msm_launch<FQ, FP>(cx, a, st);
}

void to_mont_async(int curve, u32 *d, size_t field_elems, hipStream_t st) {
    if (!field_elems) return;
    dim3 grid((unsigned)((field_elems + 255) / 256)), block(256);
    if (curve == H2_PALLAS) hipLaunchKernelGGL((k_to_mont<FP>), grid, block, 0, st, d, field_elems);
    else hipLaunchKernelGGL((k_to_mont<FQ>), grid, block, 0, st, d, field_elems);
}

}  // namespace h2

using namespace h2;

extern "C" int h2_msm_window_bits(size_t n) { return choose_c(n ? n : 1, false); }
extern "C" int h2_commit_window_bits(size_t n) { return choose_c(n ? n : 1, true); }
extern "C" int h2_commit_pair_supported(size_t n) { return pair_supported(n, msm_knobs()) ? 1 : 0; }

// copies up to `cap` {clock, tag} pairs recorded under H2_TIMELINE=1 (measurement aid, see the header)
extern "C" int h2_debug_timeline(unsigned long long *out, unsigned cap) {
    if (!timeline_on() || !out) return -1;
    u32 n = 0;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&n, g_tl_count, 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    n = std::min(std::min(n, kTlCap), cap);
    if (hipMemcpy(out, g_tl_buf, (size_t)n * 16, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    (void)hipMemset(g_tl_count, 0, 4);
    return (int)n;
}

extern "C" int h2_set_option(const char *key, double value) {
    if (!key) return H2_ERR_ARGS;
    if (strcmp(key, "msm_lane_fraction") == 0) {
        if (!(value > 0.05 && value <= 1.0)) return H2_ERR_ARGS;
        g_lane_fraction.store(value);
        return H2_OK;
    }
    if (strcmp(key, "host_commit_chunk") == 0) {        // scalars per range of a pipelined host commit (0 = default); sweeps only
        if (!(value >= 0 && value <= (double)(1u << 26))) return H2_ERR_ARGS;
        g_pipe_chunk.store((size_t)value);
        return H2_OK;
    }
    return H2_ERR_ARGS;
}

extern "C" int h2_msm_device(int curve, const void *d_scalars, const void *d_bases_xy, size_t n, int form, int out_kind,
                             void *d_out, void *stream) {
    if (bad_common(curve, form, out_kind) || !d_out || (n && (!d_scalars || !d_bases_xy)) || n > 0x7FFFFFF0u)
        return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    MsmContext &cx = msm_ctx(st);
    std::lock_guard<std::mutex> lk(cx.mu);
    const void *bases = d_bases_xy;
    if (form == H2_FORM_CANONICAL && n) {  // bases arrive canonical: convert a private copy to Montgomery
        if ((rc = cx.stage_b.reserve(n * 64)) != H2_OK) return rc;
        H2_HIP(hipMemcpyAsync(cx.stage_b.ptr, d_bases_xy, n * 64, hipMemcpyDeviceToDevice, st));
        to_mont_async(curve, cx.stage_b.as<u32>(), n * 2, st);
        bases = cx.stage_b.ptr;
    }
    MsmArgs a{d_scalars, nullptr, bases, nullptr, n, false, choose_c(n ? n : 1, false), 0, 0xFFFFFFFFu, form, out_kind, d_out};
    return msm_dispatch(cx, curve, a, st);
}

static int commit_device_impl(h2_bases_t g, const void *d_scalars, size_t n, const void *d_w_xy, const void *d_blind, int form,
                              int out_kind, void *d_out, void *stream, bool blind_base_ready, double lane_fraction = 0.0);

extern "C" int h2_commit_device(h2_bases_t g, const void *d_scalars, size_t n, const void *d_w_xy, const void *d_blind,
                                int form, int out_kind, void *d_out, void *stream) {
    return commit_device_impl(g, d_scalars, n, d_w_xy, d_blind, form, out_kind, d_out, stream, false);
}

static int commit_device_impl(h2_bases_t g, const void *d_scalars, size_t n, const void *d_w_xy, const void *d_blind, int form,
                              int out_kind, void *d_out, void *stream, bool blind_base_ready, double lane_fraction) {
    auto b = find_bases(g);
    if (!b) return H2_ERR_HANDLE;
    // d_blind without d_w_xy: the handle's own blind base (h2_bases_set_blind_base).  d_w_xy without d_blind: nothing to multiply.
    if (bad_common(b->curve, form, out_kind) || !d_out || (n && !d_scalars) || n > b->n || (d_w_xy && !d_blind)) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    MsmContext &cx = msm_ctx(st);
    std::lock_guard<std::mutex> lk(cx.mu);
    if (d_blind && !blind_base_ready) {
        if (d_w_xy) {
            if ((rc = override_blind_base_device(*b, d_w_xy, form, st)) != H2_OK) return rc;
        } else {
            std::lock_guard<std::mutex> bl(b->mu);
            if (!b->blind_set) {
                set_last_error_msg("commit with a blind but the handle has no blind base: call h2_bases_set_blind_base, or pass d_w_xy");
                return H2_ERR_ARGS;
            }
        }
    }
    MsmArgs a{d_scalars, d_blind, b->d_table, nullptr, n, true, b->c, b->stride, (u32)b->n, form, out_kind, d_out};
    a.lane_fraction = lane_fraction;
    return msm_dispatch(cx, b->curve, a, st);
}

// the commit restricted to table columns [first, first + n): d_scalars[i] multiplies registered base first + i.  One range of a
// commit that is split over GPUs (h2_commit_split_rccl_device) or over the chunks of a host transfer; the blind term (the
// handle's blind base) rides with whichever range passes d_blind.
extern "C" int h2_commit_range_device(h2_bases_t g, const void *d_scalars, size_t first, size_t n, const void *d_blind, int form,
                                      int out_kind, void *d_out, void *stream) {
    auto b = find_bases(g);
    if (!b) return H2_ERR_HANDLE;
    if (bad_common(b->curve, form, out_kind) || !d_out || (n && !d_scalars) || first > b->n || n > b->n - first) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (d_blind) {
        std::lock_guard<std::mutex> bl(b->mu);
        if (!b->blind_set) {
            set_last_error_msg("range commit with a blind but the handle has no blind base: call h2_bases_set_blind_base");
            return H2_ERR_ARGS;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    MsmContext &cx = msm_ctx(st);
    std::lock_guard<std::mutex> lk(cx.mu);
    MsmArgs a{d_scalars, d_blind, b->d_table, nullptr, n, true, b->c, b->stride, (u32)b->n, form, out_kind, d_out};
    a.col0 = (u32)first;
    return msm_dispatch(cx, b->curve, a, st);
}

extern "C" int h2_bases_set_blind_base(h2_bases_t g, const uint64_t *w_xy, int form) {
    auto b = find_bases(g);
    if (!b) return H2_ERR_HANDLE;
    if (!w_xy || (form != H2_FORM_CANONICAL && form != H2_FORM_MONTGOMERY)) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    return set_blind_base_host(*b, w_xy, form);
}

// ---- batched commits: the columns of one prover phase (plonk/prover.rs:93-101, 301-313; vanishing/prover.rs:96-108)
// are independent; spread them over internal streams so one column's latency-bound sort / reduce kernels run beside
// another's accumulate, then join on the caller's stream.  Measured at 2^20 (ms per commit):
// 1 stream 1.94; 2 streams 1.64-1.70; 3 streams 1.60-1.64; 4 streams 1.56-1.75.  An accumulate launch fills the register
// file, so the other columns' short kernels run in the gaps between accumulates; narrowing the accumulates
// (lane fraction 0.5) lets them co-reside instead and reaches 1.52 in long runs, but drains badly on short batches.
namespace {
struct BatchStreams {
    std::mutex mu;
    std::vector<hipStream_t> s;
    std::vector<hipEvent_t> done;
    hipEvent_t fork_ev = nullptr;
    // at least `want` streams, each with its `done` event, and the fork event
    int ensure(size_t want) {
        while (s.size() < want) {
            hipStream_t st;
            hipEvent_t ev;
            H2_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            H2_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            s.push_back(st);
            done.push_back(ev);
        }
        if (!fork_ev) H2_HIP(hipEventCreateWithFlags(&fork_ev, hipEventDisableTiming));
        return H2_OK;
    }
    // the first k streams wait for what `user` holds now
    int fork(hipStream_t user, size_t k) {
        H2_HIP(hipEventRecord(fork_ev, user));
        for (size_t i = 0; i < k; ++i) H2_HIP(hipStreamWaitEvent(s[i], fork_ev, 0));
        return H2_OK;
    }
    // ... and `user` for what they hold now
    int join(hipStream_t user, size_t k) {
        for (size_t i = 0; i < k; ++i) {
            H2_HIP(hipEventRecord(done[i], s[i]));
            H2_HIP(hipStreamWaitEvent(user, done[i], 0));
        }
        return H2_OK;
    }
};
BatchStreams &batch_streams() {
    static BatchStreams b[16];
    int dev = 0;
    (void)hipGetDevice(&dev);
    return b[dev & 15];
}
}  // namespace

extern "C" int h2_commit_batch_device(h2_bases_t g, const void *const *d_scalars, size_t count, size_t n, const void *d_w_xy,
                                      const void *const *d_blinds, int form, int out_kind, void *const *d_outs, void *stream) {
    if (!d_scalars || !d_outs || (d_w_xy && !d_blinds)) return H2_ERR_ARGS;      // d_blinds without d_w_xy: the handle's blind base
    if (count == 0) return H2_OK;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    BatchStreams &bs = batch_streams();
    std::lock_guard<std::mutex> lk(bs.mu);
    const size_t want = std::min<size_t>(3, count);
    const double fraction = 0.0;  // the process-wide option
    if ((rc = bs.ensure(want)) != H2_OK) return rc;
    hipStream_t user = (hipStream_t)stream;
    if (d_blinds) {  // a presented w is checked (and installed if it differs) ONCE, on the caller's stream, before forking
        auto b = find_bases(g);
        if (!b) return H2_ERR_HANDLE;
        if (form != H2_FORM_CANONICAL && form != H2_FORM_MONTGOMERY) return H2_ERR_ARGS;
        if (d_w_xy) {
            if ((rc = override_blind_base_device(*b, d_w_xy, form, user)) != H2_OK) return rc;
        } else {
            std::lock_guard<std::mutex> bl(b->mu);
            if (!b->blind_set) {
                set_last_error_msg("batch commit with blinds but the handle has no blind base: call h2_bases_set_blind_base, or pass d_w_xy");
                return H2_ERR_ARGS;
            }
        }
    }
    // The column-batched form (ColIn / ColStride above): groups of up to kMaxCols columns, each group ONE launch set with
    // blockIdx.z = column.  A single group runs on the caller's stream as it is; several groups alternate over two internal
    // streams, so that one group's sort and fold run beside the other's accumulate.  Shapes the batched form does not take
    // (narrow windows, small columns: msm_launch says so before launching anything) fall through to one commit per column
    // on three streams, as before.  H2_BATCH_COLS: sweeps only (1 = the per-column form).
    static const int batch_env = [] { const char *e = ab_env("H2_BATCH_COLS"); int v = e ? atoi(e) : 0; return v >= 1 && v <= kMaxCols ? v : 0; }();
    const size_t batch_cols = batch_env ? (size_t)batch_env : (size_t)kMaxCols;
    // Which form (measured on one MI355X, bench/tools/batch_vs_fork.py, profiles/r04_batch_vs_fork.txt; ms per column, batched / forked):
    //   2^13 x 8: 0.059 / 0.116    2^14 x 8: 0.065 / 0.115    2^16 x 8: 0.102 / 0.143    2^18 x 2, 3, 8: 0.353 / 0.386, 0.302 / 0.323, 0.287 / 0.290
    //   2^20 x 2: 1.105 / 1.177    2^20 x 3: 1.094 / 1.099    2^20 x 8: 1.064 / 1.037
    // Below ~2^18 points a commit is a chain of short launches and the batched form shares every one of them; at 2^20 the accumulate
    // is 80 % of a commit, K x 512 workgroups of it do not tile the chip as evenly as one launch per column sized to it, and three
    // streams of whole commits hide more of the tails: many full-size columns keep the forked form.
    const bool prefer_fork = !batch_env && n >= ((size_t)1 << 19) && count > 3;
    if (count >= 2 && batch_cols >= 2 && n > 0 && !prefer_fork) {
        auto b = find_bases(g);
        if (!b) return H2_ERR_HANDLE;
        if (bad_common(b->curve, form, out_kind) || n > b->n) return H2_ERR_ARGS;
        for (size_t i = 0; i < count; ++i)
            if (!d_scalars[i] || !d_outs[i] || (d_blinds && !d_blinds[i])) return H2_ERR_ARGS;
        const size_t groups = (count + batch_cols - 1) / batch_cols;
        const bool forked = groups > 1;
        if (forked && bs.fork(user, 2) != H2_OK) return H2_ERR_HIP;
        bool taken = true;
        size_t first = 0;
        for (size_t gidx = 0; gidx < groups && rc == H2_OK; ++gidx) {
            const size_t gsize = count / groups + (gidx < count % groups ? 1 : 0);      // balanced groups
            hipStream_t st = forked ? bs.s[gidx & 1] : user;
            MsmContext &cx = msm_ctx(st);
            std::lock_guard<std::mutex> cl(cx.mu);
            MsmArgs a{d_scalars[first], d_blinds ? d_blinds[first] : nullptr, b->d_table, nullptr, n, true, b->c, b->stride, (u32)b->n, form, out_kind, d_outs[first]};
            a.lane_fraction = fraction;
            if (gsize > 1) {
                a.ncols = (int)gsize;
                a.col_scalars = d_scalars + first;
                a.col_blinds = d_blinds ? d_blinds + first : nullptr;
                a.col_outs = d_outs + first;
            }
            rc = msm_dispatch(cx, b->curve, a, st);
            if (rc == H2_ERR_BATCH_SHAPE) {            // nothing was launched
                rc = H2_OK;
                taken = false;
                break;
            }
            first += gsize;
        }
        if (forked && bs.join(user, 2) != H2_OK) return H2_ERR_HIP;
        if (taken && rc == H2_OK)          // h2_commit_last_plan on the caller's stream: the last group's plan and the groups it came in
            msm_hand_last_plan(forked ? bs.s[(groups - 1) & 1] : user, user, H2_COMMIT_CALLER_BATCH_COLUMNS, (u32)groups,
                               (u32)(count / groups + (count % groups ? 1 : 0)), (u32)(count / groups));
        if (taken || rc != H2_OK) return rc;
    }
    if (bs.fork(user, want) != H2_OK) return H2_ERR_HIP;
    for (size_t i = 0; i < count && rc == H2_OK; ++i)
        rc = commit_device_impl(g, d_scalars[i], n, nullptr, d_blinds ? d_blinds[i] : nullptr, form, out_kind, d_outs[i], bs.s[i % want], true, fraction);
    if (bs.join(user, want) != H2_OK) return H2_ERR_HIP;
    if (rc == H2_OK) msm_hand_last_plan(bs.s[(count - 1) % want], user, H2_COMMIT_CALLER_BATCH_FORK, (u32)count);
    return rc;
}

// Independent multiexps over caller-supplied bases in one call (the L_j / R_j pair of an opening-argument round,
// poly/commitment/prover.rs:107-108): same fork / join as the batched commits, so the latency-bound window combine of
// one overlaps the bucket accumulation of the other.
extern "C" int h2_msm_batch_device(int curve, const void *const *d_scalars, const void *const *d_bases_xy, const size_t *n, size_t count,
                                   int form, int out_kind, void *const *d_outs, void *stream) {
    if (!d_scalars || !d_bases_xy || !n || !d_outs) return H2_ERR_ARGS;
    if (count == 0) return H2_OK;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    BatchStreams &bs = batch_streams();
    std::lock_guard<std::mutex> lk(bs.mu);
    const size_t want = std::min<size_t>(3, count);
    if ((rc = bs.ensure(want)) != H2_OK) return rc;
    hipStream_t user = (hipStream_t)stream;
    if (bs.fork(user, want) != H2_OK) return H2_ERR_HIP;
    size_t ran = 0;
    for (size_t i = 0; i < count && rc == H2_OK; ++i, ++ran)
        rc = h2_msm_device(curve, d_scalars[i], d_bases_xy[i], n[i], form, out_kind, d_outs[i], bs.s[i % want]);
    if (bs.join(user, want) != H2_OK) return H2_ERR_HIP;
    if (rc == H2_OK && ran) {         // h2_msm_last_path on the caller's stream: the form of the last multiexp of the batch
        MsmContext::LastPath lp;
        {
            MsmContext &last = msm_ctx(bs.s[(ran - 1) % want]);
            std::lock_guard<std::mutex> cl(last.mu);
            lp = last.last;
        }
        if (lp.path) {
            MsmContext &cx = msm_ctx(user);
            std::lock_guard<std::mutex> cl(cx.mu);
            cx.last = lp;
        }
    }
    return rc;
}

extern "C" int h2_msm_last_path(void *stream, int *path, int *groups, unsigned *acc_lanes, int *window_bits) {
    MsmContext *cx = msm_ctx_find((hipStream_t)stream);
    if (!cx) return H2_ERR_ARGS;
    std::lock_guard<std::mutex> lk(cx->mu);
    if (!cx->last.path) return H2_ERR_ARGS;
    if (path) *path = cx->last.path;
    if (groups) *groups = cx->last.groups;
    if (acc_lanes) *acc_lanes = cx->last.acc_lanes;
    if (window_bits) *window_bits = cx->last.c;
    return H2_OK;
}

extern "C" int h2_commit_last_plan(void *stream, h2_commit_plan_t *out) {
    MsmContext *cx = out ? msm_ctx_find((hipStream_t)stream) : nullptr;
    if (!cx) return H2_ERR_ARGS;
    std::lock_guard<std::mutex> lk(cx->mu);
    if (!cx->last_plan.caller) return H2_ERR_ARGS;
    *out = cx->last_plan;
    return H2_OK;
}

extern "C" int h2_points_sum_device(int curve, const void *d_points_xyz, size_t count, int form, int out_kind, void *d_out, void *stream) {
    if (bad_common(curve, form, out_kind) || !d_out || (count && !d_points_xyz) || count > (1u << 20)) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool mont = form == H2_FORM_MONTGOMERY;
    if (curve == H2_PALLAS) hipLaunchKernelGGL((k_points_sum<FP>), dim3(1), dim3(64), 0, st, (const u32 *)d_points_xyz, (u32)count, (u32 *)d_out, mont, out_kind, mont);
    else hipLaunchKernelGGL((k_points_sum<FQ>), dim3(1), dim3(64), 0, st, (const u32 *)d_points_xyz, (u32)count, (u32 *)d_out, mont, out_kind, mont);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

extern "C" int h2_points_sum(int curve, const uint64_t *points_xyz, size_t count, uint64_t *out_xyz) {
    if ((curve != H2_PALLAS && curve != H2_VESTA) || !out_xyz || (count && !points_xyz) || count > (1u << 20)) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    MsmContext &cx = msm_ctx();
    std::lock_guard<std::mutex> lk(cx.mu);
    if ((rc = cx.stage_b.reserve(count * 96 + 96)) != H2_OK) return rc;
    if ((rc = cx.out.reserve(128)) != H2_OK) return rc;
    if (count) H2_HIP(hipMemcpyAsync(cx.stage_b.ptr, points_xyz, count * 96, hipMemcpyHostToDevice, 0));
    if (curve == H2_PALLAS) hipLaunchKernelGGL((k_points_sum<FP>), dim3(1), dim3(64), 0, 0, cx.stage_b.as<u32>(), (u32)count, cx.out.as<u32>());
    else hipLaunchKernelGGL((k_points_sum<FQ>), dim3(1), dim3(64), 0, 0, cx.stage_b.as<u32>(), (u32)count, cx.out.as<u32>());
    H2_HIP(hipMemcpyAsync(out_xyz, cx.out.ptr, 96, hipMemcpyDeviceToHost, 0));
    H2_HIP(hipStreamSynchronize(0));
    return H2_OK;
}
