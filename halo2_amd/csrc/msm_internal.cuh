// Internal header of the multi-scalar-multiplication translation units (msm_*.hip): constants, the structures that travel between
// the host orchestration and the kernels, small device helpers more than one unit uses (among them the fold's shared pieces: head split,
// heavy ticket, gather and tree of either layer, plane arrival), and the declarations of every kernel and host function that is defined in
// one unit and used from another.  Kernels are templates on the base field FB / scalar field FS (FP = 0, FQ = 1).  A kernel of the sort or
// the accumulate lists its instances ONCE beside its declaration (H2_INSTANCES_<kernel>): `extern template` here, the instantiations at the
// foot of its unit.  The fold's kernels are declared nowhere: msm_fold.hip launches them all, behind host functions that take the base field.
// Nothing here is part of the C ABI (include/halo2_mi355x.h).
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "common.h"
#include "curve_wide.cuh"
#include "curve9.cuh"
#include "curve9_wide.cuh"
#include "glv.cuh"
#include "host_field.h"
#include "msm_plan.h"      // the planning constants and structures, msm_plan / grouped_plan and the geometries: plain C++
#include "msm_digits.h"    // the window digits of a scalar and their codes (kZeroCode, kZero32): plain C++
namespace h2 {

extern std::atomic<double> g_lane_fraction;      // h2_set_option("msm_lane_fraction")
extern std::atomic<size_t> g_pipe_chunk;         // h2_set_option("host_commit_chunk"): sweeps only

// msm_launch.hip: the laboratory's switches (read once; H2_MSM_C at every call, as a test sets it around one registration) and the lane
// fraction of this call (`lane_fraction` if positive, else h2_set_option's); the window width under them
MsmKnobs msm_knobs(double lane_fraction = 0.0);
inline int choose_c(size_t n, bool shared_buckets) { return choose_c(n, shared_buckets, msm_knobs()); }

// The sort and tail stages are short dependent chains; when another stream's msm_accumulate shares the SIMDs they
// must win issue arbitration or they stretch 3-4x and the stream they belong to feeds the chip late (timeline in
// DESIGN.md section 5).  msm_accumulate stays at priority 0.
#ifndef H2_TAIL_PRIO
#define H2_TAIL_PRIO 3      // measured again in round 4 under the bench's load (profiles/r04_ab_tail_priority.txt)
#endif
#define H2_LATENCY_STAGE() __builtin_amdgcn_s_setprio(H2_TAIL_PRIO)

#define H2_COLZ(ptr, stride) ((ptr) + (size_t)blockIdx.z * (stride))
// joined columns: the entries of the columns before this one (each column's total sits behind its pass-1 bin starts, at [nh])
__device__ __forceinline__ u32 col_entry_base(const u32 *__restrict__ bin_start_col0, const ColStride &cs) {
    u32 s = 0;
    if (cs.joined)
        for (u32 k = 0; k < blockIdx.z; ++k) s += bin_start_col0[(size_t)k * cs.plan + cs.joined];
    return s;
}

// exclusive scan of v[0 .. n) in LDS by the first wave (n <= 4096); returns the total to every lane of that wave
__device__ __forceinline__ u32 wave0_excl_scan(u32 *v, u32 n) {
    const u32 per = (n + 63) / 64, lo = min(n, threadIdx.x * per), hi = min(n, lo + per);
    u32 sum = 0;
    for (u32 h = lo; h < hi; ++h) sum += v[h];
    u32 incl = sum;
    for (int off = 1; off < 64; off <<= 1) {
        u32 t = __shfl_up(incl, off, 64);
        if ((int)threadIdx.x >= off) incl += t;
    }
    u32 run = incl - sum;
    for (u32 h = lo; h < hi; ++h) {
        u32 t = v[h];
        v[h] = run;
        run += t;
    }
    return __shfl(incl, 63, 64);
}

// lanes actually used for M sorted entries: the launch is sized for the worst case (no zero digits); sparse or tiny
// columns use fewer lanes so that a lane's range keeps >= `div` entries
// (16 entries for full-size columns; 8 for small ones, which are latency-bound: more, shorter lanes -- `div`)
__device__ __forceinline__ u32 eff_lanes(u32 M, u32 T, u32 div) { return min(T, max(256u, (M + div - 1) / div)); }

// largest b in [0, n) with arr[b] <= t  (arr non-decreasing, arr[0] = 0)
__device__ __forceinline__ u32 upper_bucket(const u32 *__restrict__ arr, u32 n, u32 t) {
    u32 lo = 0, hi = n;  // invariant: arr[lo] <= t < arr[hi]  (arr[n] = total > t)
    while (hi - lo > 1) {
        u32 mid = (lo + hi) >> 1;
        if (arr[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- the fold's shared pieces (msm_fold.hip, msm_subdigit.hip): one of each per layer -- `xyzz` on 8 x 32 limbs, `xyzz9` carry-free ------------
// buckets owning more than kHeavy range heads are parked on a list and summed by whole workgroups
static constexpr u32 kHeavy = 64;
static constexpr u32 kHeavyRows = 16;     // workgroup rows of the heavy-bucket launches: they walk the list (at most kMaxHeavy long, usually empty)
static constexpr int kOutSliceSum = 100;  // out_kind of fold9_planes / msm_combine: the sum as XYZZ (32 words) instead of a finished point
#ifndef H2_FOLD_D
#define H2_FOLD_D 2
#endif
// A fold with slack -- a group of a generic multiexp folded beside the next group's accumulate -- keeps wave priority 0 (ColStride::lowprio);
// every other fold is a latency stage.
__device__ __forceinline__ void fold9_stage(const ColStride &cs) {
    if (!cs.lowprio) H2_LATENCY_STAGE();
}
// The range heads of a bucket: the accumulate cut the M sorted entries into ranges of `chunk`, and bucket b owns the heads [h0, h1) of the
// ranges that begin inside it.  VIEW: `starts` is a slice group's view into a longer boundary array, so positions count from starts[0]
// (the carry-free kernels); the 8 x 32 kernels' array begins at zero and they do not load it.
struct HeadSplit {
    u32 base, chunk;
    __device__ __forceinline__ u32 head(u32 pos) const { return (pos - base + chunk - 1) / chunk; }
};
struct HeadRange {
    u32 h0, h1;
};
template <bool VIEW> __device__ __forceinline__ HeadSplit head_split(const u32 *__restrict__ starts, u32 total_buckets, u32 T, u32 div) {
    const u32 base = VIEW ? starts[0] : 0u, M = starts[total_buckets] - base;
    T = eff_lanes(M, T, div);
    return {base, max(1u, (M + T - 1) / T)};
}
__device__ __forceinline__ HeadRange bucket_heads(const HeadSplit &hs, const u32 *__restrict__ starts, u32 b) {
    return {hs.head(starts[b]), hs.head(starts[b + 1])};
}
template <bool VIEW> __device__ __forceinline__ HeadRange bucket_heads(const u32 *__restrict__ starts, u32 b, u32 total_buckets, u32 T, u32 div) {
    return bucket_heads(head_split<VIEW>(starts, total_buckets, T, div), starts, b);
}
// Parks bucket b on the heavy list (heavy[0]: parked, heavy[1]: tickets drawn, heavy[2 ..]: the list) and says whether it found room; a bucket
// beyond kMaxHeavy is summed in place by the caller.  LANES lanes act for the bucket: lane 0 of them (`lead`) draws the ticket, the others
// learn it by DPP.
template <int LANES> __device__ __forceinline__ bool heavy_park(u32 *__restrict__ heavy, u32 b, bool lead) {
    u32 slot = 0;
    if (LANES == 1 || lead) slot = atomicAdd(&heavy[1], 1u);
    if (LANES > 1) slot = (u32)__builtin_amdgcn_mov_dpp((int)slot, 0, 0xf, 0xf, false);   // quad lane 0's ticket
    if (slot >= kMaxHeavy) return false;
    if (LANES == 1 || lead) {
        heavy[2 + slot] = b;
        atomicAdd(&heavy[0], 1u);
    }
    return true;
}
// The 8 x 32 layer's tree.  Quad q of the workgroup sums the points src[32 * index(k)], k = q, q + nq, ... < count ...
template <int FB, class Index> __device__ __forceinline__ xyzz<FB> r256_quad_gather(const u32 *__restrict__ src, u32 count, Index index) {
    const u32 q = threadIdx.x / kGroup, nq = blockDim.x / kGroup;
    xyzz<FB> acc = xyzz_identity<FB>();
    for (u32 k = q; k < count; k += nq) {
        xyzz<FB> p = xyzz_load<FB>(src + 32 * (size_t)index(k));
        xyzz_add_wide<FB>(acc, p);
    }
    return acc;
}
// ... and the sum of the nq (a power of two) points the quads hold lands in sh[0 .. 32), behind a barrier; sh: nq points
template <int FB> __device__ __forceinline__ void r256_quads_sum(const xyzz<FB> &acc, u32 *sh, u32 nq) {
    const u32 q = threadIdx.x / kGroup;
    const bool lead = (threadIdx.x & (kGroup - 1)) == 0;
    if (lead) xyzz_store<FB>(sh + 32 * q, acc);
    __syncthreads();
    for (u32 off = nq / 2; off > 0; off >>= 1) {
        if (q < off) {
            xyzz<FB> x = xyzz_load<FB>(sh + 32 * q), y = xyzz_load<FB>(sh + 32 * (q + off));
            xyzz_add_wide<FB>(x, y);
            if (lead) xyzz_store<FB>(sh + 32 * q, x);
        }
        __syncthreads();
    }
}
// ---- the carry-free layer's tree, on quads of lanes ------------------------------------------------------------------------------
// Past the per-bucket stage every sum is a TREE (a line of the bucket matrix, the heads of a heavy bucket, a bit plane of the
// line sums): its depth in dependent point additions is the latency, and most lanes idle anyway.  A point addition on a quad
// of lanes (curve9_wide.cuh: 4 product levels of ~165 instructions) takes a wave ~850 instructions for 16 additions where
// the one-lane form takes ~2700 for up to 64 -- less wave time from the third tree level up, and a third of the latency at
// every level (a line of 256 buckets: 72 -> ~25 us).
//
// quad q of the workgroup sums the raw points src[36 * index(k)], k = q, q + nq, ... < count.  D points are in flight: each
// lane fetches ONE coordinate (9 words) of each and the quad exchanges them by DPP when the point's turn comes -- the strided
// loads of a line overlap instead of each waiting behind the previous addition.  These kernels run while other streams'
// msm_accumulate holds two waves a SIMD (2 x 168 of 512 registers): they are bounded to the 168 that still fit beside them
// (__launch_bounds__(.., 3)), which two points in flight meet without spilling the addition's own temporaries.
template <int FB, int D = 4, class Index> __device__ __forceinline__ xyzz9<FB> fold9_quad_gather(const u32 *__restrict__ src, u32 count, Index index) {
    const u32 q = threadIdx.x / kGroup, l = threadIdx.x & (kGroup - 1), nq = blockDim.x / kGroup;
    xyzz9<FB> acc = xyzz9_identity<FB>();
    for (u32 k0 = q; k0 < count; k0 += D * nq) {
        fe9 co[D];
#pragma unroll
        for (int j = 0; j < D; j++) {
            const u32 k = k0 + j * nq;
            co[j] = fe9_zero();                                  // (an all-zero point is the identity: skipped by the addition)
            if (k < count) {
                const u32 *w = src + 36 * (size_t)index(k) + 9 * l;
#pragma unroll
                for (int i = 0; i < 9; i++) co[j].v[i] = (i32)w[i];
            }
        }
#pragma unroll
        for (int j = 0; j < D; j++)
            xyzz9_add_wide<FB>(acc, xyzz9<FB>{g9_bcast<0>(co[j]), g9_bcast<1>(co[j]), g9_bcast<2>(co[j]), g9_bcast<3>(co[j])});
    }
    return acc;
}
// the sum of the nq points the quads of a workgroup hold -> quad 0 (every lane of it); sh: nq / 2 raw points.  (Rotating the
// tree by a wave per workgroup index, so that the workgroups sharing a CU do not all finish on their wave 0, was measured: the
// line sums got 5 us SLOWER.)
__device__ __forceinline__ u32 fold9_vquad() { return threadIdx.x / kGroup; }
__device__ __forceinline__ bool fold9_root() { return threadIdx.x < kGroup; }
template <int FB> __device__ __forceinline__ xyzz9<FB> fold9_quads_sum(xyzz9<FB> acc, u32 *sh, u32 first_quads = 0) {      // first_quads (a power of two): only those hold a summand
    const u32 q = fold9_vquad(), nq = first_quads ? first_quads : blockDim.x / kGroup;
    const bool lead = (threadIdx.x & (kGroup - 1)) == 0;
    for (u32 off = nq / 2; off > 0; off >>= 1) {
        if (q >= off && q < 2 * off && lead) xyzz9_store_raw<FB>(sh + 36 * (size_t)(q - off), acc);
        __syncthreads();
        if (q < off) xyzz9_add_wide<FB>(acc, xyzz9_load_raw<FB>(sh + 36 * (size_t)q));
        __syncthreads();
    }
    return acc;
}
// The arrival of bit plane t (fold9_planes, sub_planes): the root quad doubles its plane sum t times -- the plane's weight, applied here: the
// planes double side by side --, its lead lane publishes it in planes9[t] and, behind a fence, draws a ticket; true in every lane of the
// workgroup that arrives LAST of `planes` (s_last: a word of its LDS), which then reads all planes and resets the counter for the next launch.
template <int FB>
__device__ __forceinline__ bool fold9_plane_arrive(xyzz9<FB> acc, u32 t, u32 *__restrict__ planes9, u32 *__restrict__ counter, u32 planes, u32 &s_last) {
    if (fold9_root()) {
        for (u32 k = 0; k < t; ++k) acc = xyzz9_dbl_wide<FB>(acc);
        if ((threadIdx.x & (kGroup - 1)) == 0) {
            xyzz9_store_raw<FB>(planes9 + 36 * (size_t)t, acc);
            __threadfence();
            s_last = atomicAdd(counter, 1u) == planes - 1 ? 1u : 0u;
        }
    }
    __syncthreads();
    if (!s_last) return false;
    __threadfence();
    return true;
}
// The Horner step over the window slices of SEVERAL ranges of one multiexp (h2_msm's range pipeline): slice sums are linear in the
// points, so sum_q Horner(S_q) = Horner(sum_q S_q) -- quad w adds slice w's sums over the ranges (side by side), then quad 0 runs ONE
// chain of (slices - 1) c doublings instead of one chain per range.
struct RangeSums {
    const u32 *p[16];
};

// ---- host orchestration: the per-(device, stream) workspace and the argument block of one multiexp ---------------------------------
struct MsmContext {
    std::mutex mu;
    DevBuf digits, hist, counts, starts, bsums, entries, heads, heavy, hscratch, buckets, partial, ssums, stage_s, stage_b,
        out, small, tagged, tagged_low, plan, seg9, bases9, collapse, collapse_list, fold_ctr;
    void release_all() {
        for (DevBuf *b : {&digits, &hist, &counts, &starts, &bsums, &entries, &heads, &heavy, &hscratch, &buckets, &partial, &ssums,
                          &stage_s, &stage_b, &out, &small, &tagged, &tagged_low, &plan, &seg9, &bases9, &collapse, &collapse_list, &fold_ctr})
            b->release();
        if (copy_stream) (void)hipStreamDestroy(copy_stream);      // (h2_trim: the device is idle)
        if (copy_done) (void)hipEventDestroy(copy_done);
        copy_stream = nullptr;
        copy_done = nullptr;
        if (side) (void)hipStreamDestroy(side);
        for (hipEvent_t *e : {&ev_fork, &ev_conv, &ev_acc_a, &ev_join}) {
            if (*e) (void)hipEventDestroy(*e);
            *e = nullptr;
        }
        side = nullptr;
        for (hipStream_t &s : gstream) {
            if (s) (void)hipStreamDestroy(s);
            s = nullptr;
        }
        for (hipEvent_t &e : gev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        gpending = false;
        if (gdone) (void)hipEventDestroy(gdone);
        gdone = nullptr;
    }
    bool attr_set = false, attr_grouped_set = false;
    // the grouped form of a large generic multiexp (msm_generic.hip), latency form: gstream[1] carries the call's accumulates (and whatever is
    // serial with them), gstream[0] and [2] everything that runs beside them (the bases' conversion, the later groups' sorts, the groups' folds and
    // links of the Horner chain) -- three streams created back to back, so that they sit on different hardware queues whatever queue the CALLER's stream shares
    // with whom; gev: fork, conversion done, per group sorted / accumulated / chained, then begin / end (the caller's stream only waits on those)
    static constexpr int kMaxGroups = h2::kMaxGroups;
    hipStream_t gstream[1 + kMaxGroups] = {};
    hipEvent_t gev[4 + 3 * kMaxGroups] = {};
    // recorded behind every grouped multiexp of this context; other contexts ask it whether a generic multiexp is in flight on ANOTHER stream
    // (msm_other_generic_in_flight): independent calls side by side take the throughput form, a lone call the latency form
    hipEvent_t gdone = nullptr;
    std::atomic<bool> gpending{false};
    hipStream_t copy_stream = nullptr;      // h2_msm: the bases cross PCIe on this one while the sort runs (null-stream context only)
    hipEvent_t copy_done = nullptr;
    // the slice split of a large generic multiexp (msm_launch): the upper slices' fold and Horner chain run on `side` beside the lower
    // slices' accumulate; fork / conv / acc_a / join order the two streams
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_conv = nullptr, ev_acc_a = nullptr, ev_join = nullptr;
    u32 lanes[2][2] = {{0, 0}, {0, 0}};  // resident lanes of msm_accumulate<FP / FQ, 8 x 32 / M9> on this device
    // h2_msm_last_path: the form the last generic multiexp of this context took (host bookkeeping, written where the form is decided)
    struct LastPath {
        int path = 0;          // H2_MSM_PATH_*; 0: no generic multiexp yet
        int groups = 0;
        u32 acc_lanes = 0;     // the largest T of its accumulate launches
        int c = 0;
    } last;
    // h2_commit_last_plan: what the last call of msm_launch over a registered table decided (msm_launch.hip; caller == 0: none yet).  The entry
    // points that wrap it in a form of their own (host ranges, column batches, the paired commit) fill the caller fields behind it.
    h2_commit_plan_t last_plan = {};
};

MsmContext &msm_ctx(hipStream_t st = nullptr);          // msm_launch.hip
// h2_commit_last_plan for calls that ran on the library's own streams: the record of `from`'s context, with the caller form filled in, becomes
// that of `to`'s (each context's mutex taken in turn, never both)
void msm_hand_last_plan(hipStream_t from, hipStream_t to, u32 caller, u32 count, u32 cols_first = 0, u32 cols_last = 0);

// ---- msm_fold.hip: the host side of everything behind the accumulate.  The fold kernels are launched from there and nowhere else, so none of
// them is declared here; `fb` is the base field (FP / FQ) whose instances a call launches.
inline int base_field(int curve) { return curve == H2_PALLAS ? FP : FQ; }
// The carry-free fold of a contiguous GROUP of slices [slice0, slice0 + nslices) down to its slice sums -- finish (range heads into their
// buckets), the heavy buckets, line sums, bit planes: five launches on `st`.
struct Fold9Group {
    const u32 *heads9 = nullptr, *starts = nullptr;                        // the group's own areas: range heads, bucket boundaries,
    u32 *buckets9 = nullptr, *heavy = nullptr, *hscratch = nullptr;        // bucket slots, heavy list and its scratch
    u32 *lines9 = nullptr, *planes9 = nullptr, *ctr = nullptr;             // the areas of slice 0: the group's lie slice0 slices in
    u32 *out = nullptr;                                                    // ... and so does its output when that is slice sums
    int out_kind = kOutSliceSum;                                           // kOutSliceSum (32 words a slice) or a finished point per slice
    bool out_mont = true;
    u32 tb = 0;                                                            // the group's buckets (per column)
    u32 T = 0, lane_div = 0;                                               // as its accumulate was launched
    int c = 0;
    u32 wideS = 0, wideNR = 0;                                             // the bucket matrix of a slice
    u32 slice0 = 0, nslices = 0;
    u32 cols = 1;                 // columns of a batched commit: grid z of every launch, except that JOINED columns (cs.joined) are finished as one list of cols x tb buckets
    ColOut co = {};
    ColStride cs = {};
};
void fold9_group(int fb, hipStream_t st, const Fold9Group &g);
// the 8 x 32 finisher and fold of a call of msm_launch.  A range of a chunked commit stops at its finished buckets (added into add_into); the
// fold-only call starts from buckets summed that way.
int fold_r256(int fb, MsmContext &cx, const MsmPlan &p, const MsmArgs &a, hipStream_t st);
// msm_combine: the Horner step over `slices` slice sums (outputs > 1: slice i alone becomes output i); lds: dynamic LDS the launch asks for
// and never touches (the grouped form's fence, msm_generic.hip), which msm_combine_allow_lds has to have raised the limit for
void msm_combine_launch(int fb, hipStream_t st, size_t lds, u32 outputs, const u32 *slice_sums, int slices, int c, u32 *out, int out_kind, bool out_mont,
                        int extra_dbl = 0, const u32 *addend = nullptr, bool addend_first = false);
int msm_combine_allow_lds(size_t bytes);
void msm_combine_ranges_launch(int fb, hipStream_t st, const RangeSums &rs, int ranges, int slices, int c, u32 *out, int out_kind, bool out_mont);
void msm_bucket_add_launch(int fb, hipStream_t st, u32 *total, const u32 *part, u32 nb);      // total[b] += part[b], b < nb
// msm_sort.hip: pass 2 of a two-pass sort in its one-launch form -- msm_s2_bins (a workgroup per pass-1 bin; it lists the bins beyond its LDS stage
// in `big` and clears the raw bucket slots `zero9` when given) and, when max_big is non-zero, the chunked msm_s2_big_* kernels over that list
void sort2_pass2_bins(hipStream_t st, const u32 *tagged, const uint16_t *tagged_low, const u32 *bin_start, const Sort2 &S2, u32 tb, size_t cap_entries,
                      u32 *starts, u32 *entries, u32 *big, u32 max_big, u32 *zero9, u32 cols, const ColStride &cs);


// msm_generic.hip: the grouped form of a large generic multiexp (unregistered bases, endomorphism split, window slices sorted and
// accumulated in groups); H2_ERR_BATCH_SHAPE, before anything is enqueued, when the shape does not take it (msm_launch then runs its own form)
template <int FB, int FS> int msm_generic_grouped(MsmContext &cx, const MsmArgs &a, const MsmShape &sh, size_t scalars_n, u32 lanes, hipStream_t st);
extern template int msm_generic_grouped<FP, FQ>(MsmContext &cx, const MsmArgs &a, const MsmShape &sh, size_t scalars_n, u32 lanes, hipStream_t st);
extern template int msm_generic_grouped<FQ, FP>(MsmContext &cx, const MsmArgs &a, const MsmShape &sh, size_t scalars_n, u32 lanes, hipStream_t st);
bool msm_other_generic_in_flight(const MsmContext *self);                            // msm_launch.hip: a grouped multiexp of another stream of this device has not completed
int msm_dispatch(MsmContext &cx, int curve, const MsmArgs &a, hipStream_t st);      // msm_launch.hip: the whole multiexp (or one phase of it) on `st`
void to_mont_async(int curve, u32 *d, size_t field_elems, hipStream_t st);           // canonical -> Montgomery in place
bool timeline_on();                                                                  // H2_TIMELINE=1 (diagnostic; never changes a result)
void msm_release_host_pipe();                                                        // msm_host.hip (h2_trim)
void msm_release_host_msm_pipe();

// ---- registered bases -------------------------------------------------------------------------------
struct Bases {
    std::mutex mu;
    int curve = 0;
    size_t n = 0;
    int c = 16, W = 16;
    u32 stride = 0;            // n + 1: column n is the blind's base
    void *d_table = nullptr;   // [W][stride] affine Montgomery points, row w = 2^(c*w) * P
    void *d_blind_tmp = nullptr;  // 64-byte staging slot for a blind base that arrives through a host pointer
    int device = 0;            // the HIP device the table lives on (current at registration)
    // `Params::w` (poly/commitment.rs:26-33) belongs to the handle: h2_bases_set_blind_base installs its multiples as column n.
    // blind_set: the column holds SOME w.  blind_host_known: `blind_host` / `blind_form` are the 64 bytes it was installed from
    // (false after a device-pointer override, whose content the host never sees).
    bool blind_set = false, blind_host_known = false;
    int blind_form = 0;
    unsigned char blind_host[64] = {0};
    DevBuf fill_tmp;           // table_fill's staging, kept only by handles that are refilled (bases_refill_device: the opening argument's G' table)
    int glv = 0;               // != 0: an ENDOMORPHISM table (the opening argument's G', served by pair_subdigit_launch only): rows 0 .. glv - 1 are
                               // 2^(16 w) P, rows glv .. 2 glv - 1 their images phi(2^(16 w) P) = (zeta x, y) = [lambda] 2^(16 w) P; W = 2 glv
    // The table is owned here: it goes back to the allocator when the LAST reference drops -- h2_bases_free only removes
    // the handle, so a commit another host thread is still enqueueing (it holds the shared_ptr from find_bases) keeps the
    // memory alive, and every error path of h2_bases_register releases what it had allocated.
    ~Bases() {
        if (!d_table && !d_blind_tmp && !fill_tmp.ptr) return;
        int cur = 0;
        (void)hipGetDevice(&cur);
        if (cur != device) (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();
        if (d_table) (void)hipFree(d_table);
        if (d_blind_tmp) (void)hipFree(d_blind_tmp);
        fill_tmp.release();
        if (cur != device) (void)hipSetDevice(cur);
    }
};
// registered tables (msm_table.hip)
std::shared_ptr<Bases> find_bases(h2_bases_t h, bool endomorphism = false);
bool bad_common(int curve, int form, int out_kind);
int table_fill(Bases &b, u32 first, u32 count, hipStream_t st, bool keep_tmp = false);
int set_blind_base_host(Bases &b, const void *host_w_xy, int form);
int override_blind_base_device(Bases &b, const void *d_w_xy, int form, hipStream_t st);
bool pair_subdigits_apply(size_t n);                                                 // does h2_commit_pair_device take the sub-digit form for n points?
// the opening argument's table of collapsed generators (ipa.hip): refilled in place / registered, optionally as an endomorphism table
int bases_refill_device(h2_bases_t handle, const void *d_bases_xy, size_t n, int form);
int bases_register_device_internal(int curve, const void *d_bases_xy, size_t n, int form, h2_bases_t *handle, bool glv);

// compile-time A/B knobs of the accumulate (a second build under build/ab/; the defaults are what ships)
#ifndef H2_ACC_LOOP
#define H2_ACC_LOOP 2       // 1: the round-3 loop (gather issued before the point is repacked); 2: point consumed first (round 4) -- A/B builds
#endif
#ifndef H2_ACC9_WAVES
#define H2_ACC9_WAVES 2     // waves per SIMD the M9 accumulate is compiled for: 2, 3 and 4 run the adds equally fast (profiles/r02_ubench_fe9.txt);
                            // at 2 the register file keeps room for the sort / fold kernels of commits on other streams (3 streams: 903 vs 861 M/s)
#endif

// ---- kernels defined in msm_sort.hip -------------------------------------------------------------------------------------------
// A templated kernel's instances are listed ONCE, beside its declaration, as H2_INSTANCES_<kernel>(X): expanded here as `extern template`
// and at the foot of msm_sort.hip as the explicit instantiations (the signature comes from the declaration).
#define H2_EXTERN_KERNEL(...) extern template __global__ decltype(__VA_ARGS__) __VA_ARGS__;
#define H2_INSTANTIATE_KERNEL(...) template __global__ decltype(__VA_ARGS__) __VA_ARGS__;
template <int FS>
__global__ void __launch_bounds__(256) msm_recode(const u32 *__restrict__ scalars, const u32 *__restrict__ extra_scalar,
                                                  uint16_t *__restrict__ digits, u32 m, int c, int W, int mont);
#define H2_INSTANCES_msm_recode(X) X(msm_recode<FP>) X(msm_recode<FQ>)
H2_INSTANCES_msm_recode(H2_EXTERN_KERNEL)
template <int FS>
__global__ void __launch_bounds__(256) msm_recode_glv(const u32 *__restrict__ scalars, uint16_t *__restrict__ digits, u32 m, int c, int W,
                                                      int mont);
#define H2_INSTANCES_msm_recode_glv(X) X(msm_recode_glv<FP>) X(msm_recode_glv<FQ>)
H2_INSTANCES_msm_recode_glv(H2_EXTERN_KERNEL)
__global__ void __launch_bounds__(1024) msm_count(const uint16_t *__restrict__ digits, u32 *__restrict__ hist,
                                                  size_t items, u32 chunk, u32 NB);
__global__ void __launch_bounds__(256) msm_chunk_prefix(u32 *__restrict__ hist, u32 *__restrict__ counts, u32 NB,
                                                        u32 B, u32 total_buckets);
__global__ void __launch_bounds__(kScanBlock) msm_scan_blocksums(const u32 *__restrict__ counts, u32 *__restrict__ bsums,
                                                                 u32 total);
__global__ void __launch_bounds__(kScanBlock) msm_scan_top(u32 *__restrict__ bsums, u32 nblocks, u32 *__restrict__ grand);
__global__ void __launch_bounds__(kScanBlock) msm_scan_apply(const u32 *__restrict__ counts, const u32 *__restrict__ bsums,
                                                             const u32 *__restrict__ grand, u32 *__restrict__ starts,
                                                             u32 total);
__global__ void __launch_bounds__(1024) msm_scatter(const uint16_t *__restrict__ digits, const u32 *__restrict__ hist,
                                                    const u32 *__restrict__ starts, u32 *__restrict__ entries,
                                                    size_t items, u32 chunk, u32 NB, u32 m, u32 stride, u32 extra_col,
                                                    int table, u32 col0);
template <int FS, bool GLV>
__global__ void __launch_bounds__(1024) msm_s1_count(const u32 *__restrict__ scalars, const u32 *__restrict__ extra_scalar, Sort2 P,
                                                     u32 *__restrict__ hist1, ColIn ci, ColStride cs);
#define H2_INSTANCES_msm_s1_count(X) X(msm_s1_count<FP, false>) X(msm_s1_count<FP, true>) X(msm_s1_count<FQ, false>) X(msm_s1_count<FQ, true>)
H2_INSTANCES_msm_s1_count(H2_EXTERN_KERNEL)
template <int FS, bool GLV>
__global__ void __launch_bounds__(1024) msm_s1_scatter(const u32 *__restrict__ scalars, const u32 *__restrict__ extra_scalar, Sort2 P,
                                                       const u32 *__restrict__ hist1, const u32 *__restrict__ bin_count,
                                                       u32 *__restrict__ bin_start, u32 *__restrict__ tagged, uint16_t *__restrict__ tagged_low,
                                                       ColIn ci, ColStride cs);
#define H2_INSTANCES_msm_s1_scatter(X) X(msm_s1_scatter<FP, false>) X(msm_s1_scatter<FP, true>) X(msm_s1_scatter<FQ, false>) X(msm_s1_scatter<FQ, true>)
H2_INSTANCES_msm_s1_scatter(H2_EXTERN_KERNEL)
__global__ void __launch_bounds__(1024) msm_s1_prefix(u32 *__restrict__ hist1, u32 *__restrict__ bin_count, u32 B1, u32 nh, u32 *__restrict__ z2,
                                                      u32 *__restrict__ z1, u32 *__restrict__ sentinel, ColStride cs);
__global__ void __launch_bounds__(kScanBlock) msm_s2_plan(const u32 *__restrict__ bin_start, Sort2 P, u32 *__restrict__ hlo,
                                                          u32 *__restrict__ woff);
__global__ void __launch_bounds__(1024) msm_s2_count(const u32 *__restrict__ tagged, const uint16_t *__restrict__ tagged_low, const u32 *__restrict__ bin_start,
                                                     const u32 *__restrict__ hlo, const u32 *__restrict__ woff, Sort2 P, u32 *__restrict__ hist2);
__global__ void __launch_bounds__(1024) msm_s2_scatter(const u32 *__restrict__ tagged, const uint16_t *__restrict__ tagged_low, const u32 *__restrict__ bin_start,
                                                       const u32 *__restrict__ hlo, const u32 *__restrict__ woff, Sort2 P,
                                                       u32 *__restrict__ hist2, const u32 *__restrict__ starts, u32 *__restrict__ entries);
__global__ void __launch_bounds__(1024) msm_s2_bins(const u32 *__restrict__ tagged, const uint16_t *__restrict__ tagged_low, const u32 *__restrict__ bin_start,
                                                    Sort2 P, u32 total_buckets, u32 cap, u32 *__restrict__ starts, u32 *__restrict__ entries,
                                                    u32 *__restrict__ big, u32 max_big, u32 *__restrict__ zero9, ColStride cs);
__global__ void __launch_bounds__(1024) msm_s2_big_count(const u32 *__restrict__ tagged, const uint16_t *__restrict__ tagged_low, const u32 *__restrict__ bin_start,
                                                         Sort2 P, const u32 *__restrict__ big, u32 *__restrict__ gcnt, ColStride cs);
__global__ void __launch_bounds__(1024) msm_s2_big_prefix(const u32 *__restrict__ bin_start, Sort2 P, u32 total_buckets, const u32 *__restrict__ big,
                                                          u32 *__restrict__ gcnt, u32 *__restrict__ starts, ColStride cs);
__global__ void __launch_bounds__(1024) msm_s2_big_scatter(const u32 *__restrict__ tagged, const uint16_t *__restrict__ tagged_low, const u32 *__restrict__ bin_start,
                                                           Sort2 P, const u32 *__restrict__ big, const u32 *__restrict__ gcnt, u32 *__restrict__ entries,
                                                           ColStride cs);
__global__ void __launch_bounds__(256) msm_s2_prefix(u32 *__restrict__ hist2, const u32 *__restrict__ bin_start, const u32 *__restrict__ hlo,
                                                     const u32 *__restrict__ woff, Sort2 P, u32 *__restrict__ counts, u32 NB);
template <int FS>
__global__ void __launch_bounds__(256) msm_glv_digits(const u32 *__restrict__ scalars, uint16_t *__restrict__ digits, u32 m, u32 row, int c, int W, int mont);
#define H2_INSTANCES_msm_glv_digits(X) X(msm_glv_digits<FP>) X(msm_glv_digits<FQ>)
H2_INSTANCES_msm_glv_digits(H2_EXTERN_KERNEL)
__global__ void __launch_bounds__(512) msm_d1_count(const uint16_t *__restrict__ digits, GroupSort P, u32 *__restrict__ hist1);
__global__ void __launch_bounds__(512) msm_d1_scatter(const uint16_t *__restrict__ digits, GroupSort P, const u32 *__restrict__ hist1,
                                                      const u32 *__restrict__ bin_count, u32 *__restrict__ bin_start, u32 *__restrict__ tagged);


// ---- kernels defined in msm_accumulate.hip -------------------------------------------------------------------------------------
template <int FB>
__global__ void __launch_bounds__(256) msm_bases_to_m9_glv(const u32 *__restrict__ bases, u32 *__restrict__ out, u32 n);
#define H2_INSTANCES_msm_bases_to_m9_glv(X) X(msm_bases_to_m9_glv<FP>) X(msm_bases_to_m9_glv<FQ>)
H2_INSTANCES_msm_bases_to_m9_glv(H2_EXTERN_KERNEL)
// BLOCK: lanes per workgroup.  256 everywhere (two workgroups per CU) except the grouped generic multiexp (msm_generic.hip), whose accumulates
// are launched while the previous group's fold kernels hold wave slots on some CUs: with 256-lane workgroups the dispatcher then puts THREE
// accumulate workgroups on the free CUs (168 registers allow three waves per SIMD), those run at two thirds of the speed for the whole launch
// and the launch ends when they do (331 -> 477 us measured: profiles/r06_generic_grouped.txt).  One 512-lane workgroup per CU cannot double up.
template <int FB, bool GLV, bool M9 = false, int BLOCK = 256>
__global__ void __launch_bounds__(BLOCK, (M9 ? H2_ACC9_WAVES * 256 / BLOCK : 4)) msm_accumulate(const u32 *__restrict__ bases, const u32 *__restrict__ extra_base,
                                                      u32 extra_index, const u32 *__restrict__ entries,
                                                      const u32 *__restrict__ starts, u32 *__restrict__ heads,
                                                      u32 *__restrict__ buckets, u32 total_buckets, u32 T, u32 div, ColStride cs);
#define H2_INSTANCES_msm_accumulate(X)                                                                                                    \
    X(msm_accumulate<FP, false, false>) X(msm_accumulate<FP, false, true>) X(msm_accumulate<FQ, false, false>) X(msm_accumulate<FQ, false, true>) \
    X(msm_accumulate<FP, false, true, 512>) X(msm_accumulate<FQ, false, true, 512>)
H2_INSTANCES_msm_accumulate(H2_EXTERN_KERNEL)
template <int FB>
__global__ void __launch_bounds__(256) msm_segments_to_r256(const u32 *__restrict__ raw, u32 *__restrict__ heads,
                                                            u32 *__restrict__ buckets, u32 T, u32 total_buckets);
#define H2_INSTANCES_msm_segments_to_r256(X) X(msm_segments_to_r256<FP>) X(msm_segments_to_r256<FQ>)
H2_INSTANCES_msm_segments_to_r256(H2_EXTERN_KERNEL)

}  // namespace h2
