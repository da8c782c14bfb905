// What a multiexp decides before it enqueues or reserves anything: window width, sort form and geometry, lanes, LDS sizes, workspace
// strides (msm_plan, the registered and the plain generic forms) and the groups of the grouped generic form (grouped_plan).  Plain C++ --
// no HIP, no context, no environment -- so that "what does this call run as" is answered, and tested, on a CPU (tests/test_msm_plan.py).
// msm_launch.hip and msm_generic.hip fill MsmKnobs and the arguments, and enqueue what the plan says.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "../../include/halo2_mi355x.h"   // H2_OK / H2_ERR_ARGS, H2_FORM_*, h2_commit_plan_t

namespace h2 {

typedef uint32_t u32;
typedef uint64_t u64;

static constexpr int kMaxC = 16;          // generic path (and the 16-bit digit codes of the one-pass sort)
static constexpr int kMaxCShared = 20;    // registered path: one bucket slice, two-pass sort, 32-bit digit codes
static constexpr u32 kS1Scalars = 2048;   // scalars per workgroup of the two-pass sort's first pass
static constexpr u32 kS2Chunk = 16384;    // entries per workgroup of its second pass
static constexpr size_t kLdsCap = 160 * 1024 - 512;
static constexpr int kSeg = 4;     // buckets per reduce segment when the fold is latency-bound (few segments), else 2 kSeg
static constexpr u32 kScanBlock = 1024;
static constexpr u32 kMaxBig = 32, kBigChunks = 64;      // big bins sorted by the chunked kernels (msm_s2_big_*); workgroups per big bin
static constexpr u32 kS2StageWindow = 3072;
static constexpr u32 kMaxHeavy = 512;   // heavy buckets handed to the workgroup path; any beyond that are summed in place
static constexpr u32 kHeavyBlocks = 32;
static constexpr int kMaxGroups = 4;    // groups of window slices of the grouped generic form
static constexpr u32 kLaneDiv = 16;     // entries per lane the grouped form's accumulates aim at (full-size columns)
static constexpr int H2_ERR_BATCH_SHAPE = -1000;     // internal: never leaves the library

// The laboratory's switches (tuning sweeps and A/B arms only); the defaults are what the shipped library runs.  msm_knobs() (msm_launch.hip)
// fills them from the environment of the laboratory build, and the lane fraction from the call or h2_set_option.
struct MsmKnobs {
    int force_c = 0;              // H2_MSM_C: the window width, 4 .. kMaxCShared (the only way to windows beyond 16 bits)
    u32 lane_div = 0;             // H2_MSM_DIV: entries per lane of the accumulate, 1 .. 64 (0: 8 for small commits, 16 otherwise)
    bool batch_join = true;       // H2_BATCH_JOIN=0: one accumulate launch per column of a batch
    int generic_split = -1;       // H2_GENERIC_SPLIT: 0 no slice split; k > 0 the lower group's slices (-1: 3 from 2^19 scalars)
    bool grouped = true;          // H2_GENERIC_GROUPED=0: round 5's slice split instead of the grouped form
    int gg_form = 0;              // H2_GG_FORM: 1 the latency form always, 2 the throughput form always
    int gg_spare = -1;            // H2_GG_SPARE: CUs left without an accumulate workgroup (-1: one per XCD in the latency form)
    int ngroups = 0;              // H2_GENERIC_GROUPS="a,b,c": how many sizes it names (more than kMaxGroups: ignored), upper slices first
    int groups[kMaxGroups] = {0, 0, 0, 0};
    double lane_fraction = 1.0;   // share of the resident lanes an accumulate may take (MsmArgs::lane_fraction, else h2_set_option)
};

struct MsmShape {
    int c, W;
    u32 NB;          // buckets per slice = 2^(c-1)
    u32 slices;      // generic: W; registered (precomputed table): 1
    size_t m;        // digit columns per window = points used + (blind ? 1 : 0)
    size_t items;    // digit codes per slice: generic m, registered W*m
    u32 B, chunk;    // chunks per slice, codes per chunk
    u32 total_buckets;
};

// ---- two-pass sort for the registered (one bucket slice) path ------------------------------------------------------
// A counting sort straight into 2^15 buckets writes 16.8 M 4-byte entries to 16.8 M unrelated places: every workgroup
// keeps 32768 cache lines open, nothing combines in L2, and the pass runs at random-scatter speed (0.2 ms,
// bench/ubench_scatter.hip) on top of 32 MiB of per-chunk histograms.  Split the bucket id instead:
//   pass 1  partition by the top HIB bits (~512 bins): a workgroup keeps one open line per bin, so its 4-byte writes
//           combine in its XCD's L2; the low LOWB bits of the bucket ride in the unused bits of the entry;
//           the digits are recomputed from the scalars (same 32 B per scalar as a digit buffer would cost to read);
//   pass 2  chunks of 16 K entries of the pass-1 output span one or two bins = 64..128 buckets: counting sort inside
//           that window, a few hundred bytes per bucket per chunk.
// Per-chunk histograms shrink from 32 MiB to ~2.4 MiB.  Entry order inside a bucket is irrelevant to the sum.
struct Sort2 {
    u32 m;            // scalars incl. the optional blind
    int c, W, mont;
    u32 stride, extra_col;
    int lowb, lb;     // low bucket bits carried in the entry at bit `lb`
    u32 nh;           // pass-1 bins = NB >> lowb
    u32 B1;           // pass-1 workgroups (kS1Scalars scalars each)
    u32 K2, B2;       // pass-2 chunk size and worst-case chunk count
    u32 lds_window;   // widest pass-2 window (buckets) whose counters fit LDS; wider ones count in HBM
    u32 s1_scalars;   // scalars per pass-1 workgroup (a multiple of 1024)
    u32 run_lanes;    // lanes that copy one bin's run out of the pass-1 stage (a power of two <= 64)
    u32 nb;           // buckets per slice; generic path: sort key = window * nb + bucket, entry = digit column
    int side;         // 1: the low bucket bits of a tagged entry live in the 16-bit side array, not in the entry
    u32 col0;         // registered path: scalar i sits in table column col0 + i (a column RANGE of the table: the chunks of a pipelined host commit)
    int pair_shift;   // >= 0: registered PAIR commit -- column i < pair_n feeds output (i >> pair_shift) & 1, a tail column
    u32 pair_n;       //       i >= pair_n feeds output (i - pair_n) & 1; sort key = side * nb + bucket (two bucket slices)
};

// one GROUP of window slices of a large generic multiexp, sorted on its own (msm_generic.hip; kernels msm_d1_* in msm_sort.hip)
struct GroupSort {
    u32 cols;         // digit columns = 2 x scalars (column i: k1 / P_i, column m + i: k2 / phi(P_i))
    u32 row;          // digit row stride: cols rounded up to 8
    u32 w0, ns;       // the group's window slices [w0, w0 + ns)
    u32 nb;           // buckets per slice; sort key = (w - w0) nb + bucket
    int lowb, lb;     // the low `lowb` key bits ride in the tagged entry at bit `lb` (above the column index)
    u32 nh;           // pass-1 bins = ceil(ns nb >> lowb)
    u32 S;            // digit columns per pass-1 workgroup (a multiple of 8)
    u32 run_lanes;    // lanes that copy one bin's run out of the pass-1 stage
};

// ---- column-batched launches ------------------------------------------------------------------------------------------------------
// The column commits of a prover phase are independent multiexps over ONE registered table (plonk/prover.rs:93-101, 301-313;
// vanishing/prover.rs:96-108).  A batched commit (h2_commit_batch_device) runs every stage ONCE for K columns: blockIdx.z is the
// column, the per-column work areas lie a fixed stride apart, the scalar / blind / output pointers ride in the kernel arguments.
// The sort and fold stages are chains of short latency-bound launches when they serve one column; with K columns per launch they
// become throughput kernels, and the accumulate's K x 512 workgroups refill the chip as they retire instead of as whole launches.
static constexpr int kMaxCols = 8;
struct ColIn {                      // pass 1 of the sort
    const u32 *scalars[kMaxCols];
    const u32 *blinds[kMaxCols];    // null entries: no blind term
};
struct ColOut {                     // fold9_planes
    u32 *out[kMaxCols];
};
struct ColStride {                  // 32-bit words between the areas of consecutive columns (all zero for a single column)
    u32 hist, plan, items, starts, heavy, hscratch, heads, buckets, lines, planes, ctr;
    u32 entries;      // sorted entries: `items` apart, or 0 when the columns are JOINED (below)
    u32 lowprio;      // != 0: the fold kernels keep wave priority 0 (they have slack and must not stretch an accumulate that shares their SIMDs)
    u32 joined;       // != 0: the pass-1 bin count nh.  The columns' sorted entries then form ONE list (column z's behind those of the
                      // columns before it) with ONE boundary array over K x total_buckets buckets (bucket b of column z at
                      // z * total_buckets + b), which msm_accumulate and fold9_finish walk as if it were a single commit
};

struct MsmArgs {
    const void *d_scalars;       // n_used scalars
    const void *d_extra_scalar;  // blind or null
    const void *d_bases;         // generic: n_used affine points; registered: table [W][stride]
    const void *d_extra_base;    // generic + blind: w's buffer; else null
    size_t n_used;
    bool table;                  // registered (precomputed) shape
    int c;                       // window bits (fixed by the table when `table`)
    u32 stride;                  // table row stride (n_registered + 1)
    u32 extra_col;               // table column of the blind's base; 0xFFFFFFFF when unused
    int form, out_kind;
    void *d_out;
    double lane_fraction = 0.0;  // 0 = the process-wide option; the batch entry point narrows its commits
    int pair_shift = -1;         // >= 0 (registered only): two outputs from one column, see Sort2::pair_shift; d_out holds both
    u32 pair_n = 0;
    u32 col0 = 0;                // registered only: the scalars are table columns [col0, col0 + n_used)
    // A commit assembled from RANGES (the chunks of a pipelined host transfer): each range runs sort + accumulate + finish and
    // adds its finished buckets into `add_into` (XYZZ, reference Montgomery form, [NB]) instead of folding them; one fold-only
    // call (`fold_from`) then reduces the summed buckets: the ranges share ONE fold instead of paying one each.
    u32 *add_into = nullptr;
    const u32 *fold_from = nullptr;
    // Column-batched commit (registered tables, wide windows): ncols independent columns of n_used scalars each run through ONE
    // launch set, blockIdx.z = column (ColIn / ColOut / ColStride above).  Host arrays of device pointers; col_blinds may be null.
    // msm_launch answers H2_ERR_BATCH_SHAPE before launching anything when the shape does not take the batched form.
    // phase: 0 the whole multiexp; 1 stop after the sort (nothing has read d_bases yet); 2 resume after it (same arguments, same stream).
    // h2_msm uses 1 / 2 to run the sort -- which needs the scalars only -- while the bases are still crossing PCIe.  Its range
    // pipeline cuts finer: 3 = resume after the sort and stop after the accumulate (the full-chip part); 4 = the fold alone, behind a
    // phase-3 call of the same arguments (possibly on ANOTHER stream, ordered by the caller's events).  slice_sums_only (generic
    // path with window slices on the carry-free fold): the fold stops at the per-slice sums in cx.ssums (XYZZ, 32 words per slice) --
    // the caller runs ONE Horner step over the sums of several ranges (msm_combine_ranges) instead of one chain of ~128 doublings
    // per range; H2_ERR_BATCH_SHAPE, before anything is launched, when the shape does not take that form.
    int phase = 0;
    bool slice_sums_only = false;
    int ncols = 1;
    const void *const *col_scalars = nullptr;
    const void *const *col_blinds = nullptr;
    void *const *col_outs = nullptr;
};

// What one call of msm_launch decides before it enqueues or reserves anything (msm_plan): the shape, which sort / accumulate /
// fold forms the call takes, their geometries and the sizes its reservations follow from.  Plain data: no pointer into a context.
struct MsmPlan {
    MsmShape sh;
    size_t m, scalars_n;  // digit columns (twice the scalars under the endomorphism split); scalars (+ blind) before the split
    size_t all_items;     // W * m: the most entries the sorted list can hold (per column)
    bool fold_only;       // a.fold_from: nothing but the fold of buckets summed elsewhere
    bool add_only;        // a.add_into: a range of a chunked commit stops at its finished buckets
    bool glv;             // generic path: k = k1 + k2 lambda, two half-length digit columns per scalar
    bool m9;              // the accumulate runs on the carry-free layer (registered tables; generic bases converted per call)
    bool pair;            // registered pair commit: two bucket slices, two outputs
    u32 K;                // columns of a batched commit (1: a single multiexp)
    bool joined;          // ... whose sorted lists form ONE list (ColStride::joined)
    u32 tb, nblocks;      // total buckets; scan blocks over them
    u32 T, lane_div;      // lanes of the accumulate; entries per lane it aims at
    size_t head_slots;    // range heads parked in cx.seg9, in front of the K x tb bucket slots
    bool use_sort2;       // two-pass sort (S2 filled), else the one-pass sort
    Sort2 S2;
    bool s2_bins_form;    // pass 2 in its one-launch form (a workgroup per pass-1 bin) with an LDS stage of s2_cap_entries
    size_t s2_cap_entries, plan_words;
    u32 max_big;          // oversized pass-2 bins handed to the chunked msm_s2_big_* kernels (0: none, their launches are skipped)
    bool zero_in_sort;    // the one-launch pass 2 also clears the raw bucket slots
    bool fold9;           // the fold on the carry-free layer (fold9_* kernels), else the 8 x 32 finisher and fold
    bool wide_reduce;     // more than 2^15 buckets a slice on the 8 x 32 fold: row / column sums first
    u32 wideS, wideNR;    // the bucket matrix of a slice: wideS columns x wideNR rows
    bool try_grouped;     // a whole large generic multiexp: msm_generic_grouped is asked first
    int split_k;          // != 0: slice split, the lower group's slice count
    ColIn ci;             // column-batched commit: the per-column pointers and the distances between the per-column work areas
    ColOut co;
    ColStride cs;
};

// ---- dynamic LDS sizes and the layout of cx.plan: one function each, for the geometry that decides whether a shape fits and for the launch
// pass 1's stage (msm_s1_scatter): three words per bin, one more, and the digits of `scalars` scalars at `digits` digits each
constexpr size_t s1_stage_bytes(size_t nh, size_t scalars, size_t digits) { return (nh * 3 + 1 + scalars * digits) * 4; }
// the grouped form's pass 1 (msm_d1_scatter): the same stage over `cols` digit columns of the group's ns slices
constexpr size_t d1_stage_bytes(size_t nh, size_t cols, size_t ns) { return (nh * 3 + 1 + cols * ns) * 4; }
// the chunked pass 2: msm_s2_count's window counters, and msm_s2_scatter's (the same, or its staged window over one chunk)
constexpr size_t s2_count_bytes(size_t lds_window, size_t nh) { return (lds_window + nh + 1) * 4; }
constexpr size_t s2_scatter_bytes(size_t lds_window, size_t nh) {
    return std::max<size_t>(s2_count_bytes(lds_window, nh), ((size_t)kS2StageWindow * 3 + 1 + nh + kS2Chunk) * 4 + (size_t)kS2Chunk * 2);
}
// the one-launch pass 2 (msm_s2_bins): two words per bucket of the bin and a stage of `cap` entries.  The stage is the average bin + 25 %
// (two workgroups per CU where that fits: 2^20 scalars at 17 bits, 15 K-entry bins), at most what one workgroup can have; a bin beyond
// its stage takes the direct-scatter branch.
constexpr size_t s2_bins_bytes(int lowb, size_t cap) { return ((((size_t)1 << lowb) * 2) + cap) * 4; }
constexpr size_t s2_bins_cap(int lowb, size_t avg_bin) {
    const size_t nbk = (size_t)1 << lowb, cap_max = nbk * 8 + 64 < kLdsCap ? (kLdsCap - nbk * 8) / 4 : 0;
    return std::min(cap_max, std::max<size_t>(4096, avg_bin * 5 / 4 + 1024));
}
// the list of oversized bins and the chunked msm_s2_big_* kernels' counters behind it
constexpr size_t s2_big_words(int lowb) { return 64 + (((size_t)kMaxBig * (kBigChunks + 1)) << lowb); }
// where the two-pass sort keeps its tables inside cx.plan (32-bit words): bin counts, bin starts, then the chunked pass 2's plan and
// histograms -- whose area holds the list of oversized bins when pass 2 takes the one-launch form
struct Sort2Layout { size_t bin_count, bin_start, hlo, woff, hist2, hist2_words, words; };
constexpr Sort2Layout sort2_layout(size_t nh, size_t B2, int lowb) {
    const size_t hist2 = nh * 2 + 1 + B2 * 2 + 1, hist2_words = (nh + B2 + 1) << lowb;
    return {0, nh, nh * 2 + 1, nh * 2 + 1 + B2, hist2, hist2_words, (hist2 + std::max(hist2_words, s2_big_words(lowb)) + 3) & ~(size_t)3};
}
// the grouped form's cx.plan: bin counts, bin starts, the oversized bins
constexpr size_t group_big_offset(size_t nh) { return nh * 2 + 1; }
constexpr size_t group_plan_words(size_t nh, int lowb) { return (group_big_offset(nh) + s2_big_words(lowb) + 3) & ~(size_t)3; }

inline bool glv_applies(size_t n) { return n <= ((size_t)1 << 28); }      // the endomorphism split keeps 2n below 2^31

// Two-pass sort geometry for a table of `stride` columns and window width c: the low `lowb` bucket bits ride in the
// entry above the table index (`lb` bits); the remaining bucket_bits - lowb bits select the pass-1 bin.
inline bool sort2_geometry(u32 stride, int c, int *lowb_out, int *lb_out, int *side_out = nullptr, u32 *s1_out = nullptr) {
    const int W = 255 / c + 1, bucket_bits = c - 1;
    const uint64_t top = (uint64_t)W * stride - 1;
    if (top >= ((uint64_t)1 << 31)) return false;
    int lb = 0;
    while ((top >> lb) != 0) ++lb;
    // 512 pass-1 bins whenever the low bucket bits have somewhere to ride: in the entry's spare bits above the table index, or
    // -- windows of 18 bits and more at 2^20 points, where those are too few -- in a 16-bit SIDE array next to the tagged list
    // (pass 1 writes 6 bytes per entry instead of 4; without it c = 20 meant 4096 bins and 6-entry runs)
    int lowb = std::min(31 - lb, bucket_bits - 9), side = 0;
    // ... only where the entry's own spare bits would leave more than 1024 bins: at 17-bit windows over 2^20 points (1024 bins
    // without it) the side array buys nothing and costs 50 % more tagged traffic (measured: 1027 against 1026-1038 M/s)
    if (bucket_bits - lowb > 10 && bucket_bits - 9 <= 14 && W <= 64) {
        lowb = bucket_bits - 9;
        side = 1;
    }
    if (lowb < 1 || bucket_bits - lowb > 12) return false;
    const size_t nh = (size_t)1 << (bucket_bits - lowb);
    // pass-1 stage in LDS: 2048 scalars' digits per workgroup, 1024 where narrower windows mean more digits per scalar (13-bit tables:
    // 20 digits) -- only for callers that ask (s1_out); the others keep the fixed 2048 they were measured with
    u32 s1 = kS1Scalars;
    if (s1_out && s1_stage_bytes(nh, s1, W) > kLdsCap) s1 = 1024;
    if (s1_stage_bytes(nh, s1, W) > kLdsCap) return false;
    if (s1_out) *s1_out = s1;
    *lowb_out = lowb;
    *lb_out = lb;
    if (side_out) *side_out = side;
    return true;
}
// The paired commit (h2_commit_pair_device): two bucket slices, key = side * NB + bucket.  Pass 1 stages s1 scalars' digits per
// workgroup in LDS: 2048 for 16 windows, 1024 when narrower windows (smaller tables: more digits per scalar) would not fit.
inline bool pair_geometry(size_t m, int c, u32 stride, int *lowb_out, int *lb_out, u32 *nh_out, u32 *s1_out) {
    if (c > kMaxC || c < 2 || m < 8192) return false;
    const int W = 255 / c + 1;
    const u32 tb = 2u << (c - 1);
    const uint64_t top = (uint64_t)W * stride - 1;
    if (top >= ((uint64_t)1 << 31)) return false;
    int lb = 0, kb = 0;
    while ((top >> lb) != 0) ++lb;
    while (((u64)(tb - 1) >> kb) != 0) ++kb;
    const int lowb = std::min(31 - lb, std::max(1, kb - 9));
    if (lowb < 1) return false;
    const u32 nh = (tb + (1u << lowb) - 1) >> lowb;
    if (nh > 4096) return false;
    u32 s1 = kS1Scalars;
    while (s1 >= 1024 && s1_stage_bytes(nh, s1, W) > kLdsCap) s1 /= 2;
    if (s1 < 1024) return false;
    *lowb_out = lowb;
    *lb_out = lb;
    *nh_out = nh;
    *s1_out = s1;
    return true;
}
// can a table of n points (+ the blind's column) have windows of c > kMaxC bits?  Only where the two-pass sort takes them.
inline bool wide_window_fits(size_t n, int c) {
    int lowb, lb;
    return n + 1 < ((size_t)1 << 31) && sort2_geometry((u32)n + 1, c, &lowb, &lb);
}

// window width: minimise mixed adds + reduce work.  `shared_buckets`: registered bases (one slice).
// The generic path always splits scalars with the endomorphism (glv.cuh): the window Horner it halves (0.35 ms) and the
// smaller fold (9 slices instead of 16) outweigh the extra bucket additions (2n x 9 windows against n x 16, and the
// on-the-fly phi) at every size measured, 2.76 against 3.09 ms even at 2^20.  The size cap only keeps 2n below 2^31.
inline int choose_c(size_t n, bool shared_buckets, const MsmKnobs &kn) {
    // tuning sweeps only; the only way to windows beyond 16 bits (see below)
    if (kn.force_c >= 4 && kn.force_c <= kMaxCShared && (kn.force_c <= kMaxC || (shared_buckets && wide_window_fits(n, kn.force_c)))) return kn.force_c;
    // Windows of 17..20 bits (registered path) are implemented and parity-tested but not chosen: at n = 2^20, c = 20 cuts
    // the accumulate from 1.29 to 1.07 ms (13 windows instead of 16) and loses more than that in the sort (4096 pass-1
    // bins: 6-entry runs) and in the fold over 2^19 buckets (0.49 vs 0.27 ms).  DESIGN.md section 8.
    const bool glv = !shared_buckets && glv_applies(n);
    // With the split, magnitudes have 128 bits, so the TOP window of width c holds 128 - c floor(127 / c) significant
    // bits: 2 for c = 14, 8 for c = 12 or 15 -- every entry of that window then lands in a few hundred buckets, which are
    // summed by the (slow) heavy-bucket path.  c = 10, 13 and 16 fill their top window (8 of 10, 11 of 13, 16 of 16 bits).
    // Small multiexps are pure latency (a chain of ~128 doublings plus the per-slice folds); measured over c = 4..14
    // (bench/tools/c_sweep_small.py): 0.67-0.72 ms at c = 10 up to 2^12 points, c = 13 up to 2^19 (2^18: 1.08 against 1.20 ms at
    // c = 16, 2^19: 1.43 against 1.52; 2^20: equal, and the accumulate is shorter with 16), c = 16 beyond.
    // (round 3, with the fold on the carry-free layer, bench/tools/generic_ms.py: 2^12 at 13 / 10 bits 0.461 / 0.474 ms; 2^18 at 16 / 13
    // bits 0.846 / 0.851; 2^19 1.11 / 1.165: 10 bits up to 2^11, 13 up to 2^18, 16 beyond)
    if (glv) return n <= 2048 ? 10 : n <= 262144 ? 13 : 16;
    // Registered tables: a commit below ~2^17 points is a chain of latency-bound kernels, not bucket arithmetic, and the widths
    // whose top window is nearly empty (255 mod c small: 12, 14) send that window through the heavy-bucket path.  Measured, one
    // commit alone (bench/tools/c_sweep_registered.py): 8 bits up to 2^9 points (0.21-0.27 ms), 10 up to 2^10 (0.32), 13 up to
    // 2^13 (0.35-0.39; 12 bits at 2^12: 0.59; a paired commit at 2^13: 0.39 against 0.44 with 16), 16 from 2^14 on (0.41-0.49;
    // the cost model below picked 13-14 bits there: 2^15 0.48 -> 0.42).  Re-measured in round 3 with the fold on the carry-free
    // layer (bench/tools/lone_commit_ms.py, H2_MSM_C): 2^14 / 2^15 / 2^16 at 16 bits 0.24 / 0.27 / 0.27 ms, at 14 bits 0.32 / 0.37 /
    // 0.42, at 13 bits 0.37 / 0.54 / 0.59; 2^13 at 16 / 13 bits 0.244 / 0.294; 2^12 0.254 / 0.236; 2^11 0.263 / 0.222; 2^10 0.248 / 0.200
    // (10 bits: 0.258); 2^9 0.251 / 0.196 (8 bits: 0.256); 2^8 at 13 / 8 bits 0.204 / 0.196: 8 bits up to 2^8, 13 up to 2^12, 16 beyond.
    if (shared_buckets) return n <= 384 ? 8 : n <= 6144 ? 13 : 16;
    double best = 1e300;
    int bc = 4;
    for (int c = 4; c <= kMaxC; ++c) {
        // with the endomorphism split: 2n half-length scalars, 130 / c + 1 windows
        int W = glv ? 130 / c + 1 : 255 / c + 1;
        double pairs = glv ? 2.0 * (double)n : (double)n;
        double buckets = (double)(1u << (c - 1)) * (shared_buckets ? 1 : W);
        double cost = (double)W * pairs * 10.5 + buckets * 60.0;
        if (cost < best) { best = cost; bc = c; }
    }
    return bc;
}
// Window width for a table that only serves independent column commits (Params::g, g_lagrange): from 2^18 points on 17 bits --
// 255 = 15 x 17, so a scalar leaves 15 digits instead of 16 (the top window of a scalar below q never exceeds 2^16, half the
// window, so the signed recode carries nothing out of it): the accumulate is ~6 % shorter, the sort and
// the fold (2^16 buckets) ~0.07 ms longer, which independent commits hide (953-966 against 925-939 M scalar-mults/s, one box,
// one lone commit unchanged).  The paired commit and the collapsed-generator read-out of the opening argument take 16-bit
// tables, which is what h2_bases_register keeps building.  `forced` (H2_COLUMN_C): sweeps only, 0 = none.
inline int column_window_bits(size_t n, int forced, const MsmKnobs &kn) {
    const int c = choose_c(n ? n : 1, true, kn);
    if (forced >= 4 && forced <= kMaxCShared && (forced <= kMaxC || wide_window_fits(n, forced))) return forced;
    return c == 16 && n >= ((size_t)1 << 18) && wide_window_fits(n, 17) ? 17 : c;
}
// the widths h2_bases_register_ex builds a table of n points with when asked for one
inline bool register_width_ok(size_t n, int window_bits) {
    return window_bits >= 4 && window_bits <= kMaxCShared && (window_bits <= kMaxC || wide_window_fits(n, window_bits));
}
// h2_commit_pair_supported
inline bool pair_supported(size_t n, const MsmKnobs &kn) {
    int lowb, lb;
    u32 nh, s1;
    return n >= 8 && n <= (1u << 26) && pair_geometry(n, choose_c(n, true, kn), (u32)n + 1, &lowb, &lb, &nh, &s1);
}

// m: digit columns (generic path with the endomorphism split: 2 x scalars, `glv` picks the shorter window count)
inline MsmShape make_shape(size_t m, int c, bool shared_buckets, bool glv = false) {
    MsmShape s;
    s.c = c;
    s.W = glv ? 130 / c + 1 : 255 / c + 1;
    s.NB = 1u << (c - 1);
    s.slices = shared_buckets ? 1 : (u32)s.W;
    s.m = m;
    s.items = shared_buckets ? (size_t)s.W * m : m;
    u32 B = (u32)((s.items + 65535) / 65536);
    s.B = B < 1 ? 1 : B;
    s.chunk = (u32)((s.items + s.B - 1) / s.B);
    s.total_buckets = s.slices * s.NB;
    return s;
}

// The accumulate runs on the carry-free layer for registered tables (stored in M9 form: h2_bases_register) and for the generic path's endomorphism
// split (bases converted per call); only a generic call with a blind term keeps the 8 x 32 layer.
inline bool msm_glv(const MsmArgs &a) { return !a.table && !a.d_extra_scalar && glv_applies(a.n_used); }
inline bool msm_m9(const MsmArgs &a) { return a.table || msm_glv(a); }

// the fields every two-pass shape fills the same way (`scalars` per pass-1 launch, pass-2 windows over `window` buckets); the arms of msm_plan
// set what differs: stride, extra_col, side, col0, the pair fields
inline void sort2_fill(Sort2 &S2, const MsmArgs &a, const MsmShape &sh, size_t scalars, size_t all_items, int lowb, int lb, u32 nh, u32 s1, u32 window) {
    S2.m = (u32)scalars; S2.c = sh.c; S2.W = sh.W; S2.mont = a.form == H2_FORM_MONTGOMERY;
    S2.extra_col = 0xFFFFFFFFu;
    S2.lowb = lowb; S2.lb = lb; S2.nh = nh;
    S2.s1_scalars = s1; S2.nb = sh.NB; S2.B1 = (u32)((scalars + s1 - 1) / s1);
    S2.K2 = kS2Chunk; S2.B2 = (u32)((all_items + kS2Chunk - 1) / kS2Chunk);
    S2.lds_window = std::min<u32>(window, 32768u);
}
// Every decision of one call, before anything is enqueued or reserved.  `lanes`: the lanes of this call's accumulate kernel the chip
// holds at once; `instrumented` (h2_profile_enable, H2_TIMELINE=1) keeps a call off the grouped form and the slice split.
// H2_ERR_ARGS / H2_ERR_BATCH_SHAPE when the shape takes no form (or not the batched / slice-sums form it asks for).
inline int msm_plan(const MsmArgs &a, u32 lanes, bool instrumented, const MsmKnobs &kn, MsmPlan *plan) {
    MsmPlan &p = *plan;
    memset(&p, 0, sizeof p);
    size_t m = a.n_used + (a.d_extra_scalar ? 1 : 0);
    p.fold_only = a.fold_from != nullptr;
    p.add_only = a.add_into && !p.fold_only;
    // generic path: every scalar is split k = k1 + k2 lambda (glv.cuh) into two half-length digit columns, i for P_i and
    // n + i for phi(P_i): as many bucket additions (2n x 9 windows against n x 16), half the doublings in the final Horner
    const bool glv = p.glv = msm_glv(a);
    const bool m9 = p.m9 = msm_m9(a);
    const size_t scalars_n = p.scalars_n = m;
    if (glv) m *= 2;
    if (p.fold_only && m < 1) m = 1;                   // only the bucket geometry (c) matters to the fold
    p.m = m;
    MsmShape &sh = p.sh;
    sh = make_shape(m, a.c, a.table, glv);
    const u32 K = p.K = a.ncols > 1 ? (u32)a.ncols : 1u;
    if (K > 1 && (K > (u32)kMaxCols || !a.table || a.pair_shift >= 0 || a.add_into || p.fold_only || !a.col_scalars || !a.col_outs || a.n_used == 0))
        return H2_ERR_BATCH_SHAPE;
    p.pair = a.table && a.pair_shift >= 0;
    if (p.pair) {                     // one bucket slice per output
        sh.slices = 2;
        sh.total_buckets = 2 * sh.NB;
    }
    const u32 tb = p.tb = sh.total_buckets;
    const size_t all_items = p.all_items = (size_t)sh.W * m;
    if (all_items >= ((size_t)1 << 31)) return H2_ERR_ARGS;  // entry = table index | sign << 31
    p.nblocks = (tb + kScanBlock - 1) / kScanBlock;
    // one round of resident lanes; small problems use fewer lanes so a range keeps >= 16 entries
    // a lane fraction < 1 (h2_set_option) leaves wave slots free so that the latency-bound sort / reduce kernels
    // of a commit running on ANOTHER stream can overlap this kernel (independent column commits)
    const u32 usable = std::max(256u, (u32)(lanes * kn.lane_fraction) / 256u * 256u);
    // entries per lane of the accumulate: 16 for full-size columns; small commits are chains of latency-bound kernels and run
    // shorter with more, shorter lanes (one registered commit at 2^11 .. 2^15 points: 3-7 % faster at 8; H2_MSM_DIV: sweeps only)
    p.lane_div = kn.lane_div ? kn.lane_div : (all_items < ((size_t)1 << 20) ? 8u : 16u);
    // Column-batched commits are JOINED (ColStride::joined) unless H2_BATCH_JOIN=0: the K sorted lists form one, which ONE launch of
    // msm_accumulate cuts into equal ranges -- the chip is tiled exactly as by a single commit (a launch per column leaves its last
    // round of workgroups ragged, and K of them next to each other share CUs unevenly), and the finisher meets T range heads per
    // batch instead of per column.
    const bool joined = p.joined = K > 1 && kn.batch_join;
    const u32 T = p.T = (u32)std::min<size_t>(usable, std::max<size_t>(256, ((joined ? K : 1) * all_items / p.lane_div + 255) / 256 * 256));
    p.head_slots = joined ? (size_t)T : (size_t)T * K;
    // two-pass sort (registered path): always for windows beyond 16 bits, else for large bucket counts
    Sort2 &S2 = p.S2;
    S2.pair_shift = -1; S2.run_lanes = 16;
    if (p.pair) {
        // key = side * NB + bucket over both slices (the generic path's multi-slice geometry), entry = table index
        int lb = 0, lowb = 0;
        u32 nh = 0, s1 = 0;
        if (!pair_geometry(m, sh.c, a.stride, &lowb, &lb, &nh, &s1)) return H2_ERR_ARGS;
        p.use_sort2 = true;
        sort2_fill(S2, a, sh, m, all_items, lowb, lb, nh, s1, tb);
        S2.stride = a.stride; S2.pair_shift = a.pair_shift; S2.pair_n = a.pair_n;
    } else if (a.table && (sh.c > kMaxC || (sh.NB >= 4096 && (m >= 8192 || K > 1)))) {
        // (a column-batched commit exists in the two-pass form only, so it takes it from 13-bit tables on whatever the column length:
        // eight 2^12-point columns in one launch set are 0.3 ms against 0.9 ms for eight chains of one-pass sorts)
        int lowb = 0, lb = 0, side = 0;
        u32 s1 = kS1Scalars;
        if (sort2_geometry(a.stride, sh.c, &lowb, &lb, &side, &s1)) {
            p.use_sort2 = true;
            sort2_fill(S2, a, sh, m, all_items, lowb, lb, sh.NB >> lowb, s1, sh.NB);
            S2.stride = a.stride; S2.side = side; S2.col0 = a.col0;
            if (a.d_extra_scalar) S2.extra_col = a.extra_col;
        }
    } else if (glv && scalars_n >= 65536) {
        // generic path, large: sort key = window * NB + bucket over all slices, entry = digit column (< 2 * scalars)
        int lb = 0, kb = 0;
        while (((u64)(m - 1) >> lb) != 0) ++lb;
        while (((u64)(tb - 1) >> kb) != 0) ++kb;
        // bins of ~16 K entries (kb - 11 bucket bits per bin: 1152 bins for 9 slices of 2^15 buckets), so that pass 2 is the
        // one-launch form with a bin per workgroup in LDS (9 bits = the chunked pass 2 of round 2).
        // Up to 2^19 scalars only: the carry slice of the split (the window above the top of a 128-bit half) puts ~n / 2 entries
        // into ONE bucket, and a bin that large was scattered by a single workgroup (2^19: sort 0.28 -> 0.16 ms; 2^20: 0.30 -> 0.61).
        // With the oversized-bin kernels (msm_s2_big_*) that bin is chunked over 64 workgroups: 2^20 takes the one-launch form with
        // 10 bits (1.83 -> 1.71 ms on one box; 11 bits 1.80, 12 bits 1.83); from 2^21 the forms are equal within 1 %.
        const int bin_bits = scalars_n <= ((size_t)1 << 19) ? 11 : scalars_n <= ((size_t)1 << 20) ? 10 : 9;
        const int lowb = std::min(31 - lb, std::max(1, kb - bin_bits));
        const u32 nh = (tb + (1u << lowb) - 1) >> lowb;
        const u32 s1 = 1024;                               // (two digit columns per scalar)
        if (lowb >= 1 && nh <= 4096 && s1_stage_bytes(nh, s1, 2 * (size_t)sh.W) <= kLdsCap) {
            p.use_sort2 = true;
            sort2_fill(S2, a, sh, scalars_n, all_items, lowb, lb, nh, s1, tb);
        }
    }
    if (sh.c > kMaxC && !p.use_sort2) return H2_ERR_ARGS;   // choose_c only picks wide windows the two-pass sort can take
    if (K > 1 && !p.use_sort2) return H2_ERR_BATCH_SHAPE;
    p.wide_reduce = sh.NB > 32768u;                       // implies the registered path (one slice)
    // the fold on the carry-free layer (fold9_* kernels: registered tables from 16-bit windows, paired commits, and the window
    // slices of a large generic multiexp); a range of a chunked commit hands finished buckets on in the reference's form
    // (add_into), so it keeps the 8 x 32 finisher
    p.fold9 = sh.NB >= 128 && sh.slices <= 16 && m9 && !a.add_into && !p.fold_only;      // (16: arrival counters of fold9_planes)
    if (K > 1 && !p.fold9) return H2_ERR_BATCH_SHAPE;
    if (a.slice_sums_only && !(p.fold9 && glv)) return H2_ERR_BATCH_SHAPE;
    // The grouped form (round 6, msm_generic.hip; generic multiexps beyond 2^18 points): the endomorphism split once, the window slices
    // sorted / accumulated / folded in groups, upper slices first.  It answers H2_ERR_BATCH_SHAPE before enqueueing anything when the shape
    // is not its own; round 5's slice split below then still applies (and is the A/B arm, H2_GENERIC_GROUPED=0 in the laboratory build).
    p.try_grouped = glv && p.fold9 && a.phase == 0 && !a.slice_sums_only && K == 1 && !instrumented;
    // Slice split (round 5; generic multiexps from 2^19 points): the sorted list is ordered by (slice, bucket), so the upper slices
    // [split_k, slices) and the lower ones [0, split_k) are two contiguous halves of it.  They are accumulated one after the other on
    // `st`; as soon as the UPPER group is in its buckets its fold and its Horner chain -- (slices - 1) c ~ 128 dependent doublings, 0.25 ms
    // on one quad of lanes, which used to follow the whole accumulate -- run on a side stream beside the lower group's accumulate and
    // fold.  What is left behind the accumulate: the lower group's fold, (split_k - 1) c doublings and one addition.  The bases'
    // conversion to M9 form runs on the side stream beside the sort.  H2_GENERIC_SPLIT=0: off (A/B); = k: force the lower group's size.
    if (p.try_grouped && sh.slices >= 6 && kn.generic_split != 0) {
        if (kn.generic_split > 0) p.split_k = std::min<int>(kn.generic_split, (int)sh.slices - 2);
        else if (scalars_n >= ((size_t)1 << 19)) p.split_k = 3;
    }
    if (p.split_k) p.head_slots = 2 * (size_t)T;             // each group's T range heads
    // pass 2 of the two-pass sort in its one-launch form (a workgroup per pass-1 bin; the chunked form otherwise)?  Decided here, before
    // anything is launched, because a column-batched commit exists in that form only.
    if (p.use_sort2) {
        const size_t nbk = (size_t)1 << S2.lowb;
        p.s2_cap_entries = s2_bins_cap(S2.lowb, all_items / S2.nh);
        const size_t nbins = ((size_t)tb + nbk - 1) >> S2.lowb;
        p.s2_bins_form = S2.lowb <= 12 && nbins == S2.nh && p.s2_cap_entries && all_items / S2.nh <= p.s2_cap_entries * 9 / 10;
        p.plan_words = sort2_layout(S2.nh, S2.B2, S2.lowb).words;
    }
    if (K > 1 && !p.s2_bins_form) return H2_ERR_BATCH_SHAPE;
    if (p.wide_reduce || p.fold9) {
        p.wideS = 1u << ((sh.c - 1) / 2);
        p.wideNR = sh.NB / p.wideS;
    }
    // the one-launch pass 2 also clears the raw bucket slots (its workgroups own disjoint bucket ranges)
    p.zero_in_sort = m9 && p.use_sort2 && p.s2_bins_form && !p.fold_only;
    // oversized pass-2 bins (degenerate columns) go to the chunked msm_s2_big_* kernels only where a bin can be large enough for
    // that to matter: below 3 * 2^20 entries per column (2^18 scalars) the bin's own workgroup streams it (<= 2^17 entries: tens of
    // microseconds, and only for such columns), and every commit saves three launches that would find an empty list
    p.max_big = all_items >= ((size_t)3 << 20) ? kMaxBig : 0u;
    // column-batched commit: the per-column pointers and the distances between the per-column work areas (32-bit words)
    if (K > 1) {
        for (u32 k = 0; k < K; ++k) {
            p.ci.scalars[k] = (const u32 *)a.col_scalars[k];
            p.ci.blinds[k] = a.col_blinds ? (const u32 *)a.col_blinds[k] : nullptr;
            p.co.out[k] = (u32 *)a.col_outs[k];
            if (!p.ci.scalars[k] || !p.co.out[k] || (a.d_extra_scalar && !p.ci.blinds[k])) return H2_ERR_ARGS;
        }
        ColStride &cs = p.cs;
        cs.hist = (u32)((size_t)S2.B1 * S2.nh);
        cs.plan = (u32)p.plan_words;
        cs.items = (u32)all_items;
        cs.entries = joined ? 0u : (u32)all_items;
        cs.joined = joined ? S2.nh : 0u;
        cs.starts = joined ? tb : tb + 2;
        cs.heavy = kMaxHeavy + 2;
        cs.hscratch = kMaxHeavy * kHeavyBlocks * 36;
        cs.heads = T * 36;
        cs.buckets = tb * 36;
        cs.lines = sh.slices * (p.wideS + p.wideNR) * 36;
        cs.planes = sh.slices * 32 * 36;
        cs.ctr = 16;
    }
    return H2_OK;
}

// h2_commit_last_plan: the plan of a call over a registered table as plain integers, and the record of a call with nothing to sum
// (kind 1: the identity was written; 2: an empty range of a host commit)
inline h2_commit_plan_t plan_summary(const MsmPlan &p, u32 lanes) {
    h2_commit_plan_t r = {};
    r.caller = H2_COMMIT_CALLER_DIRECT;
    r.caller_count = 1;
    r.lanes = lanes;
    r.c = (u32)p.sh.c; r.W = (u32)p.sh.W; r.m = (u32)p.m; r.K = p.K; r.T = p.T; r.lane_div = p.lane_div;
    r.use_sort2 = p.use_sort2;
    if (p.use_sort2) { r.s2_lowb = (u32)p.S2.lowb; r.s2_nh = p.S2.nh; r.s2_side = (u32)p.S2.side; r.s2_s1_scalars = p.S2.s1_scalars; }
    r.s2_bins_form = p.s2_bins_form; r.max_big = p.max_big; r.zero_in_sort = p.zero_in_sort;
    r.fold9 = p.fold9; r.wide_reduce = p.wide_reduce; r.pair = p.pair; r.joined = p.joined; r.add_only = p.add_only; r.fold_only = p.fold_only;
    return r;
}
inline h2_commit_plan_t empty_summary(const MsmArgs &a, u32 kind) {
    h2_commit_plan_t r = {};
    r.caller = H2_COMMIT_CALLER_DIRECT;
    r.caller_count = 1;
    r.empty = kind;
    r.c = (u32)a.c;
    r.add_only = a.add_into != nullptr;
    return r;
}

// ---- the fold (msm_fold.hip, msm_subdigit.hip): the integer code that decides which line carries which weight, and the 8 x 32 fold's launch
// geometry.  tests/native/msm_fold_check.cpp compiles this text for the CPU and tests/test_msm_fold_planes.py adds the weights up.
#ifndef H2_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define H2_HD __host__ __device__ __forceinline__
#else
#define H2_HD inline
#endif
#endif
// the k-th (k = 0, 1, ...) non-negative integer with bit t set: bit t goes in between k's upper and lower bits
H2_HD u32 kth_with_bit(u32 k, u32 t) { return ((k >> t) << (t + 1)) | (1u << t) | (k & ((1u << t) - 1u)); }
// fold9_planes: sum_j (j + 1) B_j = sum_lo (lo + 1) C_lo + S sum_hi hi R_hi over the lines C_0 .. C_(S-1), R_0 .. R_(NR-1) of a slice's NR x S
// bucket matrix (S = 2^cb; line index: lo, or S + hi).  Plane t (weight 2^t, t < cb + log2 NR) holds the columns with bit t of lo + 1 set
// -- plane cb: lo + 1 = S alone -- and the rows with bit t - cb of hi set.
H2_HD u32 fold9_plane_cols(u32 S, int cb, u32 t) { return (int)t < cb ? S / 2 : (int)t == cb ? 1u : 0u; }
H2_HD u32 fold9_plane_rows(u32 NR, int cb, u32 t) { return (int)t >= cb ? NR / 2 : 0u; }
H2_HD u32 fold9_plane_line(u32 S, int cb, u32 t, u32 k) {      // the line of the plane's k-th summand: its columns, then its rows
    const u32 ncol = fold9_plane_cols(S, cb, t);
    if (k < ncol) return (int)t == cb ? S - 1 : kth_with_bit(k, t) - 1u;
    return S + kth_with_bit(k - ncol, t - (u32)cb);
}
inline u32 fold9_plane_count(int c) { return (u32)c - 1; }      // planes of a slice of 2^(c-1) buckets = workgroups (grid x) of fold9_planes: log2 S + log2 NR
inline int fold9_col_bits(u32 S) {
    int cb = 0;
    while ((1u << cb) < S) ++cb;
    return cb;
}
// sub_planes: a slice of 128 buckets (bucket b weighs b + 1) in 8 planes; plane t < 7 holds the 64 buckets with bit t of b + 1 set, plane 7
// bucket 127 alone
H2_HD u32 sub_plane_count(u32 t) { return t < 7 ? 64u : 1u; }
H2_HD u32 sub_plane_bucket(u32 t, u32 k) { return t < 7 ? kth_with_bit(k, t) - 1u : 127u; }

// The 8 x 32 fold behind the finished buckets (fold_r256).  Wide slices (wide_reduce) are folded through their row / column sums, laid out as
// two slices of wideNR points that a Horner step of log2 S bits joins.  A segment is 2 seg running-sum additions + a small-scalar multiple
// (~23 more dependent operations) on one quad of lanes: 4 buckets while the segments fit the chip a few times over (the fold is their
// latency: one commit 0.235 -> 0.218 ms, small commits 5-8 %), 8 when there are many slices (generic multiexps of 2^20 points: the multiples
// are throughput).  The slice tree (msm_sum_slice) has 64 quads per workgroup; its first level leaves <= 32 block sums per slice, which a
// second level of one workgroup per slice adds; few partials take that one workgroup alone.
static constexpr u32 kTreeLanes = 256;
constexpr size_t r256_tree_bytes(u32 lanes) { return (size_t)lanes / 4 * 128; }      // dynamic LDS of a tree launch: one XYZZ point per quad of lanes
struct R256Fold {
    u32 nb, slices;     // what msm_reduce_segments runs over: `slices` slices of `nb` points
    int c;              // the Horner step's window width
    int seg;            // buckets per segment
    u32 segs;           // segments in all
    int levels;         // launches of msm_sum_slice: 1 or 2
    struct Level {
        u32 blocks;     // workgroups per slice = sums this level leaves per slice (the last level: 1)
        u32 per_slice;  // points per slice it reads
        u32 share;      // ... and per workgroup
    } level[2];
};
inline R256Fold r256_fold_geometry(const MsmShape &sh, bool wide_reduce, u32 wideNR) {
    R256Fold f;
    f.nb = wide_reduce ? wideNR : sh.NB;
    f.slices = wide_reduce ? 2 : sh.slices;
    f.c = wide_reduce ? (sh.c - 1) / 2 : sh.c;      // (log2 S)
    f.seg = (size_t)f.slices * f.nb / kSeg <= 32768 ? kSeg : 2 * kSeg;
    f.segs = f.slices * f.nb / f.seg;
    const u32 per_slice = f.nb / f.seg, bps = std::max(1u, std::min(32u, per_slice / (2 * (kTreeLanes / 4))));
    f.levels = bps > 1 ? 2 : 1;
    f.level[0] = {bps, per_slice, (per_slice + bps - 1) / bps};
    f.level[1] = {1, bps, bps};
    return f;
}

// ---- the grouped form of a large generic multiexp (msm_generic.hip has the description) ---------------------------------------------
struct Group {
    u32 w0 = 0, ns = 0;     // window slices [w0, w0 + ns)
    u32 tb = 0;             // its buckets: ns * NB
    GroupSort gs;           // pass 1
    Sort2 p2;               // what the pass-2 kernels read (lowb, lb, nh; no side array)
    size_t cap = 0;         // pass-2 stage of a bin's workgroup, in entries
    size_t emax = 0;        // most entries it can hold: ns * digit columns
    size_t plan_words = 0;
    u32 B1 = 0;             // pass-1 workgroups
    u32 T = 0;              // lanes of its accumulate
    size_t ent_off = 0;     // its sorted list inside cx.entries (entries)
    size_t starts_off = 0;  // its boundary array inside cx.starts (words): tb + 2 of them
    size_t bucket_off = 0;  // its first bucket slot
};

// Pass-1 bins such that an average bin is ~16 K entries (what a pass-2 workgroup stages in LDS with room to spare), the low key bits
// riding in the tagged entry above the column index.
inline bool group_geometry(u32 cols, u32 nb, Group &g) {
    int lb = 0;
    while (((u64)(cols - 1) >> lb) != 0) ++lb;
    g.tb = g.ns * nb;
    g.emax = (size_t)g.ns * cols;
    for (int lowb = 12; lowb >= 1; --lowb) {
        if (lowb + lb > 31) continue;
        const size_t nbk = (size_t)1 << lowb;
        const u32 nh = (u32)(((size_t)g.tb + nbk - 1) >> lowb);
        if (nh > 4096) break;
        const size_t avg = g.emax / nh;
        const size_t cap = s2_bins_cap(lowb, avg);
        if (avg > 20000 || avg > cap * 9 / 10) continue;
        // digit columns per pass-1 workgroup: 4096 (two workgroups per CU) -- 8192 where that still leaves >= 512 workgroups: every workgroup
        // writes and re-reads a histogram row of nh words and copies its entries out in runs of S ns / nh, so large problems want large S
        u32 S = 4096;
        while (S > 512 && d1_stage_bytes(nh, S, g.ns) > kLdsCap / 2) S /= 2;
        if (S == 4096 && cols / 8192 >= 512 && d1_stage_bytes(nh, 8192, g.ns) <= kLdsCap) S = 8192;
        if (d1_stage_bytes(nh, S, g.ns) > kLdsCap) continue;
        memset(&g.gs, 0, sizeof g.gs);
        g.gs.cols = cols;
        g.gs.row = (cols + 7) & ~7u;
        g.gs.w0 = g.w0;
        g.gs.ns = g.ns;
        g.gs.nb = nb;
        g.gs.lowb = lowb;
        g.gs.lb = lb;
        g.gs.nh = nh;
        g.gs.S = S;
        g.gs.run_lanes = 16;
        memset(&g.p2, 0, sizeof g.p2);
        g.p2.lowb = lowb;
        g.p2.lb = lb;
        g.p2.nh = nh;
        g.p2.nb = nb;
        g.p2.pair_shift = -1;
        g.p2.extra_col = 0xFFFFFFFFu;
        g.cap = cap;
        g.B1 = (cols + S - 1) / S;
        g.plan_words = group_plan_words(nh, lowb);
        return true;
    }
    return false;
}

// What one grouped call decides before it reserves or enqueues anything: the form, the groups and the sizes its reservations follow from.
struct GroupedPlan {
    bool throughput;        // one group on the caller's stream (another stream's generic multiexp is in flight), else the latency form
    bool lds_fence;         // the chain links are fenced onto CUs without an accumulate workgroup by LDS requests
    int G;
    Group grp[kMaxGroups];
    size_t head_slots, hist_words, tagged_words, plan_words;
    u32 wideS, wideNR;      // the bucket matrix of a slice (fold9_rowcol / fold9_planes)
};

// Is the shape the grouped form's own?  (No upper bound on scalars_n here: group_geometry declines every size beyond the layouts' limits,
// msm_generic.hip has them.)
inline bool grouped_takes(const MsmShape &sh, size_t scalars_n, const MsmKnobs &kn) {
    return kn.grouped && scalars_n >= ((size_t)1 << 18) + 1 && sh.c >= 8 && sh.c <= kMaxC && sh.W >= 3 && sh.W <= 16 && sh.NB >= 128;
}
// Does a call of that shape ask whether another stream's generic multiexp is in flight (grouped_plan's `other_in_flight`)?  The answer costs
// host time, so only the calls it can change ask: from 2^22 points on the whole sort in front of a single group costs more than the grouping
// loses (837 against 900 M scalar-mults/s on three streams), and a forced form (H2_GG_FORM) needs no answer.
inline bool grouped_asks_in_flight(size_t scalars_n, const MsmKnobs &kn) { return kn.gg_form != 1 && kn.gg_form != 2 && scalars_n < ((size_t)1 << 22); }

// H2_ERR_BATCH_SHAPE when the shape is not the grouped form's own.  other_in_flight: a generic multiexp of another stream of this device has
// not completed (only read where grouped_asks_in_flight).
inline int grouped_plan(const MsmShape &sh, size_t scalars_n, u32 lanes, bool other_in_flight, const MsmKnobs &kn, GroupedPlan &gp) {
    if (!grouped_takes(sh, scalars_n, kn)) return H2_ERR_BATCH_SHAPE;
    const u32 cols = 2 * (u32)scalars_n, W = (u32)sh.W, NB = sh.NB;
    gp.throughput = kn.gg_form == 2 || (grouped_asks_in_flight(scalars_n, kn) && other_in_flight);
    // ---- the groups, upper slices first (H2_GENERIC_GROUPS="a,b,c": laboratory build only)
    int sizes[kMaxGroups] = {0, 0, 0, 0}, sum = 0, least = 1;
    int &G = gp.G = 0;
    for (int i = 0; i < kn.ngroups && i < kMaxGroups; ++i) {
        sum += kn.groups[i];
        least = std::min(least, kn.groups[i]);
    }
    if (kn.ngroups >= 1 && kn.ngroups <= kMaxGroups && sum == (int)W && least >= 1) {
        for (int i = 0; i < kn.ngroups; ++i) sizes[G++] = kn.groups[i];
    } else if (gp.throughput) {
        // independent calls on other streams are in flight: their sorts and folds hide beside this call's accumulate anyway, every accumulate
        // launch that starts beside them runs ragged, and side streams of several calls would share hardware queues: ONE group, everything on
        // the caller's stream (2^20: 1.16-1.22 ms per call on three streams against 1.26-1.46 for any grouping; 2^22: 862 M/s)
        sizes[0] = (int)W;
        G = 1;
    } else {
        // a call alone: 5 + 2 + 2 of nine slices -- the first group's sort is all that stands in front of the first addition, the last
        // (smallest) group's fold all that stands behind the last
        const int last = std::max(1, (int)W * 2 / 9), mid = last, top = (int)W - last - mid;
        sizes[0] = top; sizes[1] = mid; sizes[2] = last;
        G = 3;
    }
    Group *grp = gp.grp;
    u32 hi = W;
    size_t ent = 0, sts = 0, bkt = 0;
    for (int g = 0; g < G; ++g) {
        grp[g].ns = (u32)sizes[g];
        grp[g].w0 = hi - (u32)sizes[g];
        hi = grp[g].w0;
        if (!group_geometry(cols, NB, grp[g])) return H2_ERR_BATCH_SHAPE;
        grp[g].ent_off = ent;
        grp[g].starts_off = sts;
        grp[g].bucket_off = bkt;
        ent += grp[g].emax;
        sts += (size_t)grp[g].tb + 2;
        bkt += grp[g].tb;
    }
    if (ent >= ((size_t)1 << 31)) return H2_ERR_BATCH_SHAPE;
    // The latency form leaves one CU per XCD without an accumulate workgroup and FENCES the chain kernels onto them: every accumulate workgroup asks
    // for 64 KiB of LDS it never touches, every link of the Horner chain for 100 KiB -- so a chain wave (one wave at raised priority issuing
    // dependent multiply-adds back to back: it takes ~90 % of its SIMD) can only land on a CU that holds no accumulate workgroup, instead of
    // starving two accumulate waves for its whole 130-180 us while every other lane of the launch waits for them (measured: the second group's
    // accumulate 494 -> 429 us; profiles/r06_generic_grouped.txt).  H2_GG_SPARE: laboratory build only.
    gp.lds_fence = !gp.throughput && G > 1;
    const u32 spare = kn.gg_spare >= 0 ? (u32)kn.gg_spare : (gp.lds_fence ? std::max(1u, lanes / 512u / 32u) : 0u);      // one CU in 32: 8 of an MI355X's 256 (one per XCD)
    // (signed: a small fraction -- or few CUs -- must not wrap below the spare CUs' share and hand the accumulate every lane there is)
    const long long want_lanes = (long long)((u32)(lanes * kn.lane_fraction) / 512u * 512u) - 512LL * std::min(spare, 64u);
    const u32 usable = (u32)std::max<long long>(512, want_lanes);
    gp.head_slots = gp.hist_words = gp.tagged_words = gp.plan_words = 0;
    for (int g = 0; g < G; ++g) {
        grp[g].T = (u32)std::min<size_t>(usable, std::max<size_t>(512, (grp[g].emax / kLaneDiv + 511) / 512 * 512));
        gp.head_slots += grp[g].T;
        gp.hist_words = std::max(gp.hist_words, (size_t)grp[g].B1 * grp[g].gs.nh);
        gp.tagged_words = std::max(gp.tagged_words, grp[g].emax);
        gp.plan_words = std::max(gp.plan_words, grp[g].plan_words);
    }
    gp.wideS = 1u << ((sh.c - 1) / 2);
    gp.wideNR = NB / gp.wideS;
    return H2_OK;
}

}  // namespace h2
