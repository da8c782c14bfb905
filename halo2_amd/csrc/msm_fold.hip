// After the accumulate: finish (range heads into their buckets), the fold of a bucket slice down to its weighted sum, and the Horner step over
// window slices (reference: the running-sum fold of arithmetic.rs:86-92 and the window loop of :169-178, restructured as trees).  Two layers,
// one of everything on each: the 8 x 32 fold (msm_finish_* .. msm_sum_slice; host side fold_r256) and the carry-free fold (fold9_*; host side
// fold9_group).  The pieces they are made of -- head split, heavy ticket, gather and tree, plane arrival -- are in msm_internal.cuh, the plane
// and launch arithmetic in msm_plan.h, the point writer in curve.cuh.  Every kernel here is launched from this file alone: the host functions
// at its foot (declared in msm_internal.cuh) dispatch on the base field, which is what instantiates the kernels for both curves.
#include "msm_internal.cuh"

namespace h2 {

static_assert(r256_tree_bytes(kTreeLanes) == (kTreeLanes / kGroup) * 128, "a quad of lanes per point of the 8 x 32 tree");

// ---- finisher: bucket b = its own non-head segment + the heads of the ranges that begin inside it -----
// Buckets owning more than kHeavy heads (scalars repeated thousands of times) are parked on a list and summed
// by a whole workgroup each in msm_finish_heavy.
template <int FB>
__global__ void __launch_bounds__(256) msm_finish_buckets(const u32 *__restrict__ heads, const u32 *__restrict__ starts,
                                                          u32 *__restrict__ buckets, u32 *__restrict__ heavy,
                                                          u32 total_buckets, u32 T, u32 div) {
    H2_LATENCY_STAGE();
    // one quad of lanes per bucket (curve_wide.cuh)
    const u32 b = (blockIdx.x * blockDim.x + threadIdx.x) / kGroup;
    if (b >= total_buckets) return;
    const bool lead = (threadIdx.x & (kGroup - 1)) == 0;
    const HeadRange h = bucket_heads<false>(starts, b, total_buckets, T, div);
    if (h.h1 <= h.h0) return;
    if (h.h1 - h.h0 > kHeavy && heavy_park<kGroup>(heavy, b, lead)) return;
    xyzz<FB> acc = xyzz_load<FB>(buckets + 32 * (size_t)b);
    xyzz<FB> nxt = xyzz_load<FB>(heads + 32 * (size_t)h.h0);
    for (u32 t = h.h0; t < h.h1; ++t) {
        xyzz<FB> p = nxt;
        if (t + 1 < h.h1) nxt = xyzz_load<FB>(heads + 32 * (size_t)(t + 1));
        xyzz_add_wide<FB>(acc, p);
    }
    if (lead) xyzz_store<FB>(buckets + 32 * (size_t)b, acc);
}
template <int FB>
__global__ void __launch_bounds__(256) msm_finish_heavy(const u32 *__restrict__ heads, const u32 *__restrict__ starts,
                                                        u32 *__restrict__ scratch, const u32 *__restrict__ heavy,
                                                        u32 total_buckets, u32 T, u32 div) {
    H2_LATENCY_STAGE();
    extern __shared__ __attribute__((aligned(16))) u32 sh[];
    if (blockIdx.y >= min(heavy[1], kMaxHeavy)) return;
    const HeadRange h = bucket_heads<false>(starts, heavy[2 + blockIdx.y], total_buckets, T, div);
    const u32 share = (h.h1 - h.h0 + kHeavyBlocks - 1) / kHeavyBlocks;
    const u32 lo = h.h0 + blockIdx.x * share, hi = min(h.h1, lo + share);
    const xyzz<FB> acc = r256_quad_gather<FB>(heads, hi > lo ? hi - lo : 0u, [lo](u32 k) { return lo + k; });
    r256_quads_sum<FB>(acc, sh, blockDim.x / kGroup);
    if (threadIdx.x == 0) {
        xyzz<FB> r = xyzz_load<FB>(sh);
        xyzz_store<FB>(scratch + 32 * ((size_t)blockIdx.y * kHeavyBlocks + blockIdx.x), r);
    }
}
template <int FB>
__global__ void __launch_bounds__(64) msm_finish_heavy2(const u32 *__restrict__ scratch, u32 *__restrict__ buckets,
                                                        const u32 *__restrict__ heavy) {
    H2_LATENCY_STAGE();
    __shared__ __attribute__((aligned(16))) u32 sh[32 * 16];
    if (blockIdx.x >= min(heavy[1], kMaxHeavy)) return;
    // one wave = 16 quads: quad q adds partials q and q + 16, then a 4-level tree (5 dependent additions instead of 32)
    const u32 b = heavy[2 + blockIdx.x], q = threadIdx.x / kGroup;
    const bool lead = (threadIdx.x & (kGroup - 1)) == 0;
    const u32 *src = scratch + 32 * ((size_t)blockIdx.x * kHeavyBlocks);
    xyzz<FB> acc = xyzz_load<FB>(src + 32 * q);
    for (u32 i = q + 16; i < kHeavyBlocks; i += 16) {
        xyzz<FB> p = xyzz_load<FB>(src + 32 * i);
        xyzz_add_wide<FB>(acc, p);
    }
    r256_quads_sum<FB>(acc, sh, 16);
    if (q == 0) {
        xyzz<FB> r = xyzz_load<FB>(sh), own = xyzz_load<FB>(buckets + 32 * (size_t)b);
        xyzz_add_wide<FB>(r, own);
        if (lead) xyzz_store<FB>(buckets + 32 * (size_t)b, r);
    }
}

// total[b] += part[b] over one bucket slice (the ranges of a commit assembled from chunks share one fold): one quad per bucket
template <int FB>
__global__ void __launch_bounds__(256) msm_bucket_add(u32 *__restrict__ total, const u32 *__restrict__ part, u32 nb) {
    H2_LATENCY_STAGE();
    const u32 b = (blockIdx.x * blockDim.x + threadIdx.x) / kGroup;
    if (b >= nb) return;
    const xyzz<FB> p = xyzz_load<FB>(part + 32 * (size_t)b);
    if (fe_is_zero(p.zz)) return;                              // an empty bucket of this range
    xyzz<FB> acc = xyzz_load<FB>(total + 32 * (size_t)b);
    xyzz_add_wide<FB>(acc, p);
    if ((threadIdx.x & (kGroup - 1)) == 0) xyzz_store<FB>(total + 32 * (size_t)b, acc);
}

// ---- the first levels of the fold of a WIDE bucket slice (registered tables from 2^16 buckets), throughput form ----------------
// The quad-lane kernels below spend four lanes on a point operation to cut its latency; on the two stages that touch EVERY
// bucket -- finishing (bucket += heads) and the row / column sums -- that is 2.4x the VALU work of a one-lane addition on the
// carry-free layer, at 4096 waves, right when another stream's msm_accumulate wants the SIMDs.  These two stages therefore run
// one lane per point on the raw M9 segments msm_accumulate parks (no msm_segments_to_r256 pass), and only the S + NR row /
// column sums are converted for the latency-bound tail (msm_reduce_segments on a few hundred points).
template <int FB>
__global__ void __launch_bounds__(256) fold9_finish(const u32 *__restrict__ heads9, const u32 *__restrict__ starts, u32 *__restrict__ buckets9,
                                                    u32 *__restrict__ heavy, u32 total_buckets, u32 T, u32 div, ColStride cs) {
    fold9_stage(cs);
    const u32 b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= total_buckets) return;
    if (gridDim.z > 1) {
        heads9 = H2_COLZ(heads9, cs.heads);
        starts = H2_COLZ(starts, cs.starts);
        buckets9 = H2_COLZ(buckets9, cs.buckets);
        heavy = H2_COLZ(heavy, cs.heavy);
    }
    const HeadRange h = bucket_heads<true>(starts, b, total_buckets, T, div);      // (a slice group's view: see msm_accumulate)
    if (h.h1 <= h.h0) return;
    if (h.h1 - h.h0 > kHeavy && heavy_park<1>(heavy, b, true)) return;
    xyzz9<FB> acc = xyzz9_load_raw<FB>(buckets9 + 36 * (size_t)b);
    for (u32 t = h.h0; t < h.h1; ++t) xyzz9_add<FB>(acc, xyzz9_load_raw<FB>(heads9 + 36 * (size_t)t));
    xyzz9_store_raw<FB>(buckets9 + 36 * (size_t)b, acc);
}
template <int FB>
__global__ void __launch_bounds__(256, 3) fold9_finish_heavy(const u32 *__restrict__ heads9, const u32 *__restrict__ starts, u32 *__restrict__ scratch9,
                                                          const u32 *__restrict__ heavy, u32 total_buckets, u32 T, u32 div, ColStride cs) {
    fold9_stage(cs);
    __shared__ __attribute__((aligned(16))) u32 sh[32 * 36];
    if (gridDim.z > 1) {
        heavy = H2_COLZ(heavy, cs.heavy);
        heads9 = H2_COLZ(heads9, cs.heads);
        starts = H2_COLZ(starts, cs.starts);
        scratch9 = H2_COLZ(scratch9, cs.hscratch);
    }
    // gridDim.y = kHeavyRows workgroup rows walk the list of heavy buckets (round 5: the launch used to carry one row per POSSIBLE heavy
    // bucket -- 32 x 512 workgroups that found an empty list and left, ~12 us of dispatch per commit; a column has no heavy bucket
    // unless it is degenerate, and then a handful)
    const u32 count = min(heavy[1], kMaxHeavy);
    const HeadSplit hs = head_split<true>(starts, total_buckets, T, div);
    for (u32 slot = blockIdx.y; slot < count; slot += gridDim.y) {
        const HeadRange h = bucket_heads(hs, starts, heavy[2 + slot]);
        const u32 share = (h.h1 - h.h0 + kHeavyBlocks - 1) / kHeavyBlocks;
        const u32 lo = h.h0 + blockIdx.x * share, hi = min(h.h1, lo + share);
        xyzz9<FB> acc = fold9_quad_gather<FB, H2_FOLD_D>(heads9, hi > lo ? hi - lo : 0u, [lo](u32 k) { return lo + k; });
        acc = fold9_quads_sum<FB>(acc, sh);
        if (fold9_root() && (threadIdx.x & (kGroup - 1)) == 0) xyzz9_store_raw<FB>(scratch9 + 36 * ((size_t)slot * kHeavyBlocks + blockIdx.x), acc);
        __syncthreads();                                 // `sh` is reused by the next bucket's tree
    }
}
template <int FB>
__global__ void __launch_bounds__(64, 3) fold9_finish_heavy2(const u32 *__restrict__ scratch9, u32 *__restrict__ buckets9, const u32 *__restrict__ heavy,
                                                             ColStride cs) {
    fold9_stage(cs);
    __shared__ __attribute__((aligned(16))) u32 sh[8 * 36];
    if (gridDim.z > 1) {
        heavy = H2_COLZ(heavy, cs.heavy);
        scratch9 = H2_COLZ(scratch9, cs.hscratch);
        buckets9 = H2_COLZ(buckets9, cs.buckets);
    }
    const u32 count = min(heavy[1], kMaxHeavy);
    for (u32 slot = blockIdx.x; slot < count; slot += gridDim.x) {          // (kHeavyRows workgroups walk the list: see fold9_finish_heavy)
        // 16 quads: two partials each, a 4-level tree, then the bucket's own segment (6 dependent additions)
        const u32 b = heavy[2 + slot];
        const u32 *src = scratch9 + 36 * ((size_t)slot * kHeavyBlocks);
        xyzz9<FB> acc = fold9_quad_gather<FB, H2_FOLD_D>(src, kHeavyBlocks, [](u32 k) { return k; });
        acc = fold9_quads_sum<FB>(acc, sh);
        if (fold9_root()) {
            xyzz9_add_wide<FB>(acc, xyzz9_load_raw<FB>(buckets9 + 36 * (size_t)b));
            if ((threadIdx.x & (kGroup - 1)) == 0) xyzz9_store_raw<FB>(buckets9 + 36 * (size_t)b, acc);
        }
        __syncthreads();
    }
}
// row / column sums of the NR x S bucket matrix (see msm_rowcol_sums for the algebra): one workgroup of 64 quads per line,
// lines9[lo] = C_lo (lo < S), lines9[S + hi] = R_hi (1 <= hi < NR; row 0 carries weight 0 and is never formed), raw M9.
template <int FB>
__global__ void __launch_bounds__(256, 3) fold9_rowcol(const u32 *__restrict__ buckets9, u32 *__restrict__ lines9, u32 S, u32 NR, ColStride cs) {
    fold9_stage(cs);
    __shared__ __attribute__((aligned(16))) u32 sh[32 * 36];
    if (gridDim.z > 1) {
        buckets9 = H2_COLZ(buckets9, cs.buckets);
        lines9 = H2_COLZ(lines9, cs.lines);
    }
    const bool is_col = blockIdx.x < S;
    const u32 id = is_col ? blockIdx.x : blockIdx.x - S + 1;          // column lo, or row hi
    const u32 cnt = is_col ? NR : S;
    const u32 base = blockIdx.y * S * NR + (is_col ? id : id * S), step = is_col ? S : 1;      // blockIdx.y: the bucket slice (paired commits: 2)
    xyzz9<FB> acc = fold9_quad_gather<FB, H2_FOLD_D>(buckets9, cnt, [base, step](u32 k) { return base + k * step; });
    acc = fold9_quads_sum<FB>(acc, sh);
    if (fold9_root() && (threadIdx.x & (kGroup - 1)) == 0)
        xyzz9_store_raw<FB>(lines9 + 36 * ((size_t)blockIdx.y * (S + NR) + (is_col ? id : S + id)), acc);
}
// The rest of the fold of a wide slice in ONE launch.  sum_j (j + 1) B_j = sum_lo (lo + 1) C_lo + S sum_hi hi R_hi is a sum of
// `planes` = log2 S + log2 NR bit planes (msm_plan.h: which lines plane t holds).  Workgroup t sums plane t -- a tree over at most
// S / 2 + NR / 2 lines --, doubles the sum t times (the planes do that side by side: the top plane's t doublings are the chain
// nothing shortens, everything else hides behind it), and the workgroup that finishes LAST (fold9_plane_arrive) adds the 16 weighted
// planes with one more tree: ~8 + 15 + 5 dependent quad-lane operations, against the ~60 of a running sum over segments, a slice
// tree and a Horner step in three launches (reduce_segments + sum_slice + combine: 126 us of a 1.28 ms commit; this kernel: ~70).
template <int FB>
__global__ void __launch_bounds__(256, 3) fold9_planes(const u32 *__restrict__ lines9, u32 *__restrict__ planes9, u32 *__restrict__ counter, u32 S, u32 NR,
                                                    int cb, u32 *__restrict__ out, int out_kind, int out_mont, ColOut co, ColStride cs) {
    fold9_stage(cs);
    __shared__ __attribute__((aligned(16))) u32 sh[32 * 36];
    __shared__ u32 s_last;
    if (gridDim.z > 1) {
        lines9 = H2_COLZ(lines9, cs.lines);
        planes9 = H2_COLZ(planes9, cs.planes);
        counter = H2_COLZ(counter, cs.ctr);
        out = co.out[blockIdx.z];
    }
    const u32 t = blockIdx.x, planes = gridDim.x;
    lines9 += 36 * (size_t)blockIdx.y * (S + NR);                     // blockIdx.y: the bucket slice = the output (paired commits: 2)
    planes9 += 36 * (size_t)blockIdx.y * 32;
    counter += blockIdx.y;
    out += (out_kind == kOutSliceSum ? 32 : point_out_words(out_kind)) * (size_t)blockIdx.y;
    xyzz9<FB> acc = fold9_quad_gather<FB, H2_FOLD_D>(lines9, fold9_plane_cols(S, cb, t) + fold9_plane_rows(NR, cb, t),
                                                     [=](u32 k) { return fold9_plane_line(S, cb, t, k); });
    acc = fold9_quads_sum<FB>(acc, sh);
    if (!fold9_plane_arrive<FB>(acc, t, planes9, counter, planes, s_last)) return;
    // the workgroup that arrived last adds the weighted planes (a tree again)
    acc = fold9_quad_gather<FB, H2_FOLD_D>(planes9, planes, [](u32 k) { return k; });
    acc = fold9_quads_sum<FB>(acc, sh);
    if (!fold9_root()) return;
    const xyzz<FB> r = xyzz9_to_r256_wide<FB>(acc);
    if ((threadIdx.x & (kGroup - 1)) != 0) return;
    *counter = 0;
    if (out_kind == kOutSliceSum) {              // a window slice of a generic multiexp: XYZZ in the reference's form, for msm_combine
        xyzz_store<FB>(out, r);
        return;
    }
    point_out_store<FB>(out, r, out_kind, out_mont);
}

// The three tail kernels below run each logical lane as a quad of 4 hardware lanes (curve_wide.cuh): the chip
// is nearly idle here, so lanes are free and the dependent-multiply depth per point operation drops 3x.

// ---- reduce level 1: segment of kSeg buckets -> sum_j (j+1) * B_j restricted to the segment ------
template <int FB>
__global__ void __launch_bounds__(256) msm_reduce_segments(const u32 *__restrict__ buckets, u32 *__restrict__ partial,
                                                           u32 NB, u32 total_segments, int seg) {
    H2_LATENCY_STAGE();
    const u32 t = (blockIdx.x * blockDim.x + threadIdx.x) / kGroup;
    if (t >= total_segments) return;
    u32 segs_per_slice = NB / seg;
    u32 sl = t / segs_per_slice, sg = t % segs_per_slice;
    const u32 *base = buckets + 32 * ((size_t)sl * NB + (size_t)sg * seg);
    xyzz<FB> run = xyzz_identity<FB>(), acc = xyzz_identity<FB>();
    for (int j = seg - 1; j >= 0; --j) {
        xyzz<FB> bk = xyzz_load<FB>(base + 32 * j);
        xyzz_add_wide<FB>(run, bk);
        xyzz_add_wide<FB>(acc, run);
    }
    // buckets of this segment carry weights sg*seg + (j+1): add (sg*seg) * run
    xyzz<FB> sh = xyzz_mul_small_wide<FB>(run, sg * seg);
    xyzz_add_wide<FB>(acc, sh);
    if ((threadIdx.x & (kGroup - 1)) == 0) xyzz_store<FB>(partial + 32 * (size_t)t, acc);
}

// ---- reduce level 2: tree sum of a slice's partials, in two launches (many workgroups, then one per slice) --------
// grid (blocks_per_slice, slices); block j of slice s sums partial[s][j * share .. (j + 1) * share) into out[s][j]
template <int FB>
__global__ void __launch_bounds__(256) msm_sum_slice(const u32 *__restrict__ partial, u32 *__restrict__ out, u32 per_slice,
                                                     u32 share) {
    H2_LATENCY_STAGE();
    extern __shared__ __attribute__((aligned(16))) u32 sh[];
    const u32 sl = blockIdx.y, blk = blockIdx.x;
    const u32 lo = blk * share, hi = min(per_slice, lo + share);
    const xyzz<FB> acc = r256_quad_gather<FB>(partial + 32 * (size_t)sl * per_slice, hi > lo ? hi - lo : 0u, [lo](u32 k) { return lo + k; });
    r256_quads_sum<FB>(acc, sh, blockDim.x / kGroup);
    if (threadIdx.x == 0) {
        xyzz<FB> r = xyzz_load<FB>(sh);
        xyzz_store<FB>(out + 32 * ((size_t)sl * gridDim.x + blk), r);
    }
}

// ---- wide bucket slices (NB > 2^15, registered path with c > 16): sum_j (j + 1) B_j with j = hi * S + lo splits into
//      S * sum_hi hi * R_hi + sum_lo (lo + 1) * C_lo   (R = row sums, C = column sums of the NR x S bucket matrix),
// i.e. ~one add per bucket, all of them independent (a tree per row / column) instead of a running sum plus a
// small-scalar multiple per 8-bucket segment.  Output laid out as two slices of NR points for the ordinary reduce:
// slice 0 = C_0 .. C_{S-1} (then identities), slice 1 = R_1 .. R_{NR-1} (then one identity); msm_combine's Horner
// step with "window width" log2 S then forms S * (slice 1) + (slice 0).
template <int FB>
__global__ void __launch_bounds__(256) msm_rowcol_sums(const u32 *__restrict__ buckets, u32 *__restrict__ wide, u32 S, u32 NR) {
    H2_LATENCY_STAGE();
    extern __shared__ __attribute__((aligned(16))) u32 sh[];
    const bool is_col = blockIdx.x < S;
    const u32 id = is_col ? blockIdx.x : blockIdx.x - S + 1;          // column lo, or row hi (row 0 carries weight 0)
    const size_t base = is_col ? id : (size_t)id * S, step = is_col ? S : 1;
    const xyzz<FB> acc = r256_quad_gather<FB>(buckets, is_col ? NR : S, [base, step](u32 k) { return base + (size_t)k * step; });
    r256_quads_sum<FB>(acc, sh, blockDim.x / kGroup);
    if (threadIdx.x == 0) {
        xyzz<FB> r = xyzz_load<FB>(sh);
        xyzz_store<FB>(wide + 32 * (is_col ? (size_t)id : (size_t)NR + id - 1), r);
    }
}

// ---- combine: Horner over slices (windows), emit Jacobian / affine; one quad of lanes ---------------
// extra_dbl / addend / out_kind == kOutSliceSum serve the slice split of a large generic multiexp (msm_launch): the UPPER group of
// slices is summed by Horner, doubled extra_dbl = c x (slices below it) more times and left as XYZZ (32 words); the lower group's
// call then adds that point (`addend`) to its own Horner sum and emits the result.  addend_first (the grouped form, msm_generic.hip): the
// addend -- the chain of the groups above, already doubled down to the weight of this group's LOWEST slice -- is added BEFORE the extra
// doublings that carry the sum on to the next group: A_g = R_g + D_(g-1), D_g = 2^(extra) A_g.
template <int FB>
__global__ void __launch_bounds__(64) msm_combine(const u32 *__restrict__ slice_sums, int slices, int c, u32 *__restrict__ out,
                                                  int out_kind, int out_mont, int extra_dbl, const u32 *__restrict__ addend, int addend_first) {
    H2_LATENCY_STAGE();
    if (threadIdx.x >= kGroup) return;
    // one block: Horner over the slices.  Several blocks (pair commits): block b emits slice b alone as output b.
    if (gridDim.x > 1) {
        slice_sums += 32 * (size_t)blockIdx.x;
        out += point_out_words(out_kind) * (size_t)blockIdx.x;
        slices = 1;
    }
    // the chain runs on the carry-free layer (curve9_wide.cuh): ~850 instructions per doubling against ~1300, and the 128-130
    // doublings of a generic multiexp's Horner step ARE this kernel (355 us of a 0.6-0.7 ms small multiexp before)
    xyzz9<FB> r9 = xyzz9_identity<FB>();
    for (int w = slices - 1; w >= 0; --w) {
        if (w != slices - 1)
            for (int k = 0; k < c; ++k) r9 = xyzz9_dbl_wide<FB>(r9);
        const xyzz9<FB> s9 = xyzz9_from_r256_wide<FB>(xyzz_load<FB>(slice_sums + 32 * (size_t)w));
        xyzz9_add_wide<FB>(r9, s9);
    }
    if (addend && addend_first) xyzz9_add_wide<FB>(r9, xyzz9_from_r256_wide<FB>(xyzz_load<FB>(addend)));
    for (int k = 0; k < extra_dbl; ++k) r9 = xyzz9_dbl_wide<FB>(r9);
    if (addend && !addend_first) xyzz9_add_wide<FB>(r9, xyzz9_from_r256_wide<FB>(xyzz_load<FB>(addend)));
    const xyzz<FB> r = xyzz9_to_r256_wide<FB>(r9);
    if (threadIdx.x != 0) return;
    if (out_kind == kOutSliceSum) {
        xyzz_store<FB>(out, r);
        return;
    }
    point_out_store<FB>(out, r, out_kind, out_mont);
}

template <int FB>
__global__ void __launch_bounds__(64) msm_combine_ranges(RangeSums rs, int ranges, int slices, int c, u32 *__restrict__ out, int out_kind, int out_mont) {
    H2_LATENCY_STAGE();
    __shared__ __attribute__((aligned(16))) u32 sh[16 * 36];
    const int w = threadIdx.x / kGroup;
    const bool lead = (threadIdx.x & (kGroup - 1)) == 0;
    if (w < slices) {
        xyzz9<FB> acc = xyzz9_identity<FB>();
        for (int q = 0; q < ranges; ++q) xyzz9_add_wide<FB>(acc, xyzz9_from_r256_wide<FB>(xyzz_load<FB>(rs.p[q] + 32 * (size_t)w)));
        if (lead) xyzz9_store_raw<FB>(sh + 36 * w, acc);
    }
    __syncthreads();
    if (threadIdx.x >= kGroup) return;
    xyzz9<FB> r9 = xyzz9_identity<FB>();
    for (int s = slices - 1; s >= 0; --s) {
        if (s != slices - 1)
            for (int k = 0; k < c; ++k) r9 = xyzz9_dbl_wide<FB>(r9);
        xyzz9_add_wide<FB>(r9, xyzz9_load_raw<FB>(sh + 36 * s));
    }
    const xyzz<FB> r = xyzz9_to_r256_wide<FB>(r9);
    if (threadIdx.x == 0) point_out_store<FB>(out, r, out_kind, out_mont);
}

// ---- host: every launch of the kernels above (declared in msm_internal.cuh) -------------------------------------------------------------------
// H2_FOLD_FB(fb, f, args...): f<FP>(args...) or f<FQ>(args...)
#define H2_FOLD_FB(fb, f, ...) ((fb) == FP ? f<FP>(__VA_ARGS__) : f<FQ>(__VA_ARGS__))

// the five launches of the carry-free fold
template <int FB> static void fold9_group_launch(hipStream_t st, const Fold9Group &g) {
    const ColStride &cs = g.cs;
    const u32 fz = cs.joined ? 1 : g.cols, ftb = cs.joined ? g.cols * g.tb : g.tb;       // joined columns: one pass over the cols x tb buckets
    const u32 S = g.wideS, NR = g.wideNR;
    u32 *lines = g.lines9 + 36 * (size_t)g.slice0 * (S + NR);
    hipLaunchKernelGGL((fold9_finish<FB>), dim3((ftb + 255) / 256, 1, fz), dim3(256), 0, st, g.heads9, g.starts, g.buckets9, g.heavy, ftb, g.T, g.lane_div, cs);
    hipLaunchKernelGGL((fold9_finish_heavy<FB>), dim3(kHeavyBlocks, kHeavyRows, fz), dim3(256), 0, st, g.heads9, g.starts, g.hscratch, (const u32 *)g.heavy, ftb, g.T, g.lane_div, cs);
    hipLaunchKernelGGL((fold9_finish_heavy2<FB>), dim3(kHeavyRows, 1, fz), dim3(64), 0, st, (const u32 *)g.hscratch, g.buckets9, (const u32 *)g.heavy, cs);
    // line sums, then the bit planes of the line weights and their combination in one launch (fold9_planes)
    hipLaunchKernelGGL((fold9_rowcol<FB>), dim3(S + NR - 1, g.nslices, g.cols), dim3(256), 0, st, (const u32 *)g.buckets9, lines, S, NR, cs);
    hipLaunchKernelGGL((fold9_planes<FB>), dim3(fold9_plane_count(g.c), g.nslices, g.cols), dim3(256), 0, st, (const u32 *)lines, g.planes9 + 36 * (size_t)g.slice0 * 32, g.ctr + g.slice0, S, NR,
                       fold9_col_bits(S), g.out + 32 * (size_t)g.slice0, g.out_kind, g.out_mont ? 1 : 0, g.co, cs);
}
void fold9_group(int fb, hipStream_t st, const Fold9Group &g) { H2_FOLD_FB(fb, fold9_group_launch, st, g); }

template <int FB> static void combine_launch(hipStream_t st, size_t lds, u32 outputs, const u32 *slice_sums, int slices, int c, u32 *out, int out_kind, bool out_mont,
                                             int extra_dbl, const u32 *addend, bool addend_first) {
    hipLaunchKernelGGL((msm_combine<FB>), dim3(outputs), dim3(64), lds, st, slice_sums, slices, c, out, out_kind, out_mont ? 1 : 0, extra_dbl, addend, addend_first ? 1 : 0);
}
void msm_combine_launch(int fb, hipStream_t st, size_t lds, u32 outputs, const u32 *slice_sums, int slices, int c, u32 *out, int out_kind, bool out_mont,
                        int extra_dbl, const u32 *addend, bool addend_first) {
    H2_FOLD_FB(fb, combine_launch, st, lds, outputs, slice_sums, slices, c, out, out_kind, out_mont, extra_dbl, addend, addend_first);
}
int msm_combine_allow_lds(size_t bytes) {
    H2_HIP(hipFuncSetAttribute((const void *)msm_combine<FP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    H2_HIP(hipFuncSetAttribute((const void *)msm_combine<FQ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return H2_OK;
}
template <int FB> static void combine_ranges_launch(hipStream_t st, const RangeSums &rs, int ranges, int slices, int c, u32 *out, int out_kind, bool out_mont) {
    hipLaunchKernelGGL((msm_combine_ranges<FB>), dim3(1), dim3(64), 0, st, rs, ranges, slices, c, out, out_kind, out_mont ? 1 : 0);
}
void msm_combine_ranges_launch(int fb, hipStream_t st, const RangeSums &rs, int ranges, int slices, int c, u32 *out, int out_kind, bool out_mont) {
    H2_FOLD_FB(fb, combine_ranges_launch, st, rs, ranges, slices, c, out, out_kind, out_mont);
}
template <int FB> static void bucket_add_launch(hipStream_t st, u32 *total, const u32 *part, u32 nb) {
    hipLaunchKernelGGL((msm_bucket_add<FB>), dim3((nb * kGroup + 255) / 256), dim3(256), 0, st, total, part, nb);
}
void msm_bucket_add_launch(int fb, hipStream_t st, u32 *total, const u32 *part, u32 nb) { H2_FOLD_FB(fb, bucket_add_launch, st, total, part, nb); }

// the 8 x 32 finisher and fold (the geometry: r256_fold_geometry, msm_plan.h)
template <int FB> static int fold_r256_launch(MsmContext &cx, const MsmPlan &p, const MsmArgs &a, hipStream_t st) {
    const u32 tb = p.tb, T = p.T;
    const size_t tree_lds = r256_tree_bytes(kTreeLanes);
    if (!p.fold_only) {
        hipLaunchKernelGGL((msm_finish_buckets<FB>), dim3((tb * kGroup + 255) / 256), dim3(256), 0, st, cx.heads.as<u32>(),
                           cx.starts.as<u32>(), cx.buckets.as<u32>(), cx.heavy.as<u32>(), tb, T, p.lane_div);
        hipLaunchKernelGGL((msm_finish_heavy<FB>), dim3(kHeavyBlocks, kMaxHeavy), dim3(kTreeLanes), tree_lds, st,
                           cx.heads.as<u32>(), cx.starts.as<u32>(), cx.hscratch.as<u32>(), cx.heavy.as<u32>(), tb, T, p.lane_div);
        hipLaunchKernelGGL((msm_finish_heavy2<FB>), dim3(kMaxHeavy), dim3(64), 0, st, cx.hscratch.as<u32>(), cx.buckets.as<u32>(), cx.heavy.as<u32>());
    }
    if (p.add_only) {
        bucket_add_launch<FB>(st, a.add_into, cx.buckets.as<u32>(), tb);
        return H2_OK;
    }
    // what the fold runs over: the bucket slices themselves, or (wide slices) the row / column sums as two slices
    const R256Fold f = r256_fold_geometry(p.sh, p.wide_reduce, p.wideNR);
    const u32 *fold_src = p.fold_only ? a.fold_from : cx.buckets.as<u32>();
    if (p.wide_reduce) {
        u32 *wide = cx.partial.as<u32>() + 32 * (size_t)(2 * p.wideNR / kSeg);     // after the fold's own partials
        H2_HIP(hipMemsetAsync(wide, 0, (size_t)2 * p.wideNR * 128, st));
        hipLaunchKernelGGL((msm_rowcol_sums<FB>), dim3(p.wideS + p.wideNR - 1), dim3(kTreeLanes), tree_lds, st, fold_src, wide, p.wideS, p.wideNR);
        fold_src = wide;
    }
    hipLaunchKernelGGL((msm_reduce_segments<FB>), dim3((f.segs * kGroup + 255) / 256), dim3(256), 0, st, fold_src, cx.partial.as<u32>(), f.nb, f.segs, f.seg);
    for (int l = 0; l < f.levels; ++l) {      // partials -> (heads[], free again: the first level's output ->) slice sums
        const R256Fold::Level &v = f.level[l];
        hipLaunchKernelGGL((msm_sum_slice<FB>), dim3(v.blocks, f.slices), dim3(kTreeLanes), tree_lds, st, l ? cx.heads.as<u32>() : cx.partial.as<u32>(),
                           l == f.levels - 1 ? cx.ssums.as<u32>() : cx.heads.as<u32>(), v.per_slice, v.share);
    }
    combine_launch<FB>(st, 0, p.pair ? 2 : 1, cx.ssums.as<u32>(), (int)f.slices, f.c, (u32 *)a.d_out, a.out_kind, a.form == H2_FORM_MONTGOMERY, 0, nullptr, false);
    return H2_OK;
}
int fold_r256(int fb, MsmContext &cx, const MsmPlan &p, const MsmArgs &a, hipStream_t st) { return H2_FOLD_FB(fb, fold_r256_launch, cx, p, a, st); }

}  // namespace h2
