// The opening argument's device code: the generator collapse, the folds, the round scalars over the original generators, the round
// loop's three launches and the constant-coefficient corrections.  Templates on the field (FP = 0, FQ = 1); ipa.hip alone includes
// this file and launches what is in it.
#pragma once
#include "curve_wide.cuh"
#include "glv.cuh"

namespace h2 {

// naf1 / naf2: signed digits in {-1, 0, 1} of k1 and k2 (signs folded in), little-endian, uniform across lanes;
// g[i] <- g[i] + [k1] g[half + i] + [k2] phi(g[half + i])
template <int FB>
__global__ void __launch_bounds__(256) ipa_collapse(u32 *__restrict__ g, u32 half, const int8_t *__restrict__ naf1,
                                                    const int8_t *__restrict__ naf2, int top) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= half) return;
    const affine<FB> hi = aff_load<FB>(g + 16 * (size_t)(half + i));
    const fe neg_y = fe_neg<FB>(hi.y);
    const fe phi_x = fe_mulx<FB>(hi.x, glv_zeta<FB>());
    xyzz<FB> acc = xyzz_identity<FB>();
    for (int b = top; b >= 0; --b) {           // uniform control flow: every lane walks the same digits
        acc = xyzz_dbl<FB>(acc);
        const int d1 = naf1[b], d2 = naf2[b];
        if (d1) xyzz_madd<FB>(acc, affine<FB>{hi.x, d1 > 0 ? hi.y : neg_y});
        if (d2) xyzz_madd<FB>(acc, affine<FB>{phi_x, d2 > 0 ? hi.y : neg_y});
    }
    const affine<FB> lo = aff_load<FB>(g + 16 * (size_t)i);
    xyzz_madd<FB>(acc, lo);
    const affine<FB> r = xyzz_to_affine<FB>(acc);
    fe_store(g + 16 * (size_t)i, r.x);
    fe_store(g + 16 * (size_t)i + 8, r.y);
}

// the same walk with one point per quad of lanes: the last rounds of an argument have a handful of points and are
// bound by the ~220 sequential point operations, which the quad runs at 3-4 multiplication levels each
template <int FB>
__global__ void __launch_bounds__(256) ipa_collapse_wide(u32 *__restrict__ g, u32 half, const int8_t *__restrict__ naf1,
                                                         const int8_t *__restrict__ naf2, int top) {
    const u32 i = (blockIdx.x * blockDim.x + threadIdx.x) / kGroup;
    if (i >= half) return;
    const affine<FB> hi = aff_load<FB>(g + 16 * (size_t)(half + i));
    const fe one = fe_one<FB>();
    const fe neg_y = fe_neg<FB>(hi.y);
    const fe phi_x = fe_mulx<FB>(hi.x, glv_zeta<FB>());
    xyzz<FB> acc = xyzz_identity<FB>();
    const bool hi_id = fe_is_zero(hi.x) && fe_is_zero(hi.y);      // the identity as an affine operand: nothing to add
    for (int b = top; b >= 0 && !hi_id; --b) {
        acc = xyzz_dbl_wide<FB>(acc);
        const int d1 = naf1[b], d2 = naf2[b];
        if (d1) xyzz_add_wide<FB>(acc, xyzz<FB>{hi.x, d1 > 0 ? hi.y : neg_y, one, one});
        if (d2) xyzz_add_wide<FB>(acc, xyzz<FB>{phi_x, d2 > 0 ? hi.y : neg_y, one, one});
    }
    const affine<FB> lo = aff_load<FB>(g + 16 * (size_t)i);
    if (!(fe_is_zero(lo.x) && fe_is_zero(lo.y))) xyzz_add_wide<FB>(acc, xyzz<FB>{lo.x, lo.y, one, one});
    if ((threadIdx.x & (kGroup - 1)) != 0) return;
    const affine<FB> r = xyzz_to_affine<FB>(acc);
    fe_store(g + 16 * (size_t)i, r.x);
    fe_store(g + 16 * (size_t)i + 8, r.y);
}

template <int F>
__global__ void __launch_bounds__(256) ipa_fold(u32 *__restrict__ a, u32 half, fe factor) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= half) return;
    fe lo = fe_load(a + 8 * (size_t)i), hi = fe_load(a + 8 * (size_t)(half + i));
    fe_store(a + 8 * (size_t)i, fe_add<F>(lo, fe_mulx<F>(hi, factor)));
}

template <int F> __global__ void __launch_bounds__(256) ipa_to_mont(u32 *a, size_t n, int to) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe v = fe_load(a + 8 * i);
    fe_store(a + 8 * i, to ? fe_to_mont<F>(v) : fe_from_mont<F>(v));
}

// ---- L_j / R_j over the ORIGINAL generators (h2_ipa_round_scalars_device) ----
// s_j(h) = prod_{r < j} u_r^{bit_{j-1-r}(h)}: round r's collapse pairs index bit k-1-r, which is bit j-1-r of h = m >> (k-j).
// (verifier.rs:156-172 compute_s builds the same products for the verifier.)  One lane per h, <= j multiplications.
template <int F>
__global__ void __launch_bounds__(256) ipa_s_table(u32 *__restrict__ s, const u32 *__restrict__ u_mont, u32 j) {
    const u32 h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >> j) return;
    fe acc = fe_one<F>();
    for (u32 r = 0; r < j; ++r)
        if ((h >> (j - 1 - r)) & 1) acc = fe_mulx<F>(acc, fe_load(u_mont + 8 * r));
    fe_store(s + 8 * (size_t)h, acc);
}

// cl[m] = p'[half + i] s_j(h) for i < half (else 0); cr[m] = p'[i - half] s_j(h) for i >= half (else 0); m = h 2^(k-j) + i.
// s is Montgomery, so the products keep whatever form p' is in.
template <int F>
__global__ void __launch_bounds__(256) ipa_round_scalars(const u32 *__restrict__ p, const u32 *__restrict__ s, u32 k, u32 j,
                                                         u32 *__restrict__ cl, u32 *__restrict__ cr) {
    const u32 m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >> k) return;
    const u32 blk = k - j, half = 1u << (blk - 1);
    const u32 h = m >> blk, i = m & ((1u << blk) - 1);
    const fe v = fe_mulx<F>(fe_load(p + 8 * (size_t)(i ^ half)), fe_load(s + 8 * (size_t)h));
    const bool lo = i < half;
    if (cl == cr) {        // merged column for a pair commit (h2_commit_pair_device): L_j and R_j have disjoint supports
        fe_store(cl + 8 * (size_t)m, v);
        return;
    }
    fe_store(cl + 8 * (size_t)m, lo ? v : fe_zero());
    fe_store(cr + 8 * (size_t)m, lo ? fe_zero() : v);
}

// ---- the round loop's own launches (h2_ipa_rounds_device): three per round beside the commit -----------------------------------
// A round used to enqueue ten small launches and a copy around its commit (two inner products of two launches each, the challenge
// upload, the s table, the round scalars, the tails, two folds); the rounds after the switch to the collapsed generators are chains
// of short launches, so each one costs as much as the work it carries.
static constexpr u32 kIpBlocks = 128;       // partial sums per inner product
template <int F> __device__ __forceinline__ fe ipa_block_sum(u32 *sh, fe v) {       // 256 lanes; the sum lands in every lane of wave 0's lane 0
    fe_store(sh + 8 * threadIdx.x, v);
    __syncthreads();
    for (u32 off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) fe_store(sh + 8 * threadIdx.x, fe_add<F>(fe_load(sh + 8 * threadIdx.x), fe_load(sh + 8 * (threadIdx.x + off))));
        __syncthreads();
    }
    return fe_load(sh);
}
// blocks [0, 2 kIpBlocks): partial sums of <p'_hi, b_lo> (first kIpBlocks) and <p'_lo, b_hi>, raw Montgomery products;
// the blocks after them: the round's scalars over the original generators (ipa_round_scalars' body; s = this round's table)
template <int F>
__global__ void __launch_bounds__(256) ipa_round_prep(const u32 *__restrict__ p, const u32 *__restrict__ b, const u32 *__restrict__ s, u32 k, u32 j,
                                                      u32 *__restrict__ partial, u32 *__restrict__ cl, u32 *__restrict__ cr) {
    __shared__ __attribute__((aligned(16))) u32 sh[256 * 8];
    const u32 blk = k - j, half = 1u << (blk - 1);
    if (blockIdx.x < 2 * kIpBlocks) {
        const u32 which = blockIdx.x / kIpBlocks, bi = blockIdx.x % kIpBlocks;
        const u32 *pa = p + (which ? 0 : 8 * (size_t)half), *pb = b + (which ? 8 * (size_t)half : 0);
        fe acc = fe_zero();
        for (u32 i = bi * 256 + threadIdx.x; i < half; i += kIpBlocks * 256)
            acc = fe_add<F>(acc, fe_mulx<F>(fe_load(pa + 8 * (size_t)i), fe_load(pb + 8 * (size_t)i)));
        acc = ipa_block_sum<F>(sh, acc);
        if (threadIdx.x == 0) fe_store(partial + 8 * (size_t)blockIdx.x, acc);
        return;
    }
    const u32 m = (blockIdx.x - 2 * kIpBlocks) * 256 + threadIdx.x;
    if (m >> k) return;
    const u32 h = m >> blk, i = m & ((1u << blk) - 1);
    const fe v = fe_mulx<F>(fe_load(p + 8 * (size_t)(i ^ half)), fe_load(s + 8 * (size_t)h));
    if (cl == cr) {
        fe_store(cl + 8 * (size_t)m, v);
        return;
    }
    const bool lo = i < half;
    fe_store(cl + 8 * (size_t)m, lo ? v : fe_zero());
    fe_store(cr + 8 * (size_t)m, lo ? fe_zero() : v);
}
// one workgroup: the two inner products from their partial sums, then the rows behind the generators' (ipa_round_tails)
template <int F>
__global__ void __launch_bounds__(256) ipa_round_finish(const u32 *__restrict__ partial, fe z, fe l_rand, fe r_rand, u32 *__restrict__ vl,
                                                        u32 *__restrict__ vr, u32 *__restrict__ bl, u32 *__restrict__ br) {
    __shared__ __attribute__((aligned(16))) u32 sh[256 * 8];
    // lanes 0..127 carry the first product's partial sums, 128..255 the second's: one tree, stopped one level early
    fe_store(sh + 8 * threadIdx.x, fe_load(partial + 8 * (size_t)threadIdx.x));
    __syncthreads();
    for (u32 off = 64; off > 0; off >>= 1) {
        const u32 g = threadIdx.x >> 7, l = threadIdx.x & 127;
        if (l < off) fe_store(sh + 8 * threadIdx.x, fe_add<F>(fe_load(sh + 8 * threadIdx.x), fe_load(sh + 8 * (g * 128 + l + off))));
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        fe_store(vl, fe_mulx<F>(fe_load(sh), z));
        fe_store(bl, l_rand);
    } else if (threadIdx.x == 128) {
        fe_store(vr, fe_mulx<F>(fe_load(sh + 8 * 128), z));
        fe_store(br, r_rand);
    }
}
// blocks [0, fold_blocks): p'[i] += p'[i + half] u^-1 and b[i] += b[i + half] u (prover.rs:128-133); the blocks after them: the next
// round's s table, s_{j+1}(h) = s_j(h >> 1) * u^{h & 1} (the definition at ipa_s_table), from one buffer into the other
template <int F>
__global__ void __launch_bounds__(256) ipa_round_fold(u32 *__restrict__ p, u32 *__restrict__ b, u32 half, u32 fold_blocks, fe u_inv, fe u,
                                                      const u32 *__restrict__ s_old, u32 *__restrict__ s_new, u32 s_count) {
    if (blockIdx.x < fold_blocks) {
        const u32 i = blockIdx.x * 256 + threadIdx.x;
        if (i >= half) return;
        fe_store(p + 8 * (size_t)i, fe_add<F>(fe_load(p + 8 * (size_t)i), fe_mulx<F>(fe_load(p + 8 * (size_t)(half + i)), u_inv)));
        fe_store(b + 8 * (size_t)i, fe_add<F>(fe_load(b + 8 * (size_t)i), fe_mulx<F>(fe_load(b + 8 * (size_t)(half + i)), u)));
        return;
    }
    const u32 h = (blockIdx.x - fold_blocks) * 256 + threadIdx.x;
    if (h >= s_count) return;
    const fe v = fe_load(s_old + 8 * (size_t)(h >> 1));
    fe_store(s_new + 8 * (size_t)h, (h & 1) ? fe_mulx<F>(v, u) : v);
}

// a[0] -= *v: the constant coefficient of s_poly / p' after their evaluation at x_3 (prover.rs:51, :72), without a host round trip
template <int F> __global__ void __launch_bounds__(64) ipa_sub_at0(u32 *__restrict__ a, const u32 *__restrict__ v) {
    if (blockIdx.x == 0 && threadIdx.x == 0) fe_store(a, fe_sub<F>(fe_load(a), fe_load(v)));
}

// s[0] -= ev[0] + xp1 ev[1] + xp2 ev[2] + xp3 ev[3]: the evaluation of s_poly at x_3 from the evaluations of its four quarters (each a polynomial in the
// quarter's own index; xp_r = x_3^(r n / 4)), subtracted from the constant coefficient (prover.rs:49-51) -- one lane
template <int F> __global__ void __launch_bounds__(64) ipa_fix_s0(u32 *__restrict__ s0, const u32 *__restrict__ ev, fe xp1, fe xp2, fe xp3) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    fe t = fe_load(ev);
    t = fe_add<F>(t, fe_mulx<F>(fe_load(ev + 8), xp1));
    t = fe_add<F>(t, fe_mulx<F>(fe_load(ev + 16), xp2));
    t = fe_add<F>(t, fe_mulx<F>(fe_load(ev + 24), xp3));
    fe_store(s0, fe_sub<F>(fe_load(s0), t));
}

}  // namespace h2
