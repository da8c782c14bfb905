// The chain of a fixed-base multiplication over its window table, on one lane; shared by the fixed-base kernels (ecc_fixed.hip) and the
// Sinsemilla commitment (sinsemilla_commit.hip).  Everything is internal to the including unit.
#pragma once
#include "curve.cuh"

namespace h2 {
namespace {

// the low 3 bits of a 256-bit word, which then moves down by 3
__device__ __forceinline__ u32 take_window(u32 (&k)[8]) {
    const u32 d = k[0] & 7u;
#pragma unroll
    for (int j = 0; j < 7; j++) k[j] = (k[j] >> 3) | (k[j + 1] << 29);
    k[7] >>= 3;
    return d;
}

__device__ __forceinline__ void load_scalar(const u32 *scalars, size_t i, u32 (&k)[8]) {
    const fe s = fe_load(scalars + 8 * i);
#pragma unroll
    for (int j = 0; j < 8; j++) k[j] = s.v[j];
}

__device__ __forceinline__ xyzz<FP> xyzz_of(const affine<FP> &p) { return xyzz<FP>{p.x, p.y, fe_one<FP>(), fe_one<FP>()}; }

// acc += q, incomplete (madd-2008-s without its exceptional branches): see the head of ecc_fixed.hip for why the operands never meet
__device__ __forceinline__ void xyzz_madd_incomplete(xyzz<FP> &acc, const affine<FP> &q) {
    const fe p = fe_sub<FP>(fe_mulx<FP>(q.x, acc.zz), acc.x);
    const fe r = fe_sub<FP>(fe_mulx<FP>(q.y, acc.zzz), acc.y);
    const fe pp = fe_sqr<FP>(p), ppp = fe_mulx<FP>(p, pp);
    const fe qq = fe_mulx<FP>(acc.x, pp);
    const fe x3 = fe_sub<FP>(fe_sub<FP>(fe_sub<FP>(fe_sqr<FP>(r), ppp), qq), qq);
    acc.y = fe_sub<FP>(fe_mulx<FP>(r, fe_sub<FP>(qq, x3)), fe_mulx<FP>(acc.y, ppp));
    acc.x = x3;
    acc.zz = fe_mulx<FP>(acc.zz, pp);
    acc.zzz = fe_mulx<FP>(acc.zzz, ppp);
}

__device__ __forceinline__ const u32 *table_entry(const u32 *table, u32 w, u32 k, u32 limbs) { return table + limbs * (8 * w + k); }

// [k]B over B's table of nw windows, which consumes k: window 0's point, the incomplete additions of windows 1 .. nw-2, and the last
// window's, complete (the head of ecc_fixed.hip)
__device__ __forceinline__ xyzz<FP> fixed_base_chain(const u32 *points, u32 nw, u32 (&k)[8]) {
    xyzz<FP> acc = xyzz_of(aff_load<FP>(table_entry(points, 0, take_window(k), 16)));
#pragma unroll 1
    for (u32 w = 1; w + 1 < nw; w++) xyzz_madd_incomplete(acc, aff_load<FP>(table_entry(points, w, take_window(k), 16)));
    xyzz_madd<FP>(acc, aff_load<FP>(table_entry(points, nw - 1, take_window(k), 16)));
    return acc;
}

}  // namespace
}  // namespace h2
