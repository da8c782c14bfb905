// The Sinsemilla round and what starts and feeds a chain, on one lane; shared by the hash and trace kernels (sinsemilla.hip) and the
// commitment, private-init and their trace kernels (sinsemilla_commit.hip).  Everything is internal to the including unit.
#pragma once
#include "curve.cuh"

namespace h2 {
namespace {

constexpr unsigned kK = 10, kC = 253, kWordMask = (1u << kK) - 1, kMaxPieceWords = 25;
constexpr u32 kTableBytes = 64u << kK;                   // 1024 affine points

struct PieceWords {                                        // the piece structure of a trace, by value in the kernel arguments
    uint8_t n[kC];
};

// One round on the accumulator; p and d are the two differences that incomplete addition must not see vanish (the head
// of sinsemilla.hip), zz_r is R's ZZ.  No branch: a vanishing difference leaves ZZ = 0 behind, which the caller reports.
__device__ __forceinline__ void sinsemilla_round(xyzz<FP> &a, const affine<FP> &s, fe &p, fe &r, fe &d, fe &zz_r) {
    p = fe_sub<FP>(fe_mulx<FP>(s.x, a.zz), a.x);
    r = fe_sub<FP>(fe_mulx<FP>(s.y, a.zzz), a.y);
    const fe pp = fe_sqr<FP>(p), ppp = fe_mulx<FP>(p, pp);
    const fe xa = fe_mulx<FP>(a.x, pp), ya = fe_mulx<FP>(a.y, ppp);                       // Acc over R's denominators
    const fe xr = fe_sub<FP>(fe_sub<FP>(fe_sub<FP>(fe_sqr<FP>(r), ppp), xa), xa);
    const fe yr = fe_sub<FP>(fe_mulx<FP>(r, fe_sub<FP>(xa, xr)), ya);
    zz_r = fe_mulx<FP>(a.zz, pp);
    const fe zzz_r = fe_mulx<FP>(a.zzz, ppp);
    d = fe_sub<FP>(xa, xr);
    const fe e = fe_sub<FP>(ya, yr);
    const fe dd = fe_sqr<FP>(d), ddd = fe_mulx<FP>(d, dd);
    const fe q = fe_mulx<FP>(xr, dd);
    a.x = fe_sub<FP>(fe_sub<FP>(fe_sub<FP>(fe_sqr<FP>(e), ddd), q), q);
    a.y = fe_sub<FP>(fe_mulx<FP>(e, fe_sub<FP>(q, a.x)), fe_mulx<FP>(yr, ddd));
    a.zz = fe_mulx<FP>(zz_r, dd);
    a.zzz = fe_mulx<FP>(zzz_r, ddd);
}

struct PointArg {                                          // Q, Montgomery affine, by value
    u32 x[8], y[8];
};
__device__ __forceinline__ xyzz<FP> start_at(const PointArg &q, bool &bottom) {
    xyzz<FP> a;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        a.x.v[i] = q.x[i];
        a.y.v[i] = q.y[i];
    }
    a.zz = fe_one<FP>();
    a.zzz = fe_one<FP>();
    bottom = fe_is_zero(a.x) && fe_is_zero(a.y);           // Q = the identity: the first addition is already exceptional
    return a;
}

__device__ __forceinline__ void shift_right_k(u32 (&z)[8]) {
#pragma unroll
    for (int j = 0; j < 7; j++) z[j] = (z[j] >> kK) | (z[j + 1] << (32 - kK));
    z[7] >>= kK;
}

__device__ __forceinline__ xyzz<FP> start_at(const u32 *q_xy, bool &bottom) {      // Q in device memory, Montgomery affine
    xyzz<FP> a;
    a.x = fe_load(q_xy);
    a.y = fe_load(q_xy + 8);
    a.zz = fe_one<FP>();
    a.zzz = fe_one<FP>();
    bottom = fe_is_zero(a.x) && fe_is_zero(a.y);
    return a;
}

}  // namespace
}  // namespace h2
