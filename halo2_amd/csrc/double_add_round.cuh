// The merged double-and-add round Acc <- (Acc + S) + Acc with incomplete addition, on one lane, and what a witness trace takes from it.
// It serves both chains built on that step: Sinsemilla's, where S = S(m_i) comes from the generator table (sinsemilla_chain.cuh,
// sinsemilla.hip, sinsemilla_commit.hip), and the variable-base multiplication's, where S = +-P (ecc.hip).  Everything is internal to
// the including unit.
#pragma once
#include "curve.cuh"

namespace h2 {
namespace {

// One round on the accumulator, 18 multiplications: R = Acc + S is the mixed addition, whose by-products put Acc on R's denominators
// for free, so R + Acc adds two points with one denominator (the head of sinsemilla.hip).  p and d are the two differences that
// incomplete addition must not see vanish, r is the first addition's difference of the y, zz_r is R's ZZ.  No branch: a vanishing
// difference leaves ZZ = 0 behind, which the caller reports.
__device__ __forceinline__ void double_add_round(xyzz<FP> &a, const affine<FP> &s, fe &p, fe &r, fe &d, fe &zz_r) {
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

// A trace row needs the affine x_a, y_a of the accumulator BEFORE the round and the two slopes lambda_1 = (y_a - y_p) / (x_a - x_p),
// lambda_2 = 2 y_a / (x_a - x_r) - lambda_1: the inverses of ZZ ZZZ, P and D.  Pass A of a trace stores their product, one element a
// round; the batch inversion between the passes turns it into 1 / (ZZ ZZZ P D), which pass B splits three ways.
// zed is ZZ ZZZ of the accumulator before the round.  The caller forms it where it suits its registers: ahead of the round, pass A
// need not keep ZZ and ZZZ across it (ecc.hip); the Sinsemilla trace is the smaller for forming it after.
__device__ __forceinline__ fe round_denominators(const fe &zed, const fe &p, const fe &d) { return fe_mulx<FP>(fe_mulx<FP>(zed, p), d); }

struct RoundRow {
    fe x_a, y_a, lambda_1, lambda_2;
};
// before: the accumulator the round started from; p, r, d, zz_r: what the round gave; all: the inverse of round_denominators
__device__ __forceinline__ RoundRow round_row(const xyzz<FP> &before, const fe &zed, const fe &p, const fe &r, const fe &d,
                                              const fe &zz_r, const fe &all) {
    const fe i_zed = fe_mulx<FP>(all, fe_mulx<FP>(p, d)), az = fe_mulx<FP>(all, zed);      // 1 / (ZZ ZZZ), 1 / (P D)
    const fe i_p = fe_mulx<FP>(az, d), i_d = fe_mulx<FP>(az, p);
    const fe i_zzz = fe_mulx<FP>(before.zz, i_zed);                                        // ZZ / (ZZ ZZZ)
    RoundRow row;
    row.x_a = fe_mulx<FP>(before.x, fe_mulx<FP>(before.zzz, i_zed));                       // X / ZZ
    // y_a - y_p = -r / ZZZ and x_a - x_p = -p / ZZ:  lambda_1 = r ZZ / (ZZZ p)
    row.lambda_1 = fe_mulx<FP>(fe_mulx<FP>(r, i_zzz), fe_mulx<FP>(before.zz, i_p));
    // x_a - x_r = d / ZZ_R:  lambda_2 = 2 y_a ZZ_R / d - lambda_1
    row.y_a = fe_mulx<FP>(before.y, i_zzz);
    row.lambda_2 = fe_sub<FP>(fe_mulx<FP>(fe_dbl<FP>(row.y_a), fe_mulx<FP>(zz_r, i_d)), row.lambda_1);
    return row;
}

}  // namespace
}  // namespace h2
