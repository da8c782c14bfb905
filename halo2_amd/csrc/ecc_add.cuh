// The ECC chip's complete addition with its witnesses (halo2_gadgets ecc/chip/add.rs) and the curve check, on one lane; shared by the
// variable-base kernels (ecc.hip), the fixed-base ones (ecc_fixed.hip) and the batched addition's trace (sinsemilla_commit.hip).
#pragma once
#include "curve.cuh"

namespace h2 {

__device__ __forceinline__ fe fe_select(bool c, const fe &a, const fe &b) {
    fe r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = c ? a.v[i] : b.v[i];
    return r;
}

__device__ __forceinline__ bool on_curve(const affine<FP> &p) {          // y^2 = x^3 + 5
    fe five = fe_one<FP>();
    five = fe_add<FP>(fe_dbl<FP>(fe_dbl<FP>(five)), five);
    return fe_eq(fe_sqr<FP>(p.y), fe_add<FP>(fe_mulx<FP>(fe_sqr<FP>(p.x), p.x), five));
}

// Complete addition as add.rs:213-295 assigns it: lambda, alpha = inv0(x_q - x_p), beta = inv0(x_p), gamma = inv0(x_q),
// delta = inv0(y_q + y_p) where x_q = x_p, and the sum.  One inversion: of f0 f1 f2 with f0 the first nonzero of x_q - x_p, y_q + y_p,
// 2 y_p (the tangent's denominator when the operands are opposite), f1 = x_p, f2 = x_q, a vanishing factor replaced by one.
struct AddWitness {
    fe lambda, alpha, beta, gamma, delta;
};
__device__ __forceinline__ affine<FP> complete_add(const affine<FP> &p, const affine<FP> &q, AddWitness &w) {
    const fe a = fe_sub<FP>(q.x, p.x), d = fe_add<FP>(q.y, p.y), one = fe_one<FP>();
    const bool az = fe_is_zero(a), dz = fe_is_zero(d), pz = fe_is_zero(p.x), qz = fe_is_zero(q.x), yz = fe_is_zero(p.y);
    const fe f0 = fe_select(!az, a, fe_select(!dz, d, fe_select(!yz, fe_dbl<FP>(p.y), one)));
    const fe f1 = fe_select(pz, one, p.x), f2 = fe_select(qz, one, q.x);
    const fe f12 = fe_mulx<FP>(f1, f2);
    const fe all = fe_inv<FP>(fe_mulx<FP>(f0, f12));
    const fe i0 = fe_mulx<FP>(all, f12), t = fe_mulx<FP>(all, f0);
    const fe zero = fe_zero();
    w.alpha = fe_select(az, zero, i0);
    w.beta = fe_select(pz, zero, fe_mulx<FP>(t, f2));
    w.gamma = fe_select(qz, zero, fe_mulx<FP>(t, f1));
    w.delta = fe_select(az && !dz, i0, zero);
    const fe xx = fe_sqr<FP>(p.x);
    const fe num = fe_select(az, fe_add<FP>(fe_dbl<FP>(xx), xx), fe_sub<FP>(q.y, p.y));   // 3 x_p^2 over 2 y_p, or the chord
    w.lambda = fe_select(az && yz, zero, fe_mulx<FP>(num, i0));
    affine<FP> r;
    r.x = fe_sub<FP>(fe_sub<FP>(fe_sqr<FP>(w.lambda), p.x), q.x);
    r.y = fe_sub<FP>(fe_mulx<FP>(w.lambda, fe_sub<FP>(p.x, r.x)), p.y);
    const bool none = az && dz;                                                            // P + (-P)
    r.x = fe_select(pz, q.x, fe_select(qz, p.x, fe_select(none, zero, r.x)));
    r.y = fe_select(pz, q.y, fe_select(qz, p.y, fe_select(none, zero, r.y)));
    return r;
}

// The 11 elements a trace keeps of one complete addition: x_p y_p x_qr y_qr lambda alpha beta gamma delta x_r y_r (d_aux of
// h2_ecc_mul_fixed_trace_device and h2_ecc_add_trace_device)
__device__ __forceinline__ void store_add_aux(u32 *x, const affine<FP> &p, const affine<FP> &q, const AddWitness &w, const affine<FP> &sum) {
    fe_store(x, p.x);
    fe_store(x + 8, p.y);
    fe_store(x + 16, q.x);
    fe_store(x + 24, q.y);
    fe_store(x + 32, w.lambda);
    fe_store(x + 40, w.alpha);
    fe_store(x + 48, w.beta);
    fe_store(x + 56, w.gamma);
    fe_store(x + 64, w.delta);
    fe_store(x + 72, sum.x);
    fe_store(x + 80, sum.y);
}

}  // namespace h2
