// The field-level part of the Pasta hash-to-curve (h2c.hip): simplified SWU onto the iso curve, the affine sum of the two mapped
// points and the 3-isogeny onto y^2 = x^3 + 5.  h2c_kernel calls these after hashing; tests/native/h2c_edge_driver.hip calls the same
// text on inputs that BLAKE2b never produces (u = 0, equal and opposite mapped points, the kernel point of the isogeny).
#pragma once
#include "field_sqrt.cuh"

namespace h2 {

#include "h2c_consts.inc"

template <int F> __device__ __forceinline__ u32 fe_sgn0(const fe &a_mont) { return fe_from_mont<F>(a_mont).v[0] & 1u; }

template <int F> __device__ __forceinline__ fe iso_rhs(const fe &x) {      // x^3 + a x + b on the iso curve
    return fe_add<F>(fe_mulx<F>(fe_add<F>(fe_sqr<F>(x), h2c_iso_a<F>()), x), h2c_iso_b<F>());
}

// RFC 9380 6.6.2 (AB != 0)
template <int F> __device__ void map_to_curve_simple_swu(const fe &u, fe &x, fe &y) {
    const fe zu2 = fe_mulx<F>(h2c_swu_z<F>(), fe_sqr<F>(u));
    const fe tv = fe_add<F>(fe_sqr<F>(zu2), zu2);
    fe x1;
    if (fe_is_zero(tv)) x1 = h2c_b_over_za<F>();
    else x1 = fe_mulx<F>(h2c_neg_b_over_a<F>(), fe_add<F>(fe_one<F>(), fe_inv<F>(tv)));
    x = x1;
    if (!fe_sqrt<F>(iso_rhs<F>(x1), y)) {
        x = fe_mulx<F>(zu2, x1);
        (void)fe_sqrt<F>(iso_rhs<F>(x), y);          // one of the two is always a square
    }
    if (fe_sgn0<F>(u) != fe_sgn0<F>(y)) y = fe_neg<F>(y);
}

// Q0 + Q1 on the iso curve (affine chord / tangent); false when the sum is the identity (Q1 = -Q0), x3 and y3 are then untouched
template <int F> __device__ bool h2c_iso_add(const fe &x0, const fe &y0, const fe &x1, const fe &y1, fe &x3, fe &y3) {
    fe lam;
    if (fe_eq(x0, x1)) {
        if (fe_eq(y0, y1) && !fe_is_zero(y0)) {
            const fe xx = fe_sqr<F>(x0);
            lam = fe_mulx<F>(fe_add<F>(fe_add<F>(fe_dbl<F>(xx), xx), h2c_iso_a<F>()), fe_inv<F>(fe_dbl<F>(y0)));
        } else {
            return false;
        }
    } else {
        lam = fe_mulx<F>(fe_sub<F>(y1, y0), fe_inv<F>(fe_sub<F>(x1, x0)));
    }
    x3 = fe_sub<F>(fe_sub<F>(fe_sqr<F>(lam), x0), x1);
    y3 = fe_sub<F>(fe_mulx<F>(lam, fe_sub<F>(x0, x3)), y0);
    return true;
}

// iso_map (Velu, normalised): X = c^2 (x + t / d + u / d^2), Y = c^3 y (1 - t / d^2 - 2u / d^3), d = x - x0; ox and oy keep their
// values (the caller's (0, 0)) when d == 0
template <int F> __device__ void h2c_iso_map(const fe &x3, const fe &y3, fe &ox, fe &oy) {
    const fe d = fe_sub<F>(x3, h2c_iso_x0<F>());
    if (!fe_is_zero(d)) {                              // a kernel point maps to the identity
        const fe di = fe_inv<F>(d), di2 = fe_sqr<F>(di), di3 = fe_mulx<F>(di2, di);
        const fe X = fe_add<F>(x3, fe_add<F>(fe_mulx<F>(h2c_iso_t<F>(), di), fe_mulx<F>(h2c_iso_u<F>(), di2)));
        const fe Y = fe_mulx<F>(y3, fe_sub<F>(fe_sub<F>(fe_one<F>(), fe_mulx<F>(h2c_iso_t<F>(), di2)), fe_mulx<F>(h2c_iso_u2<F>(), di3)));
        ox = fe_mulx<F>(h2c_iso_c2<F>(), X);
        oy = fe_mulx<F>(h2c_iso_c3<F>(), Y);
    }
}

// what h2c_kernel computes from (u0, u1): iso_map(swu(u0) + swu(u1)), Montgomery; (0, 0) stands for the identity
template <int F> __device__ void h2c_map_pair(const fe &u0, const fe &u1, fe &ox, fe &oy) {
    fe x0, y0, x1, y1;
    map_to_curve_simple_swu<F>(u0, x0, y0);
    map_to_curve_simple_swu<F>(u1, x1, y1);
    ox = fe_zero();
    oy = fe_zero();
    fe x3, y3;
    if (h2c_iso_add<F>(x0, y0, x1, y1, x3, y3)) h2c_iso_map<F>(x3, y3, ox, oy);
}

}  // namespace h2
