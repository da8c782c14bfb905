// The opening argument's challenge recode (ipa.hip, collapse_launch): the endomorphism split of the round's challenge and the signed
// digits the collapse kernels walk.  Plain C++ -- no HIP, no context -- so that the lattice constants, the 6-limb two's-complement
// arithmetic and the NAF are compiled and checked on a CPU (tests/test_ipa_recode.py).
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/halo2_mi355x.h"   // H2_FP / H2_FQ

namespace h2 {

typedef uint64_t u64;
typedef unsigned __int128 u128;

// non-adjacent form of a canonical scalar below 2^256; returns the index of the top non-zero digit (-1 for zero)
inline int naf_recode(const u64 k_in[4], int8_t out[257]) {
    u64 k[5] = {k_in[0], k_in[1], k_in[2], k_in[3], 0};
    memset(out, 0, 257);
    int top = -1;
    for (int i = 0; i < 257; ++i) {
        if (k[0] & 1) {
            int d = 2 - (int)(k[0] & 3);   // +1 if k = 1 mod 4, -1 if k = 3 mod 4
            out[i] = (int8_t)d;
            top = i;
            if (d > 0) {
                k[0] -= 1;
            } else {                        // k += 1 with carry
                for (int j = 0; j < 5; ++j)
                    if (++k[j] != 0) break;
            }
        }
        for (int j = 0; j < 4; ++j) k[j] = (k[j] >> 1) | (k[j + 1] << 63);
        k[4] >>= 1;
    }
    return top;
}

// ---- GLV split of the challenge: u = k1 + k2 * lambda (mod the scalar-field modulus), |k1|, |k2| < 2^129 -----------
// Lattice basis (a1, b1), (a2, b2) with a + b * lambda = 0, and g_i = floor(2^256 * (b2, -b1) / q): all derived with
// big-integer arithmetic offline (extended Euclid on (q, lambda)); lambda is the root of X^2 + X + 1 with
// [lambda](x, y) = (zeta x, y) for the zeta in glv_zeta().  c_i = (u * g_i) >> 256 only has to be CLOSE to the exact
// quotient: any integers c1, c2 give k1 + k2 lambda = u; closeness keeps k1, k2 short.
struct GlvConst {
    u64 a1[2], b1_abs[2], a2[2], b2[2], g1[3], g2[3];   // b1 is negative for both curves, everything else positive
};
static const GlvConst kGlv[2] = {
    // scalar field Fq (Pallas)
    {{0x7fcae1c700000001ULL, 0x49e69d1640f04915ULL}, {0x8cb1279300000000ULL, 0x49e69d1640a89953ULL},
     {0x8cb1279300000000ULL, 0x49e69d1640a89953ULL}, {0x0c7c095a00000001ULL, 0x93cd3a2c8198e269ULL},
     {0x31f0256800000002ULL, 0x4f34e8b2066389a4ULL, 2}, {0x32c49e4bffffffffULL, 0x279a745902a2654eULL, 1}},
    // scalar field Fp (Vesta)
    {{0x8cb1279300000001ULL, 0x49e69d1640a89953ULL}, {0x7fcae1c700000000ULL, 0x49e69d1640f04915ULL},
     {0x0c7c095a00000001ULL, 0x93cd3a2c8198e269ULL}, {0x8cb1279300000001ULL, 0x49e69d1640a89953ULL},
     {0x32c49e4c00000003ULL, 0x279a745902a2654eULL, 1}, {0xff2b871bffffffffULL, 0x279a745903c12455ULL, 1}},
};
// out[na + nb] = a * b
inline void limbs_mul(u64 *out, const u64 *a, int na, const u64 *b, int nb) {
    memset(out, 0, (size_t)(na + nb) * 8);
    for (int i = 0; i < na; ++i) {
        u128 carry = 0;
        for (int j = 0; j < nb; ++j) {
            carry += (u128)a[i] * b[j] + out[i + j];
            out[i + j] = (u64)carry;
            carry >>= 64;
        }
        out[i + nb] = (u64)carry;
    }
}
// 6-limb two's complement: r = a +/- b (b zero-extended from nb limbs)
inline void acc6(u64 r[6], const u64 *b, int nb, bool subtract) {
    u64 t[6] = {0, 0, 0, 0, 0, 0};
    memcpy(t, b, (size_t)nb * 8);
    unsigned carry = subtract ? 1 : 0;
    for (int i = 0; i < 6; ++i) {
        const u64 x = subtract ? ~t[i] : t[i];
        const u128 v = (u128)r[i] + x + carry;
        r[i] = (u64)v;
        carry = (unsigned)(v >> 64);
    }
}
// |v| of a 6-limb two's complement value into 4 limbs; returns true when v < 0
inline bool abs6(const u64 v[6], u64 out[4]) {
    const bool neg = (v[5] >> 63) != 0;
    u64 t[6];
    memcpy(t, v, 48);
    if (neg) {
        unsigned carry = 1;
        for (int i = 0; i < 6; ++i) {
            const u128 w = (u128)(~t[i]) + carry;
            t[i] = (u64)w;
            carry = (unsigned)(w >> 64);
        }
    }
    memcpy(out, t, 32);   // |k_i| < 2^129
    return neg;
}
// digits of k1 and k2 with their signs folded in; returns the highest index used by either
inline int glv_recode(int scalar_field, const u64 u_canonical[4], int8_t naf1[257], int8_t naf2[257]) {
    const GlvConst &G = kGlv[scalar_field == H2_FQ ? 0 : 1];
    u64 prod[7], c1[3], c2[3];
    limbs_mul(prod, u_canonical, 4, G.g1, 3);
    memcpy(c1, prod + 4, 24);
    limbs_mul(prod, u_canonical, 4, G.g2, 3);
    memcpy(c2, prod + 4, 24);
    // k1 = u - c1 a1 - c2 a2;   k2 = -c1 b1 - c2 b2 = c1 |b1| - c2 b2
    u64 k1[6] = {u_canonical[0], u_canonical[1], u_canonical[2], u_canonical[3], 0, 0}, k2[6] = {0, 0, 0, 0, 0, 0}, t[5];
    limbs_mul(t, c1, 3, G.a1, 2);
    acc6(k1, t, 5, true);
    limbs_mul(t, c2, 3, G.a2, 2);
    acc6(k1, t, 5, true);
    limbs_mul(t, c1, 3, G.b1_abs, 2);
    acc6(k2, t, 5, false);
    limbs_mul(t, c2, 3, G.b2, 2);
    acc6(k2, t, 5, true);
    u64 m1[4], m2[4];
    const bool n1 = abs6(k1, m1), n2 = abs6(k2, m2);
    int top1 = naf_recode(m1, naf1), top2 = naf_recode(m2, naf2);
    if (n1)
        for (int i = 0; i <= top1; ++i) naf1[i] = (int8_t)-naf1[i];
    if (n2)
        for (int i = 0; i <= top2; ++i) naf2[i] = (int8_t)-naf2[i];
    return top1 > top2 ? top1 : top2;
}

}  // namespace h2
