// The signed window digits of a multiexp's scalars: how a scalar is cut into digits and how a digit is written as a code.  Plain integer
// code on limb arrays, __host__ __device__, no HIP in it: msm_sort.hip cuts its digits through these functions (but for one copy of the
// endomorphism loop, kept in emit_entries for speed), and tests/native/msm_digits_check.cpp runs the very same functions on the CPU against a
// recode from the definition (tests/test_msm_digits.py).
//
// A scalar k = sum_w d_w 2^(c w) with d_w in [-2^(c-1) + 1, 2^(c-1)]: window w's c bits plus the carry of the window below give raw in
// [0, 2^c]; raw > 2^(c-1) becomes raw - 2^c and carries 1 into the next window (raw = 2^c: digit 0 with a carry).  The windows W a caller
// asks for (msm_plan.h: 255 / c + 1, or 130 / c + 1 for a half of the endomorphism split) reach past the top bit, so the last carry is 0.
#pragma once
#include <stdint.h>

#ifndef H2_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define H2_HD __host__ __device__ __forceinline__
#else
#define H2_HD inline
#endif
#endif

namespace h2 {

typedef uint32_t u32;
typedef uint64_t u64;

// digit codes.  16 bits (windows up to 16 bits): (|d| - 1) | (d < 0) << 15, digit 0: kZeroCode.  32 bits: (|d| - 1) | (d < 0) << 31, digit 0: kZero32.
static constexpr u32 kZeroCode = 0xFFFFu;
static constexpr u32 kZero32 = 0xFFFFFFFFu;
H2_HD u32 digit_code16(u32 mag, u32 negative) { return mag ? ((mag - 1) | (negative ? 0x8000u : 0u)) : kZeroCode; }
H2_HD u32 digit_code32(u32 mag, u32 negative) { return mag ? ((mag - 1) | (negative ? 0x80000000u : 0u)) : kZero32; }
// the 16-bit code of the digit a 32-bit code stands for (|d| - 1 < 2^15)
H2_HD u32 narrow_code(u32 code32) { return (code32 & 0xFFFFu) | ((code32 >> 16) & 0x8000u); }

// limb idx of an 8-limb value by register selects (a dynamic index would send the limbs through scratch); 0 for idx = 8
H2_HD u32 limb_at(const u32 *v, int idx) {
    u32 r = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) r = (idx == i) ? v[i] : r;
    return r;
}

// the digits of the 8-limb scalar s at the compile-time width C, handed to f(w, 32-bit code) for w = 0 .. 255 / C
template <int C, typename Fn> H2_HD void for_each_digit_static(const u32 *s, Fn f) {
    constexpr int W = 255 / C + 1;
    constexpr u32 mask = (1u << C) - 1, half = 1u << (C - 1), full = 1u << C;
    u32 carry = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const int bit = w * C, word = bit >> 5, sh = bit & 31;     // compile-time after unrolling: plain register picks
        u32 v = s[word] >> sh;
        if (sh + C > 32 && word + 1 < 8) v |= s[word + 1] << (32 - sh);
        const u32 raw = (v & mask) + carry;
        carry = raw > half;
        f(w, carry ? (raw == full ? kZero32 : digit_code32(full - raw, 1)) : digit_code32(raw, 0));      // raw = 2^c: digit 0, carry out
    }
}
// the same at a width known at run time, for w = 0 .. W - 1
template <typename Fn> H2_HD void for_each_digit_runtime(const u32 *s, int c, int W, Fn f) {
    u32 carry = 0;
    const u32 mask = (1u << c) - 1, half = 1u << (c - 1), full = 1u << c;
    for (int w = 0; w < W; ++w) {
        const int bit = w * c, word = bit >> 5, sh = bit & 31;
        const u64 two = (u64)limb_at(s, word) | ((u64)limb_at(s, word + 1) << 32);  // limb_at(.., 8) = 0
        const u32 raw = ((u32)(two >> sh) & mask) + carry;
        carry = raw > half;
        f(w, carry ? (raw == full ? kZero32 : digit_code32(full - raw, 1)) : digit_code32(raw, 0));      // raw = 2^c: digit 0, carry out
    }
}
template <typename Fn> H2_HD void for_each_digit(const u32 *s, int c, int W, Fn f) {
    // compile-time widths: the limb picks become plain register selects (the run-time loop picks the limbs by compares: at
    // c = 17 the pass-1 kernels took 29 + 78 us against 16 + 53 us for the unrolled c = 20)
    if (c == 16) { for_each_digit_static<16>(s, f); return; }
    if (c == 17) { for_each_digit_static<17>(s, f); return; }
    if (c == 18) { for_each_digit_static<18>(s, f); return; }
    if (c == 19) { for_each_digit_static<19>(s, f); return; }
    if (c == 20) { for_each_digit_static<20>(s, f); return; }
    if (c == 13) { for_each_digit_static<13>(s, f); return; }
    for_each_digit_runtime(s, c, W, f);
}

// the digits of the two halves of an endomorphism-split scalar (glv.cuh: mag[part] = |k_part| < 2^129, neg[part] = its sign), handed to
// f(part, w, |d|, negative) for every window, |d| = 0 included.  The digits of |k_part| lie in [-half + 1, half]; those of a NEGATIVE
// part are rounded at raw >= half instead, into [-half, half - 1], because they are stored with their sign flipped (`negative` is the
// sign of the digit of k_part itself) and the code has no room for -half.
template <typename Fn> H2_HD void for_each_glv_digit(const u32 (*mag)[5], const u32 *neg, int c, int W, Fn f) {
    const u32 mask = (1u << c) - 1, half = 1u << (c - 1);
#pragma unroll
    for (int part = 0; part < 2; ++part) {
        u32 carry = 0;
        for (int w = 0; w < W; ++w) {
            const int bit = w * c, word = bit >> 5, sh = bit & 31;
            u32 lo = 0, hi = 0;
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                lo = (word == q) ? mag[part][q] : lo;
                hi = (word + 1 == q) ? mag[part][q] : hi;
            }
            const u32 raw = ((u32)(((u64)lo | ((u64)hi << 32)) >> sh) & mask) + carry;
            const bool up = neg[part] ? raw >= half : raw > half;
            carry = up;
            f(part, w, up ? (1u << c) - raw : raw, (up ? 1u : 0u) ^ neg[part]);      // |d| = 0 when raw = 0 or raw = 2^c
        }
    }
}

}  // namespace h2
