// The two fixed-base multiplications whose scalar is a RUNNING SUM (halo2_gadgets ecc/chip/mul_fixed/short.rs, base_field_elem.rs), their
// witness in bulk, one lane per multiplication:
//
//   h2_ecc_mul_fixed_short_trace_device        [sign magnitude]B over 22 windows: the value commitment's [v]V
//   h2_ecc_mul_fixed_base_field_trace_device   [alpha]B over 85 windows with the cells of its canonicity check: the nullifier's [alpha]K
//
// Both walk the tables h2_ecc_fixed_tables_device writes, window by window as ecc_fixed_trace (ecc_fixed.hip) does, with the additions of
// ecc_fixed_chain.cuh around two_pass_trace (common.h): pass A stores ZZ ZZZ of the accumulator before windows 2 .. nw-1, the batch
// inversion turns them over, pass B emits the rows and closes on complete_add and its record (ecc_add.cuh).  What differs from the
// full-width form: the `window` column holds the running sum z_0 .. z_nw (utilities/decompose_running_sum.rs), not the window's value, so
// a multiplication takes nw + 1 rows, and the aux goes on after the addition's record -- the signed y, or alpha_0', alpha_1, alpha_2.
//
// The running sum needs no division.  The input is a canonical integer v below p and window w < nw reads bits 3w .. 3w+2 of it, so
// v - (v mod 8^w) is a multiple of 8^w AS AN INTEGER and z_w = v >> 3w: one conversion to Montgomery form per row.  That covers every
// row of the base-field form (85 windows read 255 bits, z_85 = 0).  The short form reads 64 bits: its window 21 is bit 63 alone, and a
// magnitude of 2^64 and above -- which the circuit must reject, and the reference's negative tests feed -- leaves bits 64 and 65 in
// z_21 - k_21, an even integer that is no multiple of 8.  There z_22 = (v >> 66) + ((v >> 64) & 3) / 4 in the field, from two halvings
// of one.
//
// The unit keeps NO device memory: the inverses' scratch is the caller's (the descriptor names it and its capacity) and the stream
// travels in the descriptor.  The table gather stays in global memory as ecc_fixed.hip's header argues.  A workgroup is 64 lanes, one
// wave: the lanes share nothing, and no other width was measured.
#include "common.h"
#include "ecc_add.cuh"
#include "ecc_fixed_chain.cuh"

namespace h2 {
namespace {

constexpr int kSumLanes = 64;                              // lanes per workgroup
constexpr size_t kMaxSumMuls = (size_t)1 << 30;
constexpr unsigned kShortWindows = 22, kBaseFieldWindows = 85;
constexpr unsigned kShortAux = 12, kBaseFieldAux = 15;

__device__ __forceinline__ fe fe_of_words(const u32 (&k)[8]) {
    fe r;
#pragma unroll
    for (int j = 0; j < 8; j++) r.v[j] = k[j];
    return r;
}

// a / 2 for a below p: a + p is below 2^256
__device__ __forceinline__ fe fe_half(const fe &a) {
    const bool odd = a.v[0] & 1u;
    fe s;
    u64 c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        c += (u64)a.v[j] + (odd ? mod_limb<FP>(j) : 0u);
        s.v[j] = (u32)c;
        c >>= 32;
    }
#pragma unroll
    for (int j = 0; j < 7; j++) s.v[j] = (s.v[j] >> 1) | (s.v[j + 1] << 31);
    s.v[7] >>= 1;
    return s;
}

// m / 4 as a Montgomery element, m = 0 .. 3
__device__ __forceinline__ fe quarters(u32 m) {
    const fe q = fe_half(fe_half(fe_one<FP>())), h = fe_dbl<FP>(q);
    return m == 0 ? fe_zero() : m == 1 ? q : m == 2 ? h : fe_add<FP>(h, q);
}

__device__ __forceinline__ bool is_minus_one(const fe &c) {                 // the canonical p - 1
    u32 d = c.v[0];
#pragma unroll
    for (int j = 1; j < 8; j++) d |= c.v[j] ^ mod_limb<FP>(j);
    return d == 0;
}

// alpha_0' = (alpha mod 2^252) + 2^130 - t_p with t_p = p - 2^254 (base_field_elem.rs:300-310), canonical: the sum is below
// 2^252 + 2^130 < p, so nothing is reduced
__device__ __forceinline__ fe alpha_0_prime(const fe &alpha) {
    u32 shift[8];                                          // 2^130 - t_p; t_p is the low four limbs of p
    long long borrow = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const long long d = (long long)(j == 4 ? 4u : 0u) - (long long)(j < 4 ? mod_limb<FP>(j) : 0u) + borrow;
        shift[j] = (u32)d;
        borrow = d < 0 ? -1 : 0;
    }
    fe r;
    u64 c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        c += (u64)(j == 7 ? alpha.v[7] & 0x0fffffffu : alpha.v[j]) + shift[j];
        r.v[j] = (u32)c;
        c >>= 32;
    }
    return r;
}

// Columns x_p y_p x_qr y_qr window u = 0 .. 5, nw + 1 rows a multiplication; rows 0 .. nw-1 as ecc_fixed_trace's but for `window`, which
// holds z_w; row nw holds z_nw there and zeros in the other five.  SHORT: window 21 is one bit wide, `signs` are read and the aux is
// the addition's record and the signed y; otherwise the aux is the record, alpha_0', alpha_1, alpha_2 and alpha_0' again, canonical.
// Pass A (EMIT = false) stores ZZ ZZZ of the accumulator before windows 2 .. nw-1, element (w - 2) chunk + lane; pass B finds the
// inverses there.
template <bool EMIT, bool SHORT>
__global__ void __launch_bounds__(kSumLanes) ecc_fixed_sum_trace(const u32 *__restrict__ points, const u32 *__restrict__ roots, u32 nw,
                                                                 const u32 *__restrict__ values, const u32 *__restrict__ signs, size_t first,
                                                                 size_t chunk, size_t count, u32 *__restrict__ inv,
                                                                 u32 *__restrict__ columns, u32 *__restrict__ aux) {
    const size_t local = (size_t)blockIdx.x * kSumLanes + threadIdx.x;
    if (local >= chunk) return;
    const size_t i = first + local;
    u32 k[8];
    load_scalar(values, i, k);
    const size_t column = 8 * (size_t)(nw + 1) * count;
    u32 *out = columns + 8 * (i * (nw + 1));               // row 0 of this multiplication in column 0
    xyzz<FP> acc = xyzz_identity<FP>();
    u32 beyond = 0;                                        // what the last window leaves of its three bits: bits 64 and 65
#pragma unroll 1
    for (u32 w = 0; w < nw; w++) {
        fe z;
        if (EMIT) z = fe_to_mont<FP>(fe_of_words(k));      // z_w = value >> 3w
        u32 d = take_window(k);
        if (SHORT && w + 1 == nw) {
            beyond = d >> 1;
            d &= 1u;
        }
        const affine<FP> q = aff_load<FP>(table_entry(points, w, d, 16));
        affine<FP> a{fe_zero(), fe_zero()};                 // the accumulator before this window; row 0 has none
        if (w == 1) {
            a.x = acc.x;
            a.y = acc.y;
        } else if (w > 1) {
            u32 *slot = inv + 8 * ((size_t)(w - 2) * chunk + local);
            if (!EMIT) {
                fe_store(slot, fe_mulx<FP>(acc.zz, acc.zzz));
            } else {
                const fe i_zed = fe_load(slot);
                a.x = fe_mulx<FP>(acc.x, fe_mulx<FP>(acc.zzz, i_zed));
                a.y = fe_mulx<FP>(acc.y, fe_mulx<FP>(acc.zz, i_zed));
            }
        }
        if (EMIT) {
            fe_store(out + 8 * w, q.x);
            fe_store(out + column + 8 * w, q.y);
            fe_store(out + 2 * column + 8 * w, a.x);
            fe_store(out + 3 * column + 8 * w, a.y);
            fe_store(out + 4 * column + 8 * w, z);
            fe_store(out + 5 * column + 8 * w, fe_load(table_entry(roots, w, d, 8)));
        }
        if (w == 0) {
            acc = xyzz_of(q);
        } else if (w + 1 < nw) {
            xyzz_madd_incomplete(acc, q);
        } else if (EMIT) {                                  // short.rs:140-150, base_field_elem.rs:200-210: the window's point first
            AddWitness wit;
            const affine<FP> sum = complete_add(q, a, wit);
            u32 *x = aux + 8 * (size_t)(SHORT ? kShortAux : kBaseFieldAux) * i;
            store_add_aux(x, q, a, wit, sum);
            if (SHORT) {                                    // short.rs:178-184: -y for the sign -1, y for anything else
                const fe sign = fe_load(signs + 8 * i);
                fe_store(x + 88, is_minus_one(sign) ? fe_neg<FP>(sum.y) : sum.y);
            }
        }
    }
    if (!EMIT) return;
    // row nw: z_nw = (z_(nw-1) - k_(nw-1)) / 8, the rest of the value and what the narrow last window left behind
    fe z = fe_to_mont<FP>(fe_of_words(k));
    if (SHORT && beyond) z = fe_add<FP>(z, quarters(beyond));
    const fe zero = fe_zero();
    fe_store(out + 8 * nw, zero);
    fe_store(out + column + 8 * nw, zero);
    fe_store(out + 2 * column + 8 * nw, zero);
    fe_store(out + 3 * column + 8 * nw, zero);
    fe_store(out + 4 * column + 8 * nw, z);
    fe_store(out + 5 * column + 8 * nw, zero);
    if (!SHORT) {
        const fe alpha = fe_load(values + 8 * i), prime = alpha_0_prime(alpha);
        fe small = zero;
        u32 *x = aux + 8 * (size_t)kBaseFieldAux * i;
        fe_store(x + 88, fe_to_mont<FP>(prime));
        small.v[0] = (alpha.v[7] >> 28) & 3u;               // alpha_1 = alpha[252..254)
        fe_store(x + 96, fe_to_mont<FP>(small));
        small.v[0] = (alpha.v[7] >> 30) & 1u;               // alpha_2 = alpha[254]
        fe_store(x + 104, fe_to_mont<FP>(small));
        fe_store(x + 112, prime);
    }
}

// the checks both entry points share, before anything touches the device
inline bool sum_args_ok(const h2_ecc_fixed_sum_t *d, unsigned nw, size_t count) {
    if (!d || d->num_windows != nw || count > kMaxSumMuls) return false;
    return !count || (d->d_points && d->d_u && d->d_scratch && d->scratch_elems >= nw - 2);
}

template <bool SHORT>
int sum_trace(const h2_ecc_fixed_sum_t *d, const void *d_values, const void *d_signs, size_t count, void *d_columns, void *d_aux) {
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!count) return H2_OK;
    hipStream_t st = (hipStream_t)d->stream;
    const u32 nw = d->num_windows;
    // num_windows - 2 elements per lane; two windows have none
    return two_pass_trace((u32 *)d->d_scratch, d->scratch_elems, count, nw - 2, st, [&](bool emit, size_t first, size_t chunk, u32 *scratch) {
        hipLaunchKernelGGL(!emit ? (ecc_fixed_sum_trace<false, SHORT>) : (ecc_fixed_sum_trace<true, SHORT>), dim3(grid_of(chunk, kSumLanes)),
                           dim3(kSumLanes), 0, st, (const u32 *)d->d_points, (const u32 *)d->d_u, nw, (const u32 *)d_values,
                           (const u32 *)d_signs, first, chunk, count, scratch, (u32 *)d_columns, (u32 *)d_aux);
        return H2_OK;
    });
}

}  // namespace
}  // namespace h2

using namespace h2;

extern "C" int h2_ecc_mul_fixed_short_trace_device(const h2_ecc_fixed_sum_t *d, const void *d_magnitudes, const void *d_signs, size_t count,
                                                   void *d_columns, void *d_aux) {
    if (!sum_args_ok(d, kShortWindows, count) || (count && (!d_magnitudes || !d_signs || !d_columns || !d_aux))) return H2_ERR_ARGS;
    return sum_trace<true>(d, d_magnitudes, d_signs, count, d_columns, d_aux);
}

extern "C" int h2_ecc_mul_fixed_base_field_trace_device(const h2_ecc_fixed_sum_t *d, const void *d_alphas, size_t count, void *d_columns,
                                                        void *d_aux) {
    if (!sum_args_ok(d, kBaseFieldWindows, count) || (count && (!d_alphas || !d_columns || !d_aux))) return H2_ERR_ARGS;
    return sum_trace<false>(d, d_alphas, nullptr, count, d_columns, d_aux);
}
