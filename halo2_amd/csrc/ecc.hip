// Variable-base scalar multiplication over Pallas (halo2_gadgets/src/ecc/chip/mul.rs, mul/incomplete.rs, mul/complete.rs,
// mul/overflow.rs, add.rs), batched: one lane per multiplication.
//
//   h2_ecc_mul_device         n independent products [k_i]P_i (no sum: this is not an MSM) -> n affine points
//   h2_ecc_mul_trace_device   what mul::Config::assign witnesses for `count` pairs (base, alpha): the ten advice columns of the region
//                             "variable-base scalar mul" (137 rows per multiplication) and the overflow check's 16 witnesses
//
// The product is plain double-and-add from the top bit on an XYZZ accumulator with the complete operations of curve.cuh, so every scalar
// below 2^255 and every base is right, the identity included; the lane inverts once, at the end.
//
// The trace follows the reference's algorithm, not the fastest one: Acc = [2]P, then 251 merged steps Acc <- (Acc + (+-P)) + Acc with
// INCOMPLETE addition over the bits k_254 .. k_4 of k = alpha + t_q, three steps with complete addition, and the last bit.  The merged
// step is Sinsemilla's round (double_add_round.cuh, shared with sinsemilla.hip) with S = +-P, and the same answer to the 502 inversions
// per lane: pass A runs the chain in XYZZ and stores one element per row, the product ZZ ZZZ P D; h2_batch_invert_device inverts them
// all (zeros stay zero: inv0); pass B runs the chain again, splits each inverse (round_row, the same header) and emits affine rows; the
// chunks and the inversion between the passes are two_pass_trace's (common.h).  Two more elements ride in the same batch: ZZ ZZZ of
// the last accumulator, and z_130 whose inverse is the overflow check's eta.
// The 8 complete additions (row 0's [2]P, two per complete bit, one for the last bit) take their operands from the previous result
// and run in a kernel of their own after pass B, which keeps the inversion's registers out of the chain's loop;
// each (complete_add, ecc_add.cuh) forms the product of its nonzero denominators -- x_q - x_p (or y_q + y_p, or 2 y_p, when that vanishes), x_p, x_q -- inverts it
// on the lane (field_inv.cuh) and splits it: 8 inversions against the 251 rounds of 32 products, measured in profiles/ecc.txt.
#include "common.h"
#include "double_add_round.cuh"
#include "ecc_add.cuh"

namespace h2 {
namespace {

constexpr int kET = 256;                                   // lanes per workgroup
constexpr size_t kMaxMuls = (size_t)1 << 30;
constexpr u32 kRows = 137, kHiLen = 125, kRounds = 251;    // rows of one multiplication; bits of the hi half; hi + lo
constexpr u32 kLoEnd = 2 + kRounds - kHiLen;               // row 128: the last of the incomplete range
constexpr u32 kScratch = kRounds + 2;                      // scratch elements per lane: the rounds, the last accumulator, z_130
// Elements of scratch per chunk of the trace: 256 MiB, 33 156 multiplications.  A chunk's time is one wave's chain (~8 ms) until the
// device is full, and at sinsemilla.hip's 2^20 elements a chunk is 4 143 lanes, 65 waves on 256 compute units: 32 768 multiplications
// took eight chunks one after the other (profiles/ecc.txt).  Their ten columns are 1.4 GiB, so the scratch stays a fraction of the output.
constexpr size_t kTraceScratchRows = (size_t)1 << 23;

// the top bit of a 256-bit word, which then moves up by one
__device__ __forceinline__ u32 take_top_bit(u32 (&k)[8]) {
    const u32 bit = k[7] >> 31;
#pragma unroll
    for (int j = 7; j > 0; j--) k[j] = (k[j] << 1) | (k[j - 1] >> 31);
    k[0] <<= 1;
    return bit;
}

__global__ void __launch_bounds__(kET) ecc_mul(const u32 *__restrict__ bases, const u32 *__restrict__ scalars, size_t n,
                                               u32 *__restrict__ out_xy, uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * kET + threadIdx.x;
    if (i >= n) return;
    const affine<FP> p = aff_load<FP>(bases + 16 * i);
    u32 k[8];
    {
        const fe s = fe_load(scalars + 8 * i);
#pragma unroll
        for (int j = 0; j < 8; j++) k[j] = s.v[j];
    }
    take_top_bit(k);                                       // bit 255 is not part of the scalar
    xyzz<FP> acc = xyzz_identity<FP>();
#pragma unroll 1
    for (u32 b = 0; b < 255; b++) {
        acc = xyzz_dbl<FP>(acc);
        if (take_top_bit(k)) xyzz_madd<FP>(acc, p);
    }
    const affine<FP> res = xyzz_to_affine<FP>(acc);
    fe_store(out_xy + 16 * i, res.x);
    fe_store(out_xy + 16 * i + 8, res.y);
    status[i] = aff_is_identity(p) || on_curve(p) ? 0 : 1;
}

// k = alpha + t_q, not reduced (mul.rs:421-455), as a 256-bit word
__device__ __forceinline__ void scalar_of(const fe &alpha, u32 (&k)[8]) {
    const fe c = fe_from_mont<FP>(alpha);
    u32 carry = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        u32 co;
        k[j] = __builtin_addc(c.v[j], j < 4 ? mod_limb<FQ>(j) : 0u, carry, &co);
        carry = co;
    }
}

// The incomplete range, rows 1 - 128.
// Pass A (EMIT = false): inv[j] <- ZZ ZZZ P D of round j, inv[251] <- ZZ ZZZ of the last accumulator, inv[252] <- z_130.
// Pass B (EMIT = true): inv holds their inverses; the rows are written (the columns were zeroed by the caller), and the accumulator and
// running sum the range ends on, where ecc_mul_complete picks them up.  `first` is the first multiplication of the chunk: inv is indexed
// from it, everything else from multiplication 0.
// Columns (chip.rs:280-292, mul.rs:71-79): complete addition x_p y_p x_qr y_qr lambda alpha beta gamma delta = 0 .. 8;
// hi half z x_a lambda_1 lambda_2 = 9 3 4 5; lo half = 6 7 8 2; both halves x_p y_p = 0 1; z_complete = 9.
template <bool EMIT>
__global__ void __launch_bounds__(kET) ecc_mul_trace(const u32 *__restrict__ bases, const u32 *__restrict__ alphas, size_t first,
                                                     size_t chunk, size_t count, u32 *__restrict__ inv, u32 *__restrict__ columns,
                                                     uint8_t *__restrict__ status) {
    const size_t local = (size_t)blockIdx.x * kET + threadIdx.x;
    if (local >= chunk) return;
    const size_t i = first + local;
    const affine<FP> base = aff_load<FP>(bases + 16 * i);
    u32 k[8];
    scalar_of(fe_load(alphas + 8 * i), k);
    take_top_bit(k);                                       // bit 254 is the top one now
    u32 *t = inv + 8 * (local * kScratch);
    if (!EMIT) {                                           // z_130 = k >> 130: the top 125 bits, below p
        fe z_130;
#pragma unroll
        for (int j = 0; j < 4; j++) z_130.v[j] = (k[j + 4] >> 3) | (j < 3 ? k[j + 5] << 29 : 0u);
#pragma unroll
        for (int j = 4; j < 8; j++) z_130.v[j] = 0;
        fe_store(t + 8 * (kRounds + 1), fe_to_mont<FP>(z_130));
    }
    xyzz<FP> a = xyzz_dbl_affine<FP>(base);                // [2]P; ZZ = 0 for the identity, which is reported
    bool bad = aff_is_identity(base);
    fe z = fe_zero();
    const size_t column = 8 * (size_t)kRows * count;
    u32 *out = columns + 8 * (i * kRows);                  // row 0 of this multiplication in column 0
#pragma unroll 1
    for (u32 j = 0; j < kRounds; j++) {
        const bool hi = j < kHiLen;
        const u32 row = 2 + (hi ? j : j - kHiLen);
        const u32 bit = take_top_bit(k);
        affine<FP> s;
        s.x = base.x;
        s.y = bit ? base.y : fe_neg<FP>(base.y);
        const xyzz<FP> before = a;
        const fe zed = fe_mulx<FP>(a.zz, a.zzz);
        fe p, r, d, zz_r;
        double_add_round(a, s, p, r, d, zz_r);
        bad = bad || fe_is_zero(p) || fe_is_zero(d);
        if (!EMIT) {
            fe_store(t + 8 * j, round_denominators(zed, p, d));
        } else {
            const RoundRow v = round_row(before, zed, p, r, d, zz_r, fe_load(t + 8 * j));
            const u32 c_z = hi ? 9 : 6, c_xa = hi ? 3 : 7, c_l1 = hi ? 4 : 8, c_l2 = hi ? 5 : 2;
            if (j == 0 || j == kHiLen) {                                                   // a half starts: z and y_a one row above
                fe_store(out + c_z * column + 8, z);
                fe_store(out + c_l1 * column + 8, v.y_a);
            }
            z = fe_dbl<FP>(z);
            if (bit) z = fe_add<FP>(z, fe_one<FP>());
            fe_store(out + c_z * column + 8 * row, z);
            fe_store(out + c_xa * column + 8 * row, v.x_a);
            fe_store(out + c_l1 * column + 8 * row, v.lambda_1);
            fe_store(out + c_l2 * column + 8 * row, v.lambda_2);
            if (!hi) {                                                                     // the lo half spans every row of the range
                fe_store(out + 8 * row, base.x);
                fe_store(out + column + 8 * row, base.y);
            }
            if (j == kHiLen) {                                                             // and the hi half ends on the same point
                fe_store(out + 3 * column + 8 * (2 + kHiLen), v.x_a);
                fe_store(out + 4 * column + 8 * (2 + kHiLen), v.y_a);
            }
        }
    }
    if (!EMIT) {
        fe_store(t + 8 * kRounds, fe_mulx<FP>(a.zz, a.zzz));
        return;
    }
    const fe i_zed = fe_load(t + 8 * kRounds);
    fe_store(out + 7 * column + 8 * kLoEnd, fe_mulx<FP>(a.x, fe_mulx<FP>(a.zzz, i_zed)));  // the accumulator the lo half ends on
    fe_store(out + 8 * column + 8 * kLoEnd, fe_mulx<FP>(a.y, fe_mulx<FP>(a.zz, i_zed)));
    fe_store(out + 9 * column + 8 * (kLoEnd + 1), z);                                      // complete.rs:115-123
    status[i] = bad ? 1 : 0;
}

// Rows 0 and 129 - 136 and aux, after pass B: the 8 complete additions in one loop.  Step 0 is row 0's P + P; steps 1, 3, 5 are U + Acc
// of a complete bit (row 129 + 2 iter), steps 2, 4, 6 Acc + (U + Acc) one row below; step 7 is the last bit's (row 135).  From step 2
// on, q is the previous sum.  The accumulator and running sum of the incomplete range are read back from the rows pass B wrote.
__global__ void __launch_bounds__(kET) ecc_mul_complete(const u32 *__restrict__ bases, const u32 *__restrict__ alphas, size_t first,
                                                        size_t chunk, size_t count, const u32 *__restrict__ inv, u32 *columns,
                                                        u32 *__restrict__ aux) {
    const size_t local = (size_t)blockIdx.x * kET + threadIdx.x;
    if (local >= chunk) return;
    const size_t i = first + local;
    const affine<FP> base = aff_load<FP>(bases + 16 * i);
    const fe alpha = fe_load(alphas + 8 * i);
    u32 k[8];
    scalar_of(alpha, k);
    const u32 k_254 = (k[7] >> 30) & 1u;
    u32 low = k[0] << 28;                                                                  // k_3 at the top
    const size_t column = 8 * (size_t)kRows * count;
    u32 *out = columns + 8 * (i * kRows);
    const fe neg_y = fe_neg<FP>(base.y);
    fe z = fe_load(out + 9 * column + 8 * (kLoEnd + 1));
    affine<FP> p = base, q = base, sum = base;
#pragma unroll 1
    for (u32 step = 0; step < 8; step++) {
        const u32 row = step ? kLoEnd + step : 0;
        if (step & 1) {
            if (step == 1) {
                sum.x = fe_load(out + 7 * column + 8 * kLoEnd);
                sum.y = fe_load(out + 8 * column + 8 * kLoEnd);
            }
            q = sum;
            const bool bit = low >> 31;
            low <<= 1;
            z = fe_dbl<FP>(z);
            if (bit) z = fe_add<FP>(z, fe_one<FP>());
            p.x = base.x;
            p.y = fe_select(bit, base.y, neg_y);
            if (step < 7) {                                                                // complete.rs:140-176
                fe_store(out + 9 * column + 8 * (row + 1), base.y);
                fe_store(out + 9 * column + 8 * (row + 2), z);
            } else {                                                                       // mul.rs:331-374: bit set adds the identity
                if (bit) p.x = p.y = fe_zero();
                fe_store(out + 9 * column + 8 * (row + 1), z);
                fe_store(out + 8 * (row + 1), base.x);
                fe_store(out + column + 8 * (row + 1), base.y);
            }
        } else if (step) {
            p = q;
            q = sum;
        }
        AddWitness w;
        sum = complete_add(p, q, w);
        fe_store(out + 8 * row, p.x);
        fe_store(out + column + 8 * row, p.y);
        fe_store(out + 2 * column + 8 * row, q.x);
        fe_store(out + 3 * column + 8 * row, q.y);
        fe_store(out + 4 * column + 8 * row, w.lambda);
        fe_store(out + 5 * column + 8 * row, w.alpha);
        fe_store(out + 6 * column + 8 * row, w.beta);
        fe_store(out + 7 * column + 8 * row, w.gamma);
        fe_store(out + 8 * column + 8 * row, w.delta);
        fe_store(out + 2 * column + 8 * (row + 1), sum.x);
        fe_store(out + 3 * column + 8 * (row + 1), sum.y);
    }
    // overflow.rs:111-129 and lookup_range_check's running sum of s: s, s >> 0, s >> 10, ... s >> 130, eta = inv0(z_130)
    u32 *x = aux + 8 * 16 * i;
    fe two_130 = fe_zero();
    two_130.v[4] = 4u;
    const fe s = k_254 ? fe_add<FP>(alpha, fe_to_mont<FP>(two_130)) : alpha;
    fe_store(x, s);
    fe shifted = fe_from_mont<FP>(s);
#pragma unroll 1
    for (u32 w = 1; w < 15; w++) {
        fe_store(x + 8 * w, fe_to_mont<FP>(shifted));
#pragma unroll
        for (int j = 0; j < 7; j++) shifted.v[j] = (shifted.v[j] >> 10) | (shifted.v[j + 1] << 22);
        shifted.v[7] >>= 10;
    }
    fe_store(x + 8 * 15, fe_load(inv + 8 * (local * kScratch + kRounds + 1)));
}

StreamContexts<ScratchContext> g_ecc_ctxs;

}  // namespace

void ecc_release_workspaces() { g_ecc_ctxs.release_current_device(); }   // h2_trim

}  // namespace h2

using namespace h2;

extern "C" int h2_ecc_mul_device(const void *d_bases_xy, const void *d_scalars, size_t n, void *d_out_xy, void *d_status, void *stream) {
    if (n > kMaxMuls || (n && (!d_bases_xy || !d_scalars || !d_out_xy || !d_status))) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!n) return H2_OK;
    hipLaunchKernelGGL(ecc_mul, dim3(grid_of(n, kET)), dim3(kET), 0, (hipStream_t)stream, (const u32 *)d_bases_xy, (const u32 *)d_scalars, n,
                       (u32 *)d_out_xy, (uint8_t *)d_status);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

extern "C" int h2_ecc_mul_trace_device(const void *d_bases_xy, const void *d_alphas, size_t count, void *d_columns, void *d_aux,
                                       void *d_status, void *stream) {
    if (count > kMaxMuls || (count && (!d_bases_xy || !d_alphas || !d_columns || !d_aux || !d_status))) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!count) return H2_OK;
    hipStream_t st = (hipStream_t)stream;
    ScratchContext &ctx = g_ecc_ctxs.get(st);
    std::lock_guard<std::mutex> lk(ctx.mu);
    H2_HIP(hipMemsetAsync(d_columns, 0, (size_t)10 * kRows * count * 32, st));    // zero where the reference assigns nothing
    return two_pass_trace(ctx.scratch, count, kScratch, kTraceScratchRows, st, [&](bool emit, size_t first, size_t chunk, u32 *scratch) {
        hipLaunchKernelGGL(!emit ? ecc_mul_trace<false> : ecc_mul_trace<true>, dim3(grid_of(chunk, kET)), dim3(kET), 0, st,
                           (const u32 *)d_bases_xy, (const u32 *)d_alphas, first, chunk, count, scratch, (u32 *)d_columns, (uint8_t *)d_status);
        if (!emit) return H2_OK;
        H2_HIP(hipGetLastError());
        hipLaunchKernelGGL(ecc_mul_complete, dim3(grid_of(chunk, kET)), dim3(kET), 0, st, (const u32 *)d_bases_xy, (const u32 *)d_alphas, first,
                           chunk, count, (const u32 *)scratch, (u32 *)d_columns, (u32 *)d_aux);   // the rows pass B left to it, same chunk
        return H2_OK;
    });
}
