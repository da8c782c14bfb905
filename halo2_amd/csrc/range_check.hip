// The witness of the K = 10 lookup range check (halo2_gadgets utilities/lookup_range_check.rs), in bulk.
//
//   h2_range_check_trace_device         the running sums z_0 .. z_W of `count` values: W + 1 rows each
//   h2_short_range_check_trace_device   the three rows of a short range check: value, value 2^(K - s), 2^-s
//
// The reference divides in the field, z_{j+1} = (z_j - a_j) / 2^K with a_j the j-th K-bit word.  z_j - a_j is a multiple of 2^K as an
// integer below p, so the quotient is the integer's shift: z_j = value >> K j.  No inversion, one conversion to Montgomery form a cell.
//
// Both kernels are bound by their stores: 32 bytes out per cell for one multiplication.  ONE LANE PER OUTPUT ROW, not per value, so the
// lanes of a wave store 64 consecutive cells, 2 KiB in one piece; a lane per value would store its cells (W + 1) * 32 bytes from its
// neighbour's.  The price is that the W + 1 lanes of a value each read it again (an L2 hit) and shift it themselves.  The shift is a
// barrel shifter over the eight registers (three conditional moves by 4, 2 and 1 limbs, then one funnel shift a limb): no register is
// indexed by a variable, so nothing goes to scratch.  No LDS, no atomics; a lane owns its cell and the last lane of a value its status.
#include "common.h"
#include "field.cuh"

namespace h2 {
namespace {

constexpr int kPT = 256;                                 // lanes per workgroup
constexpr size_t kMaxValues = (size_t)1 << 30;           // values per call: count * 26 rows of 32 bytes stay far below 2^63
constexpr unsigned kK = 10;                              // sinsemilla::K, the lookup table's width in bits
constexpr unsigned kMaxWords = 25;                       // floor(CAPACITY / K) = floor(254 / 10)

// a >> s as a 256-bit integer, s < 256
__device__ __forceinline__ fe shift_right(fe a, u32 s) {
    const u32 limbs = s >> 5, bits = s & 31;
    if (limbs & 4) {
#pragma unroll
        for (int i = 0; i < 8; i++) a.v[i] = i + 4 < 8 ? a.v[i + 4] : 0;
    }
    if (limbs & 2) {
#pragma unroll
        for (int i = 0; i < 8; i++) a.v[i] = i + 2 < 8 ? a.v[i + 2] : 0;
    }
    if (limbs & 1) {
#pragma unroll
        for (int i = 0; i < 8; i++) a.v[i] = i + 1 < 8 ? a.v[i + 1] : 0;
    }
    fe r;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const u64 pair = ((u64)(i + 1 < 8 ? a.v[i + 1] : 0) << 32) | a.v[i];
        r.v[i] = (u32)(pair >> bits);
    }
    return r;
}

// a / 2 in the field (any form): (a + p) / 2 for an odd a; a + p < 2^256
template <int F> __device__ __forceinline__ fe fe_half(const fe &a) {
    const u32 odd = 0u - (a.v[0] & 1);
    u32 t[8];
    u32 carry = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) t[i] = __builtin_addc(a.v[i], mod_limb<F>(i) & odd, carry, &carry);
    fe r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = (t[i] >> 1) | ((i + 1 < 8 ? t[i + 1] : 0) << 31);
    return r;
}

// Row r of a launch is cell (r / per, r % per).  The 64-bit division is the workgroup's (uniform), the lane's is of a number below
// kPT + per.
__device__ __forceinline__ bool cell_of(size_t rows, u32 per, size_t &value, u32 &row) {
    const size_t first = (size_t)blockIdx.x * kPT;
    if (first + threadIdx.x >= rows) return false;
    const size_t value0 = first / per;
    const u32 t = (u32)(first - value0 * per) + threadIdx.x;
    value = value0 + t / per;
    row = t % per;
    return true;
}

template <int F> __global__ void __launch_bounds__(kPT) range_check_trace(const u32 *__restrict__ values, size_t count, u32 num_words,
                                                                          u32 *__restrict__ out_rows, unsigned char *__restrict__ status) {
    size_t i;
    u32 j;
    if (!cell_of(count * (num_words + 1), num_words + 1, i, j)) return;
    const fe z = shift_right(fe_load(values + 8 * i), kK * j);                // j <= 25: a shift of at most 250 bits
    fe_store(out_rows + 8 * (i * (num_words + 1) + j), fe_to_mont<F>(z));
    if (status && j == num_words) status[i] = !fe_is_zero(z);
}

#ifdef H2_AB
// The laboratory's other arm (H2_RANGE_CHECK_PER_VALUE=1, not in the product): one lane per VALUE, which reads its value once, shifts
// it ten bits a row and stores its W + 1 cells (W + 1) * 32 bytes from its neighbour's.  bench/tools/range_check_time.py times it
// beside the kernel above.
template <int F> __global__ void __launch_bounds__(kPT) range_check_trace_per_value(const u32 *__restrict__ values, size_t count, u32 num_words,
                                                                                    u32 *__restrict__ out_rows, unsigned char *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * kPT + threadIdx.x;
    if (i >= count) return;
    fe z = fe_load(values + 8 * i);
    u32 *out = out_rows + 8 * i * (num_words + 1);
#pragma unroll 1
    for (u32 j = 0; j < num_words; j++) {
        fe_store(out + 8 * j, fe_to_mont<F>(z));
        z = shift_right(z, kK);
    }
    fe_store(out + 8 * num_words, fe_to_mont<F>(z));
    if (status) status[i] = !fe_is_zero(z);
}
#endif

template <int F> __global__ void __launch_bounds__(kPT) short_range_check_trace(const u32 *__restrict__ values, size_t count, u32 num_bits,
                                                                                u32 *__restrict__ out_rows, unsigned char *__restrict__ status) {
    size_t i;
    u32 j;
    if (!cell_of(count * 3, 3, i, j)) return;
    const fe v = fe_load(values + 8 * i);
    fe r = j == 2 ? fe_one<F>() : fe_to_mont<F>(v);
    // row 1: the field's value 2^(K - s) by doublings (a value above K bits still gives the product the gate checks);
    // row 2: 2^-s by halvings of one.  num_bits is uniform, at most ten steps either way.
    if (j == 1) {
#pragma unroll 1
        for (u32 k = num_bits; k < kK; k++) r = fe_dbl<F>(r);
    } else if (j == 2) {
#pragma unroll 1
        for (u32 k = 0; k < num_bits; k++) r = fe_half<F>(r);
    }
    fe_store(out_rows + 8 * (3 * i + j), r);
    if (status && j == 0) status[i] = ((v.v[0] >> num_bits) | v.v[1] | v.v[2] | v.v[3] | v.v[4] | v.v[5] | v.v[6] | v.v[7]) != 0;
}

inline unsigned grid_of(size_t rows) { return (unsigned)((rows + kPT - 1) / kPT); }

}  // namespace
}  // namespace h2

using namespace h2;

extern "C" int h2_range_check_trace_device(int field, const void *d_values, size_t count, unsigned num_words, void *d_rows, void *d_status,
                                           void *stream) {
    if ((field != H2_FP && field != H2_FQ) || num_words < 1 || num_words > kMaxWords || count > kMaxValues || (count && (!d_values || !d_rows)))
        return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!count) return H2_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(grid_of(count * (num_words + 1)));
#ifdef H2_AB
    static const bool per_value = [] { const char *e = ab_env("H2_RANGE_CHECK_PER_VALUE"); return e && e[0] == '1'; }();
    if (per_value) {
        if (field == H2_FP)
            hipLaunchKernelGGL((range_check_trace_per_value<FP>), dim3(grid_of(count)), dim3(kPT), 0, st, (const u32 *)d_values, count,
                               (u32)num_words, (u32 *)d_rows, (unsigned char *)d_status);
        else
            hipLaunchKernelGGL((range_check_trace_per_value<FQ>), dim3(grid_of(count)), dim3(kPT), 0, st, (const u32 *)d_values, count,
                               (u32)num_words, (u32 *)d_rows, (unsigned char *)d_status);
        H2_HIP(hipGetLastError());
        return H2_OK;
    }
#endif
    if (field == H2_FP)
        hipLaunchKernelGGL((range_check_trace<FP>), grid, dim3(kPT), 0, st, (const u32 *)d_values, count, (u32)num_words, (u32 *)d_rows,
                           (unsigned char *)d_status);
    else
        hipLaunchKernelGGL((range_check_trace<FQ>), grid, dim3(kPT), 0, st, (const u32 *)d_values, count, (u32)num_words, (u32 *)d_rows,
                           (unsigned char *)d_status);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

extern "C" int h2_short_range_check_trace_device(int field, const void *d_values, size_t count, unsigned num_bits, void *d_rows,
                                                 void *d_status, void *stream) {
    if ((field != H2_FP && field != H2_FQ) || num_bits > kK || count > kMaxValues || (count && (!d_values || !d_rows))) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!count) return H2_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(grid_of(count * 3));
    if (field == H2_FP)
        hipLaunchKernelGGL((short_range_check_trace<FP>), grid, dim3(kPT), 0, st, (const u32 *)d_values, count, (u32)num_bits, (u32 *)d_rows,
                           (unsigned char *)d_status);
    else
        hipLaunchKernelGGL((short_range_check_trace<FQ>), grid, dim3(kPT), 0, st, (const u32 *)d_values, count, (u32)num_bits, (u32 *)d_rows,
                           (unsigned char *)d_status);
    H2_HIP(hipGetLastError());
    return H2_OK;
}
