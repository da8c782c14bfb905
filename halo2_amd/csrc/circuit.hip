// Selector compression (plonk/circuit.rs:1237-1343, plonk/circuit/compress_selectors.rs:51-227): the two parts that scale with the
// circuit.  The greedy grouping itself is a few hundred host operations (halo2_amd/compress_selectors.py); what costs S^2 * n in the
// reference is the exclusion matrix (:103-124, one pass over two activation vectors per pair), and what costs S * n is writing the
// combined columns (:180-213).
//
//   h2_selector_conflicts_device   one workgroup per pair (i, j <= i): lanes stride over the bit-packed words of both selectors
//                                  (coalesced 4 or 16 bytes per lane), OR the ANDs, the workgroup reduces with one barrier vote
//   h2_selector_combine_device     one lane per (column, row): the root of the selector of that column enabled on the row, in
//                                  Montgomery form, 32-byte vector stores; no atomics (a lane owns its element)
#include "common.h"
#include "field.cuh"

namespace h2 {
namespace {

constexpr int kCT = 256;                                 // lanes per workgroup, as in poly.hip
constexpr size_t kMaxSelectors = 4096;                   // S * S bytes of matrix, S * S workgroups
constexpr size_t kMaxRows = (size_t)1 << 30;

// blockIdx.x = i, blockIdx.y = j; the workgroups above the diagonal leave at once, (i, j <= i) writes both (i, j) and (j, i)
__global__ void __launch_bounds__(kCT) selector_conflicts(const u32 *__restrict__ bits, u32 n_selectors, size_t n_words, int vec4,
                                                         uint8_t *__restrict__ out) {
    const u32 i = blockIdx.x, j = blockIdx.y;
    if (j > i) return;
    u32 acc = 0;
    if (j < i) {
        const u32 *a = bits + (size_t)i * n_words, *b = bits + (size_t)j * n_words;
        if (vec4) {                                       // n_words % 4 == 0 and a 16-byte aligned base: every row is aligned
            const uint4 *a4 = reinterpret_cast<const uint4 *>(a), *b4 = reinterpret_cast<const uint4 *>(b);
            for (size_t w = threadIdx.x; w < n_words / 4; w += kCT) {
                const uint4 x = a4[w], y = b4[w];
                acc |= (x.x & y.x) | (x.y & y.y) | (x.z & y.z) | (x.w & y.w);
            }
        } else {
            for (size_t w = threadIdx.x; w < n_words; w += kCT) acc |= a[w] & b[w];
        }
    }
    const int any = __syncthreads_or(acc != 0);
    if (threadIdx.x == 0) {
        out[(size_t)i * n_selectors + j] = (uint8_t)(any ? 1 : 0);
        out[(size_t)j * n_selectors + i] = (uint8_t)(any ? 1 : 0);
    }
}

// blockIdx.y = column c, one lane per row
template <int F>
__global__ void __launch_bounds__(kCT) selector_combine(const u32 *__restrict__ bits, const u32 *__restrict__ root_of, const u32 *__restrict__ column_of,
                                                       u32 n_selectors, size_t n, size_t n_words, u32 *__restrict__ out) {
    const size_t r = (size_t)blockIdx.x * kCT + threadIdx.x;
    const u32 c = blockIdx.y;
    if (r >= n) return;
    u32 root = 0;
    for (u32 s = 0; s < n_selectors; ++s) {
        if (column_of[s] != c) continue;                  // uniform over the workgroup
        if ((bits[(size_t)s * n_words + (r >> 5)] >> (r & 31)) & 1) root = root_of[s];
    }
    fe v = fe_zero();
    if (root) v = fe_to_mont<F>(fe{{root, 0, 0, 0, 0, 0, 0, 0}});
    fe_store(out + 8 * ((size_t)c * n + r), v);
}

}  // namespace
}  // namespace h2

using namespace h2;

extern "C" int h2_selector_conflicts_device(const uint32_t *bits, size_t n_selectors, size_t n_words, uint8_t *out, void *stream) {
    if (n_selectors > kMaxSelectors || n_words > kMaxRows / 32 || (n_selectors && (!out || (n_words && !bits)))) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!n_selectors) return H2_OK;
    const int vec4 = (n_words % 4 == 0) && (reinterpret_cast<uintptr_t>(bits) % 16 == 0);
    hipLaunchKernelGGL(selector_conflicts, dim3((unsigned)n_selectors, (unsigned)n_selectors), dim3(kCT), 0, (hipStream_t)stream, bits,
                       (u32)n_selectors, n_words, vec4, out);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

extern "C" int h2_selector_combine_device(int field, const uint32_t *bits, const uint32_t *root_of_selector, const uint32_t *column_of_selector,
                                          size_t n_selectors, size_t n, void *out_columns, size_t n_columns, void *stream) {
    if ((field != H2_FP && field != H2_FQ) || n_selectors > kMaxSelectors || n_columns > kMaxSelectors || n > kMaxRows ||
        (n_columns && n && !out_columns) || (n_selectors && n && (!bits || !root_of_selector || !column_of_selector)))
        return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!n_columns || !n) return H2_OK;
    const size_t n_words = (n + 31) / 32;
    const dim3 grid((unsigned)((n + kCT - 1) / kCT), (unsigned)n_columns);
    if (field == H2_FP)
        hipLaunchKernelGGL((selector_combine<FP>), grid, dim3(kCT), 0, (hipStream_t)stream, bits, root_of_selector, column_of_selector,
                           (u32)n_selectors, n, n_words, (u32 *)out_columns);
    else
        hipLaunchKernelGGL((selector_combine<FQ>), grid, dim3(kCT), 0, (hipStream_t)stream, bits, root_of_selector, column_of_selector,
                           (u32)n_selectors, n, n_words, (u32 *)out_columns);
    H2_HIP(hipGetLastError());
    return H2_OK;
}
