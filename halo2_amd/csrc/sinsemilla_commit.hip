// Sinsemilla commitments and hashing from a private point over Pallas (Zcash protocol specification 5.4.8.4; halo2_gadgets
// src/sinsemilla.rs CommitDomain, sinsemilla/chip/hash_to_point.rs hash_message_with_private_init), batched: one lane per message.
//
//   h2_sinsemilla_hash_from_device    h2_sinsemilla_hash_device with one initial point Q_i per message, read from device memory
//   h2_sinsemilla_commit_device       SinsemillaHashToPoint(Q, M_i) + [r_i]R in one launch and one inversion per lane
//   h2_sinsemilla_trace_from_device   the witness of a hash whose Q is a cell: the rows of h2_sinsemilla_trace_device from Q_i, under
//                                     one more row that holds y_Q
//   h2_ecc_add_trace_device           n complete additions P_i + Q_i with their add.rs witness rows
//
// A commitment runs two chains on the lane, one after the other: the Sinsemilla rounds (hash_chain, sinsemilla_chain.cuh, 18
// multiplications a word) to the hash M, which stays in XYZZ, then the 85-window sum of the fixed-base product over R's table
// (fixed_base_chain, ecc_fixed_chain.cuh, 10 multiplications a window, the last addition complete).  The two meet in the complete
// add-2008-s and the lane inverts once, where the composition hash -> mul_fixed -> add inverts three times and launches three
// kernels.  Only the HASH can be bottom: the final addition is the group's, so M = [r]R doubles and M = -[r]R is the identity with
// status 0.
//
// The trace is sinsemilla.hip's -- the same kernel body (trace_chain, sinsemilla_chain.cuh) from a Q per message and under one more
// row, the same two passes around h2_batch_invert_device (two_pass_trace, common.h) -- with the same budget of scratch rows per chunk.
#include "common.h"
#include "ecc_add.cuh"
#include "ecc_fixed_chain.cuh"
#include "sinsemilla_chain.cuh"

namespace h2 {
namespace {

constexpr int kCT = 256;                                   // lanes per workgroup
constexpr size_t kMaxMessages = (size_t)1 << 30;
constexpr u32 kCommitWindows = 85;                         // NUM_WINDOWS of a full-width scalar: the blinding factor's
constexpr size_t kTraceScratchRows = (size_t)1 << 20;      // rows per chunk of the trace, as sinsemilla.hip: 32 MiB of scratch

__global__ void __launch_bounds__(kCT) sinsemilla_hash_from(const uint16_t *__restrict__ words, size_t n, u32 n_words,
                                                            const u32 *__restrict__ q_xy, const u32 *__restrict__ table,
                                                            u32 *__restrict__ out_xy, uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * kCT + threadIdx.x;
    if (i >= n) return;
    bool bottom;
    xyzz<FP> a = start_at(q_xy + 16 * i, bottom);
    hash_chain(a, bottom, words + i * (size_t)n_words, n_words, table);
    store_point(out_xy, status, i, xyzz_to_affine<FP>(a), bottom);
}

// q_dev: one Q per message, or null for the shared q.  r_points is R's window table of kCommitWindows rows.
__global__ void __launch_bounds__(kCT) sinsemilla_commit(const uint16_t *__restrict__ words, size_t n, u32 n_words, PointArg q,
                                                         const u32 *__restrict__ q_dev, const u32 *__restrict__ table,
                                                         const u32 *__restrict__ r_points, const u32 *__restrict__ scalars,
                                                         u32 *__restrict__ out_xy, uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * kCT + threadIdx.x;
    if (i >= n) return;
    bool bottom;
    xyzz<FP> m = q_dev ? start_at(q_dev + 16 * i, bottom) : start_at(q, bottom);
    hash_chain(m, bottom, words + i * (size_t)n_words, n_words, table);
    u32 k[8];
    load_scalar(scalars, i, k);
    xyzz<FP> acc = fixed_base_chain(r_points, kCommitWindows, k);
    xyzz_add<FP>(acc, m);                                  // complete; a bottom hash is reported below, whatever this gave
    store_point(out_xy, status, i, xyzz_to_affine<FP>(acc), bottom);
}

// The two passes of sinsemilla.hip's trace from Q_i, under one more row that holds y_Q (trace_chain with LEAD = 1, sinsemilla_chain.cuh).
template <bool EMIT>
__global__ void __launch_bounds__(kCT) sinsemilla_trace_from(const u32 *__restrict__ pieces, size_t first, size_t chunk, size_t count,
                                                             u32 n_pieces, u32 rows, PieceWords nw, const u32 *__restrict__ q_xy,
                                                             const u32 *__restrict__ table, u32 *__restrict__ inv,
                                                             u32 *__restrict__ columns, uint8_t *__restrict__ status) {
    const size_t local = (size_t)blockIdx.x * kCT + threadIdx.x;
    if (local >= chunk) return;
    bool bottom;
    const xyzz<FP> a = start_at(q_xy + 16 * (first + local), bottom);
    trace_chain<EMIT, 1>(pieces, local, first + local, count, n_pieces, rows, nw, a, bottom, table, inv, columns, status);
}

// aux: x_p y_p x_qr y_qr lambda alpha beta gamma delta x_r y_r, the order of h2_ecc_mul_fixed_trace_device's d_aux
__global__ void __launch_bounds__(kCT) ecc_add_trace(const u32 *__restrict__ p_xy, const u32 *__restrict__ q_xy, size_t n,
                                                     u32 *__restrict__ aux) {
    const size_t i = (size_t)blockIdx.x * kCT + threadIdx.x;
    if (i >= n) return;
    const affine<FP> p = aff_load<FP>(p_xy + 16 * i), q = aff_load<FP>(q_xy + 16 * i);
    AddWitness wit;
    const affine<FP> sum = complete_add(p, q, wit);
    store_add_aux(aux + 8 * 11 * i, p, q, wit, sum);
}

StreamContexts<ScratchContext> g_commit_ctxs;

}  // namespace

void sinsemilla_commit_release_workspaces() { g_commit_ctxs.release_current_device(); }   // h2_trim

}  // namespace h2

using namespace h2;

extern "C" int h2_sinsemilla_hash_from_device(const void *d_words, size_t n, size_t words, const void *d_q_xy, const void *d_table,
                                              void *d_out_xy, void *d_status, void *stream) {
    if (words > kC || n > kMaxMessages || (n && (!d_q_xy || !d_table || !d_out_xy || !d_status || (words && !d_words)))) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!n) return H2_OK;
    hipLaunchKernelGGL(sinsemilla_hash_from, dim3(grid_of(n, kCT)), dim3(kCT), 0, (hipStream_t)stream, (const uint16_t *)d_words, n, (u32)words,
                       (const u32 *)d_q_xy, (const u32 *)d_table, (u32 *)d_out_xy, (uint8_t *)d_status);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

extern "C" int h2_sinsemilla_commit_device(const void *d_words, size_t n, size_t words, const uint64_t *q_xy, const void *d_q_xy,
                                           const void *d_table, const void *d_r_points, const void *d_scalars, void *d_out_xy,
                                           void *d_status, void *stream) {
    if (words > kC || n > kMaxMessages || !q_xy == !d_q_xy) return H2_ERR_ARGS;
    if (n && (!d_table || !d_r_points || !d_scalars || !d_out_xy || !d_status || (words && !d_words))) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!n) return H2_OK;
    const PointArg q = q_xy ? point_arg(q_xy) : PointArg{};
    hipLaunchKernelGGL(sinsemilla_commit, dim3(grid_of(n, kCT)), dim3(kCT), 0, (hipStream_t)stream, (const uint16_t *)d_words, n, (u32)words, q,
                       (const u32 *)d_q_xy, (const u32 *)d_table, (const u32 *)d_r_points, (const u32 *)d_scalars, (u32 *)d_out_xy,
                       (uint8_t *)d_status);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

extern "C" int h2_sinsemilla_trace_from_device(const void *d_pieces, size_t count, const uint32_t *num_words, size_t n_pieces,
                                               const void *d_q_xy, const void *d_table, void *d_columns, void *d_status, void *stream) {
    PieceWords nw;
    size_t total;
    if (!piece_words(num_words, n_pieces, nw, total) || count > kMaxMessages) return H2_ERR_ARGS;
    if (count && (!d_pieces || !d_q_xy || !d_table || !d_columns || !d_status)) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!count) return H2_OK;
    const u32 rows = (u32)total + 2;                       // at most 255; rows - 1 of them need an inverse
    hipStream_t st = (hipStream_t)stream;
    ScratchContext &ctx = g_commit_ctxs.get(st);
    std::lock_guard<std::mutex> lk(ctx.mu);
    // a chunk is kTraceScratchRows / rows messages: the budget counts a message's rows, y_Q's among them, not its rows - 1 elements
    return two_pass_trace(ctx.scratch, count, rows - 1, kTraceScratchRows / rows * (rows - 1), st,
                          [&](bool emit, size_t first, size_t chunk, u32 *scratch) {
        hipLaunchKernelGGL(!emit ? sinsemilla_trace_from<false> : sinsemilla_trace_from<true>, dim3(grid_of(chunk, kCT)), dim3(kCT), 0, st,
                           (const u32 *)d_pieces, first, chunk, count, (u32)n_pieces, rows, nw, (const u32 *)d_q_xy, (const u32 *)d_table,
                           scratch, (u32 *)d_columns, (uint8_t *)d_status);
        return H2_OK;
    });
}

extern "C" int h2_ecc_add_trace_device(const void *d_p_xy, const void *d_q_xy, size_t n, void *d_aux, void *stream) {
    if (n > kMaxMessages || (n && (!d_p_xy || !d_q_xy || !d_aux))) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!n) return H2_OK;
    hipLaunchKernelGGL(ecc_add_trace, dim3(grid_of(n, kCT)), dim3(kCT), 0, (hipStream_t)stream, (const u32 *)d_p_xy, (const u32 *)d_q_xy, n,
                       (u32 *)d_aux);
    H2_HIP(hipGetLastError());
    return H2_OK;
}
