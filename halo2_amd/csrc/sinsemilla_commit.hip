// Sinsemilla commitments and hashing from a private point over Pallas (Zcash protocol specification 5.4.8.4; halo2_gadgets
// src/sinsemilla.rs CommitDomain, sinsemilla/chip/hash_to_point.rs hash_message_with_private_init), batched: one lane per message.
//
//   h2_sinsemilla_hash_from_device    h2_sinsemilla_hash_device with one initial point Q_i per message, read from device memory
//   h2_sinsemilla_commit_device       SinsemillaHashToPoint(Q, M_i) + [r_i]R in one launch and one inversion per lane
//   h2_sinsemilla_trace_from_device   the witness of a hash whose Q is a cell: the rows of h2_sinsemilla_trace_device from Q_i, under
//                                     one more row that holds y_Q
//   h2_ecc_add_trace_device           n complete additions P_i + Q_i with their add.rs witness rows
//
// A commitment runs two chains on the lane, one after the other: the Sinsemilla rounds (sinsemilla_round.cuh, 18 multiplications a
// word) to the hash M, which stays in XYZZ, then the 85-window sum of the fixed-base product over R's table (ecc_fixed_chain.cuh, 10
// multiplications a window, the last addition complete).  The two meet in the complete add-2008-s and the lane inverts once, where the
// composition hash -> mul_fixed -> add inverts three times and launches three kernels.  Only the HASH can be bottom: the final
// addition is the group's, so M = [r]R doubles and M = -[r]R is the identity with status 0.
//
// The trace keeps the two-pass scheme of sinsemilla.hip -- pass A stores one product of denominators per row, h2_batch_invert_device
// inverts them, pass B runs the chain again and emits -- with the same budget of scratch rows per chunk.
#include "common.h"
#include "ecc_add.cuh"
#include "ecc_fixed_chain.cuh"
#include "sinsemilla_round.cuh"

#include <string.h>

namespace h2 {
namespace {

constexpr int kCT = 256;                                   // lanes per workgroup
constexpr size_t kMaxMessages = (size_t)1 << 30;
constexpr u32 kCommitWindows = 85;                         // NUM_WINDOWS of a full-width scalar: the blinding factor's
constexpr size_t kTraceScratchRows = (size_t)1 << 20;      // rows per chunk of the trace, as sinsemilla.hip: 32 MiB of scratch

__device__ __forceinline__ void hash_chain(xyzz<FP> &a, bool &bottom, const uint16_t *m, u32 n_words, const u32 *table) {
#pragma unroll 1
    for (u32 w = 0; w < n_words; w++) {
        const u32 word = m[w] & kWordMask;                 // the mask keeps the gather inside the table whatever the caller sent
        const affine<FP> s = aff_load<FP>(table + 16 * (size_t)word);
        fe p, r, d, zz_r;
        sinsemilla_round(a, s, p, r, d, zz_r);
        bottom = bottom || fe_is_zero(p) || fe_is_zero(d);
    }
}

__device__ __forceinline__ void store_point(u32 *out_xy, uint8_t *status, size_t i, affine<FP> res, bool bottom) {
    if (bottom) res.x = res.y = fe_zero();
    fe_store(out_xy + 16 * i, res.x);
    fe_store(out_xy + 16 * i + 8, res.y);
    status[i] = bottom ? 1 : 0;
}

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
    xyzz<FP> acc = xyzz_of(aff_load<FP>(table_entry(r_points, 0, take_window(k), 16)));
#pragma unroll 1
    for (u32 w = 1; w + 1 < kCommitWindows; w++) xyzz_madd_incomplete(acc, aff_load<FP>(table_entry(r_points, w, take_window(k), 16)));
    xyzz_madd<FP>(acc, aff_load<FP>(table_entry(r_points, kCommitWindows - 1, take_window(k), 16)));
    xyzz_add<FP>(acc, m);                                  // complete; a bottom hash is reported below, whatever this gave
    store_point(out_xy, status, i, xyzz_to_affine<FP>(acc), bottom);
}

// The two passes of sinsemilla.hip's trace from Q_i, with the message's rows moved down by one: row 0 holds y_Q in x_p
// (hash_to_point.rs:117-121, :179-182), the round rows and the closing row follow.  inv holds rows - 1 elements per message.
template <bool EMIT>
__global__ void __launch_bounds__(kCT) sinsemilla_trace_from(const u32 *__restrict__ pieces, size_t first, size_t chunk, size_t count,
                                                             u32 n_pieces, u32 rows, PieceWords nw, const u32 *__restrict__ q_xy,
                                                             const u32 *__restrict__ table, u32 *__restrict__ inv,
                                                             u32 *__restrict__ columns, uint8_t *__restrict__ status) {
    const size_t local = (size_t)blockIdx.x * kCT + threadIdx.x;
    if (local >= chunk) return;
    const size_t i = first + local;
    bool bottom;
    xyzz<FP> a = start_at(q_xy + 16 * i, bottom);
    u32 *t = inv + 8 * (local * (rows - 1));
    const size_t column = 8 * (size_t)rows * count;
    u32 *out = columns + 8 * (i * rows);                   // row 0 of this message in column 0 (x_a)
    if (EMIT) {
        fe_store(out, fe_zero());
        fe_store(out + column, a.y);
        fe_store(out + 2 * column, fe_zero());
        fe_store(out + 3 * column, fe_zero());
        fe_store(out + 4 * column, fe_zero());
    }
    out += 8;
    u32 row = 0;
#pragma unroll 1
    for (u32 k = 0; k < n_pieces; k++) {
        u32 z[8];
        {
            const fe piece = fe_load(pieces + 8 * (i * n_pieces + k));
#pragma unroll
            for (int j = 0; j < 8; j++) z[j] = piece.v[j];
        }
#pragma unroll 1
        for (u32 w = 0; w < nw.n[k]; w++, row++) {
            const u32 word = z[0] & kWordMask;
            const affine<FP> s = aff_load<FP>(table + 16 * (size_t)word);
            const xyzz<FP> before = a;
            fe p, r, d, zz_r;
            sinsemilla_round(a, s, p, r, d, zz_r);
            bottom = bottom || fe_is_zero(p) || fe_is_zero(d);
            const fe zed = fe_mulx<FP>(before.zz, before.zzz);
            if (!EMIT) {
                fe_store(t + 8 * row, fe_mulx<FP>(fe_mulx<FP>(zed, p), d));
            } else {
                const fe all = fe_load(t + 8 * row);                                       // 1 / (ZZ ZZZ P D)
                const fe i_zed = fe_mulx<FP>(all, fe_mulx<FP>(p, d)), az = fe_mulx<FP>(all, zed);
                const fe i_p = fe_mulx<FP>(az, d), i_d = fe_mulx<FP>(az, p);
                const fe i_zzz = fe_mulx<FP>(before.zz, i_zed);
                const fe x_a = fe_mulx<FP>(before.x, fe_mulx<FP>(before.zzz, i_zed));
                const fe lambda_1 = fe_mulx<FP>(fe_mulx<FP>(r, i_zzz), fe_mulx<FP>(before.zz, i_p));
                const fe y_a = fe_mulx<FP>(before.y, i_zzz);
                const fe lambda_2 = fe_sub<FP>(fe_mulx<FP>(fe_dbl<FP>(y_a), fe_mulx<FP>(zz_r, i_d)), lambda_1);
                fe zf;
#pragma unroll
                for (int j = 0; j < 8; j++) zf.v[j] = z[j];
                fe_store(out + 8 * row, x_a);
                fe_store(out + column + 8 * row, s.x);
                fe_store(out + 2 * column + 8 * row, fe_to_mont<FP>(zf));
                fe_store(out + 3 * column + 8 * row, lambda_1);
                fe_store(out + 4 * column + 8 * row, lambda_2);
            }
            shift_right_k(z);
        }
    }
    const fe zed = fe_mulx<FP>(a.zz, a.zzz);
    if (!EMIT) {
        fe_store(t + 8 * row, zed);
    } else {
        const fe i_zed = fe_load(t + 8 * row);
        fe_store(out + 8 * row, fe_mulx<FP>(a.x, fe_mulx<FP>(a.zzz, i_zed)));
        fe_store(out + column + 8 * row, fe_zero());
        fe_store(out + 2 * column + 8 * row, fe_zero());
        fe_store(out + 3 * column + 8 * row, fe_mulx<FP>(a.y, fe_mulx<FP>(a.zz, i_zed)));  // y_a
        fe_store(out + 4 * column + 8 * row, fe_zero());
        status[i] = bottom ? 1 : 0;
    }
}

// aux: x_p y_p x_qr y_qr lambda alpha beta gamma delta x_r y_r, the order of h2_ecc_mul_fixed_trace_device's d_aux
__global__ void __launch_bounds__(kCT) ecc_add_trace(const u32 *__restrict__ p_xy, const u32 *__restrict__ q_xy, size_t n,
                                                     u32 *__restrict__ aux) {
    const size_t i = (size_t)blockIdx.x * kCT + threadIdx.x;
    if (i >= n) return;
    const affine<FP> p = aff_load<FP>(p_xy + 16 * i), q = aff_load<FP>(q_xy + 16 * i);
    AddWitness wit;
    const affine<FP> sum = complete_add(p, q, wit);
    u32 *x = aux + 8 * 11 * i;
    fe_store(x, p.x);
    fe_store(x + 8, p.y);
    fe_store(x + 16, q.x);
    fe_store(x + 24, q.y);
    fe_store(x + 32, wit.lambda);
    fe_store(x + 40, wit.alpha);
    fe_store(x + 48, wit.beta);
    fe_store(x + 56, wit.gamma);
    fe_store(x + 64, wit.delta);
    fe_store(x + 72, sum.x);
    fe_store(x + 80, sum.y);
}

struct SinsemillaCommitContext {
    std::mutex mu;
    DevBuf scratch;
    void release_all() { scratch.release(); }
};
StreamContexts<SinsemillaCommitContext> g_commit_ctxs;

inline unsigned grid_of(size_t n) { return (unsigned)((n + kCT - 1) / kCT); }

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
    hipLaunchKernelGGL(sinsemilla_hash_from, dim3(grid_of(n)), dim3(kCT), 0, (hipStream_t)stream, (const uint16_t *)d_words, n, (u32)words,
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
    PointArg q = {};
    if (q_xy) {
        memcpy(q.x, q_xy, 32);
        memcpy(q.y, q_xy + 4, 32);
    }
    hipLaunchKernelGGL(sinsemilla_commit, dim3(grid_of(n)), dim3(kCT), 0, (hipStream_t)stream, (const uint16_t *)d_words, n, (u32)words, q,
                       (const u32 *)d_q_xy, (const u32 *)d_table, (const u32 *)d_r_points, (const u32 *)d_scalars, (u32 *)d_out_xy,
                       (uint8_t *)d_status);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

extern "C" int h2_sinsemilla_trace_from_device(const void *d_pieces, size_t count, const uint32_t *num_words, size_t n_pieces,
                                               const void *d_q_xy, const void *d_table, void *d_columns, void *d_status, void *stream) {
    if (!num_words || n_pieces == 0 || n_pieces > kC || count > kMaxMessages) return H2_ERR_ARGS;
    PieceWords nw = {};
    size_t total = 0;
    for (size_t k = 0; k < n_pieces; k++) {
        if (num_words[k] == 0 || num_words[k] > kMaxPieceWords) return H2_ERR_ARGS;
        nw.n[k] = (uint8_t)num_words[k];
        total += num_words[k];
    }
    if (total > kC || (count && (!d_pieces || !d_q_xy || !d_table || !d_columns || !d_status))) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!count) return H2_OK;
    const size_t rows = total + 2, per_chunk = kTraceScratchRows / rows;          // rows <= 255; rows - 1 of them need an inverse
    hipStream_t st = (hipStream_t)stream;
    SinsemillaCommitContext &ctx = g_commit_ctxs.get(st);
    std::lock_guard<std::mutex> lk(ctx.mu);
    const size_t widest = count < per_chunk ? count : per_chunk;
    if ((rc = ctx.scratch.reserve(widest * (rows - 1) * 32)) != H2_OK) return rc;
    for (size_t first = 0; first < count; first += per_chunk) {
        const size_t chunk = count - first < per_chunk ? count - first : per_chunk;
        hipLaunchKernelGGL(sinsemilla_trace_from<false>, dim3(grid_of(chunk)), dim3(kCT), 0, st, (const u32 *)d_pieces, first, chunk, count,
                           (u32)n_pieces, (u32)rows, nw, (const u32 *)d_q_xy, (const u32 *)d_table, ctx.scratch.as<u32>(), (u32 *)d_columns,
                           (uint8_t *)d_status);
        H2_HIP(hipGetLastError());
        if ((rc = h2_batch_invert_device(H2_FP, ctx.scratch.ptr, chunk * (rows - 1), H2_FORM_MONTGOMERY, stream)) != H2_OK) return rc;
        hipLaunchKernelGGL(sinsemilla_trace_from<true>, dim3(grid_of(chunk)), dim3(kCT), 0, st, (const u32 *)d_pieces, first, chunk, count,
                           (u32)n_pieces, (u32)rows, nw, (const u32 *)d_q_xy, (const u32 *)d_table, ctx.scratch.as<u32>(), (u32 *)d_columns,
                           (uint8_t *)d_status);
        H2_HIP(hipGetLastError());
    }
    return H2_OK;
}

extern "C" int h2_ecc_add_trace_device(const void *d_p_xy, const void *d_q_xy, size_t n, void *d_aux, void *stream) {
    if (n > kMaxMessages || (n && (!d_p_xy || !d_q_xy || !d_aux))) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!n) return H2_OK;
    hipLaunchKernelGGL(ecc_add_trace, dim3(grid_of(n)), dim3(kCT), 0, (hipStream_t)stream, (const u32 *)d_p_xy, (const u32 *)d_q_xy, n,
                       (u32 *)d_aux);
    H2_HIP(hipGetLastError());
    return H2_OK;
}
