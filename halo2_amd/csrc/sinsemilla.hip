// Sinsemilla over Pallas (Zcash protocol specification 5.4.1.9; halo2_gadgets/src/sinsemilla.rs, sinsemilla/chip/hash_to_point.rs), batched:
// one lane per message.
//
//   h2_sinsemilla_hash_device    n messages of `words` 10-bit words -> n affine points, with the specification's INCOMPLETE addition:
//                                a message whose chain meets equal or opposite operands is reported (status 1, the reference's bottom)
//   h2_sinsemilla_merkle_layer_device   MerkleCRH of n pairs of field elements: the 52 words are cut on the lane
//   h2_sinsemilla_trace_device   what SinsemillaChip::hash_message witnesses for `count` messages of one piece structure: the columns
//                                x_a, x_p, bits, lambda_1, lambda_2
//
// A hash is the chain Acc <- (Acc + S(m_i)) + Acc over the message's words, Acc_0 = Q.  The accumulator stays in XYZZ coordinates
// (curve.cuh) and a round is 18 multiplications: R = Acc + S is the mixed addition (8M + 2S), whose by-products put Acc on R's
// denominators for free -- Acc = (X PP, Y PPP) over (ZZ PP, ZZZ PPP), both numerators already formed -- so R + Acc is an addition of two
// points with one denominator (6M + 2S).  Its two differences are exactly what incomplete addition must not see vanish:
//     P = x_p ZZ - X          = 0  <=>  Acc and S(m_i) share their x (a doubling or an inverse pair)
//     D = X PP - X_R          = 0  <=>  R and Acc share theirs
// and with both nonzero no sum is the identity.  The hash inverts once per message, at the end.
//
// The trace needs affine values on every row -- x_a, lambda_1 = (y_a - y_p) / (x_a - x_p), lambda_2 = 2 y_a / (x_a - x_r) - lambda_1 --
// that is the inverses of ZZ ZZZ, P and D of every round.  No lane inverts inside its chain (an inversion is ~130 multiplications on
// the lane's dependent path against 18 for the round): pass A runs the projective chain and stores ONE element per row, the product
// ZZ ZZZ P D; h2_batch_invert_device inverts them all; pass B runs the chain again, splits each inverse three ways and emits the
// row (32 multiplications).  Running the chain twice costs less than storing and reloading the six elements per row that pass B would
// otherwise need, and keeps the scratch at 32 bytes per row; messages go through in chunks so it stays under kTraceScratchRows rows.
//
// The 1024-point table S (64 KiB, Montgomery affine) is gathered from global memory, 64 bytes per lane and round; it is read by
// every lane of every launch and stays in L2.
#include "common.h"
#include "curve.cuh"
#include "sinsemilla_round.cuh"

#include <string.h>

namespace h2 {
namespace {

constexpr int kST = 256;                                   // lanes per workgroup
constexpr size_t kMaxMessages = (size_t)1 << 30;
constexpr size_t kTraceScratchRows = (size_t)1 << 20;      // rows of scratch per chunk of the trace: 32 MiB

// LDS_TABLE is the other placement of the table, kept as a laboratory arm (H2_SINSEMILLA_LDS in the ab build): every workgroup copies
// the 64 KiB into LDS first and gathers from there.  It caps a CU at two workgroups and pays the copy per workgroup; measured beside
// the global gather in profiles/sinsemilla.txt.
template <bool LDS_TABLE>
__global__ void __launch_bounds__(kST) sinsemilla_hash(const uint16_t *__restrict__ words, size_t n, u32 n_words, PointArg q,
                                                       const u32 *__restrict__ table, u32 *__restrict__ out_xy,
                                                       uint8_t *__restrict__ status) {
    extern __shared__ uint4 lds_table[];
    if (LDS_TABLE) {
        const uint4 *src = reinterpret_cast<const uint4 *>(table);
        for (u32 at = threadIdx.x; at < kTableBytes / 16; at += kST) lds_table[at] = src[at];
        __syncthreads();
    }
    const size_t i = (size_t)blockIdx.x * kST + threadIdx.x;
    if (i >= n) return;
    bool bottom;
    xyzz<FP> a = start_at(q, bottom);
    const uint16_t *m = words + i * (size_t)n_words;
#pragma unroll 1
    for (u32 w = 0; w < n_words; w++) {
        const u32 word = m[w] & kWordMask;                 // the mask keeps the gather inside the table whatever the caller sent
        const affine<FP> s = LDS_TABLE ? aff_load<FP>(lds_table + 4 * word) : aff_load<FP>(table + 16 * (size_t)word);
        fe p, r, d, zz_r;
        sinsemilla_round(a, s, p, r, d, zz_r);
        bottom = bottom || fe_is_zero(p) || fe_is_zero(d);
    }
    affine<FP> res = xyzz_to_affine<FP>(a);
    if (bottom) res.x = res.y = fe_zero();
    fe_store(out_xy + 16 * i, res.x);
    fe_store(out_xy + 16 * i + 8, res.y);
    status[i] = bottom ? 1 : 0;
}

// MerkleCRH (Zcash protocol specification 5.4.1.3): the hash's x coordinate of the 52 words  layer (10 bits) || left (255 bits) ||
// right (255 bits), low bits first.  The words are cut from the two canonical values as the chain consumes them: word 0 is the layer,
// words 1-25 the low 250 bits of left, word 26 its top 5 bits under the low 5 of right, words 27-51 the remaining 250 bits of right.
__global__ void __launch_bounds__(kST) sinsemilla_merkle(const u32 *__restrict__ pairs, size_t n, u32 layer, PointArg q,
                                                         const u32 *__restrict__ table, u32 *__restrict__ out_x,
                                                         uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * kST + threadIdx.x;
    if (i >= n) return;
    bool bottom;
    xyzz<FP> a = start_at(q, bottom);
    u32 z[8], right[8];
    {
        const fe l = fe_from_mont<FP>(fe_load(pairs + 16 * i)), r = fe_from_mont<FP>(fe_load(pairs + 16 * i + 8));
#pragma unroll
        for (int j = 0; j < 8; j++) {
            z[j] = l.v[j];
            right[j] = r.v[j];
        }
    }
#pragma unroll 1
    for (u32 w = 0; w < 52; w++) {
        u32 word;
        if (w == 0) {
            word = layer & kWordMask;
        } else if (w == 26) {
            word = (z[0] & 31u) | ((right[0] & 31u) << 5);
#pragma unroll
            for (int j = 0; j < 7; j++) z[j] = (right[j] >> 5) | (right[j + 1] << 27);
            z[7] = right[7] >> 5;
        } else {
            word = z[0] & kWordMask;
            shift_right_k(z);
        }
        const affine<FP> s = aff_load<FP>(table + 16 * (size_t)word);
        fe p, r, d, zz_r;
        sinsemilla_round(a, s, p, r, d, zz_r);
        bottom = bottom || fe_is_zero(p) || fe_is_zero(d);
    }
    fe x = xyzz_to_affine<FP>(a).x;
    if (bottom) x = fe_zero();
    fe_store(out_x + 8 * i, x);
    status[i] = bottom ? 1 : 0;
}

// Pass A (EMIT = false): inv[row] <- ZZ ZZZ P D of every word row, ZZ ZZZ of the final accumulator on the last row.
// Pass B (EMIT = true): inv holds their inverses; the five columns are written.  `first` is the first message of the chunk: inv is
// indexed from it, the columns and the pieces from message 0.
template <bool EMIT>
__global__ void __launch_bounds__(kST) sinsemilla_trace(const u32 *__restrict__ pieces, size_t first, size_t chunk, size_t count,
                                                        u32 n_pieces, u32 rows, PieceWords nw, PointArg q,
                                                        const u32 *__restrict__ table, u32 *__restrict__ inv,
                                                        u32 *__restrict__ columns, uint8_t *__restrict__ status) {
    const size_t local = (size_t)blockIdx.x * kST + threadIdx.x;
    if (local >= chunk) return;
    const size_t i = first + local;
    bool bottom;
    xyzz<FP> a = start_at(q, bottom);
    u32 *t = inv + 8 * (local * rows);
    const size_t column = 8 * (size_t)rows * count;
    u32 *out = columns + 8 * (i * rows);                   // row 0 of this message in column 0 (x_a)
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
                // y_a - y_p = -r / ZZZ and x_a - x_p = -p / ZZ:  lambda_1 = r ZZ / (ZZZ p)
                const fe lambda_1 = fe_mulx<FP>(fe_mulx<FP>(r, i_zzz), fe_mulx<FP>(before.zz, i_p));
                // x_a - x_r = d / ZZ_R:  lambda_2 = 2 y_a ZZ_R / d - lambda_1
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

struct SinsemillaContext {
    std::mutex mu;
    DevBuf scratch;
    void release_all() { scratch.release(); }
};
StreamContexts<SinsemillaContext> g_sinsemilla_ctxs;

inline unsigned grid_of(size_t n) { return (unsigned)((n + kST - 1) / kST); }
inline PointArg point_arg(const uint64_t *q_xy) {
    PointArg q;
    memcpy(q.x, q_xy, 32);
    memcpy(q.y, q_xy + 4, 32);
    return q;
}

}  // namespace

void sinsemilla_release_workspaces() { g_sinsemilla_ctxs.release_current_device(); }   // h2_trim

}  // namespace h2

using namespace h2;

extern "C" int h2_sinsemilla_hash_device(const void *d_words, size_t n, size_t words, const uint64_t *q_xy, const void *d_table,
                                         void *d_out_xy, void *d_status, void *stream) {
    if (words > kC || n > kMaxMessages || !q_xy || (n && (!d_table || !d_out_xy || !d_status || (words && !d_words)))) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!n) return H2_OK;
    const char *lds = ab_env("H2_SINSEMILLA_LDS");
    if (lds && lds[0] == '1')
        hipLaunchKernelGGL(sinsemilla_hash<true>, dim3(grid_of(n)), dim3(kST), kTableBytes, (hipStream_t)stream, (const uint16_t *)d_words, n,
                           (u32)words, point_arg(q_xy), (const u32 *)d_table, (u32 *)d_out_xy, (uint8_t *)d_status);
    else
        hipLaunchKernelGGL(sinsemilla_hash<false>, dim3(grid_of(n)), dim3(kST), 0, (hipStream_t)stream, (const uint16_t *)d_words, n,
                           (u32)words, point_arg(q_xy), (const u32 *)d_table, (u32 *)d_out_xy, (uint8_t *)d_status);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

extern "C" int h2_sinsemilla_merkle_layer_device(unsigned layer, const void *d_pairs, size_t n, const uint64_t *q_xy, const void *d_table,
                                                 void *d_out_x, void *d_status, void *stream) {
    if (layer > kWordMask || n > kMaxMessages || !q_xy || (n && (!d_pairs || !d_table || !d_out_x || !d_status))) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!n) return H2_OK;
    hipLaunchKernelGGL(sinsemilla_merkle, dim3(grid_of(n)), dim3(kST), 0, (hipStream_t)stream, (const u32 *)d_pairs, n, (u32)layer,
                       point_arg(q_xy), (const u32 *)d_table, (u32 *)d_out_x, (uint8_t *)d_status);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

extern "C" int h2_sinsemilla_trace_device(const void *d_pieces, size_t count, const uint32_t *num_words, size_t n_pieces,
                                          const uint64_t *q_xy, const void *d_table, void *d_columns, void *d_status, void *stream) {
    if (!num_words || n_pieces == 0 || n_pieces > kC || count > kMaxMessages || !q_xy) return H2_ERR_ARGS;
    PieceWords nw = {};
    size_t total = 0;
    for (size_t k = 0; k < n_pieces; k++) {
        if (num_words[k] == 0 || num_words[k] > kMaxPieceWords) return H2_ERR_ARGS;
        nw.n[k] = (uint8_t)num_words[k];
        total += num_words[k];
    }
    if (total > kC || (count && (!d_pieces || !d_table || !d_columns || !d_status))) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!count) return H2_OK;
    const size_t rows = total + 1, per_chunk = kTraceScratchRows / rows;          // rows <= 254: thousands of messages per chunk
    hipStream_t st = (hipStream_t)stream;
    SinsemillaContext &ctx = g_sinsemilla_ctxs.get(st);
    std::lock_guard<std::mutex> lk(ctx.mu);
    const size_t widest = count < per_chunk ? count : per_chunk;
    if ((rc = ctx.scratch.reserve(widest * rows * 32)) != H2_OK) return rc;
    const PointArg q = point_arg(q_xy);
    for (size_t first = 0; first < count; first += per_chunk) {
        const size_t chunk = count - first < per_chunk ? count - first : per_chunk;
        hipLaunchKernelGGL(sinsemilla_trace<false>, dim3(grid_of(chunk)), dim3(kST), 0, st, (const u32 *)d_pieces, first, chunk, count,
                           (u32)n_pieces, (u32)rows, nw, q, (const u32 *)d_table, ctx.scratch.as<u32>(), (u32 *)d_columns, (uint8_t *)d_status);
        H2_HIP(hipGetLastError());
        if ((rc = h2_batch_invert_device(H2_FP, ctx.scratch.ptr, chunk * rows, H2_FORM_MONTGOMERY, stream)) != H2_OK) return rc;
        hipLaunchKernelGGL(sinsemilla_trace<true>, dim3(grid_of(chunk)), dim3(kST), 0, st, (const u32 *)d_pieces, first, chunk, count,
                           (u32)n_pieces, (u32)rows, nw, q, (const u32 *)d_table, ctx.scratch.as<u32>(), (u32 *)d_columns, (uint8_t *)d_status);
        H2_HIP(hipGetLastError());
    }
    return H2_OK;
}
