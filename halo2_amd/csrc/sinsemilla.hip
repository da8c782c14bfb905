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
// The pieces live where the other gadget units take them from too: the round and the split of an inverse in double_add_round.cuh
// (ecc.hip's chain is the same step), the hash loop and the body of the two passes in sinsemilla_chain.cuh (sinsemilla_commit.hip),
// the chunks and the inversion between the passes in two_pass_trace (common.h; all four trace entry points).
//
// The 1024-point table S (64 KiB, Montgomery affine) is gathered from global memory, 64 bytes per lane and round; it is read by
// every lane of every launch and stays in L2.
#include "common.h"
#include "sinsemilla_chain.cuh"

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
    if (LDS_TABLE) hash_chain(a, bottom, words + i * (size_t)n_words, n_words, lds_table);
    else hash_chain(a, bottom, words + i * (size_t)n_words, n_words, table);
    store_point(out_xy, status, i, xyzz_to_affine<FP>(a), bottom);
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
        hash_word(a, bottom, word, table);
    }
    fe x = xyzz_to_affine<FP>(a).x;
    if (bottom) x = fe_zero();
    fe_store(out_x + 8 * i, x);
    status[i] = bottom ? 1 : 0;
}

// The two passes of the trace from the shared Q (trace_chain, sinsemilla_chain.cuh).  `first` is the first message of the chunk.
template <bool EMIT>
__global__ void __launch_bounds__(kST) sinsemilla_trace(const u32 *__restrict__ pieces, size_t first, size_t chunk, size_t count,
                                                        u32 n_pieces, u32 rows, PieceWords nw, PointArg q,
                                                        const u32 *__restrict__ table, u32 *__restrict__ inv,
                                                        u32 *__restrict__ columns, uint8_t *__restrict__ status) {
    const size_t local = (size_t)blockIdx.x * kST + threadIdx.x;
    if (local >= chunk) return;
    bool bottom;
    const xyzz<FP> a = start_at(q, bottom);
    trace_chain<EMIT, 0>(pieces, local, first + local, count, n_pieces, rows, nw, a, bottom, table, inv, columns, status);
}

StreamContexts<ScratchContext> g_sinsemilla_ctxs;

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
        hipLaunchKernelGGL(sinsemilla_hash<true>, dim3(grid_of(n, kST)), dim3(kST), kTableBytes, (hipStream_t)stream, (const uint16_t *)d_words, n,
                           (u32)words, point_arg(q_xy), (const u32 *)d_table, (u32 *)d_out_xy, (uint8_t *)d_status);
    else
        hipLaunchKernelGGL(sinsemilla_hash<false>, dim3(grid_of(n, kST)), dim3(kST), 0, (hipStream_t)stream, (const uint16_t *)d_words, n,
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
    hipLaunchKernelGGL(sinsemilla_merkle, dim3(grid_of(n, kST)), dim3(kST), 0, (hipStream_t)stream, (const u32 *)d_pairs, n, (u32)layer,
                       point_arg(q_xy), (const u32 *)d_table, (u32 *)d_out_x, (uint8_t *)d_status);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

extern "C" int h2_sinsemilla_trace_device(const void *d_pieces, size_t count, const uint32_t *num_words, size_t n_pieces,
                                          const uint64_t *q_xy, const void *d_table, void *d_columns, void *d_status, void *stream) {
    PieceWords nw;
    size_t total;
    if (!piece_words(num_words, n_pieces, nw, total) || count > kMaxMessages || !q_xy) return H2_ERR_ARGS;
    if (count && (!d_pieces || !d_table || !d_columns || !d_status)) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!count) return H2_OK;
    const u32 rows = (u32)total + 1;                       // at most 254: thousands of messages per chunk
    hipStream_t st = (hipStream_t)stream;
    ScratchContext &ctx = g_sinsemilla_ctxs.get(st);
    std::lock_guard<std::mutex> lk(ctx.mu);
    const PointArg q = point_arg(q_xy);
    return two_pass_trace(ctx.scratch, count, rows, kTraceScratchRows, st, [&](bool emit, size_t first, size_t chunk, u32 *scratch) {
        hipLaunchKernelGGL(!emit ? sinsemilla_trace<false> : sinsemilla_trace<true>, dim3(grid_of(chunk, kST)), dim3(kST), 0, st,
                           (const u32 *)d_pieces, first, chunk, count, (u32)n_pieces, rows, nw, q, (const u32 *)d_table, scratch,
                           (u32 *)d_columns, (uint8_t *)d_status);
        return H2_OK;
    });
}
