// A Sinsemilla chain on one lane: what starts it, the hash loop over the generator table, and the body of the witness trace's two
// passes; shared by the hash and trace kernels (sinsemilla.hip) and the commitment, private-init and their trace kernels
// (sinsemilla_commit.hip).  The round itself is double_add_round.cuh's.  Everything is internal to the including unit.
#pragma once
#include <string.h>

#include "double_add_round.cuh"

namespace h2 {
namespace {

constexpr unsigned kK = 10, kC = 253, kWordMask = (1u << kK) - 1, kMaxPieceWords = 25;
constexpr u32 kTableBytes = 64u << kK;                   // 1024 affine points

struct PieceWords {                                        // the piece structure of a trace, by value in the kernel arguments
    uint8_t n[kC];
};
// num_words[0 .. n_pieces) as a trace entry point receives it -> nw and the words of a message; false where it is no piece structure
inline bool piece_words(const uint32_t *num_words, size_t n_pieces, PieceWords &nw, size_t &total) {
    if (!num_words || n_pieces == 0 || n_pieces > kC) return false;
    nw = {};
    total = 0;
    for (size_t k = 0; k < n_pieces; k++) {
        if (num_words[k] == 0 || num_words[k] > kMaxPieceWords) return false;
        nw.n[k] = (uint8_t)num_words[k];
        total += num_words[k];
    }
    return total <= kC;
}

struct PointArg {                                          // Q, Montgomery affine, by value
    u32 x[8], y[8];
};
inline PointArg point_arg(const uint64_t *q_xy) {
    PointArg q;
    memcpy(q.x, q_xy, 32);
    memcpy(q.y, q_xy + 4, 32);
    return q;
}
__device__ __forceinline__ xyzz<FP> start_at(const PointArg &q, bool &bottom) {
    xyzz<FP> a;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        a.x.v[i] = q.x[i];
        a.y.v[i] = q.y[i];
    }
    a.zz = fe_one<FP>();
    a.zzz = fe_one<FP>();
    bottom = fe_is_zero(a.x) && fe_is_zero(a.y);           // Q = the identity: the first addition is already exceptional
    return a;
}

__device__ __forceinline__ void shift_right_k(u32 (&z)[8]) {
#pragma unroll
    for (int j = 0; j < 7; j++) z[j] = (z[j] >> kK) | (z[j + 1] << (32 - kK));
    z[7] >>= kK;
}

__device__ __forceinline__ xyzz<FP> start_at(const u32 *q_xy, bool &bottom) {      // Q in device memory, Montgomery affine
    xyzz<FP> a;
    a.x = fe_load(q_xy);
    a.y = fe_load(q_xy + 8);
    a.zz = fe_one<FP>();
    a.zzz = fe_one<FP>();
    bottom = fe_is_zero(a.x) && fe_is_zero(a.y);
    return a;
}

// One word of a hash: gather S(word), run the round, fold bottom.  T is what the table is read as: u32 in global memory, uint4 in
// sinsemilla_hash's LDS copy.
template <typename T> __device__ __forceinline__ void hash_word(xyzz<FP> &a, bool &bottom, u32 word, const T *table) {
    const affine<FP> s = aff_load<FP>(table + (64 / sizeof(T)) * (size_t)word);
    fe p, r, d, zz_r;
    double_add_round(a, s, p, r, d, zz_r);
    bottom = bottom || fe_is_zero(p) || fe_is_zero(d);
}
template <typename T>
__device__ __forceinline__ void hash_chain(xyzz<FP> &a, bool &bottom, const uint16_t *m, u32 n_words, const T *table) {
#pragma unroll 1
    for (u32 w = 0; w < n_words; w++) hash_word(a, bottom, m[w] & kWordMask, table);      // the mask keeps the gather inside the table
}

__device__ __forceinline__ void store_point(u32 *out_xy, uint8_t *status, size_t i, affine<FP> res, bool bottom) {
    if (bottom) res.x = res.y = fe_zero();
    fe_store(out_xy + 16 * i, res.x);
    fe_store(out_xy + 16 * i + 8, res.y);
    status[i] = bottom ? 1 : 0;
}

// The two passes of a trace of message i from the accumulator a, which the kernel has formed (and bottom with it).
// Pass A (EMIT = false): inv[row] <- ZZ ZZZ P D of every word row, ZZ ZZZ of the final accumulator on the last row.
// Pass B (EMIT = true): inv holds their inverses; the five columns x_a, x_p, bits, lambda_1, lambda_2 are written.
// `local` is the message's place in its chunk: inv is indexed from it, the columns and the pieces from message 0.
// LEAD = 1 moves the message's rows down by one, under a row that holds y_Q in x_p (hash_to_point.rs:117-121, :179-182): the trace
// from a private point.  `rows` counts that row; it has no denominator, so inv holds rows - LEAD elements per message.
template <bool EMIT, int LEAD>
__device__ __forceinline__ void trace_chain(const u32 *__restrict__ pieces, size_t local, size_t i, size_t count, u32 n_pieces, u32 rows,
                                            const PieceWords &nw, xyzz<FP> a, bool bottom, const u32 *__restrict__ table,
                                            u32 *__restrict__ inv, u32 *__restrict__ columns, uint8_t *__restrict__ status) {
    u32 *t = inv + 8 * (local * (rows - LEAD));
    const size_t column = 8 * (size_t)rows * count;
    u32 *out = columns + 8 * (i * rows);                   // row 0 of this message in column 0 (x_a)
    if (LEAD) {
        if (EMIT) {
            fe_store(out, fe_zero());
            fe_store(out + column, a.y);
            fe_store(out + 2 * column, fe_zero());
            fe_store(out + 3 * column, fe_zero());
            fe_store(out + 4 * column, fe_zero());
        }
        out += 8;
    }
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
            double_add_round(a, s, p, r, d, zz_r);
            bottom = bottom || fe_is_zero(p) || fe_is_zero(d);
            const fe zed = fe_mulx<FP>(before.zz, before.zzz);
            if (!EMIT) {
                fe_store(t + 8 * row, round_denominators(zed, p, d));
            } else {
                const RoundRow v = round_row(before, zed, p, r, d, zz_r, fe_load(t + 8 * row));
                fe zf;
#pragma unroll
                for (int j = 0; j < 8; j++) zf.v[j] = z[j];
                fe_store(out + 8 * row, v.x_a);
                fe_store(out + column + 8 * row, s.x);
                fe_store(out + 2 * column + 8 * row, fe_to_mont<FP>(zf));
                fe_store(out + 3 * column + 8 * row, v.lambda_1);
                fe_store(out + 4 * column + 8 * row, v.lambda_2);
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

}  // namespace
}  // namespace h2
