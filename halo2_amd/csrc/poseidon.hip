// Poseidon P128Pow5T3 over the Pasta fields (halo2_poseidon/src/lib.rs:106-151, p128pow5t3.rs), batched: one lane per permutation.
//
//   h2_poseidon_permute_device   n states of 3 elements -> n states
//   h2_poseidon_hash_device      Hash<_, P128Pow5T3, ConstantLength<len>, 3, 2> of n messages: the sponge around the permutation
//   h2_poseidon_trace_device     the witness the Pow5 chip (halo2_gadgets poseidon/pow5.rs) assigns cell by cell: the state before
//                                every gate row and the first S-box output of every pair of partial rounds
//
// One permutation is 816 field multiplications (8 full rounds x 18, 56 partial rounds x 12) on three register-resident words.  All
// 64 rounds run through ONE loop body (`#pragma unroll 1`) with ONE S-box in it, which a full round runs three times (the round
// index is uniform over the wave): 12 inlined multipliers, about 50 KB of code per kernel; 816 of them would be 3 MB.
// Round constants and the MDS matrix are read from constant memory by that uniform index (scalar loads).  A lane owns its outputs:
// 32-byte fe_store, no atomics, no LDS.  The trace is the same routine with stores behind the round index; its stores are 37 * 32
// bytes apart between neighbouring lanes.
#include "common.h"
#include "field.cuh"

namespace h2 {
namespace {

#include "poseidon_consts.inc"

constexpr int kPT = 256;                                 // lanes per workgroup
constexpr size_t kMaxStates = (size_t)1 << 30;           // permutations / messages per call: the grid and every byte offset fit
constexpr size_t kMaxHashElements = (size_t)1 << 40;     // n * len of one hash call
constexpr int kFull = 8, kPartial = 56, kRounds = kFull + kPartial;
constexpr int kRows = kFull + kPartial / 2 + 1;          // 37 rows of the chip per permutation

__device__ __forceinline__ fe fe_const(const u32 (&c)[8]) { return fe{{c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]}}; }

template <int F> __device__ __forceinline__ fe pow5(const fe &x) {
    const fe x2 = fe_sqr<F>(x);
    return fe_mulx<F>(fe_sqr<F>(x2), x);
}

// Where the trace of one permutation goes: row 0 of this permutation in each of the four columns.
struct TraceOut {
    u32 *state[3];
    u32 *sbox;
};

template <int F, bool TRACE> __device__ __forceinline__ void store_state(const TraceOut &out, int row, const fe (&s)[3]) {
    if (TRACE) {
#pragma unroll
        for (int j = 0; j < 3; j++) fe_store(out.state[j] + 8 * row, s[j]);
    }
}

// The permutation.  TRACE: rows 0 .. 36 of the three state columns and of partial_sbox are written as the chip lays them out --
// a full round r < 4 ends on row r + 1, r >= 60 on row r - 27; the partial rounds 4 + 2 i and 5 + 2 i share row 4 + i, whose
// partial_sbox cell is the S-box output of the first and whose next row is the state after the second.
template <int F, bool TRACE> __device__ __forceinline__ void permutation(fe (&s)[3], const TraceOut &out) {
    store_state<F, TRACE>(out, 0, s);
#pragma unroll 1
    for (int r = 0; r < kRounds; r++) {
        const bool full = r < kFull / 2 || r >= kFull / 2 + kPartial;
#pragma unroll
        for (int j = 0; j < 3; j++) s[j] = fe_add<F>(s[j], fe_const(poseidon_round_constants[F][3 * r + j]));
        // ONE inlined S-box: a full round runs it three times and rotates the words in between (three rotations are the identity)
#pragma unroll 1
        for (int k = 0; k < (full ? 3 : 1); k++) {
            s[0] = pow5<F>(s[0]);
            if (full) {
                const fe first = s[0];
                s[0] = s[1];
                s[1] = s[2];
                s[2] = first;
            }
        }
        const bool first_of_pair = !full && ((r - kFull / 2) & 1) == 0;
        if (TRACE && first_of_pair) fe_store(out.sbox + 8 * (kFull / 2 + (r - kFull / 2) / 2), s[0]);
        fe t[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            t[i] = fe_mulx<F>(fe_const(poseidon_mds[F][3 * i]), s[0]);
#pragma unroll
            for (int j = 1; j < 3; j++) t[i] = fe_add<F>(t[i], fe_mulx<F>(fe_const(poseidon_mds[F][3 * i + j]), s[j]));
        }
#pragma unroll
        for (int i = 0; i < 3; i++) s[i] = t[i];
        if (TRACE && !first_of_pair) {
            const int row = r < kFull / 2 ? r + 1 : full ? r - (kPartial / 2 - 1) : kFull / 2 + 1 + (r - kFull / 2) / 2;
            store_state<F, TRACE>(out, row, s);
            if (full) fe_store(out.sbox + 8 * (row - 1), fe_zero());          // rows 0-3 and 32-35
        }
    }
    if (TRACE) fe_store(out.sbox + 8 * (kRows - 1), fe_zero());              // row 36
}

// in and out may be the same buffer (hence no __restrict__): a lane reads its state before it writes it, and touches no other lane's
template <int F> __global__ void __launch_bounds__(kPT) poseidon_permute(const u32 *in, size_t n, u32 *out_states) {
    const size_t i = (size_t)blockIdx.x * kPT + threadIdx.x;
    if (i >= n) return;
    fe s[3];
#pragma unroll
    for (int j = 0; j < 3; j++) s[j] = fe_load(in + 8 * (3 * i + j));
    permutation<F, false>(s, TraceOut{});
#pragma unroll
    for (int j = 0; j < 3; j++) fe_store(out_states + 8 * (3 * i + j), s[j]);
}

template <int F> __global__ void __launch_bounds__(kPT) poseidon_hash(const u32 *__restrict__ messages, size_t n, u32 len, u32 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * kPT + threadIdx.x;
    if (i >= n) return;
    const u32 *m = messages + 8 * (i * (size_t)len);
    fe s[3] = {fe_zero(), fe_zero(), fe_to_mont<F>(fe{{0, 0, len, 0, 0, 0, 0, 0}})};       // capacity: len * 2^64
#pragma unroll 1
    for (u32 at = 0; at < len; at += 2) {
        s[0] = fe_add<F>(s[0], fe_load(m + 8 * (size_t)at));
        if (at + 1 < len) s[1] = fe_add<F>(s[1], fe_load(m + 8 * ((size_t)at + 1)));       // else the zero padding
        permutation<F, false>(s, TraceOut{});
    }
    fe_store(out + 8 * i, s[0]);
}

template <int F> __global__ void __launch_bounds__(kPT) poseidon_trace(const u32 *__restrict__ in, size_t count, u32 *__restrict__ columns) {
    const size_t i = (size_t)blockIdx.x * kPT + threadIdx.x;
    if (i >= count) return;
    fe s[3];
#pragma unroll
    for (int j = 0; j < 3; j++) s[j] = fe_load(in + 8 * (3 * i + j));
    const size_t column = 8 * (size_t)kRows * count, first = 8 * (size_t)kRows * i;
    TraceOut out;
#pragma unroll
    for (int j = 0; j < 3; j++) out.state[j] = columns + j * column + first;
    out.sbox = columns + 3 * column + first;
    permutation<F, true>(s, out);
}

inline unsigned grid_of(size_t n) { return (unsigned)((n + kPT - 1) / kPT); }

}  // namespace
}  // namespace h2

using namespace h2;

extern "C" int h2_poseidon_permute_device(int field, const void *d_states, size_t n, void *d_out, void *stream) {
    if ((field != H2_FP && field != H2_FQ) || n > kMaxStates || (n && (!d_states || !d_out))) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!n) return H2_OK;
    hipStream_t st = (hipStream_t)stream;
    if (field == H2_FP) hipLaunchKernelGGL((poseidon_permute<FP>), dim3(grid_of(n)), dim3(kPT), 0, st, (const u32 *)d_states, n, (u32 *)d_out);
    else hipLaunchKernelGGL((poseidon_permute<FQ>), dim3(grid_of(n)), dim3(kPT), 0, st, (const u32 *)d_states, n, (u32 *)d_out);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

extern "C" int h2_poseidon_hash_device(int field, const void *d_messages, size_t n, size_t len, void *d_out, void *stream) {
    if ((field != H2_FP && field != H2_FQ) || len == 0 || len >= ((size_t)1 << 32) || n > kMaxStates || (n && len > kMaxHashElements / n) ||
        (n && (!d_messages || !d_out)))
        return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!n) return H2_OK;
    hipStream_t st = (hipStream_t)stream;
    if (field == H2_FP) hipLaunchKernelGGL((poseidon_hash<FP>), dim3(grid_of(n)), dim3(kPT), 0, st, (const u32 *)d_messages, n, (u32)len, (u32 *)d_out);
    else hipLaunchKernelGGL((poseidon_hash<FQ>), dim3(grid_of(n)), dim3(kPT), 0, st, (const u32 *)d_messages, n, (u32)len, (u32 *)d_out);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

extern "C" int h2_poseidon_trace_device(int field, const void *d_states, size_t count, void *d_columns, void *stream) {
    if ((field != H2_FP && field != H2_FQ) || count > kMaxStates || (count && (!d_states || !d_columns))) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!count) return H2_OK;
    hipStream_t st = (hipStream_t)stream;
    if (field == H2_FP) hipLaunchKernelGGL((poseidon_trace<FP>), dim3(grid_of(count)), dim3(kPT), 0, st, (const u32 *)d_states, count, (u32 *)d_columns);
    else hipLaunchKernelGGL((poseidon_trace<FQ>), dim3(grid_of(count)), dim3(kPT), 0, st, (const u32 *)d_states, count, (u32 *)d_columns);
    H2_HIP(hipGetLastError());
    return H2_OK;
}
