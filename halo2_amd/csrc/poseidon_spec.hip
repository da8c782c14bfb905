// Poseidon for any specification (halo2_poseidon/src/lib.rs:40-151: Spec<F, T, RATE>) over the Pasta fields, batched: one lane per
// permutation, the width, the rate and the round counts taken at run time.
//
//   h2_poseidon_spec_permute_device   n states of `width` elements -> n states
//   h2_poseidon_spec_hash_device      Hash<_, S, ConstantLength<len>, T, RATE> of n messages: the sponge around the permutation
//   h2_poseidon_spec_trace_device     the witness Pow5Chip<F, WIDTH, RATE> assigns cell by cell, width + 1 columns
//
// csrc/poseidon.hip keeps the three words of P128Pow5T3 in registers and unrolls its 3 x 3 MDS product: twelve multiplier bodies.
// That shape at width 12 would be 144 of them, and a register array indexed by a run-time word would go to scratch.  Here a lane's
// state and the accumulator of its MDS product live in LDS, limb-major across the 64 lanes of the workgroup
// (lds[((word * 8 + limb) * 64 + lane)], so the lanes of a wave read consecutive banks), and every loop over words is a real loop:
// ONE round loop with ONE inlined S-box (three multiplier bodies) and ONE inlined multiplier in the MDS product.  The two LDS halves
// swap roles every round, so the product is never copied back.  Round constants and the MDS matrix are the CALLER's device buffer
// (h2_poseidon_spec_t::d_constants), read by the wave-uniform round and word index; this unit keeps no device memory of its own and
// touches no stream but the descriptor's.  A workgroup is one wave and uses 4096 * width bytes of LDS; a lane touches only its own
// LDS slots, so there is no barrier anywhere.
#include "common.h"
#include "field.cuh"

namespace h2 {
namespace {

constexpr unsigned kLanes = 64;                          // lanes per workgroup: one wave
constexpr unsigned kMaxWidth = H2_POSEIDON_MAX_WIDTH;
constexpr unsigned kMaxRounds = 1024;                    // full + partial
constexpr size_t kMaxStates = (size_t)1 << 30;           // permutations / messages per call: the grid and every byte offset fit
constexpr size_t kMaxHashElements = (size_t)1 << 40;     // n * len of one hash call

struct SpecArgs {
    const u32 *constants;                                // (full + partial) * width round constants, then width * width MDS entries
    unsigned width, rate, full, partial;
};

__device__ __forceinline__ fe lds_get(const u32 *lane, unsigned word) {
    fe r;
#pragma unroll
    for (int l = 0; l < 8; l++) r.v[l] = lane[(word * 8 + l) * kLanes];
    return r;
}

__device__ __forceinline__ void lds_put(u32 *lane, unsigned word, const fe &a) {
#pragma unroll
    for (int l = 0; l < 8; l++) lane[(word * 8 + l) * kLanes] = a.v[l];
}

template <int F> __device__ __forceinline__ fe pow5(const fe &x) {
    const fe x2 = fe_sqr<F>(x);
    return fe_mulx<F>(fe_sqr<F>(x2), x);
}

// Where the trace of one permutation goes: row 0 of this permutation in column 0; `column` u32 words from one column to the next.
struct TraceOut {
    u32 *first;
    size_t column;
};

template <bool TRACE> __device__ __forceinline__ void store_state(const TraceOut &out, const SpecArgs &a, unsigned row, const u32 *lane, unsigned at) {
    if (TRACE) {
#pragma unroll 1
        for (unsigned j = 0; j < a.width; j++) fe_store(out.first + j * out.column + 8 * (size_t)row, lds_get(lane, at + j));
    }
}

// The permutation of the `width` words at LDS word `at` (0 or width) of this lane; returns where the result lies (the other half after
// an odd number of rounds).  TRACE (partial is even): the rows of the chip -- a full round r < full / 2 ends on row r + 1; the partial
// rounds full / 2 + 2 i and + 2 i + 1 share row full / 2 + i, whose partial_sbox cell is the S-box output of the first and whose next
// row is the state after the second; the last full rounds follow, the output on row full + partial / 2.
template <int F, bool TRACE> __device__ __forceinline__ unsigned permutation(u32 *lane, unsigned at, const SpecArgs &a, const TraceOut &out) {
    const unsigned width = a.width, half = a.full / 2, rounds = a.full + a.partial;
    const u32 *mds = a.constants + 8 * (size_t)rounds * width;
    u32 *sbox_column = TRACE ? out.first + width * out.column : nullptr;
    store_state<TRACE>(out, a, 0, lane, at);
#pragma unroll 1
    for (unsigned r = 0; r < rounds; r++) {
        const bool full = r < half || r >= half + a.partial;
        const unsigned boxes = full ? width : 1;
        const u32 *rc = a.constants + 8 * (size_t)r * width;
        fe first = fe_zero();
#pragma unroll 1
        for (unsigned j = 0; j < width; j++) {
            fe x = fe_add<F>(lds_get(lane, at + j), fe_load(rc + 8 * j));
            if (j < boxes) x = pow5<F>(x);                                     // the ONE inlined S-box
            if (j == 0) first = x;
            lds_put(lane, at + j, x);
        }
        const bool first_of_pair = !full && ((r - half) & 1) == 0;
        if (TRACE && first_of_pair) fe_store(sbox_column + 8 * (size_t)(half + (r - half) / 2), first);
        const unsigned to = at ? 0 : width;
#pragma unroll 1
        for (unsigned i = 0; i < width; i++) {
            fe acc = fe_zero();
#pragma unroll 1
            for (unsigned j = 0; j < width; j++)                              // the ONE inlined multiplier of the product
                acc = fe_add<F>(acc, fe_mulx<F>(fe_load(mds + 8 * (i * width + j)), lds_get(lane, at + j)));
            lds_put(lane, to + i, acc);
        }
        at = to;
        if (TRACE && !first_of_pair) {
            const unsigned row = r < half ? r + 1 : full ? r - a.partial / 2 + 1 : half + 1 + (r - half) / 2;
            store_state<TRACE>(out, a, row, lane, at);
            if (full) fe_store(sbox_column + 8 * (size_t)(row - 1), fe_zero());
        }
    }
    if (TRACE) fe_store(sbox_column + 8 * (size_t)(a.full + a.partial / 2), fe_zero());
    return at;
}

extern __shared__ u32 spec_lds[];                        // 2 * width words of 8 limbs for each of the 64 lanes

// in and out may be the same buffer (hence no __restrict__): a lane reads its state before it writes it, and touches no other lane's
template <int F> __global__ void __launch_bounds__(kLanes) poseidon_spec_permute(SpecArgs a, const u32 *in, size_t n, u32 *out_states) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= n) return;
    u32 *lane = spec_lds + threadIdx.x;
#pragma unroll 1
    for (unsigned j = 0; j < a.width; j++) lds_put(lane, j, fe_load(in + 8 * (i * a.width + j)));
    const unsigned at = permutation<F, false>(lane, 0, a, TraceOut{});
#pragma unroll 1
    for (unsigned j = 0; j < a.width; j++) fe_store(out_states + 8 * (i * a.width + j), lds_get(lane, at + j));
}

template <int F> __global__ void __launch_bounds__(kLanes) poseidon_spec_hash(SpecArgs a, const u32 *__restrict__ messages, size_t n, u32 len, u32 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= n) return;
    u32 *lane = spec_lds + threadIdx.x;
    const u32 *m = messages + 8 * (i * (size_t)len);
#pragma unroll 1
    for (unsigned j = 0; j < a.width; j++) lds_put(lane, j, fe_zero());
    lds_put(lane, a.rate, fe_to_mont<F>(fe{{0, 0, len, 0, 0, 0, 0, 0}}));     // capacity: len * 2^64
    unsigned at = 0;
#pragma unroll 1
    for (size_t done = 0; done < len; done += a.rate) {
        const unsigned block = (unsigned)(len - done < a.rate ? len - done : a.rate);      // the rest of the block is the zero padding
#pragma unroll 1
        for (unsigned j = 0; j < block; j++) lds_put(lane, at + j, fe_add<F>(lds_get(lane, at + j), fe_load(m + 8 * (done + j))));
        at = permutation<F, false>(lane, at, a, TraceOut{});
    }
    fe_store(out + 8 * i, lds_get(lane, at));
}

template <int F> __global__ void __launch_bounds__(kLanes) poseidon_spec_trace(SpecArgs a, const u32 *__restrict__ in, size_t count, u32 *__restrict__ columns) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= count) return;
    u32 *lane = spec_lds + threadIdx.x;
#pragma unroll 1
    for (unsigned j = 0; j < a.width; j++) lds_put(lane, j, fe_load(in + 8 * (i * a.width + j)));
    const size_t rows = a.full + a.partial / 2 + 1;
    permutation<F, true>(lane, 0, a, TraceOut{columns + 8 * rows * i, 8 * rows * count});
}

inline unsigned grid_of(size_t n) { return (unsigned)((n + kLanes - 1) / kLanes); }
inline size_t lds_bytes(const SpecArgs &a) { return (size_t)2 * a.width * 8 * kLanes * sizeof(u32); }

// What every entry point refuses before anything touches the device.
inline bool spec_ok(const h2_poseidon_spec_t *s) {
    if (!s || (s->field != H2_FP && s->field != H2_FQ)) return false;
    if (s->width < 2 || s->width > kMaxWidth || s->rate < 1 || s->rate >= s->width) return false;
    if (s->full_rounds < 2 || (s->full_rounds & 1) || s->full_rounds > kMaxRounds || s->partial_rounds > kMaxRounds - s->full_rounds) return false;
    return true;
}

inline SpecArgs args_of(const h2_poseidon_spec_t *s) { return SpecArgs{(const u32 *)s->d_constants, s->width, s->rate, s->full_rounds, s->partial_rounds}; }

}  // namespace
}  // namespace h2

using namespace h2;

extern "C" int h2_poseidon_spec_permute_device(const h2_poseidon_spec_t *spec, const void *d_states, size_t n, void *d_out) {
    if (!spec_ok(spec) || n > kMaxStates || (n && (!d_states || !d_out || !spec->d_constants))) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!n) return H2_OK;
    const SpecArgs a = args_of(spec);
    hipStream_t st = (hipStream_t)spec->stream;
    if (spec->field == H2_FP) hipLaunchKernelGGL((poseidon_spec_permute<FP>), dim3(grid_of(n)), dim3(kLanes), lds_bytes(a), st, a, (const u32 *)d_states, n, (u32 *)d_out);
    else hipLaunchKernelGGL((poseidon_spec_permute<FQ>), dim3(grid_of(n)), dim3(kLanes), lds_bytes(a), st, a, (const u32 *)d_states, n, (u32 *)d_out);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

extern "C" int h2_poseidon_spec_hash_device(const h2_poseidon_spec_t *spec, const void *d_messages, size_t n, size_t len, void *d_out) {
    if (!spec_ok(spec) || len == 0 || len >= ((size_t)1 << 32) || n > kMaxStates || (n && len > kMaxHashElements / n) ||
        (n && (!d_messages || !d_out || !spec->d_constants)))
        return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!n) return H2_OK;
    const SpecArgs a = args_of(spec);
    hipStream_t st = (hipStream_t)spec->stream;
    if (spec->field == H2_FP) hipLaunchKernelGGL((poseidon_spec_hash<FP>), dim3(grid_of(n)), dim3(kLanes), lds_bytes(a), st, a, (const u32 *)d_messages, n, (u32)len, (u32 *)d_out);
    else hipLaunchKernelGGL((poseidon_spec_hash<FQ>), dim3(grid_of(n)), dim3(kLanes), lds_bytes(a), st, a, (const u32 *)d_messages, n, (u32)len, (u32 *)d_out);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

extern "C" int h2_poseidon_spec_trace_device(const h2_poseidon_spec_t *spec, const void *d_states, size_t count, void *d_columns) {
    if (!spec_ok(spec) || (spec->partial_rounds & 1) || count > kMaxStates || (count && (!d_states || !d_columns || !spec->d_constants))) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!count) return H2_OK;
    const SpecArgs a = args_of(spec);
    hipStream_t st = (hipStream_t)spec->stream;
    if (spec->field == H2_FP) hipLaunchKernelGGL((poseidon_spec_trace<FP>), dim3(grid_of(count)), dim3(kLanes), lds_bytes(a), st, a, (const u32 *)d_states, count, (u32 *)d_columns);
    else hipLaunchKernelGGL((poseidon_spec_trace<FQ>), dim3(grid_of(count)), dim3(kLanes), lds_bytes(a), st, a, (const u32 *)d_states, count, (u32 *)d_columns);
    H2_HIP(hipGetLastError());
    return H2_OK;
}
