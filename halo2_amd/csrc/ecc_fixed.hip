// Fixed-base scalar multiplication over Pallas (halo2_gadgets/src/ecc/chip/constants.rs, mul_fixed.rs, mul_fixed/full_width.rs):
// the tables of a fixed base, built on the device, and the batched product and witness over them, one lane per multiplication.
//
//   h2_ecc_fixed_tables_device      compute_window_table, compute_lagrange_coeffs and find_zs_and_us of one base in one call
//   h2_ecc_mul_fixed_device         n products [k_i]B from the window table: num_windows - 1 additions, no doubling
//   h2_ecc_mul_fixed_trace_device   what mul_fixed::Config::assign_region_inner and full_width's closing complete addition witness
//
// A scalar is cut into 3-bit windows k_0 .. k_(nw-1), low bits first.  Window w < nw - 1 contributes points[w][k_w] = [(k_w + 2) 8^w]B
// and the last one points[nw-1][k] = [k 8^(nw-1) - sum_{j < nw-1} 2^(3j+1)]B, which takes the +2's back out (constants.rs:40-82).
//
// The additions of windows 1 .. nw-2 are INCOMPLETE and need no exceptional branch: before window w the accumulator is [s]B with
// 0 < s = sum_{j<w} (k_j + 2) 8^j < 2 8^w <= (k_w + 2) 8^w, so s differs from the window's scalar, and their sum is below 11 8^83 < q
// (the group's order) through window 83, so they are not opposite either.  The last addition is complete: k = 0 ends on the identity,
// and the octal strings 1333...3334 and its unreduced twin (full_width.rs, LAST_DOUBLING) end on a doubling.  The chain is
// fixed_base_chain (ecc_fixed_chain.cuh), which the Sinsemilla commitment runs too; the trace walks the same windows one by one around
// two_pass_trace (common.h) and closes on complete_add and its record (ecc_add.cuh).
//
// The table (680 points, 43.5 KB at 85 windows) is gathered from global memory: the window is uniform across a wave, so its 64 lanes
// read within one 512-byte row of eight points, which the vector cache serves; staging in LDS was not measured.
//
// find_zs_and_us is the one search here: per window the smallest z such that z + y is a square or zero and z - y is neither for all
// eight y of the window.  One lane per (window, candidate z); residuosity by the uniform exponentiation a^((p-1)/2) (Euler), a lane
// leaving on its first failing test; survivors take an atomic minimum per window.  The host launches rounds of kSearchRound candidates
// per unfinished window and reads the minima back after each: a round has run to its end before its minimum is accepted, so the z is the
// smallest, not merely a valid one.
#include <vector>

#include "common.h"
#include "ecc_add.cuh"
#include "ecc_fixed_chain.cuh"
#include "field_sqrt.cuh"
#include "host_field.h"

namespace h2 {
namespace {

constexpr int kFT = 256;                                   // lanes per workgroup
constexpr size_t kMaxMuls = (size_t)1 << 30;
constexpr unsigned kMinWindows = 2, kMaxWindows = 85;
constexpr uint64_t kDefaultZLimit = (uint64_t)1000 << 16;  // constants.rs:129: 1000 * 2^(2 H)
constexpr uint64_t kSearchRound = (uint64_t)1 << 15;       // candidates per window and round: 128 workgroups a window
constexpr unsigned long long kNoZ = ~0ull;
// Elements of scratch per chunk of the trace, as ecc.hip: 256 MiB, 101 067 multiplications of 85 windows (83 elements each), one and a
// half waves per SIMD of 256 compute units.
constexpr size_t kTraceScratchElems = (size_t)1 << 23;

__device__ __forceinline__ fe fe_small(u64 v) {           // a small integer as a Montgomery element
    fe c = fe_zero();
    c.v[0] = (u32)v;
    c.v[1] = (u32)(v >> 32);
    return fe_to_mont<FP>(c);
}

// ---- the tables ---------------------------------------------------------------------------------------------------------------------------
// coefficient c of window w: row c of the inverse Vandermonde matrix of the nodes 0 .. 7 times the x of the window's eight points
__global__ void __launch_bounds__(kFT) ecc_fixed_lagrange(const u32 *__restrict__ points, const u32 *__restrict__ matrix, u32 n,
                                                          u32 *__restrict__ out) {
    const u32 i = blockIdx.x * kFT + threadIdx.x;
    if (i >= n) return;
    const u32 w = i >> 3, c = i & 7u;
    fe acc = fe_zero();
#pragma unroll 1
    for (u32 k = 0; k < 8; k++) acc = fe_add<FP>(acc, fe_mulx<FP>(fe_load(matrix + 8 * (8 * c + k)), fe_load(table_entry(points, w, k, 16))));
    fe_store(out + 8 * i, acc);
}

// a^((p-1)/2): one for a square, minus one for a non-residue, zero for zero.  The exponent's bits are the same on every lane.
__device__ __forceinline__ fe euler(const fe &a) {
    u32 e[8];                                              // (p - 1) / 2 with its top bit, 253, moved to bit 255
#pragma unroll
    for (int j = 0; j < 8; j++) e[j] = j ? mod_limb<FP>(j) : 0u;
#pragma unroll
    for (int j = 7; j > 0; j--) e[j] = (e[j] << 1) | (e[j - 1] >> 31);
    e[0] <<= 1;
    fe acc = a;                                            // bit 253
#pragma unroll 1
    for (u32 b = 0; b < 253; b++) {
#pragma unroll
        for (int j = 7; j > 0; j--) e[j] = (e[j] << 1) | (e[j - 1] >> 31);
        e[0] <<= 1;
        acc = fe_sqr<FP>(acc);
        if (e[7] >> 31) acc = fe_mulx<FP>(acc, a);
    }
    return acc;
}

// Candidate z = first + x of window active[y]: 16 tests, z - y_k a non-residue and z + y_k not one, for k = 0 .. 7.  A candidate above
// a minimum another lane has already posted cannot lower it and leaves at once.
__global__ void __launch_bounds__(kFT) ecc_fixed_search(const u32 *__restrict__ points, const u32 *__restrict__ active, u64 first, u64 limit,
                                                        unsigned long long *z_min) {
    const u32 w = active[blockIdx.y];
    const u64 z = first + (u64)blockIdx.x * kFT + threadIdx.x;
    if (z >= limit || z > __hip_atomic_load(&z_min[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    const fe zm = fe_small(z), minus_one = fe_neg<FP>(fe_one<FP>());
    bool ok = true;
#pragma unroll 1
    for (u32 t = 0; t < 16 && ok; t++) {
        const fe y = fe_load(table_entry(points, w, t >> 1, 16) + 8);
        const bool plus = t & 1u;
        const bool non_residue = fe_eq(euler(plus ? fe_add<FP>(zm, y) : fe_sub<FP>(zm, y)), minus_one);
        ok = non_residue != plus;
    }
    if (ok) atomicMin(&z_min[w], (unsigned long long)z);
}

// u[w][k] = sqrt(y + z_w), the root fe_sqrt returns
__global__ void __launch_bounds__(kFT) ecc_fixed_roots(const u32 *__restrict__ points, const unsigned long long *__restrict__ z_min, u32 n,
                                                       u32 *__restrict__ out) {
    const u32 i = blockIdx.x * kFT + threadIdx.x;
    if (i >= n) return;
    const fe y = fe_load(points + 16 * i + 8);
    fe u;
    if (!fe_sqrt<FP>(fe_add<FP>(fe_small(z_min[i >> 3]), y), u)) u = fe_zero();      // the search has ruled this out
    fe_store(out + 8 * i, u);
}

// ---- the product --------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kFT) ecc_fixed_mul(const u32 *__restrict__ points, u32 nw, const u32 *__restrict__ scalars, size_t n,
                                                     u32 *__restrict__ out_xy) {
    const size_t i = (size_t)blockIdx.x * kFT + threadIdx.x;
    if (i >= n) return;
    u32 k[8];
    load_scalar(scalars, i, k);
    const affine<FP> res = xyzz_to_affine<FP>(fixed_base_chain(points, nw, k));
    fe_store(out_xy + 16 * i, res.x);
    fe_store(out_xy + 16 * i + 8, res.y);
}

// ---- the witness --------------------------------------------------------------------------------------------------------------------------
// Columns (chip.rs:280-292, mul_fixed.rs): x_p y_p x_qr y_qr window u = 0 .. 5.  Row w of a multiplication holds the window's point, its
// value and its root; rows 1 .. nw-1 also hold the accumulator the row's addition starts from -- on row nw-1, where the complete addition
// of the next region starts from.  The accumulator is affine before window 1 and needs 1 / (ZZ ZZZ) before windows 2 .. nw-1:
// pass A (EMIT = false) stores those nw - 2 products, element (w - 2) chunk + lane; pass B (EMIT = true) finds their inverses there.
template <bool EMIT>
__global__ void __launch_bounds__(kFT) ecc_fixed_trace(const u32 *__restrict__ points, const u32 *__restrict__ roots, u32 nw,
                                                       const u32 *__restrict__ scalars, size_t first, size_t chunk, size_t count,
                                                       u32 *__restrict__ inv, u32 *__restrict__ columns, u32 *__restrict__ aux) {
    const size_t local = (size_t)blockIdx.x * kFT + threadIdx.x;
    if (local >= chunk) return;
    const size_t i = first + local;
    u32 k[8];
    load_scalar(scalars, i, k);
    const size_t column = 8 * (size_t)nw * count;
    u32 *out = columns + 8 * (i * nw);                      // row 0 of this multiplication in column 0
    xyzz<FP> acc = xyzz_identity<FP>();
#pragma unroll 1
    for (u32 w = 0; w < nw; w++) {
        const u32 d = take_window(k);
        const affine<FP> q = aff_load<FP>(table_entry(points, w, d, 16));
        affine<FP> a{fe_zero(), fe_zero()};                 // the accumulator before this window; row 0 has none
        if (w == 1) {
            a.x = acc.x;
            a.y = acc.y;
        } else if (w > 1) {
            u32 *slot = inv + 8 * ((size_t)(w - 2) * chunk + local);
            if (!EMIT) {
                fe_store(slot, fe_mulx<FP>(acc.zz, acc.zzz));
            } else {
                const fe i_zed = fe_load(slot);
                a.x = fe_mulx<FP>(acc.x, fe_mulx<FP>(acc.zzz, i_zed));
                a.y = fe_mulx<FP>(acc.y, fe_mulx<FP>(acc.zz, i_zed));
            }
        }
        if (EMIT) {
            fe_store(out + 8 * w, q.x);
            fe_store(out + column + 8 * w, q.y);
            fe_store(out + 2 * column + 8 * w, a.x);
            fe_store(out + 3 * column + 8 * w, a.y);
            fe_store(out + 4 * column + 8 * w, fe_small(d));
            fe_store(out + 5 * column + 8 * w, fe_load(table_entry(roots, w, d, 8)));
        }
        if (w == 0) {
            acc = xyzz_of(q);
        } else if (w + 1 < nw) {
            xyzz_madd_incomplete(acc, q);
        } else if (EMIT) {                                  // full_width.rs:150-159: the window's point first, the accumulator second
            AddWitness wit;
            const affine<FP> sum = complete_add(q, a, wit);
            store_add_aux(aux + 8 * 11 * i, q, a, wit, sum);
        }
    }
}

StreamContexts<ScratchContext> g_ecc_fixed_ctxs;

// ---- host arithmetic of the table build ---------------------------------------------------------------------------------------------------
void host_neg(int f, u64 r[4], const u64 a[4]) {
    if (host_is_zero(a)) memset(r, 0, 32);
    else host_sub_raw(r, kHostField[f].p, a);
}
void host_from_int(int f, u64 r[4], long long v) {
    const u64 a[4] = {(u64)(v < 0 ? -v : v), 0, 0, 0};
    host_to_mont(f, r, a, H2_FORM_CANONICAL);
    if (v < 0) host_neg(f, r, r);
}
bool host_on_curve(const u64 *xy) {                        // Montgomery coordinates below p with y^2 = x^3 + 5
    const u64 *p = kHostField[H2_FP].p;
    if (host_ge(xy, p) || host_ge(xy + 4, p)) return false;
    u64 yy[4], xxx[4], five[4];
    host_mul(H2_FP, yy, xy + 4, xy + 4);
    host_mul(H2_FP, xxx, xy, xy);
    host_mul(H2_FP, xxx, xxx, xy);
    host_from_int(H2_FP, five, 5);
    host_add(H2_FP, xxx, xxx, five);
    return !memcmp(yy, xxx, 32);
}
// m 2^shift as a 256-bit integer (m below 16, shift at most 252)
void host_small_shl(u64 r[4], u64 m, unsigned shift) {
    memset(r, 0, 32);
    r[shift >> 6] = m << (shift & 63);
    if ((shift & 63) > 60 && (shift >> 6) < 3) r[(shift >> 6) + 1] = m >> (64 - (shift & 63));
}
// The 8 nw scalars of compute_window_table as integers below 2^255, which is all the product kernel asks: (k + 2) 8^w, and for the last
// window k 8^w - sum, plus q where that is negative (k = 0).
void window_scalars(unsigned nw, std::vector<u64> &out) {
    out.assign((size_t)32 * nw, 0);
    for (unsigned w = 0; w + 1 < nw; w++)
        for (unsigned k = 0; k < 8; k++) host_small_shl(&out[4 * (8 * w + k)], k + 2, 3 * w);
    u64 sum[4] = {0, 0, 0, 0};
    for (unsigned j = 0; j + 1 < nw; j++) sum[(3 * j + 1) >> 6] |= (u64)1 << ((3 * j + 1) & 63);
    for (unsigned k = 0; k < 8; k++) {
        u64 *s = &out[4 * (8 * (nw - 1) + k)];
        if (k) {
            host_small_shl(s, k, 3 * (nw - 1));
            host_sub_raw(s, s, sum);
        } else {
            host_sub_raw(s, kHostField[H2_FQ].p, sum);
        }
    }
}
// matrix[c][i]: coefficient c of the Lagrange basis polynomial of node i, prod_{j != i} (x - j) / (i - j), Montgomery
void lagrange_matrix(u64 (&matrix)[64][4]) {
    for (int i = 0; i < 8; i++) {
        long long num[8] = {1, 0, 0, 0, 0, 0, 0, 0}, den = 1;     // integer coefficients: below 7! 2^7 in magnitude
        int deg = 0;
        for (int j = 0; j < 8; j++) {
            if (j == i) continue;
            for (int c = ++deg; c > 0; c--) num[c] = num[c - 1] - j * num[c];
            num[0] *= -j;
            den *= i - j;
        }
        u64 d[4], d_inv[4], v[4];
        host_from_int(H2_FP, d, den);
        host_inv(H2_FP, d_inv, d);
        for (int c = 0; c < 8; c++) {
            host_from_int(H2_FP, v, num[c]);
            host_mul(H2_FP, matrix[8 * c + i], v, d_inv);
        }
    }
}

}  // namespace

void ecc_fixed_release_workspaces() { g_ecc_fixed_ctxs.release_current_device(); }   // h2_trim

}  // namespace h2

using namespace h2;

// The host side of a table build.  Every array the asynchronous copies read or write belongs to the caller below, which does not
// return, on any path, with work pending on the stream.
struct TableHost {
    std::vector<u64> bases, scalars;
    u64 matrix[64][4];
    std::vector<unsigned long long> z;
    std::vector<u32> active;
};
static int tables_run(TableHost &host, unsigned nw, uint64_t limit, char *scratch, void *d_points, void *d_lagrange, void *d_z, void *d_u,
                      hipStream_t st) {
    const u32 entries = 8 * nw;
    // scratch: the base once per entry, the entries' scalars, the interpolation matrix, the product's status, the unfinished windows
    const size_t off_scalars = (size_t)64 * entries, off_matrix = off_scalars + (size_t)32 * entries, off_status = off_matrix + 64 * 32,
                 off_active = off_status + 32 * nw;
    H2_HIP(hipMemcpyAsync(scratch, host.bases.data(), (size_t)64 * entries, hipMemcpyHostToDevice, st));
    H2_HIP(hipMemcpyAsync(scratch + off_scalars, host.scalars.data(), (size_t)32 * entries, hipMemcpyHostToDevice, st));
    H2_HIP(hipMemcpyAsync(scratch + off_matrix, host.matrix, sizeof host.matrix, hipMemcpyHostToDevice, st));
    int rc = h2_ecc_mul_device(scratch, scratch + off_scalars, entries, d_points, scratch + off_status, st);
    if (rc != H2_OK) return rc;
    hipLaunchKernelGGL(ecc_fixed_lagrange, dim3(grid_of(entries, kFT)), dim3(kFT), 0, st, (const u32 *)d_points, (const u32 *)(scratch + off_matrix),
                       entries, (u32 *)d_lagrange);
    H2_HIP(hipGetLastError());
    H2_HIP(hipMemcpyAsync(d_z, host.z.data(), (size_t)8 * nw, hipMemcpyHostToDevice, st));
    for (uint64_t first = 0; !host.active.empty(); first += kSearchRound) {
        if (first >= limit) {
            set_last_error_msg("h2_ecc_fixed_tables_device: a window has no z below z_limit");
            return H2_ERR_NOTFOUND;
        }
        const uint64_t span = limit - first < kSearchRound ? limit - first : kSearchRound;
        H2_HIP(hipMemcpyAsync(scratch + off_active, host.active.data(), 4 * host.active.size(), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(ecc_fixed_search, dim3(grid_of(span, kFT), (unsigned)host.active.size()), dim3(kFT), 0, st, (const u32 *)d_points,
                           (const u32 *)(scratch + off_active), (u64)first, (u64)limit, (unsigned long long *)d_z);
        H2_HIP(hipGetLastError());
        H2_HIP(hipMemcpyAsync(host.z.data(), d_z, (size_t)8 * nw, hipMemcpyDeviceToHost, st));
        H2_HIP(hipStreamSynchronize(st));                  // the round is over: its minima stand
        host.active.clear();
        for (unsigned w = 0; w < nw; w++)
            if (host.z[w] == kNoZ) host.active.push_back(w);
    }
    hipLaunchKernelGGL(ecc_fixed_roots, dim3(grid_of(entries, kFT)), dim3(kFT), 0, st, (const u32 *)d_points, (const unsigned long long *)d_z, entries,
                       (u32 *)d_u);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

extern "C" int h2_ecc_fixed_tables_device(const uint64_t *base_xy, unsigned num_windows, uint64_t z_limit, void *d_points, void *d_lagrange,
                                          void *d_z, void *d_u, void *stream) {
    if (!base_xy || num_windows < kMinWindows || num_windows > kMaxWindows || !d_points || !d_lagrange || !d_z || !d_u) return H2_ERR_ARGS;
    if (!host_on_curve(base_xy)) return H2_ERR_ARGS;       // the identity, (0, 0), is not on the curve either
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    const unsigned nw = num_windows;
    hipStream_t st = (hipStream_t)stream;
    ScratchContext &ctx = g_ecc_fixed_ctxs.get(st);
    std::lock_guard<std::mutex> lk(ctx.mu);
    if ((rc = ctx.scratch.reserve((size_t)(64 + 32) * 8 * nw + 64 * 32 + 32 * nw + 4 * nw)) != H2_OK) return rc;
    TableHost host;
    host.bases.resize((size_t)64 * nw);
    for (u32 e = 0; e < 8 * nw; e++) memcpy(&host.bases[8 * e], base_xy, 64);
    window_scalars(nw, host.scalars);
    lagrange_matrix(host.matrix);
    host.z.assign(nw, kNoZ);
    host.active.resize(nw);
    for (unsigned w = 0; w < nw; w++) host.active[w] = w;
    rc = tables_run(host, nw, z_limit ? z_limit : kDefaultZLimit, ctx.scratch.as<char>(), d_points, d_lagrange, d_z, d_u, st);
    // `host` is read and written by copies on the stream: idle before it goes, whatever tables_run returned
    const hipError_t e = hipStreamSynchronize(st);
    if (rc == H2_OK) H2_HIP(e);
    return rc;
}

extern "C" int h2_ecc_mul_fixed_device(const void *d_points, unsigned num_windows, const void *d_scalars, size_t n, void *d_out_xy,
                                       void *stream) {
    if (num_windows < kMinWindows || num_windows > kMaxWindows || n > kMaxMuls || (n && (!d_points || !d_scalars || !d_out_xy)))
        return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!n) return H2_OK;
    hipLaunchKernelGGL(ecc_fixed_mul, dim3(grid_of(n, kFT)), dim3(kFT), 0, (hipStream_t)stream, (const u32 *)d_points, num_windows,
                       (const u32 *)d_scalars, n, (u32 *)d_out_xy);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

extern "C" int h2_ecc_mul_fixed_trace_device(const void *d_points, const void *d_u, unsigned num_windows, const void *d_scalars, size_t count,
                                             void *d_columns, void *d_aux, void *stream) {
    if (num_windows < kMinWindows || num_windows > kMaxWindows || count > kMaxMuls ||
        (count && (!d_points || !d_u || !d_scalars || !d_columns || !d_aux)))
        return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!count) return H2_OK;
    hipStream_t st = (hipStream_t)stream;
    ScratchContext &ctx = g_ecc_fixed_ctxs.get(st);
    std::lock_guard<std::mutex> lk(ctx.mu);
    // num_windows - 2 elements per lane; two windows have none, and pass B runs alone
    return two_pass_trace(ctx.scratch, count, num_windows - 2, kTraceScratchElems, st, [&](bool emit, size_t first, size_t chunk, u32 *scratch) {
        hipLaunchKernelGGL(!emit ? ecc_fixed_trace<false> : ecc_fixed_trace<true>, dim3(grid_of(chunk, kFT)), dim3(kFT), 0, st,
                           (const u32 *)d_points, (const u32 *)d_u, num_windows, (const u32 *)d_scalars, first, chunk, count, scratch,
                           (u32 *)d_columns, (u32 *)d_aux);
        return H2_OK;
    });
}
