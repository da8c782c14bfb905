// `dev::MockProver::verify` over device-resident columns (halo2_proofs/src/dev.rs:576-904): which constraints does a witness break?
// Three checks, each leaving one bit per row in a bit plane (a 64-bit wave ballot per wave, written by one lane) and exact counts:
//   * h2_check_expressions_device  the gate polynomials at every row with the Real / Poison algebra of dev.rs:104-156: the bytecode of
//                                  evaluator.cuh (Lagrange basis), several programs per launch, a poison bit beside every stack slot;
//   * h2_lookup_check_device       exact membership of input tuples among table tuples (dev.rs:709-833): every component is replaced
//                                  by its rank in the sorted table column, up to seven ranks pack into one 224-bit key whose order
//                                  is the tuples' lexicographic order, the packed table keys are sorted (lookup.hip's bitonic
//                                  network) and the packed input keys binary-searched;
//   * h2_permutation_check_device  one gather and one 256-bit compare per cell of the copy-constraint mapping (dev.rs:835-881).
// A satisfied circuit costs the caller one read of the counts; the planes are fetched only for what failed.  None of the three
// synchronises or allocates per call beyond the grow-only workspaces of its (device, stream) context.
// A fourth check works on the regions a circuit's synthesis recorded, not on values: h2_cells_assigned_check (dev.rs:581-641), host
// memory in and out like h2_points_sum.  ra_mark paints who assigned each cell into an owner plane, ra_check asks it about every cell
// an enabled gate queries; the records are born on the host and the answer is read there, so this one synchronises.
#include <algorithm>
#include <vector>

#include "common.h"
#include "evaluator.cuh"
#include "field.cuh"
#include "host_field.h"
#include "lookup_keys.cuh"

namespace h2 {

namespace {

constexpr u32 kAbsent = 0xFFFFFFFFu;   // rank of an input value (or packed key) that its table column does not hold

// adds a wave's ballot to the workgroup's counter (lane 0 of every wave), the workgroup's sum to the global one (thread 0)
__device__ __forceinline__ void mp_count_wave(u32 *s_cnt, unsigned long long ballot) {
    if ((threadIdx.x & 63) == 0 && ballot) atomicAdd(s_cnt, (u32)__popcll(ballot));
}

// One lane per row, every program in turn.  fe_mulx and fe_add return fully reduced values and the columns hold values below p,
// so `fe_is_zero` (all limbs zero) is exact for a Montgomery value: x R = 0 mod p iff x = 0.
template <int F>
__global__ void __launch_bounds__(kEvalThreads) mp_check(const u32 *__restrict__ programs, const u32 *__restrict__ offsets, u32 n_programs,
                                                         const u32 *__restrict__ consts, const u32 *const *__restrict__ polys,
                                                         const unsigned char *__restrict__ is_advice, unsigned log_len, u32 usable,
                                                         unsigned long long *__restrict__ nz_bits, unsigned long long *__restrict__ po_bits,
                                                         u32 *__restrict__ counts, u32 *const *__restrict__ values) {
    extern __shared__ __attribute__((aligned(16))) u32 lds[];
    const size_t len = (size_t)1 << log_len, i = (size_t)blockIdx.x * kEvalThreads + threadIdx.x;
    const size_t words = (len + 63) >> 6;
    const bool active = i < len;          // 2^log_len < 64: the rest of the wave votes 0 (no early return: ballots and barriers below)
    for (u32 p = 0; p < n_programs; ++p) {
        fe top = fe_zero();
        bool ptop = false;                // the top of the stack is Poison
        u32 pbits = 0;                    // bit l: stack level l (spilled to LDS) is Poison
        if (active) {
            int depth = 0;
            const u32 end = offsets[p + 1];
            for (u32 pc = offsets[p]; pc < end; ++pc) {
                const u32 word = programs[pc], op = word & 0xFFu, arg = word >> 8;
                if (op == EV_POLY || op == EV_CONST) {
                    if (depth > 0) {
                        ev_spill(lds, depth - 1, top);
                        pbits = (pbits & ~(1u << (depth - 1))) | ((ptop ? 1u : 0u) << (depth - 1));
                    }
                    ++depth;
                    if (op == EV_POLY) {
                        const int shift = (int)programs[++pc];
                        const size_t j = (i + (size_t)((long long)shift + (long long)len)) & (len - 1);   // |shift| <= len
                        top = fe_load(polys[arg] + 8 * j);
                        ptop = is_advice[arg] && j >= usable;                                             // dev.rs:529-533
                    } else {
                        top = fe_load(consts + 8 * (size_t)arg);
                        ptop = false;
                    }
                } else if (op == EV_SCALE) {                                                              // Mul<F>, dev.rs:144-156
                    const fe c = fe_load(consts + 8 * (size_t)arg);
                    if (ptop && fe_is_zero(c)) {
                        top = fe_zero();
                        ptop = false;
                    } else if (!ptop) {
                        top = fe_mulx<F>(top, c);
                    }
                } else {
                    fe below = ev_fill(lds, depth - 2);
                    bool pbelow = (pbits >> (depth - 2)) & 1u;
                    --depth;
                    if (op == EV_MULADD) {                                                                // SCALE of the accumulator, then ADD
                        const fe c = fe_load(consts + 8 * (size_t)arg);
                        if (pbelow && fe_is_zero(c)) {
                            below = fe_zero();
                            pbelow = false;
                        } else if (!pbelow) {
                            below = fe_mulx<F>(below, c);
                        }
                    }
                    if (op == EV_MUL) {                                                                   // dev.rs:126-142
                        if (!pbelow && !ptop) {
                            top = fe_mulx<F>(below, top);
                        } else if ((!pbelow && fe_is_zero(below)) || (!ptop && fe_is_zero(top))) {
                            top = fe_zero();
                            ptop = false;
                        } else {
                            ptop = true;
                        }
                    } else {                                                                              // dev.rs:115-124
                        ptop = ptop || pbelow;
                        if (!ptop) top = fe_add<F>(below, top);
                    }
                }
            }
        }
        const bool nz = active && !ptop && !fe_is_zero(top), po = active && ptop;
        const unsigned long long bn = __ballot(nz), bp = __ballot(po);
        if ((threadIdx.x & 63) == 0 && (i >> 6) < words) {
            nz_bits[(size_t)p * words + (i >> 6)] = bn;
            po_bits[(size_t)p * words + (i >> 6)] = bp;
        }
        if (values && active) fe_store(values[p] + 8 * i, ptop ? fe_zero() : top);
        // counts: the stack's LDS is dead once every lane is through the program, so its first two words hold the workgroup's sums
        // (the kernel's 64 KiB stay 64 KiB).  A workgroup with no bit set -- every one of a satisfied circuit -- pays one barrier.
        if (!__syncthreads_or((bn | bp) != 0)) continue;
        if (threadIdx.x == 0) lds[0] = lds[1] = 0;
        __syncthreads();
        mp_count_wave(&lds[0], bn);
        mp_count_wave(&lds[1], bp);
        __syncthreads();
        if (threadIdx.x == 0) {
            if (lds[0]) atomicAdd(&counts[2 * p], lds[0]);
            if (lds[1]) atomicAdd(&counts[2 * p + 1], lds[1]);
        }
        __syncthreads();
    }
}

// Slot `slot` of the packed keys of `rows` rows <- the rank of src[r] in the sorted table column S (n_s entries): its lower bound.
// Equal values share a rank and the order of ranks is the order of values.  Poison ranks one past the largest (n_s).  An INPUT value
// the column does not hold would share the rank of the next larger one: it gets kAbsent instead, which no table key carries.
// init: the key is created ({rank, 0 ...}); the table's rows in [rows, padded) become the all-ones padding the sort wants.
template <int F>
__global__ void __launch_bounds__(256) mp_rank_column(const u32 *__restrict__ S, u32 n_s, const u32 *__restrict__ src,
                                                      const unsigned long long *__restrict__ poison, int from_mont, u32 rows, u32 padded,
                                                      u32 *__restrict__ packed, int slot, int init, int is_input) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) {
        if (init && r < padded) key_store(packed + 8 * (size_t)r, key256{{~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u}});
        return;
    }
    u32 rank;
    if (poison && ((poison[r >> 6] >> (r & 63)) & 1ull)) {
        rank = n_s;
    } else {
        fe v = fe_load(src + 8 * (size_t)r);
        if (from_mont) v = fe_from_mont<F>(v);
        key256 key;
#pragma unroll
        for (int q = 0; q < 8; ++q) key.v[q] = v.v[q];
        rank = lower_bound(S, n_s, key);
        if (is_input && (rank >= n_s || !key_eq(key_load(S + 8 * (size_t)rank), key))) rank = kAbsent;
    }
    if (init) {
        key256 k{{0, 0, 0, 0, 0, 0, 0, 0}};
        k.v[6 - slot] = rank;
        key_store(packed + 8 * (size_t)r, k);
    } else {
        packed[8 * (size_t)r + (6 - slot)] = rank;
    }
}

// seven ranks are one key: the key's own rank among the sorted packed table keys becomes slot 0 of the next group
__global__ void __launch_bounds__(256) mp_rank_packed(const u32 *__restrict__ S, u32 n_s, u32 rows, u32 *__restrict__ packed, int is_input) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const key256 key = key_load(packed + 8 * (size_t)r);
    u32 rank = lower_bound(S, n_s, key);
    if (is_input && (rank >= n_s || !key_eq(key_load(S + 8 * (size_t)rank), key))) rank = kAbsent;
    key256 k{{0, 0, 0, 0, 0, 0, 0, 0}};
    k.v[6] = rank;
    key_store(packed + 8 * (size_t)r, k);
}

// fail bit of row r < rows: its packed key is not among the sorted packed table keys.  Covers ceil(n / 64) words.
__global__ void __launch_bounds__(256) mp_member(const u32 *__restrict__ S, u32 n_s, const u32 *__restrict__ packed, u32 rows, u32 n,
                                                 unsigned long long *__restrict__ fail_bits, u32 *__restrict__ count) {
    __shared__ u32 s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    bool fail = false;
    if (r < rows) {
        const key256 key = key_load(packed + 8 * (size_t)r);
        const u32 p = lower_bound(S, n_s, key);
        fail = p >= n_s || !key_eq(key_load(S + 8 * (size_t)p), key);
    }
    const unsigned long long b = __ballot(fail);
    if ((threadIdx.x & 63) == 0 && (r >> 6) < (n + 63) / 64) fail_bits[r >> 6] = b;
    mp_count_wave(&s_cnt, b);
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(count, s_cnt);
}

// cell (c, r) against the cell its mapping entry names; blockIdx.y = c
__global__ void __launch_bounds__(256) mp_permutation(const u32 *const *__restrict__ cols, const unsigned char *__restrict__ is_advice, u32 n_cols,
                                                      const long long *__restrict__ mapping, unsigned log_len, u32 usable,
                                                      unsigned long long *__restrict__ fail_bits, u32 *__restrict__ counts) {
    __shared__ u32 s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const size_t len = (size_t)1 << log_len, words = (len + 63) >> 6;
    const u32 c = blockIdx.y;
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool fail = false;
    if (r < len) {
        const long long m = mapping[(size_t)c * len + r];
        const unsigned long long c2 = (unsigned long long)m >> log_len;
        const size_t r2 = (size_t)m & (len - 1);
        if (m < 0 || c2 >= n_cols) {
            fail = true;
        } else {
            const bool pa = is_advice[c] && r >= usable, pb = is_advice[c2] && r2 >= usable;
            if (pa || pb) fail = !(pa && pb && cols[c] == cols[c2] && r == r2);       // CellValue::Poison(usize): equal to itself only
            else fail = !fe_eq(fe_load(cols[c] + 8 * r), fe_load(cols[c2] + 8 * r2));
        }
    }
    const unsigned long long b = __ballot(fail);
    if ((threadIdx.x & 63) == 0 && (r >> 6) < words) fail_bits[(size_t)c * words + (r >> 6)] = b;
    mp_count_wave(&s_cnt, b);
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(&counts[c], s_cnt);
}

// ---- the regions' check (dev.rs:581-641): is every cell that an enabled gate queries assigned by the region that enabled it? ----------
// ra_mark: one lane per ASSIGNED CELL, not per range.  `prefix` holds the exclusive prefix sums of the ranges' counts (n_ranges + 1
// entries, 64-bit, from the host); lane i finds the last range r with prefix[r] <= i (ranges of no cells share a prefix value and are
// stepped over) and claims cell i - prefix[r] of it in the owner plane: 0 = unassigned, region + 1 = owned.  A cell that another region
// holds already is a conflict; the same region assigning a cell twice is not.
__global__ void __launch_bounds__(256) ra_mark(const u32 *__restrict__ ranges, const unsigned long long *__restrict__ prefix, u32 n_ranges,
                                               unsigned long long total, u32 *__restrict__ owner, unsigned log_len,
                                               unsigned long long *__restrict__ conflicts) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    bool conflict = false;
    if (i < total) {
        u32 lo = 0, hi = n_ranges;                       // prefix[lo] <= i < prefix[hi]
        while (hi - lo > 1) {
            const u32 mid = lo + (hi - lo) / 2;
            if (prefix[mid] <= i) lo = mid;
            else hi = mid;
        }
        const u32 *r = ranges + 4 * (size_t)lo;
        const size_t at = ((size_t)r[0] << log_len) + r[1] + (size_t)(i - prefix[lo]);
        const u32 want = r[3] + 1, old = atomicCAS(&owner[at], 0u, want);
        conflict = old != 0 && old != want;
    }
    const unsigned long long b = __ballot(conflict);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(conflicts, (unsigned long long)__popcll(b));
}

// ra_check: one (gate, selector) pair per launch, one lane per enable event of the selector, every queried cell of the gate in turn.
// cells: (column code, rotation) pairs; a code is a plane index or 0x80000000 | instance column.  planes: n_cells planes of `words`
// 64-bit words, cell-major; bit e of plane c: cell c of event e is not assigned.  Consecutive events are mostly consecutive rows of
// one region, so a wave's owner reads are one or two cache lines per cell.
__global__ void __launch_bounds__(256) ra_check(const u32 *__restrict__ event_rows, const u32 *__restrict__ event_regions, size_t n_events,
                                                const u32 *__restrict__ cells, u32 n_cells, const u32 *__restrict__ owner, unsigned log_len,
                                                const unsigned long long *__restrict__ instance_lens, unsigned long long *__restrict__ planes,
                                                size_t words, unsigned long long *__restrict__ count) {
    __shared__ u32 s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, len = (size_t)1 << log_len;
    const bool active = e < n_events;                    // no early return: the ballots below want the whole wave
    const u32 row = active ? event_rows[e] : 0, want = active ? event_regions[e] + 1 : 0;
    for (u32 c = 0; c < n_cells; ++c) {
        const u32 code = cells[2 * c];
        const int rotation = (int)cells[2 * c + 1];
        bool fail = false;
        if (active) {
            const size_t cell_row = (size_t)((long long)row + rotation) & (len - 1);          // dev.rs:603
            if (code & 0x80000000u) fail = cell_row >= instance_lens[code & 0x7FFFFFFFu];      // InstanceValue::Padding, dev.rs:606-619
            else fail = owner[((size_t)code << log_len) + cell_row] != want;
        }
        const unsigned long long b = __ballot(fail);
        if ((threadIdx.x & 63) == 0 && (e >> 6) < words) planes[(size_t)c * words + (e >> 6)] = b;
        mp_count_wave(&s_cnt, b);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(count, (unsigned long long)s_cnt);
}

struct MockContext {
    std::mutex mu;
    DevBuf prog, offsets, consts, ptrs, flags, vals;      // staging of the expression / permutation checks
    std::vector<u32> offs;                                // program offsets as the kernel reads them
    DevBuf sorted, pack_t, pack_i;                        // lookup check: a sorted column or sorted packed keys; packed table / input keys
    DevBuf ra_ranges, ra_prefix, ra_owner, ra_events, ra_cells, ra_lens, ra_planes, ra_counts;      // the regions' check
    std::vector<unsigned long long> ra_host;              // its host staging: the prefix sums going up, counts and planes coming back
    void release_all() {
        ra_ranges.release();
        ra_prefix.release();
        ra_owner.release();
        ra_events.release();
        ra_cells.release();
        ra_lens.release();
        ra_planes.release();
        ra_counts.release();
        prog.release();
        offsets.release();
        consts.release();
        ptrs.release();
        flags.release();
        vals.release();
        sorted.release();
        pack_t.release();
        pack_i.release();
    }
};
StreamContexts<MockContext> g_mock_ctxs;

}  // namespace

void mock_release_workspaces() { g_mock_ctxs.release_current_device(); }

}  // namespace h2

using namespace h2;

extern "C" int h2_check_expressions_device(int field, const uint32_t *programs, const size_t *prog_offsets, size_t n_programs,
                                           const uint64_t *consts, size_t n_consts, const void *const *d_polys, const uint8_t *poly_is_advice,
                                           size_t n_polys, unsigned log_len, size_t usable_rows, void *d_nonzero_bits, void *d_poison_bits,
                                           void *d_counts, void *const *d_values, void *stream) {
    if ((field != H2_FP && field != H2_FQ) || !programs || !prog_offsets || n_programs == 0 || n_programs > 4096 || log_len > 30 ||
        (n_consts && !consts) || (n_polys && (!d_polys || !poly_is_advice)) || !d_nonzero_bits || !d_poison_bits || !d_counts)
        return H2_ERR_ARGS;
    const size_t len = (size_t)1 << log_len;
    if (usable_rows > len) return H2_ERR_ARGS;
    const size_t n_words = prog_offsets[n_programs];
    if (n_words == 0 || n_words > ((size_t)1 << 20)) return H2_ERR_ARGS;
    for (size_t p = 0; p <= n_programs; ++p) {
        if (prog_offsets[p] > n_words || (p && prog_offsets[p] <= prog_offsets[p - 1])) return H2_ERR_ARGS;
    }
    for (size_t p = 0; p < n_programs; ++p) {
        // a Lagrange-basis program without LINEAR, which lowered expressions do not have
        if (!ev_program_ok(programs, prog_offsets[p], prog_offsets[p + 1], n_consts, d_polys, n_polys, len, 1, nullptr)) return H2_ERR_ARGS;
        if (d_values && !d_values[p]) return H2_ERR_ARGS;
    }
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    MockContext &cx = g_mock_ctxs.get(st);
    std::lock_guard<std::mutex> lk(cx.mu);
    if ((rc = cx.prog.reserve(n_words * 4)) != H2_OK || (rc = cx.offsets.reserve((n_programs + 1) * 4)) != H2_OK ||
        (rc = cx.consts.reserve(n_consts * 32 + 32)) != H2_OK || (rc = cx.ptrs.reserve(n_polys * 8 + 8)) != H2_OK ||
        (rc = cx.flags.reserve(n_polys + 8)) != H2_OK || (rc = cx.vals.reserve(n_programs * 8)) != H2_OK)
        return rc;
    // the staging buffers belong to this (device, stream): the copies are stream-ordered after the kernel that last read them
    H2_HIP(hipMemcpyAsync(cx.prog.ptr, programs + prog_offsets[0], (n_words - prog_offsets[0]) * 4, hipMemcpyHostToDevice, st));
    cx.offs.resize(n_programs + 1);                  // lives in the context: the copy below may outlast this call
    for (size_t p = 0; p <= n_programs; ++p) cx.offs[p] = (u32)(prog_offsets[p] - prog_offsets[0]);
    H2_HIP(hipMemcpyAsync(cx.offsets.ptr, cx.offs.data(), cx.offs.size() * 4, hipMemcpyHostToDevice, st));
    if (n_consts) H2_HIP(hipMemcpyAsync(cx.consts.ptr, consts, n_consts * 32, hipMemcpyHostToDevice, st));
    if (n_polys) {
        H2_HIP(hipMemcpyAsync(cx.ptrs.ptr, d_polys, n_polys * 8, hipMemcpyHostToDevice, st));
        H2_HIP(hipMemcpyAsync(cx.flags.ptr, poly_is_advice, n_polys, hipMemcpyHostToDevice, st));
    }
    if (d_values) H2_HIP(hipMemcpyAsync(cx.vals.ptr, d_values, n_programs * 8, hipMemcpyHostToDevice, st));
    H2_HIP(hipMemsetAsync(d_counts, 0, n_programs * 8, st));
    const dim3 grid((unsigned)((len + kEvalThreads - 1) / kEvalThreads)), block(kEvalThreads);
    const size_t lds = (size_t)kEvalDepth * 8 * kEvalThreads * 4;
    u32 *const *vals = d_values ? (u32 *const *)cx.vals.ptr : nullptr;
    H2_FIELD_LAUNCH(field, mp_check, grid, block, lds, st, cx.prog.as<u32>(), cx.offsets.as<u32>(), (u32)n_programs, cx.consts.as<u32>(),
                    (const u32 *const *)cx.ptrs.ptr, cx.flags.as<unsigned char>(), log_len, (u32)usable_rows,
                    (unsigned long long *)d_nonzero_bits, (unsigned long long *)d_poison_bits, (u32 *)d_counts, vals);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

extern "C" int h2_lookup_check_device(int field, const void *const *d_inputs, const void *const *d_input_poison, const void *const *d_tables,
                                      const void *const *d_table_poison, size_t w, size_t n, size_t usable_rows, int form, void *d_fail_bits,
                                      void *d_count, void *stream) {
    if ((field != H2_FP && field != H2_FQ) || (form != H2_FORM_CANONICAL && form != H2_FORM_MONTGOMERY) || !d_inputs || !d_tables || w == 0 ||
        w > 4096 || n == 0 || n > ((size_t)1 << 30) || usable_rows > n || !d_fail_bits || !d_count)
        return H2_ERR_ARGS;
    for (size_t c = 0; c < w; ++c) {
        if (!d_inputs[c] || !d_tables[c]) return H2_ERR_ARGS;
    }
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    H2_HIP(hipMemsetAsync(d_count, 0, 4, st));
    const u32 rows = (u32)usable_rows, un = (u32)n;
    const int log_p = ceil_log2(rows ? rows : 1);
    const u32 padded = 1u << log_p;
    MockContext &cx = g_mock_ctxs.get(st);
    std::lock_guard<std::mutex> lk(cx.mu);
    if ((rc = cx.sorted.reserve((size_t)padded * 32)) != H2_OK || (rc = cx.pack_t.reserve((size_t)padded * 32)) != H2_OK ||
        (rc = cx.pack_i.reserve((size_t)padded * 32)) != H2_OK)
        return rc;
    const dim3 block(256), grid_t((padded + 255) / 256), grid_i((rows + 255) / 256 + (rows ? 0 : 1));
    const int from_mont = form == H2_FORM_MONTGOMERY;
    u32 *S = nullptr;
    // the packed table keys, sorted: what a full group's keys are ranked in and what the input keys are searched in at the end
    auto sort_packed = [&]() -> int {
        H2_HIP(hipMemcpyAsync(cx.sorted.ptr, cx.pack_t.ptr, (size_t)padded * 32, hipMemcpyDeviceToDevice, st));
        return lookup_sort_padded(cx.sorted.as<u32>(), log_p, st);
    };
    int slot = 0;
    for (size_t c = 0; rows && c < w; ++c) {
        if (slot == 7) {
            if ((rc = sort_packed()) != H2_OK) return rc;
            S = cx.sorted.as<u32>();
            hipLaunchKernelGGL(mp_rank_packed, grid_i, block, 0, st, (const u32 *)S, rows, rows, cx.pack_t.as<u32>(), 0);
            hipLaunchKernelGGL(mp_rank_packed, grid_i, block, 0, st, (const u32 *)S, rows, rows, cx.pack_i.as<u32>(), 1);
            slot = 1;
        }
        if ((rc = lookup_prepare_and_sort(field, d_tables[c], rows, form, cx.sorted, st)) != H2_OK) return rc;
        S = cx.sorted.as<u32>();
        const unsigned long long *pt = d_table_poison ? (const unsigned long long *)d_table_poison[c] : nullptr;
        const unsigned long long *pi = d_input_poison ? (const unsigned long long *)d_input_poison[c] : nullptr;
        const int init = c == 0;
        H2_FIELD_LAUNCH(field, mp_rank_column, grid_t, block, 0, st, (const u32 *)S, rows, (const u32 *)d_tables[c], pt, from_mont, rows, padded,
                        cx.pack_t.as<u32>(), slot, init, 0);
        H2_FIELD_LAUNCH(field, mp_rank_column, grid_i, block, 0, st, (const u32 *)S, rows, (const u32 *)d_inputs[c], pi, from_mont, rows, 0u,
                        cx.pack_i.as<u32>(), slot, init, 1);
        ++slot;
    }
    if (rows && (rc = sort_packed()) != H2_OK) return rc;
    const u32 lanes = ((un + 63) / 64) * 64;
    hipLaunchKernelGGL(mp_member, dim3((lanes + 255) / 256), block, 0, st, (const u32 *)cx.sorted.ptr, rows, (const u32 *)cx.pack_i.ptr, rows, un,
                       (unsigned long long *)d_fail_bits, (u32 *)d_count);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

extern "C" int h2_permutation_check_device(int field, const void *const *d_columns, const uint8_t *column_is_advice, size_t n_columns,
                                           const void *d_mapping, unsigned log_len, size_t usable_rows, int form, void *d_fail_bits,
                                           void *d_counts, void *stream) {
    if ((field != H2_FP && field != H2_FQ) || (form != H2_FORM_CANONICAL && form != H2_FORM_MONTGOMERY) || !d_columns || !column_is_advice ||
        n_columns == 0 || n_columns > 65535 || !d_mapping || log_len > 30 || usable_rows > ((size_t)1 << log_len) || !d_fail_bits || !d_counts)
        return H2_ERR_ARGS;
    for (size_t c = 0; c < n_columns; ++c) {
        if (!d_columns[c]) return H2_ERR_ARGS;
    }
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    MockContext &cx = g_mock_ctxs.get(st);
    std::lock_guard<std::mutex> lk(cx.mu);
    if ((rc = cx.ptrs.reserve(n_columns * 8)) != H2_OK || (rc = cx.flags.reserve(n_columns)) != H2_OK) return rc;
    H2_HIP(hipMemcpyAsync(cx.ptrs.ptr, d_columns, n_columns * 8, hipMemcpyHostToDevice, st));
    H2_HIP(hipMemcpyAsync(cx.flags.ptr, column_is_advice, n_columns, hipMemcpyHostToDevice, st));
    H2_HIP(hipMemsetAsync(d_counts, 0, n_columns * 4, st));
    const size_t len = (size_t)1 << log_len, lanes = ((len + 63) / 64) * 64;
    hipLaunchKernelGGL(mp_permutation, dim3((unsigned)((lanes + 255) / 256), (unsigned)n_columns), dim3(256), 0, st, (const u32 *const *)cx.ptrs.ptr,
                       cx.flags.as<unsigned char>(), (u32)n_columns, (const long long *)d_mapping, log_len, (u32)usable_rows,
                       (unsigned long long *)d_fail_bits, (u32 *)d_counts);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

namespace h2 {
namespace {

struct RegionCheckArgs {
    unsigned log_len;
    size_t n_planes;
    const uint32_t *ranges;
    size_t n_ranges;
    const uint64_t *instance_lens;
    size_t n_instance;
    const uint32_t *event_rows, *event_regions;
    const size_t *selector_offsets;
    size_t n_selectors;
    const uint32_t *pair_selector;
    const size_t *pair_cell_offsets;
    size_t n_pairs;
    const uint32_t *cells;
    uint64_t *counts;
    uint32_t *records;
    size_t max_records, *n_records;
    uint64_t *n_conflicts;
};

// everything h2_cells_assigned_check refuses, decided before a device is looked for and before an output is written
bool region_check_args_ok(const RegionCheckArgs &a) {
    if (a.log_len > 30 || a.n_planes > 65535 || a.n_instance > 0x7FFFFFFFu || a.n_pairs > 0xFFFFFFFFu || !a.selector_offsets ||
        !a.pair_cell_offsets || !a.n_records || !a.n_conflicts || (a.n_ranges && !a.ranges) || (a.n_instance && !a.instance_lens) ||
        (a.n_pairs && (!a.pair_selector || !a.counts)) || (a.max_records && !a.records))
        return false;
    const size_t len = (size_t)1 << a.log_len;
    unsigned long long total = 0;
    for (size_t r = 0; r < a.n_ranges; ++r) {
        const uint32_t *g = a.ranges + 4 * r;
        if (g[0] >= a.n_planes || (unsigned long long)g[1] + g[2] > len || g[3] == 0xFFFFFFFFu) return false;
        total += g[2];
    }
    if (total >> 32) return false;
    for (size_t s = 0; s < a.n_selectors; ++s) {
        if (a.selector_offsets[s + 1] < a.selector_offsets[s]) return false;
    }
    const size_t n_events = a.selector_offsets[a.n_selectors] - a.selector_offsets[0];
    if (a.selector_offsets[0] != 0 || n_events > 0xFFFFFFFFu || (n_events && (!a.event_rows || !a.event_regions))) return false;
    for (size_t e = 0; e < n_events; ++e) {
        if (a.event_rows[e] >= len || a.event_regions[e] == 0xFFFFFFFFu) return false;
    }
    for (size_t p = 0; p < a.n_pairs; ++p) {
        if (a.pair_cell_offsets[p + 1] < a.pair_cell_offsets[p] || a.pair_selector[p] >= a.n_selectors) return false;
    }
    const size_t n_cells = a.pair_cell_offsets[a.n_pairs] - a.pair_cell_offsets[0];
    if (a.pair_cell_offsets[0] != 0 || n_cells > 0xFFFFFFFFu || (n_cells && !a.cells)) return false;
    for (size_t c = 0; c < n_cells; ++c) {
        const uint32_t code = a.cells[2 * c];
        if ((code & 0x80000000u) ? (code & 0x7FFFFFFFu) >= a.n_instance : code >= a.n_planes) return false;
    }
    return true;
}

int region_check_run(MockContext &cx, const RegionCheckArgs &a) {
    hipStream_t st = 0;
    const size_t len = (size_t)1 << a.log_len, n_events = a.selector_offsets[a.n_selectors], n_cells = a.pair_cell_offsets[a.n_pairs];
    // the planes: pair p has one plane per cell of ceil(events of its selector / 64) words, at plane_at[p]
    std::vector<size_t> plane_at(a.n_pairs + 1, 0);
    auto events_of = [&](size_t p) { return a.selector_offsets[a.pair_selector[p] + 1] - a.selector_offsets[a.pair_selector[p]]; };
    auto cells_of = [&](size_t p) { return a.pair_cell_offsets[p + 1] - a.pair_cell_offsets[p]; };
    for (size_t p = 0; p < a.n_pairs; ++p) plane_at[p + 1] = plane_at[p] + cells_of(p) * ((events_of(p) + 63) / 64);
    int rc;
    if ((rc = cx.ra_ranges.reserve(a.n_ranges * 16 + 16)) != H2_OK || (rc = cx.ra_prefix.reserve((a.n_ranges + 1) * 8)) != H2_OK ||
        (rc = cx.ra_owner.reserve(a.n_planes * len * 4 + 4)) != H2_OK || (rc = cx.ra_events.reserve(n_events * 8 + 8)) != H2_OK ||
        (rc = cx.ra_cells.reserve(n_cells * 8 + 8)) != H2_OK || (rc = cx.ra_lens.reserve(a.n_instance * 8 + 8)) != H2_OK ||
        (rc = cx.ra_planes.reserve(plane_at[a.n_pairs] * 8 + 8)) != H2_OK || (rc = cx.ra_counts.reserve((a.n_pairs + 1) * 8)) != H2_OK)
        return rc;
    std::vector<unsigned long long> &host = cx.ra_host;                     // lives in the context: the copies below are asynchronous
    host.assign(a.n_ranges + 1, 0);
    for (size_t r = 0; r < a.n_ranges; ++r) host[r + 1] = host[r] + a.ranges[4 * r + 2];
    const unsigned long long total = host[a.n_ranges];
    unsigned long long *d_counts = cx.ra_counts.as<unsigned long long>(), *d_conflicts = d_counts + a.n_pairs;
    H2_HIP(hipMemsetAsync(d_counts, 0, (a.n_pairs + 1) * 8, st));
    if (a.n_planes) H2_HIP(hipMemsetAsync(cx.ra_owner.ptr, 0, a.n_planes * len * 4, st));
    if (total) {
        H2_HIP(hipMemcpyAsync(cx.ra_ranges.ptr, a.ranges, a.n_ranges * 16, hipMemcpyHostToDevice, st));
        H2_HIP(hipMemcpyAsync(cx.ra_prefix.ptr, host.data(), (a.n_ranges + 1) * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(ra_mark, dim3(grid_of(total, 256)), dim3(256), 0, st, cx.ra_ranges.as<u32>(), cx.ra_prefix.as<unsigned long long>(),
                           (u32)a.n_ranges, total, cx.ra_owner.as<u32>(), a.log_len, d_conflicts);
        H2_HIP(hipGetLastError());
    }
    if (n_events) {
        H2_HIP(hipMemcpyAsync(cx.ra_events.ptr, a.event_rows, n_events * 4, hipMemcpyHostToDevice, st));
        H2_HIP(hipMemcpyAsync(cx.ra_events.as<u32>() + n_events, a.event_regions, n_events * 4, hipMemcpyHostToDevice, st));
    }
    if (n_cells) H2_HIP(hipMemcpyAsync(cx.ra_cells.ptr, a.cells, n_cells * 8, hipMemcpyHostToDevice, st));
    if (a.n_instance) H2_HIP(hipMemcpyAsync(cx.ra_lens.ptr, a.instance_lens, a.n_instance * 8, hipMemcpyHostToDevice, st));
    for (size_t p = 0; p < a.n_pairs; ++p) {
        const size_t events = events_of(p), first = a.selector_offsets[a.pair_selector[p]];
        if (!events || !cells_of(p)) continue;                              // a selector nobody enabled launches nothing
        hipLaunchKernelGGL(ra_check, dim3(grid_of(events, 256)), dim3(256), 0, st, cx.ra_events.as<u32>() + first,
                           cx.ra_events.as<u32>() + n_events + first, events, cx.ra_cells.as<u32>() + 2 * a.pair_cell_offsets[p], (u32)cells_of(p),
                           cx.ra_owner.as<u32>(), a.log_len, cx.ra_lens.as<unsigned long long>(), cx.ra_planes.as<unsigned long long>() + plane_at[p],
                           (events + 63) / 64, d_counts + p);
    }
    H2_HIP(hipGetLastError());
    std::vector<unsigned long long> got(a.n_pairs + 1);
    H2_HIP(hipMemcpyAsync(got.data(), d_counts, (a.n_pairs + 1) * 8, hipMemcpyDeviceToHost, st));
    H2_HIP(hipStreamSynchronize(st));
    // only the planes of a pair that failed somewhere come back; the first max_records set bits in the order (pair, event, cell)
    size_t written = 0;
    for (size_t p = 0; p < a.n_pairs && written < a.max_records; ++p) {
        if (!got[p]) continue;
        const size_t nc = cells_of(p), words = (events_of(p) + 63) / 64;
        host.resize(nc * words);
        H2_HIP(hipMemcpyAsync(host.data(), cx.ra_planes.as<unsigned long long>() + plane_at[p], nc * words * 8, hipMemcpyDeviceToHost, st));
        H2_HIP(hipStreamSynchronize(st));
        for (size_t w = 0; w < words && written < a.max_records; ++w) {
            unsigned long long any = 0;
            for (size_t c = 0; c < nc; ++c) any |= host[c * words + w];
            for (; any && written < a.max_records; any &= any - 1) {
                const int bit = __builtin_ctzll(any);
                for (size_t c = 0; c < nc && written < a.max_records; ++c) {
                    if (!((host[c * words + w] >> bit) & 1ull)) continue;
                    uint32_t *rec = a.records + 3 * written++;
                    rec[0] = (uint32_t)p;
                    rec[1] = (uint32_t)(w * 64 + bit);
                    rec[2] = (uint32_t)c;
                }
            }
        }
    }
    for (size_t p = 0; p < a.n_pairs; ++p) a.counts[p] = got[p];
    *a.n_records = written;
    *a.n_conflicts = got[a.n_pairs];
    return H2_OK;
}

}  // namespace
}  // namespace h2

extern "C" int h2_cells_assigned_check(unsigned log_len, size_t n_planes, const uint32_t *ranges, size_t n_ranges, const uint64_t *instance_lens,
                                       size_t n_instance, const uint32_t *event_rows, const uint32_t *event_regions, const size_t *selector_offsets,
                                       size_t n_selectors, const uint32_t *pair_selector, const size_t *pair_cell_offsets, size_t n_pairs,
                                       const uint32_t *cells, uint64_t *counts, uint32_t *records, size_t max_records, size_t *n_records,
                                       uint64_t *n_conflicts) {
    const RegionCheckArgs a{log_len, n_planes, ranges, n_ranges, instance_lens, n_instance, event_rows, event_regions, selector_offsets,
                            n_selectors, pair_selector, pair_cell_offsets, n_pairs, cells, counts, records, max_records, n_records, n_conflicts};
    if (!region_check_args_ok(a)) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    MockContext &cx = g_mock_ctxs.get(0);
    std::lock_guard<std::mutex> lk(cx.mu);
    rc = region_check_run(cx, a);
    if (rc != H2_OK) (void)hipStreamSynchronize(0);      // nothing enqueued may still read the caller's arrays after the return
    return rc;
}
