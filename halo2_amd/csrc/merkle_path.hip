// Sinsemilla Merkle PATHS over Pallas (halo2_gadgets sinsemilla/merkle.rs MerklePath::calculate_root, merkle/chip.rs hash_layer,
// utilities/cond_swap.rs), batched:
//
//   h2_sinsemilla_merkle_paths_device   n paths of `depth` layers: leaf, position, siblings -> every node up to the root, ONE launch
//   h2_sinsemilla_merkle_trace_device   what MerkleChip::hash_layer and CondSwapChip::swap assign outside the 53-row hash region, for
//                                       the layers [layer_lo, layer_hi) of every path, as whole column vectors
//
// The walk is one lane per path.  A layer is the 52-word chain  l || left || right  of sinsemilla.hip's MerkleCRH kernel, the words cut on
// the lane the same way, and its x coordinate is the next layer's node: the layers of one path are a dependent chain, so nothing is won
// by a launch per layer but `depth` launch latencies and a round trip of the nodes through memory.  A lane inverts once per layer, as
// the layer kernel does per hash.  Beside that kernel's live state it holds the node, the position and the layer counter.
//
// The trace is bit slicing of canonical 255-bit values: bound by its stores (736 bytes out per item for 64 in).  ONE LANE PER ITEM:
// the outputs are column vectors, so the lanes of a wave store consecutive elements of the same vector whichever cell it is; the
// vectors of two or three rows per item are stored at that stride.  No register is indexed by a variable, nothing goes to scratch.
//
// THE UNIT OWNS NO DEVICE MEMORY: no workspace, no cached table, no per-stream context.  Every buffer is the caller's, the stream
// travels in the descriptor, and h2_trim has nothing to release here.
#include "common.h"
#include "sinsemilla_chain.cuh"

namespace h2 {
namespace {

constexpr int kST = 256;                                   // lanes per workgroup
constexpr unsigned kMaxDepth = 32;                         // the reference's leaf_pos is a u32
constexpr size_t kMaxItems = (size_t)1 << 30;              // n * depth: what h2_sinsemilla_trace_device takes as `count`

// MerkleCRH of (left, right) at `layer` from Q -> the hash's x (Montgomery), zero and bottom = true where the chain has no value.
// left and right are CANONICAL.  The cut is sinsemilla.hip's: word 0 the layer, words 1-25 the low 250 bits of left, word 26 its top
// 5 bits under the low 5 of right, words 27-51 the remaining 250 bits of right.
__device__ __forceinline__ fe merkle_layer_x(const PointArg &q, u32 layer, const fe &left, const fe &right_, const u32 *__restrict__ table,
                                             bool &bottom) {
    xyzz<FP> a = start_at(q, bottom);
    u32 z[8], right[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        z[j] = left.v[j];
        right[j] = right_.v[j];
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
    const fe x = xyzz_to_affine<FP>(a).x;
    return bottom ? fe_zero() : x;
}

__device__ __forceinline__ fe fe_pick(bool second, const fe &a, const fe &b) {
    fe r;
#pragma unroll
    for (int j = 0; j < 8; j++) r.v[j] = second ? b.v[j] : a.v[j];
    return r;
}

__global__ void __launch_bounds__(kST) merkle_paths(const u32 *__restrict__ leaves, const u32 *__restrict__ siblings,
                                                    const u32 *__restrict__ positions, size_t n, u32 depth, PointArg q,
                                                    const u32 *__restrict__ table, u32 *__restrict__ nodes, uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * kST + threadIdx.x;
    if (i >= n) return;
    const u32 pos = positions[i];
    fe node = fe_load(leaves + 8 * i);                     // Montgomery, as it is stored
    u32 *out = nodes + 8 * i * (depth + 1);
    fe_store(out, node);
#pragma unroll 1
    for (u32 l = 0; l < depth; l++) {
        const fe sibling = fe_load(siblings + 8 * (i * depth + l));
        const bool swap = (pos >> l) & 1u;
        const fe left = fe_from_mont<FP>(fe_pick(swap, node, sibling)), right = fe_from_mont<FP>(fe_pick(swap, sibling, node));
        bool bottom;
        node = merkle_layer_x(q, l, left, right, table, bottom);       // zero where bottom: the walk goes on from 0
        fe_store(out + 8 * (l + 1), node);
        status[i * depth + l] = bottom ? 1 : 0;
    }
}

__device__ __forceinline__ fe fe_small(u32 v) { return fe{{v, 0, 0, 0, 0, 0, 0, 0}}; }

// The cells of one item before any conversion: the swapped pair as it is stored (Montgomery), the pieces and their parts CANONICAL.
struct LayerCells {
    fe node, sibling, left_m, right_m;
    fe a, b, c, z1_a;
    u32 b_1, b_2, z1_b, l;
    bool swap;
};
__device__ __forceinline__ LayerCells layer_cells(const u32 *__restrict__ nodes, const u32 *__restrict__ siblings,
                                                  const u32 *__restrict__ positions, size_t t, u32 depth, u32 layer_lo, u32 layers) {
    LayerCells k;
    const size_t path = t / layers;
    k.l = layer_lo + (u32)(t - path * layers);
    k.node = fe_load(nodes + 8 * (path * (depth + 1) + k.l));
    k.sibling = fe_load(siblings + 8 * (path * depth + k.l));
    k.swap = (positions[path] >> k.l) & 1u;
    k.left_m = fe_pick(k.swap, k.node, k.sibling);
    k.right_m = fe_pick(k.swap, k.sibling, k.node);
    const fe left = fe_from_mont<FP>(k.left_m), right = fe_from_mont<FP>(k.right_m);
    k.z1_a = left;                                         // left[0..240)
    k.z1_a.v[7] &= 0xFFFFu;
#pragma unroll
    for (int j = 7; j > 0; j--) k.a.v[j] = (k.z1_a.v[j] << 10) | (k.z1_a.v[j - 1] >> 22);      // l | left[0..240) << 10
    k.a.v[0] = (k.z1_a.v[0] << 10) | k.l;
    const u32 b_0 = (left.v[7] >> 16) & 0x3FFu;
    k.b_1 = (left.v[7] >> 26) & 31u;
    k.b_2 = right.v[0] & 31u;
    k.z1_b = k.b_1 | (k.b_2 << 5);
    k.b = fe_small(b_0 | (k.z1_b << 10));
#pragma unroll
    for (int j = 0; j < 7; j++) k.c.v[j] = (right.v[j] >> 5) | (right.v[j + 1] << 27);          // right[5..255)
    k.c.v[7] = (right.v[7] >> 5) & 0x3FFFFFFu;
    return k;
}

// Item t = path * layers + (l - layer_lo); `count` = n * layers items.  The vectors, in elements from `out` (c = count):
//   [0, 5c)     swap rows: a (node), b (sibling), a_swapped (left), b_swapped (right), swap          c each
//   [5c, 8c)    the pieces a, b, c of item t at 3t, 3t + 1, 3t + 2                                   Montgomery
//   [8c, 18c)   decomposition rows, five vectors of 2c: rows 2t and 2t + 1 of item t hold
//               (a, z1_a), (b, z1_b), (c, b_1), (left, b_2), (right, l)
//   [18c, 21c)  the pieces again, CANONICAL: h2_sinsemilla_trace_device's d_pieces
//   [21c, 23c)  b_1 (c elements), b_2 (c elements), CANONICAL: what the short range checks take
__global__ void __launch_bounds__(kST) merkle_trace(const u32 *__restrict__ nodes, const u32 *__restrict__ siblings,
                                                    const u32 *__restrict__ positions, size_t count, u32 depth, u32 layer_lo, u32 layers,
                                                    u32 *__restrict__ out) {
    const size_t t = (size_t)blockIdx.x * kST + threadIdx.x;
    if (t >= count) return;
    const LayerCells k = layer_cells(nodes, siblings, positions, t, depth, layer_lo, layers);
    const size_t v = 8 * count;                            // u32 words of a vector of `count` elements
    const fe a_m = fe_to_mont<FP>(k.a), b_m = fe_to_mont<FP>(k.b), c_m = fe_to_mont<FP>(k.c);
    u32 *swap_rows = out + 8 * t;
    fe_store(swap_rows, k.node);
    fe_store(swap_rows + v, k.sibling);
    fe_store(swap_rows + 2 * v, k.left_m);
    fe_store(swap_rows + 3 * v, k.right_m);
    fe_store(swap_rows + 4 * v, k.swap ? fe_one<FP>() : fe_zero());
    u32 *pieces = out + 5 * v + 24 * t;
    fe_store(pieces, a_m);
    fe_store(pieces + 8, b_m);
    fe_store(pieces + 16, c_m);
    u32 *dec = out + 8 * v + 16 * t;
    fe_store(dec, a_m);
    fe_store(dec + 8, fe_to_mont<FP>(k.z1_a));
    fe_store(dec + 2 * v, b_m);
    fe_store(dec + 2 * v + 8, fe_to_mont<FP>(fe_small(k.z1_b)));
    fe_store(dec + 4 * v, c_m);
    fe_store(dec + 4 * v + 8, fe_to_mont<FP>(fe_small(k.b_1)));
    fe_store(dec + 6 * v, k.left_m);
    fe_store(dec + 6 * v + 8, fe_to_mont<FP>(fe_small(k.b_2)));
    fe_store(dec + 8 * v, k.right_m);
    fe_store(dec + 8 * v + 8, fe_to_mont<FP>(fe_small(k.l)));
    u32 *canonical = out + 18 * v + 24 * t;
    fe_store(canonical, k.a);
    fe_store(canonical + 8, k.b);
    fe_store(canonical + 16, k.c);
    fe_store(out + 21 * v + 8 * t, fe_small(k.b_1));
    fe_store(out + 22 * v + 8 * t, fe_small(k.b_2));
}

#ifdef H2_AB
// The laboratory's other arm (H2_MERKLE_TRACE_PER_CELL=1, not in the product): one lane per OUTPUT ELEMENT, in the order of the
// buffer, so a wave stores 2 KiB in one piece everywhere; each of the 23 lanes of an item loads its node and sibling again and forms
// the item's cells to keep one.  bench/tools/merkle_paths_time.py times it beside the kernel above.
__global__ void __launch_bounds__(kST) merkle_trace_per_cell(const u32 *__restrict__ nodes, const u32 *__restrict__ siblings,
                                                             const u32 *__restrict__ positions, size_t count, u32 depth, u32 layer_lo,
                                                             u32 layers, u32 *__restrict__ out) {
    const size_t e = (size_t)blockIdx.x * kST + threadIdx.x;
    if (e >= 23 * count) return;
    // which = 0 .. 4 swap rows; 5, 6, 7 pieces; 8 .. 17 decomposition (column * 2 + row); 18, 19, 20 canonical pieces; 21, 22 b_1, b_2
    size_t t;
    u32 which;
    if (e < 5 * count) {
        which = (u32)(e / count);
        t = e - which * count;
    } else if (e < 8 * count) {
        t = (e - 5 * count) / 3;
        which = 5 + (u32)(e - 5 * count - 3 * t);
    } else if (e < 18 * count) {
        const size_t r = e - 8 * count;
        const u32 column = (u32)(r / (2 * count));
        const size_t rr = r - column * 2 * count;
        t = rr / 2;
        which = 8 + 2 * column + (u32)(rr & 1);
    } else if (e < 21 * count) {
        t = (e - 18 * count) / 3;
        which = 18 + (u32)(e - 18 * count - 3 * t);
    } else {
        which = 21 + (u32)((e - 21 * count) / count);
        t = e - which * count;
    }
    const LayerCells k = layer_cells(nodes, siblings, positions, t, depth, layer_lo, layers);
    fe plain = k.a;                                        // the canonical value of the cell, where it has one
    bool convert = true, stored = false;                   // stored: the cell is one of the four Montgomery inputs
    fe value = k.node;
    switch (which) {
    case 0: stored = true; break;
    case 1: value = k.sibling; stored = true; break;
    case 2: case 14: value = k.left_m; stored = true; break;
    case 3: case 16: value = k.right_m; stored = true; break;
    case 4: value = k.swap ? fe_one<FP>() : fe_zero(); stored = true; break;
    case 5: case 8: break;
    case 6: case 10: plain = k.b; break;
    case 7: case 12: plain = k.c; break;
    case 9: plain = k.z1_a; break;
    case 11: plain = fe_small(k.z1_b); break;
    case 13: plain = fe_small(k.b_1); break;
    case 15: plain = fe_small(k.b_2); break;
    case 17: plain = fe_small(k.l); break;
    case 18: convert = false; break;
    case 19: plain = k.b; convert = false; break;
    case 20: plain = k.c; convert = false; break;
    case 21: plain = fe_small(k.b_1); convert = false; break;
    default: plain = fe_small(k.b_2); convert = false; break;
    }
    if (!stored) value = convert ? fe_to_mont<FP>(plain) : plain;
    fe_store(out + 8 * e, value);
}
#endif

// the checks both entry points share; n * depth <= 2^30
inline bool paths_ok(const h2_merkle_paths_t *paths, size_t n) {
    return paths && paths->depth >= 1 && paths->depth <= kMaxDepth && n <= kMaxItems / paths->depth;
}

}  // namespace
}  // namespace h2

using namespace h2;

extern "C" int h2_sinsemilla_merkle_paths_device(const h2_merkle_paths_t *paths, const void *d_leaves, const void *d_siblings,
                                                 const void *d_positions, size_t n, void *d_nodes, void *d_status) {
    if (!paths_ok(paths, n) || !paths->q_xy) return H2_ERR_ARGS;
    if (n && (!paths->d_table || !d_leaves || !d_siblings || !d_positions || !d_nodes || !d_status)) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!n) return H2_OK;
    hipLaunchKernelGGL(merkle_paths, dim3(grid_of(n, kST)), dim3(kST), 0, (hipStream_t)paths->stream, (const u32 *)d_leaves,
                       (const u32 *)d_siblings, (const u32 *)d_positions, n, (u32)paths->depth, point_arg(paths->q_xy),
                       (const u32 *)paths->d_table, (u32 *)d_nodes, (uint8_t *)d_status);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

extern "C" int h2_sinsemilla_merkle_trace_device(const h2_merkle_paths_t *paths, const void *d_nodes, const void *d_siblings,
                                                 const void *d_positions, size_t n, unsigned layer_lo, unsigned layer_hi, void *d_out) {
    if (!paths_ok(paths, n) || layer_lo >= layer_hi || layer_hi > paths->depth) return H2_ERR_ARGS;
    if (n && (!d_nodes || !d_siblings || !d_positions || !d_out)) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!n) return H2_OK;
    const u32 layers = layer_hi - layer_lo;
    const size_t count = n * layers;
#ifdef H2_AB
    static const bool per_cell = [] { const char *e = ab_env("H2_MERKLE_TRACE_PER_CELL"); return e && e[0] == '1'; }();
    if (per_cell) {
        hipLaunchKernelGGL(merkle_trace_per_cell, dim3(grid_of(23 * count, kST)), dim3(kST), 0, (hipStream_t)paths->stream,
                           (const u32 *)d_nodes, (const u32 *)d_siblings, (const u32 *)d_positions, count, (u32)paths->depth, (u32)layer_lo,
                           layers, (u32 *)d_out);
        H2_HIP(hipGetLastError());
        return H2_OK;
    }
#endif
    hipLaunchKernelGGL(merkle_trace, dim3(grid_of(count, kST)), dim3(kST), 0, (hipStream_t)paths->stream, (const u32 *)d_nodes,
                       (const u32 *)d_siblings, (const u32 *)d_positions, count, (u32)paths->depth, (u32)layer_lo, layers, (u32 *)d_out);
    H2_HIP(hipGetLastError());
    return H2_OK;
}
