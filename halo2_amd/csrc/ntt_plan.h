// The NTT's pass plan and its workgroup -> tile map (5.3): plain C++ -- no HIP, no context, no environment --
// so that "what does a 2^21 transform run as" is answered, and tested, on a CPU (tests/test_ntt_plan.py).  ntt.hip fills PassArgs from it.
#pragma once
#include "../../include/halo2_mi355x.h"   // <stddef.h>, <stdint.h>, H2_OK / H2_ERR_ARGS

#ifdef __HIPCC__
#define NTT_HD __host__ __device__ __forceinline__
#else
#define NTT_HD inline
#endif

namespace h2 {

struct NttKnobs {      // laboratory switches (H2_NTT_MAXR / _LOGT / _LOGT_FIRST / _LDS: tuning sweeps only); the shipped library runs the defaults
    int maxr = 10, logT = 3, logT_first = -1;   // stages per pass at most, 1 .. 12; log2 of the tile columns asked for, 0 .. 5; the same for the first pass alone (-1: as logT)
    uint32_t lds = 131072;                      // tile bytes at most (8 x 32 layout), 32768 .. 131072
};
struct NttPassPlan {
    int s0, r, logT;                            // first stage, stages, log2 of tile columns
    uint32_t threads, tiles;
    size_t lds, lds9;                           // dynamic LDS bytes of ntt_pass (8 x 32) / ntt_pass9 (nine limbs)
    bool first, last;
};
struct NttPlan {
    int passes;
    NttPassPlan pass[32];
    bool use_fe9;             // ntt_pass9 and the M9 twiddle table; false: the 8 x 32 kernel
    bool needs_scratch;       // an in-place call of more than one pass: between the passes the vector lives in a scratch buffer
};

// nine limbs per element in three planes (36 B for the 8 x 32 layout's 32) + the 129-entry table of q p, 12 words apart (ntt_fold9)
constexpr size_t ntt_lds9_bytes(size_t lds) { return lds / 32 * 36 + 129 * 48; }
constexpr size_t kNttLds9Max = 160 * 1024;   // what ntt_pass9 may be given; a 12-stage tile takes 147 KiB + 6 KiB

// ceil(L / maxr) passes, stages spread evenly, odd counts paired up (a pass with an even stage count fuses its loads and stores into
// its first and last radix-4 round).
// Plan 0 (a transform alone): up to 10 stages per pass with 128 KiB tiles -- 2^20 runs as TWO passes of 10 stages (one workgroup per
// CU, the whole vector resident in LDS across the chip) instead of three of 7, 7, 6: 0.137 -> 0.128 ms; 2^22 still needs three.
// Plan 1 (the batch entry points: independent column transforms on internal streams): at most 8 stages and 64 KiB, so workgroups of
// several transforms share a CU and one column's load / store phases hide under another's butterflies (0.105 ms per 2^20 transform
// over 3 streams, against 0.131 with plan 0).
// Round 5: 11- and 12-stage passes exist (2048 rows x 2 columns / 4096 rows x 1 column of nine-limb elements = 147 KiB, 1024 lanes; odd
// stage counts open with a radix-2 round), so 2^21 .. 2^24 CAN run as two passes -- and measured on the same box
// (profiles/r05_ntt_two_pass_ab.txt) that is SLOWER: 2^22 as 11 + 11 0.398 ms against 0.342 as 8 + 8 + 6, 2^24 as 12 + 12 2.09 against
// 1.45.  The passes are issue-bound, not byte-bound: two passes carry ~10 800 instructions per lane-quadruple against ~11 170 for three
// (3 % fewer), while their 64- / 32-byte rows and one-workgroup-per-CU tiles lose more than that to the memory phases no second
// workgroup covers.  The default stays at 10 stages; maxr = 11 / 12 reproduces the A/B.
// A transform alone on the chip, below 2^20: wide tiles are FEW tiles (2^18 as 10 + 8 stages at four columns = 64 workgroups on 256
// CUs) -- narrow them until there is one per CU.  Measured (profiles/r04_ntt_tile_width.txt): 2^19 0.0615 -> 0.0545 ms, 2^18 0.0518 ->
// 0.0375, 2^17 0.0498 -> 0.0288, 2^16 0.0342 -> 0.0243.  Batched column transforms (plan 1) fill the chip with columns instead and keep
// their 128-byte rows.
// The carry-free passes keep in-stage twiddle indices in 32-bit lane offsets (tw9_load32): transforms up to 2^28; beyond that (16 GiB
// vectors and up) the 8 x 32 kernel with its 32-byte table entries takes over.
// SAFETY: both kernels give a radix-4 round one lane per group under `if (tid < ngrp)`, with no loop: every pass of r >= 2 stages needs
// 2^(r + logT) / 4 <= threads.  It holds because no tile exceeds 4096 elements: 128 KiB, or one column of 2^12 rows
// (tests/test_ntt_plan.py checks it, with the plan's other invariants, over every size and knob).
inline int ntt_plan(int L, int plan_kind, bool in_place, bool fe9_on, const NttKnobs &K, NttPlan *out) {
    if (L < 1 || L > 32 || K.maxr < 1) return H2_ERR_ARGS;
    const int maxr = plan_kind == 1 && K.maxr > 8 ? 8 : K.maxr;
    const uint32_t lds_cap = plan_kind == 1 && K.lds > 65536u ? 65536u : K.lds;
    const int P = (L + maxr - 1) / maxr;
    int stages[32];
    for (int i = 0; i < P; ++i) stages[i] = L / P + (i < L % P ? 1 : 0);
    for (int i = 0; i < P; ++i) {
        if (!(stages[i] & 1)) continue;
        for (int j = i + 1; j < P; ++j)
            if ((stages[j] & 1) && stages[i] + 1 <= maxr && stages[j] >= 2) {
                stages[i] += 1;
                stages[j] -= 1;
                break;
            }
    }
    const size_t n = (size_t)1 << L;
    out->passes = P;
    out->use_fe9 = fe9_on && L <= 28;
    out->needs_scratch = P > 1 && in_place;
    int s0 = 0;
    for (int i = 0; i < P; ++i) {
        NttPassPlan &A = out->pass[i];
        A.s0 = s0;
        A.r = stages[i];
        if (A.r < 1 || A.r > 12) return H2_ERR_ARGS;
        A.first = i == 0;
        A.last = i == P - 1;
        const int colbits = A.first ? (L - A.r) : s0, want = A.first && K.logT_first >= 0 ? K.logT_first : K.logT;
        A.logT = want < colbits ? want : colbits;
        while (A.logT > 0 && ((32u << A.r) << A.logT) > lds_cap) A.logT--;
        if (plan_kind == 0)
            while (A.logT > 0 && (n >> (A.r + A.logT)) < 256) A.logT--;
        // keep >= 256 lanes per workgroup when the pass is narrow
        while (A.logT < colbits && ((1 << A.r) << A.logT) < 1024 && ((32u << A.r) << (A.logT + 1)) <= lds_cap) A.logT++;
        // one lane per radix-4 group (tile / 4); a 1-stage pass needs tile / 2 butterflies, looped
        const size_t quarter = ((size_t)1 << A.r << A.logT) / 4;
        A.threads = (uint32_t)(quarter < 64 ? 64 : quarter > 1024 ? 1024 : quarter);
        A.tiles = (uint32_t)(n >> (A.r + A.logT));
        A.lds = ((size_t)32 << A.r) << A.logT;
        A.lds9 = ntt_lds9_bytes(A.lds);
        s0 += A.r;
    }
    return H2_OK;
}

// Workgroup -> tile map of the passes after the first.  A tile is (hi, lo): elements hi 2^(s0+r) + mid 2^s0 + lo T + col; its
// in-pass twiddles omega^((low 2^s0 + lo T + col) ...) depend on `lo` alone.  So (1) the tiles of one `lo` -- one per `hi` -- read
// the SAME table entries, and (2) neighbouring `lo` read NEIGHBOURING entries: T consecutive entries per tile row, i.e. T / 8 of a
// 128-byte line of the two 16-byte planes and T / 32 of a line of the 4-byte plane.  The dispatcher puts workgroup b on XCD b % 8
// (observed, MI355X_MICROARCH.md -- a speed assumption only: any placement gives the same results), each XCD with its own L2.
// With tile = b the 32 / T tiles that share a line sat on as many different XCDs and each fetched the line for itself: the second
// pass of a 2^20 transform fetched 166 MiB for 68 MiB of data + twiddles (profiles/r04_pmc_traffic.json; FETCH_SIZE calibrated
// on these very patterns, bench/ubench_fetch.hip).  Here XCD x takes the x-th CONTIGUOUS EIGHTH of the `lo` range, for every
// `hi`; in dispatch order `lo` runs fastest (the line sharers run side by side), then `hi` (the next tiles re-read what the XCD's
// L2 already holds): 72 MiB at 2^20.  Measured alternatives: a contiguous eighth of the TILES (right for one `hi`, but at 2^22
// every XCD then needs every twiddle of the middle pass: 159 -> 266 MiB), groups of the 32 / T line sharers dealt round-robin
// (2^20: 81 MiB, the last pass of 2^22 319 against 272).  A permutation of [0, nblocks) for every shape (tests/test_ntt_plan.py).
NTT_HD uint32_t ntt_tile_of_block(uint32_t b, uint32_t nblocks, int s0, int logT) {
    const int lt = s0 - logT;                           // log2 tiles per hi
    if (lt < 3 || (nblocks & 7u)) return b;             // fewer than eight tiles per hi: dispatch order as it is
    const uint32_t xcd = b & 7u, k = b >> 3;            // k-th workgroup of its XCD
    const uint32_t lo_local = k & ((1u << (lt - 3)) - 1u), hi = k >> (lt - 3);
    return (hi << lt) | (xcd << (lt - 3)) | lo_local;
}

}  // namespace h2
