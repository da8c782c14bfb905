// The launch geometry of poly.hip: tile shape, LDS sizes, grid caps and the split of a scan's tiles over the carry kernels' lanes.  Plain
// constexpr C++ with no HIP in it: poly.hip computes every one of these through this header, and tests/native/poly_plan_check.cpp
// compiles the same text for the CPU and prints it, so that the replica of tests/scan_sort_cases.py is held to the arithmetic the
// kernels run with (tests/test_scan_sort_case_coverage.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace h2 {

constexpr int kPT = 256;             // lanes per workgroup
constexpr int kPC = 8;               // consecutive elements per lane
constexpr int kTile = kPT * kPC;     // elements per tile
constexpr int kPitch = 8 * kPC + 1;  // LDS words per lane row
constexpr int kSPitch = 9;           // scan array pitch
constexpr int kInvGroup = 8;         // lanes that share one Fermat inversion (poly_batch_invert)
constexpr unsigned kTileLds = kPT * kPitch * 4;                  // the element tile
constexpr unsigned kScanLds = kTileLds + kPT * kSPitch * 4;      // + one lane-aggregate array

// workgroups of a reduction over n elements: one lane per element up to the cap, strided lanes beyond it
constexpr unsigned kReduceCap = 1024;
constexpr unsigned reduce_blocks(size_t n) {
    const size_t blocks = (n + kPT - 1) / kPT;
    return (unsigned)(blocks < kReduceCap ? blocks : kReduceCap);
}
// The Horner evaluation's grid.  Every lane pays x^t (square and multiply, ~27 multiplications at 2^18 lanes) on top of its Horner steps:
// 65536 lanes x 16 coefficients keep that a third of the work (1024 blocks x 4 coefficients: 87 % of it; 79 -> ~35 us at n = 2^20)
constexpr unsigned kEvalCap = 256;
constexpr unsigned eval_blocks(size_t n) { return reduce_blocks(n) < kEvalCap ? reduce_blocks(n) : kEvalCap; }

// tiles (workgroups of the tile kernels) of n elements
constexpr unsigned tile_count(size_t n) { return (unsigned)((n + kTile - 1) / kTile); }

// The carry kernels run one workgroup over the nblk tile aggregates of a scan: lane t owns the `per` tiles from t * per on, of which
// [lo, hi) exist.  The last working lane walks per - (hi - lo) phantom steps past the last tile.
struct CarrySpan {
    uint32_t per, lo, hi;
};
constexpr CarrySpan carry_span(uint32_t nblk, uint32_t lane) {
    const uint32_t per = (nblk + kPT - 1) / kPT, lo = lane * per < nblk ? lane * per : nblk, hi = lo + per < nblk ? lo + per : nblk;
    return CarrySpan{per, lo, hi};
}

}  // namespace h2
