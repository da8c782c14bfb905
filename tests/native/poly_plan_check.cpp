// Prints the launch geometry of poly.hip as csrc/poly_plan.h computes it -- the header the kernels and their launches compile -- for
// tests/test_scan_sort_case_coverage.py, which holds every line to the replica of tests/scan_sort_cases.py.
//   poly_plan_check LENGTHS     LENGTHS: a file with one vector length per line
// First line: the constants.  Then per length n: n, the workgroups of a reduction and of the Horner evaluation, the tiles of a scan, the
// tiles per lane of its carry kernel, and the real and phantom steps of the last lane that has a tile.
#include <stdio.h>
#include <stdlib.h>

#include "../../halo2_amd/csrc/poly_plan.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    printf("constants: kPT %d kPC %d kTile %d kPitch %d kSPitch %d kInvGroup %d kTileLds %u kScanLds %u kReduceCap %u kEvalCap %u\n", h2::kPT, h2::kPC,
           h2::kTile, h2::kPitch, h2::kSPitch, h2::kInvGroup, h2::kTileLds, h2::kScanLds, h2::kReduceCap, h2::kEvalCap);
    unsigned long long n;
    while (fscanf(f, "%llu", &n) == 1) {
        if (n == 0) return 3;
        const unsigned nblk = h2::tile_count((size_t)n);
        const uint32_t per = h2::carry_span(nblk, 0).per;
        if (per == 0) return 4;
        const uint32_t last = (nblk - 1) / per;
        const h2::CarrySpan span = h2::carry_span(nblk, last);
        if (last >= (uint32_t)h2::kPT || span.hi != nblk || h2::carry_span(nblk, last + 1).lo != nblk) return 5;      // 256 lanes own every tile
        printf("%llu %u %u %u %u %u %u\n", n, h2::reduce_blocks((size_t)n), h2::eval_blocks((size_t)n), nblk, per, span.hi - span.lo,
               per - (span.hi - span.lo));
    }
    fclose(f);
    return 0;
}
