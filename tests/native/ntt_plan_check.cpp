// Host check of csrc/ntt_plan.h (plain C++: the plan and the workgroup -> tile map compile here exactly as the library and the kernel
// use them).  tests/test_ntt_plan.py builds this with g++ and reads the three summary lines.
//   ntt_plan_check <table>      <table>: tests/ntt_plans_parent.txt, the plans of the commit before the header existed
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../halo2_amd/csrc/ntt_plan.h"

using namespace h2;

static long violations = 0, bad_maps = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (++violations <= 20) {                      \
                printf("VIOLATION %s: ", #cond);           \
                printf(__VA_ARGS__);                       \
                printf("\n");                              \
            }                                              \
        }                                                  \
    } while (0)

// every pass after the first: b -> ntt_tile_of_block(b) over b < tiles is a permutation of [0, tiles)
static long check_tile_map(const NttPlan &P, int L) {
    long maps = 0;
    for (int i = 1; i < P.passes; ++i) {
        const NttPassPlan &p = P.pass[i];
        std::vector<bool> seen(p.tiles, false);
        bool ok = true;
        for (uint32_t b = 0; b < p.tiles && ok; ++b) {
            const uint32_t t = ntt_tile_of_block(b, p.tiles, p.s0, p.logT);
            ok = t < p.tiles && !seen[t];
            if (ok) seen[t] = true;
        }
        if (!ok) ++bad_maps;
        CHECK(ok, "tile map of L=%d pass %d (s0 %d, logT %d, %u tiles) is no permutation", L, i, p.s0, p.logT, p.tiles);
        ++maps;
    }
    return maps;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    // ---- invariants, every L x plan kind x in place / out of place x maxr x logT
    long plans = 0, maps = 0;
    const int maxrs[] = {4, 10, 11, 12}, logTs[] = {0, 3, 5};
    for (int L = 1; L <= 32; ++L)
        for (int kind = 0; kind < 2; ++kind)
            for (int in_place = 0; in_place < 2; ++in_place)
                for (int maxr : maxrs)
                    for (int logT : logTs)
                        for (int fe9 = 0; fe9 < 2; ++fe9) {
                            NttKnobs K;
                            K.maxr = maxr;
                            K.logT = logT;
                            NttPlan P;
                            const int rc = ntt_plan(L, kind, in_place != 0, fe9 != 0, K, &P);
                            CHECK(rc == H2_OK, "L=%d kind=%d maxr=%d logT=%d: rc %d", L, kind, maxr, logT, rc);
                            if (rc != H2_OK) continue;
                            ++plans;
                            const uint32_t cap = kind == 1 ? 65536u : K.lds;
                            int sum = 0;
                            for (int i = 0; i < P.passes; ++i) {
                                const NttPassPlan &p = P.pass[i];
                                const int colbits = i == 0 ? L - p.r : sum;
                                CHECK(p.s0 == sum, "L=%d pass %d: s0 %d after %d stages", L, i, p.s0, sum);
                                CHECK(p.r >= 1 && p.r <= maxr, "L=%d kind=%d maxr=%d pass %d: r %d", L, kind, maxr, i, p.r);
                                CHECK(p.lds == ((size_t)32 << (p.r + p.logT)) && p.lds <= cap, "L=%d kind=%d maxr=%d logT=%d pass %d: lds %zu", L, kind, maxr, logT, i, p.lds);
                                CHECK(p.lds9 == p.lds / 32 * 36 + 129 * 48 && p.lds9 <= 160 * 1024, "L=%d pass %d: lds9 %zu", L, i, p.lds9);
                                CHECK(((uint64_t)p.tiles << (p.r + p.logT)) == ((uint64_t)1 << L) && p.tiles >= 1, "L=%d pass %d: %u tiles of 2^%d", L, i, p.tiles, p.r + p.logT);
                                CHECK(p.logT >= 0 && p.logT <= colbits, "L=%d pass %d: logT %d of %d column bits", L, i, p.logT, colbits);
                                CHECK(p.threads >= 64 && p.threads <= 1024, "L=%d pass %d: %u threads", L, i, p.threads);
                                // the unlooped radix-4 rounds: one lane per group of four elements
                                CHECK(p.r < 2 || ((uint64_t)1 << (p.r + p.logT)) / 4 <= p.threads, "L=%d kind=%d maxr=%d logT=%d pass %d: tile 2^%d on %u threads", L, kind, maxr, logT, i, p.r + p.logT, p.threads);
                                CHECK(p.first == (i == 0) && p.last == (i == P.passes - 1), "L=%d pass %d: first / last", L, i);
                                sum += p.r;
                            }
                            CHECK(sum == L, "L=%d kind=%d maxr=%d: stages sum to %d", L, kind, maxr, sum);
                            CHECK(P.use_fe9 == (fe9 && L <= 28), "L=%d: use_fe9 %d", L, (int)P.use_fe9);
                            CHECK(P.needs_scratch == (in_place && P.passes > 1), "L=%d: needs_scratch %d", L, (int)P.needs_scratch);
                            if (L <= 26 && !in_place && !fe9) maps += check_tile_map(P, L);
                        }
    NttPlan Q;
    CHECK(ntt_plan(0, 0, true, true, NttKnobs(), &Q) == H2_ERR_ARGS && ntt_plan(33, 0, true, true, NttKnobs(), &Q) == H2_ERR_ARGS, "L outside 1 .. 32 is refused");
    printf("invariants: %ld plans, %ld violations\n", plans, violations);
    printf("tile map: %ld passes, %ld not a permutation\n", maps, bad_maps);

    // ---- the parent's plans: L plan maxr logT logT_first lds passes, then per pass r logT threads tiles lds lds9
    std::ifstream f(argv[1]);
    std::string line;
    long rows = 0, mismatches = 0;
    while (std::getline(f, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream in(line);
        int L, kind, passes;
        NttKnobs K;
        in >> L >> kind >> K.maxr >> K.logT >> K.logT_first >> K.lds >> passes;
        NttPlan P;
        bool same = ntt_plan(L, kind, true, true, K, &P) == H2_OK && P.passes == passes;
        for (int i = 0; same && i < passes; ++i) {
            long long r, logT, threads, tiles, lds, lds9;
            in >> r >> logT >> threads >> tiles >> lds >> lds9;
            const NttPassPlan &p = P.pass[i];
            same = !in.fail() && p.r == r && p.logT == logT && p.threads == threads && p.tiles == tiles && (long long)p.lds == lds && (long long)p.lds9 == lds9;
        }
        ++rows;
        if (!same) {
            if (++mismatches <= 10) printf("MISMATCH %s\n", line.c_str());
        }
    }
    printf("parent plans: %ld rows, %ld mismatches\n", rows, mismatches);
    return violations || mismatches || !rows ? 1 : 0;
}
