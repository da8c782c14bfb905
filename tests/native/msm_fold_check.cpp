// Host check of the fold's integer code in csrc/msm_plan.h (plain C++: the text the fold kernels' index maps and fold_r256 call compiles here as
// it stands).  tests/test_msm_fold_planes.py builds this with g++ -- plain and under -fsanitize=address,undefined --, reads what it prints and
// checks it from the definitions; nothing is judged here.
//   K t n : v_0 v_1 ...                 kth_with_bit(k, t) for k < 2^(n-1), every t in 0 .. 15 and n in t + 1 .. 16
//   B t count : b_0 b_1 ...             sub_planes: the buckets of plane t of a 128-bucket slice
//   C <call> = fold9 c S NR cb          a plan that folds on the carry-free layer: window width and the bucket matrix fold9_group is given
//   C <call> = r256 nb slices c seg segs levels (blocks per_slice share)... lds      a plan on the 8 x 32 fold: r256_fold_geometry and the tree's LDS
//   C <call> = none rc                  msm_plan refused the call, or it stops before the fold (add_into)
//   P c S NR cb planes                  one block per distinct (c, S, NR) of the C lines, followed by, for t < planes = the grid fold9_group launches,
//   p t ncol nrow : l_0 l_1 ...         the line index of each of the ncol + nrow summands of plane t
#include <cstdio>
#include <set>
#include <tuple>

#include "../../halo2_amd/csrc/msm_plan.h"
using namespace h2;

static const MsmKnobs kShipped;
static const u32 kSome[16] = {0};      // stands for every device pointer: the plan only asks whether one is null
static const void *const kCols[kMaxCols] = {kSome, kSome, kSome, kSome, kSome, kSome, kSome, kSome};
static void *const kOuts[kMaxCols] = {(void *)kSome, (void *)kSome, (void *)kSome, (void *)kSome, (void *)kSome, (void *)kSome, (void *)kSome, (void *)kSome};
static std::set<std::tuple<int, u32, u32>> g_shapes;

static void fold_of(const char *what, const MsmArgs &a, u32 lanes, const MsmKnobs &kn) {
    MsmPlan p;
    const int rc = msm_plan(a, lanes, false, kn, &p);
    if (rc != H2_OK || p.add_only) {
        printf("C %s = none %d\n", what, rc);
        return;
    }
    if (p.fold9) {
        printf("C %s = fold9 %d %u %u %d\n", what, p.sh.c, p.wideS, p.wideNR, fold9_col_bits(p.wideS));
        g_shapes.insert(std::make_tuple(p.sh.c, p.wideS, p.wideNR));
        if (p.try_grouped) {      // the grouped form folds its groups over a matrix of its own plan
            GroupedPlan gp;
            if (grouped_plan(p.sh, p.scalars_n, lanes, false, kn, gp) == H2_OK) {
                printf("C %s grouped = fold9 %d %u %u %d\n", what, p.sh.c, gp.wideS, gp.wideNR, fold9_col_bits(gp.wideS));
                g_shapes.insert(std::make_tuple(p.sh.c, gp.wideS, gp.wideNR));
            }
        }
        return;
    }
    const R256Fold f = r256_fold_geometry(p.sh, p.wide_reduce, p.wideNR);
    printf("C %s = r256 %u %u %d %d %u %d", what, f.nb, f.slices, f.c, f.seg, f.segs, f.levels);
    for (int l = 0; l < f.levels; ++l) printf(" %u %u %u", f.level[l].blocks, f.level[l].per_slice, f.level[l].share);
    printf(" %zu\n", r256_tree_bytes(kTreeLanes));
}

int main() {
    printf("constants: LDS_CAP %zu MAX_C %d MAX_C_SHARED %d TREE_LANES %u\n", kLdsCap, kMaxC, kMaxCShared, kTreeLanes);
    for (u32 t = 0; t < 16; ++t)
        for (u32 n = t + 1; n <= 16; ++n) {
            printf("K %u %u :", t, n);
            for (u32 k = 0; k < (1u << (n - 1)); ++k) printf(" %u", kth_with_bit(k, t));
            printf("\n");
        }
    for (u32 t = 0; t < 8; ++t) {
        printf("B %u %u :", t, sub_plane_count(t));
        for (u32 k = 0; k < sub_plane_count(t); ++k) printf(" %u", sub_plane_bucket(t, k));
        printf("\n");
    }
    // registered tables at every width (4 .. 7 take the 8 x 32 fold), a few sizes, the forms an entry point can ask for; H2_MSM_C is the only
    // way to some of the widths, so the knob forces none here: the table's width is an argument of the call
    const u32 lanes = 256u * 2u * 256u;
    char what[160];
    for (int c = 4; c <= kMaxCShared; ++c)
        for (size_t points : {(size_t)512, (size_t)4096, (size_t)1 << 14, (size_t)1 << 17, (size_t)1 << 20})
            for (int form = 0; form < 5; ++form) {      // plain, blind, batch of 4, pair, fold-only
                if (c > kMaxC && !wide_window_fits(points, c)) continue;
                MsmArgs a{kSome, form == 1 ? kSome : nullptr, kSome, nullptr, points, true, c, (u32)points + 1, (u32)points, H2_FORM_MONTGOMERY, H2_OUT_AFFINE, (void *)kSome};
                if (form == 2) { a.ncols = 4; a.col_scalars = kCols; a.col_outs = kOuts; }
                if (form == 3) { a.pair_shift = 0; a.pair_n = (u32)points - 4; }
                if (form == 4) a.fold_from = kSome;
                snprintf(what, sizeof what, "table %d %zu %d", c, points, form);
                fold_of(what, a, lanes, kShipped);
            }
    // generic multiexps: the width is choose_c's; with a blind term they keep the 8 x 32 layer
    for (size_t n : {(size_t)1, (size_t)100, (size_t)1 << 10, (size_t)2049, (size_t)1 << 12, (size_t)1 << 16, (size_t)1 << 18, ((size_t)1 << 18) + 1, (size_t)1 << 19, (size_t)1 << 20,
                     (size_t)1 << 22})
        for (int blind = 0; blind < 2; ++blind) {
            MsmArgs a{kSome, blind ? kSome : nullptr, kSome, blind ? kSome : nullptr, n, false, choose_c(n, false, kShipped), 0, 0xFFFFFFFFu, H2_FORM_MONTGOMERY, H2_OUT_AFFINE, (void *)kSome};
            snprintf(what, sizeof what, "generic %zu %d", n, blind);
            fold_of(what, a, lanes, kShipped);
        }
    for (const auto &s : g_shapes) {
        const int c = std::get<0>(s);
        const u32 S = std::get<1>(s), NR = std::get<2>(s);
        const int cb = fold9_col_bits(S);
        const u32 planes = fold9_plane_count(c);      // the grid x of fold9_planes (fold9_group)
        printf("P %d %u %u %d %u\n", c, S, NR, cb, planes);
        for (u32 t = 0; t < planes; ++t) {
            const u32 ncol = fold9_plane_cols(S, cb, t), nrow = fold9_plane_rows(NR, cb, t);
            printf("p %u %u %u :", t, ncol, nrow);
            for (u32 k = 0; k < ncol + nrow; ++k) printf(" %u", fold9_plane_line(S, cb, t, k));
            printf("\n");
        }
    }
    printf("done\n");
    return 0;
}
