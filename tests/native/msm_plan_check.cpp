// Host check of csrc/msm_plan.h (plain C++: both multiexp plans compile here exactly as the library uses them).  tests/test_msm_plan.py builds
// this with g++, feeds it calls and reads one answer line per call and the summary lines.
//   msm_plan_check <calls> <table>      <calls>: one call per line (below); <table>: tests/msm_plans_parent.txt, the plans of the commit before
//                                       the header existed, which are replayed against the header
// Call lines and their answers:
//   P lanes points c n_used blind K pair add_into fold_only    msm_plan over a table -> "ERR <code>" or the 26 words of h2_commit_plan_t
//   G lanes n instrumented in_flight                           a whole generic multiexp -> c, the form it takes, T, split_k, try_grouped; a grouped form's G and (ns lowb nh S T) per group
//   Q cols ns nb                                               group_geometry -> lowb nh S, or NONE
//   C n shared / W n / S n / R n bits                          choose_c / column_window_bits / pair_supported / register_width_ok
// Built with -DMSM_PLAN_TEXT='"file"', where the file holds a stand-alone copy of an earlier commit's text of the same functions (with its
// environment reads, lane-fraction global and in-flight query stubbed), `msm_plan_check --rows <inputs>` prints table rows instead: that is how
// tests/msm_plans_parent.txt was made, so that the table does not come from the code it checks.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#ifdef MSM_PLAN_TEXT
#include MSM_PLAN_TEXT      // defines g_lane_fraction and g_other_in_flight beside the functions
using namespace h2;
static int plan_call(const MsmArgs &a, u32 lanes, bool instrumented, MsmPlan *p) { return msm_plan(a, lanes, instrumented, p); }
static int grouped_call(const MsmArgs &a, const MsmShape &sh, size_t n, u32 lanes, bool in_flight, GroupedPlan &gp) {
    MsmContext cx;
    g_other_in_flight = in_flight;
    return grouped_plan(cx, a, sh, n, lanes, gp);
}
static int width_call(size_t n, bool shared) { return choose_c(n, shared); }
#else
#include "../../halo2_amd/csrc/msm_plan.h"
using namespace h2;
static const MsmKnobs kShipped;      // the defaults: what the shipped library runs
static int plan_call(const MsmArgs &a, u32 lanes, bool instrumented, MsmPlan *p) { return msm_plan(a, lanes, instrumented, kShipped, p); }
static int grouped_call(const MsmArgs &, const MsmShape &sh, size_t n, u32 lanes, bool in_flight, GroupedPlan &gp) {
    return grouped_plan(sh, n, lanes, in_flight, kShipped, gp);
}
static int width_call(size_t n, bool shared) { return choose_c(n, shared, kShipped); }
#endif

static const u32 kSome[16] = {0};      // stands for every device pointer: the plans only ask whether one is null
static const void *const kCols[kMaxCols] = {kSome, kSome, kSome, kSome, kSome, kSome, kSome, kSome};
static void *const kOuts[kMaxCols] = {(void *)kSome, (void *)kSome, (void *)kSome, (void *)kSome, (void *)kSome, (void *)kSome, (void *)kSome, (void *)kSome};

struct TableCall { u32 lanes; size_t points; int c; size_t n_used; int blind, K, pair, add_into, fold_only; };
struct GenericCall { u32 lanes; size_t n; int instrumented, in_flight; };

// the arguments the entry points build for a call over a registered table of `points` points (msm_launch.hip, msm_host.hip, msm_subdigit.hip)
static MsmArgs table_args(const TableCall &t) {
    MsmArgs a{kSome, t.blind ? kSome : nullptr, kSome, nullptr, t.n_used, true, t.c, (u32)t.points + 1, (u32)t.points, H2_FORM_MONTGOMERY, H2_OUT_AFFINE, (void *)kSome};
    if (t.pair) { a.pair_shift = 0; a.pair_n = (u32)t.n_used - 4; }
    if (t.add_into) a.add_into = (u32 *)kSome;
    if (t.fold_only) a.fold_from = kSome;
    if (t.K > 1) { a.ncols = t.K; a.col_scalars = kCols; a.col_blinds = t.blind ? kCols : nullptr; a.col_outs = kOuts; }
    return a;
}
static MsmArgs generic_args(const GenericCall &g) {
    return MsmArgs{kSome, nullptr, kSome, nullptr, g.n, false, width_call(g.n ? g.n : 1, false), 0, 0xFFFFFFFFu, H2_FORM_MONTGOMERY, H2_OUT_AFFINE, (void *)kSome};
}

// ---- table rows: every word of a plan that is not a copy of an argument or of another word (check_plan / check_grouped hold the copies)
template <class... A> static void put(std::string &s, A... v) { ((s += ' ', s += std::to_string((long long)v)), ...); }
static std::string plan_words_of(const MsmPlan &p) {
    std::string s;
    const MsmShape &h = p.sh;
    const Sort2 &S = p.S2;
    const ColStride &c = p.cs;      // (all zero for a single column)
    put(s, h.c, h.W, h.NB, h.slices, h.items, h.B, h.chunk);
    put(s, p.m, p.scalars_n, p.all_items, p.fold_only, p.add_only, p.glv, p.m9, p.pair, p.K, p.joined, p.tb, p.nblocks, p.T, p.lane_div, p.head_slots, p.use_sort2);
    if (p.use_sort2)
        put(s, S.m, S.stride, S.extra_col, S.lowb, S.lb, S.nh, S.B1, S.B2, S.lds_window, S.s1_scalars, S.side, S.col0, S.pair_shift, S.pair_n);
    put(s, p.s2_bins_form, p.s2_cap_entries, p.plan_words, p.max_big, p.zero_in_sort, p.fold9, p.wide_reduce, p.wideS, p.wideNR, p.try_grouped, p.split_k);
    if (p.K > 1) put(s, c.hist, c.plan, c.items, c.starts, c.heavy, c.hscratch, c.heads, c.buckets, c.lines, c.planes, c.ctr, c.entries, c.lowprio, c.joined);
    return s;
}
static std::string grouped_words_of(const GroupedPlan &gp) {
    std::string s;
    put(s, gp.throughput, gp.lds_fence, gp.G, gp.head_slots, gp.hist_words, gp.tagged_words, gp.plan_words, gp.wideS, gp.wideNR);
    for (int i = 0; i < gp.G; ++i) {
        const Group &g = gp.grp[i];
        put(s, g.w0, g.ns, g.tb, g.cap, g.emax, g.plan_words, g.B1, g.T, g.ent_off, g.starts_off, g.bucket_off);
        put(s, g.gs.row, g.gs.lowb, g.gs.lb, g.gs.nh, g.gs.S);
    }
    return s;
}
// "T <inputs> = rc <plan>" / "G <inputs> = c rc <plan> | rc <grouped plan>": a refused call ends at its code
static std::string table_row(const TableCall &t) {
    char head[160];
    snprintf(head, sizeof head, "T %u %zu %d %zu %d %d %d %d %d = ", t.lanes, t.points, t.c, t.n_used, t.blind, t.K, t.pair, t.add_into, t.fold_only);
    MsmPlan p;
    const int rc = plan_call(table_args(t), t.lanes, false, &p);
    return std::string(head) + std::to_string(rc) + (rc == H2_OK ? plan_words_of(p) : std::string());
}
static std::string generic_row(const GenericCall &g) {
    char head[160];
    const MsmArgs a = generic_args(g);
    snprintf(head, sizeof head, "G %u %zu %d %d = %d ", g.lanes, g.n, g.instrumented, g.in_flight, a.c);
    MsmPlan p;
    const int rc = plan_call(a, g.lanes, g.instrumented != 0, &p);
    std::string s = std::string(head) + std::to_string(rc);
    if (rc != H2_OK) return s;
    s += plan_words_of(p);
    if (p.try_grouped) {
        GroupedPlan gp;
        const int grc = grouped_call(a, p.sh, p.scalars_n, g.lanes, g.in_flight != 0, gp);
        s += " | " + std::to_string(grc) + (grc == H2_OK ? grouped_words_of(gp) : std::string());
    }
    return s;
}
static bool parse_row_inputs(const std::string &line, TableCall *t, GenericCall *g) {
    std::istringstream in(line);
    char kind = 0;
    in >> kind;
    if (kind == 'T') in >> t->lanes >> t->points >> t->c >> t->n_used >> t->blind >> t->K >> t->pair >> t->add_into >> t->fold_only;
    else if (kind == 'G') in >> g->lanes >> g->n >> g->instrumented >> g->in_flight;
    else return false;
    return !in.fail();
}
static std::string row_of(const std::string &line) {
    TableCall t;
    GenericCall g;
    if (!parse_row_inputs(line, &t, &g)) return "?";
    return line[0] == 'T' ? table_row(t) : generic_row(g);
}

#ifdef MSM_PLAN_TEXT
int main(int argc, char **argv) {
    if (argc < 3 || std::string(argv[1]) != "--rows") return 2;
    std::ifstream f(argv[2]);
    std::string line;
    while (std::getline(f, line))
        if (!line.empty() && line[0] != '#') printf("%s\n", row_of(line).c_str());
    return 0;
}
#else
static long violations = 0;
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

// what the kernels and msm_context_setup assume of every plan: the dynamic LDS sizes the stages ask for, the areas of cx.plan, the bits of a
// tagged entry, the accumulate's grid
static void check_plan(const MsmPlan &p, u32 lanes, const char *what) {
    const Sort2 &S = p.S2;
    if (p.use_sort2) {
        CHECK(s1_stage_bytes(S.nh, S.s1_scalars, (size_t)(p.glv ? 2 : 1) * p.sh.W) <= kLdsCap, "%s: pass-1 stage", what);
        CHECK(S.nh * 4 <= kLdsCap, "%s: pass-1 count", what);
        const Sort2Layout l = sort2_layout(S.nh, S.B2, S.lowb);
        CHECK(l.bin_count + S.nh <= l.bin_start && l.bin_start + S.nh + 1 <= l.hlo && l.hlo + S.B2 <= l.woff && l.woff + S.B2 + 1 <= l.hist2, "%s: plan areas overlap", what);
        CHECK(l.words == p.plan_words, "%s: plan_words %zu, layout %zu", what, p.plan_words, l.words);
        if (p.s2_bins_form) {
            CHECK(s2_bins_bytes(S.lowb, p.s2_cap_entries) <= kLdsCap, "%s: one-launch pass 2 stage of %zu entries", what, p.s2_cap_entries);
            CHECK(l.hist2 + s2_big_words(S.lowb) <= p.plan_words, "%s: oversized-bin list beyond plan_words", what);
        } else {
            CHECK(s2_count_bytes(S.lds_window, S.nh) <= kLdsCap && s2_scatter_bytes(S.lds_window, S.nh) <= kLdsCap, "%s: chunked pass 2", what);
            CHECK(l.hist2 + l.hist2_words <= p.plan_words, "%s: chunked pass 2's histograms beyond plan_words", what);
        }
        CHECK(S.c == p.sh.c && S.W == p.sh.W && S.nb == p.sh.NB && S.K2 == kS2Chunk && S.run_lanes == 16 && S.mont == 1, "%s: Sort2's copies of the shape", what);
        CHECK(S.side || S.lowb + S.lb <= 31, "%s: lowb %d + lb %d", what, S.lowb, S.lb);
    } else {
        CHECK((size_t)p.sh.NB * 4 <= 131072, "%s: one-pass sort over %u buckets", what, p.sh.NB);
    }
    CHECK(p.sh.m == p.m && p.sh.total_buckets == p.tb, "%s: the shape's copies", what);
    CHECK(p.T % 256 == 0 && p.T >= 256 && p.T <= std::max(256u, lanes / 256u * 256u), "%s: T %u of %u lanes", what, p.T, lanes);
    CHECK(p.K == 1 || (p.use_sort2 && p.s2_bins_form && p.fold9), "%s: batched plan without its forms", what);
}
static void check_grouped(const GroupedPlan &gp, const char *what) {
    for (int i = 0; i < gp.G; ++i) {
        const Group &g = gp.grp[i];
        CHECK(d1_stage_bytes(g.gs.nh, g.gs.S, g.ns) <= kLdsCap && g.gs.nh * 4 <= kLdsCap, "%s: group %d pass 1", what, i);
        CHECK(s2_bins_bytes(g.gs.lowb, g.cap) <= kLdsCap, "%s: group %d pass 2", what, i);
        CHECK(g.gs.lowb + g.gs.lb <= 31, "%s: group %d lowb %d + lb %d", what, i, g.gs.lowb, g.gs.lb);
        CHECK(group_big_offset(g.gs.nh) + s2_big_words(g.gs.lowb) <= g.plan_words && g.plan_words <= gp.plan_words, "%s: group %d plan area", what, i);
        CHECK(g.gs.w0 == g.w0 && g.gs.ns == g.ns && g.gs.nb * g.ns == g.tb && (size_t)g.gs.cols * g.ns == g.emax && g.gs.run_lanes == 16 && g.gs.row == ((g.gs.cols + 7) & ~7u), "%s: group %d pass-1 copies", what, i);
        CHECK(g.p2.lowb == g.gs.lowb && g.p2.lb == g.gs.lb && g.p2.nh == g.gs.nh && g.p2.nb == g.gs.nb && g.p2.pair_shift == -1, "%s: group %d pass-2 copies", what, i);
        CHECK(g.T % 512 == 0 && g.T >= 512, "%s: group %d T %u", what, i, g.T);
    }
}
static bool geometry(u32 cols, u32 ns, u32 nb, Group &g) {
    g = Group();
    g.ns = ns;
    return group_geometry(cols, nb, g);
}
// smallest n in (lo, hi] with pred(n); pred monotone, false at lo
template <class F> static size_t first(F pred, size_t lo, size_t hi) {
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (pred(mid)) hi = mid; else lo = mid;
    }
    return hi;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    printf("constants: LDS_CAP %zu MAX_C %d MAX_C_SHARED %d S1_SCALARS %u MAX_BIG %u MAX_COLS %d ERR_BATCH_SHAPE %d\n", kLdsCap, kMaxC, kMaxCShared, kS1Scalars, kMaxBig, kMaxCols, H2_ERR_BATCH_SHAPE);
    {   // the grouped form's size limits, by bisection on group_geometry at 16-bit windows (5 + 2 + 2 slices alone, one group of 9 beside others)
        Group g;
        auto fits = [&](size_t n, std::initializer_list<u32> slices) {
            for (u32 ns : slices)
                if (!geometry(2 * (u32)n, ns, 1u << 15, g)) return false;
            return true;
        };
        auto low = [&](size_t n) { geometry(2 * (u32)n, 5, 1u << 15, g); return g.gs.lowb; };
        const size_t latency_max = first([&](size_t n) { return !fits(n, {5, 2, 2}); }, (size_t)1 << 20, (size_t)1 << 24) - 1;
        const size_t throughput_max = first([&](size_t n) { return !fits(n, {9}); }, (size_t)1 << 19, (size_t)1 << 23) - 1;
        const size_t lowb7 = first([&](size_t n) { return low(n) <= 7; }, ((size_t)1 << 18) + 1, latency_max);
        const size_t lowb6 = first([&](size_t n) { return low(n) <= 6; }, lowb7, latency_max);
        printf("limits: LATENCY_MAX %zu THROUGHPUT_MAX %zu LOWB_7 %zu LOWB_6 %zu\n", latency_max, throughput_max, lowb7, lowb6);
    }
    long plans = 0, calls = 0;
    std::ifstream f(argv[1]);
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream in(line);
        char kind = 0;
        in >> kind;
        ++calls;
        if (kind == 'P') {
            TableCall t;
            in >> t.lanes >> t.points >> t.c >> t.n_used >> t.blind >> t.K >> t.pair >> t.add_into >> t.fold_only;
            const MsmArgs a = table_args(t);
            h2_commit_plan_t r;
            if (t.n_used + t.blind == 0 && !t.fold_only) {      // nothing to sum: msm_launch records that and plans nothing
                r = empty_summary(a, t.add_into ? 2u : 1u);
            } else {
                MsmPlan p;
                const int rc = plan_call(a, t.lanes, false, &p);
                if (rc != H2_OK) {
                    printf("ERR %d\n", rc);
                    continue;
                }
                ++plans;
                check_plan(p, t.lanes, line.c_str());
                r = plan_summary(p, t.lanes);
            }
            const uint32_t *w = &r.caller;
            for (size_t i = 0; i < sizeof r / 4; ++i) printf("%s%u", i ? " " : "", w[i]);
            printf("\n");
        } else if (kind == 'G') {
            GenericCall g;
            in >> g.lanes >> g.n >> g.instrumented >> g.in_flight;
            const MsmArgs a = generic_args(g);
            MsmPlan p;
            const int rc = plan_call(a, g.lanes, g.instrumented != 0, &p);
            if (rc != H2_OK) {
                printf("ERR %d\n", rc);
                continue;
            }
            ++plans;
            check_plan(p, g.lanes, line.c_str());
            // the form the call takes, as msm_launch decides it (h2_msm_last_path): the grouped form is asked first and may decline
            GroupedPlan gp;
            const bool grouped = p.try_grouped && grouped_call(a, p.sh, p.scalars_n, g.lanes, g.in_flight != 0, gp) == H2_OK;
            printf("c %d %s T %u split_k %d try_grouped %d", a.c, grouped ? (gp.throughput ? "grouped_throughput" : "grouped_latency") : p.split_k ? "slice_split" : p.use_sort2 ? "two_pass" : "one_pass",
                   p.T, p.split_k, (int)p.try_grouped);
            if (grouped) {
                check_grouped(gp, line.c_str());
                printf(" G %d", gp.G);
                for (int i = 0; i < gp.G; ++i) printf(" (%u %d %u %u %u)", gp.grp[i].ns, gp.grp[i].gs.lowb, gp.grp[i].gs.nh, gp.grp[i].gs.S, gp.grp[i].T);
            }
            printf("\n");
        } else if (kind == 'Q') {
            u32 cols, ns, nb;
            in >> cols >> ns >> nb;
            Group g;
            if (geometry(cols, ns, nb, g)) printf("%d %u %u\n", g.gs.lowb, g.gs.nh, g.gs.S);
            else printf("NONE\n");
        } else {
            size_t n;
            int x = 0;
            in >> n;
            if (kind == 'C' || kind == 'R') in >> x;
            printf("%d\n", kind == 'C' ? width_call(n, x != 0) : kind == 'W' ? column_window_bits(n, 0, kShipped) : kind == 'S' ? (int)pair_supported(n, kShipped)
                                                                                                                         : (int)register_width_ok(n, x));
        }
        if (in.fail()) {
            printf("bad call line: %s\n", line.c_str());
            return 2;
        }
    }
    printf("invariants: %ld plans of %ld calls, %ld violations\n", plans, calls, violations);

    // ---- the parent's plans: every word of them
    std::ifstream table(argv[2]);
    long rows = 0, mismatches = 0;
    while (std::getline(table, line)) {
        if (line.empty() || line[0] == '#') continue;
        ++rows;
        const std::string now = row_of(line);
        if (now != line && ++mismatches <= 10) printf("MISMATCH\n  was %s\n  now %s\n", line.c_str(), now.c_str());
    }
    printf("parent plans: %ld rows, %ld mismatches\n", rows, mismatches);
    return violations || mismatches || !rows ? 1 : 0;
}
#endif
