// Host driver of csrc/msm_digits.h (plain C++: the digit cutters of the bucket sort compile here exactly as the kernels use them).
// tests/test_msm_digits.py builds this with g++, feeds it values and judges the codes it prints; nothing is checked in here.
//   msm_digits_check <values>      one value per line (hex, no prefix):
//     S k              a scalar k < 2^256.  One answer line per width c = 2 .. kMaxCShared:
//                        "S c W <runtime cutter> <dispatcher> <compile-time cutter, or - where the dispatcher has none at c> <narrowed, or - beyond kMaxC>"
//                      32-bit codes as 8 hex digits each, the narrowed (16-bit) ones as 4, no separators inside a list
//     G n0 n1 m0 m1    the halves of a split scalar: signs n0, n1 (0 / 1) and magnitudes m0, m1 < 2^160.  One answer line per c = 2 .. kMaxC:
//                        "G c W <part 0, 16-bit codes> <part 0, 32-bit codes> <part 1, 16-bit> <part 1, 32-bit>"
// W comes from msm_plan.h's make_shape for that width and form.  The first line printed names the two width limits.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "../../halo2_amd/csrc/msm_digits.h"
#include "../../halo2_amd/csrc/msm_plan.h"
using namespace h2;

template <int N> static void limbs_of(const std::string &hex, u32 (&v)[N]) {
    memset(v, 0, sizeof(v));
    for (size_t i = 0; i < hex.size() && i < 8 * N; ++i) {
        const char ch = hex[hex.size() - 1 - i];
        const u32 nib = ch <= '9' ? ch - '0' : (ch | 0x20) - 'a' + 10;
        v[i / 8] |= nib << (4 * (i % 8));
    }
}

template <int C> static bool cut_static(int c, const u32 *s, std::string &out) {
    if (c != C) return false;
    char b[16];
    for_each_digit_static<C>(s, [&](int, u32 code) { snprintf(b, sizeof(b), "%08x", code); out += b; });
    return true;
}

static void scalar_lines(const u32 (&s)[8]) {
    for (int c = 2; c <= kMaxCShared; ++c) {
        const int W = make_shape(1, c, c > kMaxC).W;
        std::string rt, disp, stat, narrow;
        char b[16];
        for_each_digit_runtime(s, c, W, [&](int, u32 code) {
            snprintf(b, sizeof(b), "%08x", code); rt += b;
            snprintf(b, sizeof(b), "%04x", narrow_code(code)); narrow += b;
        });
        for_each_digit(s, c, W, [&](int, u32 code) { snprintf(b, sizeof(b), "%08x", code); disp += b; });
        if (!(cut_static<13>(c, s, stat) || cut_static<16>(c, s, stat) || cut_static<17>(c, s, stat) || cut_static<18>(c, s, stat) ||
              cut_static<19>(c, s, stat) || cut_static<20>(c, s, stat)))
            stat = "-";
        printf("S %d %d %s %s %s %s\n", c, W, rt.c_str(), disp.c_str(), stat.c_str(), c <= kMaxC ? narrow.c_str() : "-");
    }
}

static void glv_lines(const u32 (&mag)[2][5], const u32 (&neg)[2]) {
    for (int c = 2; c <= kMaxC; ++c) {
        const int W = make_shape(2, c, false, true).W;
        std::string c16[2], c32[2];
        char b[16];
        for_each_glv_digit(mag, neg, c, W, [&](int part, int, u32 digit_mag, u32 negative) {
            snprintf(b, sizeof(b), "%04x", digit_code16(digit_mag, negative)); c16[part] += b;
            snprintf(b, sizeof(b), "%08x", digit_code32(digit_mag, negative)); c32[part] += b;
        });
        printf("G %d %d %s %s %s %s\n", c, W, c16[0].c_str(), c32[0].c_str(), c16[1].c_str(), c32[1].c_str());
    }
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    printf("constants: MAX_C %d MAX_C_SHARED %d\n", kMaxC, kMaxCShared);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string kind, a, b;
        ls >> kind;
        if (kind == "S") {
            u32 s[8];
            ls >> a;
            limbs_of(a, s);
            scalar_lines(s);
        } else if (kind == "G") {
            u32 mag[2][5], neg[2];
            ls >> neg[0] >> neg[1] >> a >> b;
            limbs_of(a, mag[0]);
            limbs_of(b, mag[1]);
            glv_lines(mag, neg);
        } else if (!kind.empty()) {
            return 3;
        }
    }
    return 0;
}
