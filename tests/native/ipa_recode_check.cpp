// Host driver of csrc/ipa_recode.h (plain C++: the challenge recode compiles here exactly as collapse_launch uses it).
// tests/test_ipa_recode.py builds this with g++ under the address and undefined-behaviour sanitizers and checks what it prints.
//   ipa_recode_check fp|fq             canonical scalars on stdin, one per line as 64 hex digits; per scalar one line:
//                                      top, then the 257 digits of k1 and the 257 digits of k2 as glv_recode wrote them
//   ipa_recode_check fp|fq constants   the field's kGlv row: a1 |b1| a2 b2 g1 g2, one hex integer per line
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../halo2_amd/csrc/ipa_recode.h"

using namespace h2;

static void print_limbs(const char *name, const u64 *v, int n) {
    printf("%s 0x", name);
    for (int i = n - 1; i >= 0; --i) printf("%016llx", (unsigned long long)v[i]);
    printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 2 || (strcmp(argv[1], "fp") && strcmp(argv[1], "fq"))) return 2;
    const int field = strcmp(argv[1], "fq") ? H2_FP : H2_FQ;
    if (argc > 2) {
        const GlvConst &G = kGlv[field == H2_FQ ? 0 : 1];
        print_limbs("a1", G.a1, 2);
        print_limbs("b1_abs", G.b1_abs, 2);
        print_limbs("a2", G.a2, 2);
        print_limbs("b2", G.b2, 2);
        print_limbs("g1", G.g1, 3);
        print_limbs("g2", G.g2, 3);
        return 0;
    }
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        if (strspn(line, "0123456789abcdefABCDEF") != 64) return 3;
        u64 k[4];
        for (int i = 0; i < 4; ++i) {                  // limb 0 is the last 16 digits
            char limb[17];
            memcpy(limb, line + 16 * (3 - i), 16);
            limb[16] = 0;
            k[i] = strtoull(limb, nullptr, 16);
        }
        int8_t naf[2 * 264];                           // zeroed and sized as in collapse_launch
        memset(naf, 0, sizeof naf);
        const int top = glv_recode(field, k, naf, naf + 264);
        printf("%d", top);
        for (int r = 0; r < 2; ++r)
            for (int i = 0; i < 257; ++i) printf(" %d", naf[264 * r + i]);
        printf("\n");
    }
    return 0;
}
