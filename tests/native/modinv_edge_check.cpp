// The divstep inversion of halo2_amd/csrc/field_inv.cuh compiled for the HOST and applied to inputs read from a file.  TEST CODE with no checker
// in it: tests/test_field_inv_host.py builds the inputs (tests/field_edge_cases.py), builds this file with the undefined-behaviour and address
// sanitizers (the limb arithmetic is signed 32- and 64-bit: an overflow there would be undefined, and hipcc need not compile it as g++ does)
// and judges the outputs against pow(x, -1, p).
// Build: g++ -O1 -std=c++17 -fsanitize=undefined,address -fno-sanitize-recover=all tests/native/modinv_edge_check.cpp -o build/modinv_edge_check
// Usage: modinv_edge_check <fp|fq> <in> <out>
//   in:  x < p, 32 bytes little-endian each
//   out: 18 words of 32 bits per input: modinv30(x) (8 words); the same by modinv30's loop spelled out here, batch by batch (8 words); the sign
//        of the final f (+1 / -1, as int32); the number of 30-divstep batches after which g was zero for the first time (0 when x = 0)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../halo2_amd/csrc/field_inv.cuh"

static const uint32_t kP[2][8] = {{0x00000001u, 0x992d30edu, 0x094cf91bu, 0x224698fcu, 0, 0, 0, 0x40000000u},
                                  {0x00000001u, 0x8c46eb21u, 0x0994a8ddu, 0x224698fcu, 0, 0, 0, 0x40000000u}};

static bool s30_is_zero(const h2::s30 &a) {
    int32_t any = 0;
    for (int i = 0; i < 9; ++i) any |= a.v[i];
    return any == 0;
}

int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s <fp|fq> <in> <out>\n", argv[0]); return 2; }
    const int field = !strcmp(argv[1], "fp") ? 0 : !strcmp(argv[1], "fq") ? 1 : -1;
    if (field < 0) { fprintf(stderr, "unknown field\n"); return 2; }
    FILE *f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    std::vector<unsigned char> in;
    unsigned char buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) in.insert(in.end(), buf, buf + got);
    fclose(f);
    if (in.empty() || in.size() % 32) { fprintf(stderr, "bad input size %zu\n", in.size()); return 2; }
    const size_t n = in.size() / 32;
    std::vector<uint32_t> out(18 * n);
    for (size_t k = 0; k < n; ++k) {
        uint32_t x[8];
        memcpy(x, &in[32 * k], 32);
        uint32_t *o = &out[18 * k];
        h2::modinv30(x, kP[field], o);
        // modinv30's own loop, with a look at g after every batch
        const h2::s30 p = h2::s30_from_words(kP[field]);
        h2::s30 d = {{0, 0, 0, 0, 0, 0, 0, 0, 0}}, e = {{1, 0, 0, 0, 0, 0, 0, 0, 0}}, ff = p, g = h2::s30_from_words(x);
        int32_t zeta = -1, first_zero = s30_is_zero(g) ? 0 : -1;
        for (int i = 0; i < 20; ++i) {
            h2::t2x2 t;
            zeta = h2::divsteps_30(zeta, (uint32_t)ff.v[0], (uint32_t)g.v[0], t);
            h2::update_de_30(d, e, t, p);
            h2::update_fg_30(ff, g, t);
            if (first_zero < 0 && s30_is_zero(g)) first_zero = i + 1;
        }
        h2::normalize_30(d, ff.v[8], p);
        h2::s30_to_words(d, o + 8);
        const int32_t sign = ff.v[8] < 0 ? -1 : 1;
        memcpy(o + 16, &sign, 4);
        memcpy(o + 17, &first_zero, 4);
    }
    f = fopen(argv[3], "wb");
    if (!f) { perror(argv[3]); return 2; }
    const bool wrote = fwrite(out.data(), 4, out.size(), f) == out.size();
    if (fclose(f) != 0 || !wrote) { fprintf(stderr, "short write to %s\n", argv[3]); return 2; }
    printf("modinv30 %s: %zu inputs\n", argv[1], n);
    return 0;
}
