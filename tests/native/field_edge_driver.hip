// Applies one device function of the field layer (csrc/field.cuh, field9.cuh, field_inv.cuh) per lane to operands read from a file and writes
// the raw result words.  TEST CODE with no checker, no oracle and no timing in it: tests/test_gpu_field_edges.py builds the operands
// (tests/field_edge_cases.py) and judges the results with Python integers.  The product headers are included as the library includes them
// (no H2_FIELD_EXPERIMENTS): fe_mulx, fe9_mul and fe_inv are the shipped implementations, and `config` prints the switches that pick them.
// Build: hipcc --offload-arch=gfx950 -O3 tests/native/field_edge_driver.hip -o build/field_edge_driver
// Usage: field_edge_driver <mode> <fp|fq> <in> <out>      |      field_edge_driver config
//   in / out: per lane the operands / the result, 32-bit little-endian words.  f: a field element or 256-bit word, 8 x u32;
//   n: a 9 x 29 limb vector, 9 x i32; w: one word (a predicate).  Nothing is converted on the way: what the file holds is what the function sees.
//   mode             operands  result     function
//   mul              f f       f          fe_mulx(a, b)
//   sqr              f         f          fe_sqr(a)
//   mul_c            f f       f          fe_mul_c(a, b)
//   to_mont          f         f          fe_to_mont(a)
//   from_mont        f         f          fe_from_mont(a)
//   redc             f         f          fe_redc(a)
//   add sub          f f       f          fe_add / fe_sub
//   neg dbl          f         f          fe_neg / fe_dbl
//   reduce_once      f         f          fe_reduce_once(a)
//   mul_lazy         f f       f          fe_mul_lazy(a, b), as it leaves it
//   add_lazy         f f       f          fe_add_lazy(a, b)
//   sub_lazy         f f       f          fe_sub_lazy(a, b)
//   reduce_lazy      f         f          fe_reduce_lazy(a)
//   is_zero_lazy     f         w          fe_is_zero_lazy(a)
//   inv              f         f          fe_inv(a)
//   modinv30         f         f          modinv30(a, p)
//   unpack9          f         n          fe9_unpack(a)
//   pack9            n         f          fe9_pack(a)
//   from_r256        f         n          fe9_from_r256(a)
//   to_r256          n         f          fe9_to_r256(a)
//   mul9 mul9_c      n n       n          fe9_mul / fe9_mul_c
//   sqr9             n         n          fe9_sqr(a)
//   dot2             n n n n   n          fe9_dot2(a, b, c, d)
//   sqr_minus        n n       n          fe9_sqr_minus(a, s)
//   norm9            n         n          fe9_norm(a)
//   quadruple_norm9  n         n          fe9_quadruple_norm(a)
//   canonical9       n         f          fe9_canonical(a)
//   canonical_small9 n         f          fe9_canonical_small(a)
//   maybe_zero9      n         w          fe9_maybe_zero_mod_p(a)
//   is_zero9         n         w          fe9_is_zero_mod_p(a)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../halo2_amd/csrc/field9.cuh"

using namespace h2;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

enum { M_MUL, M_SQR, M_MUL_C, M_TO_MONT, M_FROM_MONT, M_REDC, M_ADD, M_SUB, M_NEG, M_DBL, M_REDUCE_ONCE, M_MUL_LAZY, M_ADD_LAZY, M_SUB_LAZY,
       M_REDUCE_LAZY, M_IS_ZERO_LAZY, M_INV, M_MODINV30, M_UNPACK9, M_PACK9, M_FROM_R256, M_TO_R256, M_MUL9, M_SQR9, M_MUL9_C, M_DOT2,
       M_SQR_MINUS, M_NORM9, M_QUADRUPLE_NORM9, M_CANONICAL9, M_CANONICAL_SMALL9, M_MAYBE_ZERO9, M_IS_ZERO9, M_COUNT };
struct mode_info { const char *name; const char *in; char out; };
static constexpr mode_info kModes[M_COUNT] = {
    {"mul", "ff", 'f'}, {"sqr", "f", 'f'}, {"mul_c", "ff", 'f'}, {"to_mont", "f", 'f'}, {"from_mont", "f", 'f'}, {"redc", "f", 'f'},
    {"add", "ff", 'f'}, {"sub", "ff", 'f'}, {"neg", "f", 'f'}, {"dbl", "f", 'f'}, {"reduce_once", "f", 'f'},
    {"mul_lazy", "ff", 'f'}, {"add_lazy", "ff", 'f'}, {"sub_lazy", "ff", 'f'}, {"reduce_lazy", "f", 'f'}, {"is_zero_lazy", "f", 'w'},
    {"inv", "f", 'f'}, {"modinv30", "f", 'f'},
    {"unpack9", "f", 'n'}, {"pack9", "n", 'f'}, {"from_r256", "f", 'n'}, {"to_r256", "n", 'f'}, {"mul9", "nn", 'n'}, {"sqr9", "n", 'n'},
    {"mul9_c", "nn", 'n'}, {"dot2", "nnnn", 'n'}, {"sqr_minus", "nn", 'n'}, {"norm9", "n", 'n'}, {"quadruple_norm9", "n", 'n'},
    {"canonical9", "n", 'f'}, {"canonical_small9", "n", 'f'}, {"maybe_zero9", "n", 'w'}, {"is_zero9", "n", 'w'}};
static constexpr int kind_words(char k) { return k == 'f' ? 8 : k == 'n' ? 9 : 1; }
static constexpr int words_in(int mode) {
    int n = 0;
    for (const char *k = kModes[mode].in; *k; ++k) n += kind_words(*k);
    return n;
}
static constexpr int words_out(int mode) { return kind_words(kModes[mode].out); }

__device__ __forceinline__ fe ld_fe(const u32 *p) {
    fe r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = p[i];
    return r;
}
__device__ __forceinline__ fe9 ld_fe9(const u32 *p) {
    fe9 r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.v[i] = (i32)p[i];
    return r;
}
__device__ __forceinline__ void st(u32 *p, const fe &a) {
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = a.v[i];
}
__device__ __forceinline__ void st(u32 *p, const fe9 &a) {
#pragma unroll
    for (int i = 0; i < 9; ++i) p[i] = (u32)a.v[i];
}
__device__ __forceinline__ void st(u32 *p, bool flag) { p[0] = flag ? 1u : 0u; }

template <int F, int MODE> __global__ void __launch_bounds__(256) k_edge(const u32 *__restrict__ in, u32 *__restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int WI = words_in(MODE), WO = words_out(MODE);
    const u32 *q = in + (size_t)WI * i;
    u32 *o = out + (size_t)WO * i;
    if constexpr (MODE == M_MUL) st(o, fe_mulx<F>(ld_fe(q), ld_fe(q + 8)));
    if constexpr (MODE == M_SQR) st(o, fe_sqr<F>(ld_fe(q)));
    if constexpr (MODE == M_MUL_C) st(o, fe_mul_c<F>(ld_fe(q), ld_fe(q + 8)));
    if constexpr (MODE == M_TO_MONT) st(o, fe_to_mont<F>(ld_fe(q)));
    if constexpr (MODE == M_FROM_MONT) st(o, fe_from_mont<F>(ld_fe(q)));
    if constexpr (MODE == M_REDC) st(o, fe_redc<F>(ld_fe(q)));
    if constexpr (MODE == M_ADD) st(o, fe_add<F>(ld_fe(q), ld_fe(q + 8)));
    if constexpr (MODE == M_SUB) st(o, fe_sub<F>(ld_fe(q), ld_fe(q + 8)));
    if constexpr (MODE == M_NEG) st(o, fe_neg<F>(ld_fe(q)));
    if constexpr (MODE == M_DBL) st(o, fe_dbl<F>(ld_fe(q)));
    if constexpr (MODE == M_REDUCE_ONCE) st(o, fe_reduce_once<F>(ld_fe(q)));
    if constexpr (MODE == M_MUL_LAZY) st(o, fe_mul_lazy<F>(ld_fe(q), ld_fe(q + 8)));
    if constexpr (MODE == M_ADD_LAZY) st(o, fe_add_lazy<F>(ld_fe(q), ld_fe(q + 8)));
    if constexpr (MODE == M_SUB_LAZY) st(o, fe_sub_lazy<F>(ld_fe(q), ld_fe(q + 8)));
    if constexpr (MODE == M_REDUCE_LAZY) st(o, fe_reduce_lazy<F>(ld_fe(q)));
    if constexpr (MODE == M_IS_ZERO_LAZY) st(o, fe_is_zero_lazy<F>(ld_fe(q)));
    if constexpr (MODE == M_INV) st(o, fe_inv<F>(ld_fe(q)));
    if constexpr (MODE == M_MODINV30) {
        const fe x = ld_fe(q);
        u32 p[8];
        fe y;
#pragma unroll
        for (int j = 0; j < 8; ++j) p[j] = mod_limb<F>(j);
        modinv30(x.v, p, y.v);
        st(o, y);
    }
    if constexpr (MODE == M_UNPACK9) st(o, fe9_unpack(ld_fe(q)));
    if constexpr (MODE == M_PACK9) st(o, fe9_pack(ld_fe9(q)));
    if constexpr (MODE == M_FROM_R256) st(o, fe9_from_r256<F>(ld_fe(q)));
    if constexpr (MODE == M_TO_R256) st(o, fe9_to_r256<F>(ld_fe9(q)));
    if constexpr (MODE == M_MUL9) st(o, fe9_mul<F>(ld_fe9(q), ld_fe9(q + 9)));
    if constexpr (MODE == M_SQR9) st(o, fe9_sqr<F>(ld_fe9(q)));
    if constexpr (MODE == M_MUL9_C) st(o, fe9_mul_c<F>(ld_fe9(q), ld_fe9(q + 9)));
    if constexpr (MODE == M_DOT2) st(o, fe9_dot2<F>(ld_fe9(q), ld_fe9(q + 9), ld_fe9(q + 18), ld_fe9(q + 27)));
    if constexpr (MODE == M_SQR_MINUS) st(o, fe9_sqr_minus<F>(ld_fe9(q), ld_fe9(q + 9)));
    if constexpr (MODE == M_NORM9) st(o, fe9_norm(ld_fe9(q)));
    if constexpr (MODE == M_QUADRUPLE_NORM9) st(o, fe9_quadruple_norm(ld_fe9(q)));
    if constexpr (MODE == M_CANONICAL9) st(o, fe9_canonical<F>(ld_fe9(q)));
    if constexpr (MODE == M_CANONICAL_SMALL9) st(o, fe9_canonical_small<F>(ld_fe9(q)));
    if constexpr (MODE == M_MAYBE_ZERO9) st(o, fe9_maybe_zero_mod_p(ld_fe9(q)));
    if constexpr (MODE == M_IS_ZERO9) st(o, fe9_is_zero_mod_p<F>(ld_fe9(q)));
}

template <int F, int MODE> static void launch_mode(int mode, const u32 *in, u32 *out, size_t n) {
    if constexpr (MODE < M_COUNT) {
        if (mode == MODE) hipLaunchKernelGGL((k_edge<F, MODE>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, in, out, n);
        else launch_mode<F, MODE + 1>(mode, in, out, n);
    }
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "config")) {
        printf("H2_MUL_IMPL %d\nH2_FE9_IMPL %d\nH2_FE_INV_FERMAT %d\n", H2_MUL_IMPL, H2_FE9_IMPL, H2_FE_INV_FERMAT);
#ifdef H2_FIELD_EXPERIMENTS
        printf("H2_FIELD_EXPERIMENTS defined\n");
#endif
        return 0;
    }
    if (argc != 5) { fprintf(stderr, "usage: %s <mode> <fp|fq> <in> <out>   |   %s config\n", argv[0], argv[0]); return 2; }
    int mode = -1;
    for (int m = 0; m < M_COUNT; ++m) if (!strcmp(argv[1], kModes[m].name)) mode = m;
    const int field = !strcmp(argv[2], "fp") ? FP : !strcmp(argv[2], "fq") ? FQ : -1;
    if (mode < 0 || field < 0) { fprintf(stderr, "unknown mode or field\n"); return 2; }
    int wi = 0;
    for (const char *k = kModes[mode].in; *k; ++k) wi += kind_words(*k);
    const int wo = kind_words(kModes[mode].out);
    FILE *f = fopen(argv[3], "rb");
    if (!f) { perror(argv[3]); return 2; }
    std::vector<unsigned char> in;
    unsigned char buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) in.insert(in.end(), buf, buf + got);
    fclose(f);
    const size_t case_bytes = 4 * (size_t)wi;
    if (in.empty() || in.size() % case_bytes || in.size() / case_bytes > ((size_t)1 << 20)) { fprintf(stderr, "bad input size %zu\n", in.size()); return 2; }
    const size_t n = in.size() / case_bytes, out_bytes = 4 * (size_t)wo * n;
    std::vector<unsigned char> out(out_bytes);
    u32 *d_in = nullptr, *d_out = nullptr;
    CK(hipMalloc(&d_in, in.size()));
    CK(hipMalloc(&d_out, out_bytes));
    CK(hipMemcpy(d_in, in.data(), in.size(), hipMemcpyHostToDevice));
    CK(hipMemset(d_out, 0xff, out_bytes));                       // a lane that stored nothing shows as all ones, not as a value
    if (field == FP) launch_mode<FP, 0>(mode, d_in, d_out, n);
    else launch_mode<FQ, 0>(mode, d_in, d_out, n);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out.data(), d_out, out_bytes, hipMemcpyDeviceToHost));
    CK(hipFree(d_in));
    CK(hipFree(d_out));
    f = fopen(argv[4], "wb");
    if (!f) { perror(argv[4]); return 2; }
    const bool wrote = fwrite(out.data(), 1, out_bytes, f) == out_bytes;
    if (fclose(f) != 0 || !wrote) { fprintf(stderr, "short write to %s\n", argv[4]); return 2; }
    printf("%s %s: %zu lanes\n", kModes[mode].name, argv[2], n);
    return 0;
}
