// Applies the device functions of the square root (csrc/field_sqrt.cuh) and of the hash-to-curve map (csrc/h2c_map.cuh) to inputs read
// from a file and writes what they return.  TEST CODE with no checker in it: tests/test_gpu_h2c_edges.py builds the inputs
// (tests/h2c_edge_cases.py) and judges the outputs against big-integer arithmetic.
// Build: hipcc --offload-arch=gfx950 -O3 tests/native/h2c_edge_driver.hip -o build/h2c_edge_driver
// Usage: h2c_edge_driver <sqrt|swu|add|iso|pair> <fp|fq> <in> <out>
//   in / out: canonical integers, 32 bytes little-endian each; the device converts with fe_to_mont / fe_from_mont.
//   mode  words in           words out
//   sqrt  a                  flag fe_sqrt returned, the root it wrote (0 where it wrote none)
//   swu   u                  x, y on the iso curve
//   add   x0, y0, x1, y1     x3, y3, identity flag ((0, 0, 1) for the identity)
//   iso   x, y               X, Y on y^2 = x^3 + 5, (0, 0) for the identity
//   pair  u0, u1             what h2c_kernel computes from (u0, u1) after hashing, (0, 0) for the identity
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../halo2_amd/csrc/h2c_map.cuh"

using namespace h2;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

enum { M_SQRT, M_SWU, M_ADD, M_ISO, M_PAIR, M_COUNT };
static const char *kModes[M_COUNT] = {"sqrt", "swu", "add", "iso", "pair"};
static const int kWordsIn[M_COUNT] = {1, 1, 4, 2, 2}, kWordsOut[M_COUNT] = {2, 2, 3, 2, 2};

__device__ __forceinline__ fe fe_small(u32 v) { fe r = fe_zero(); r.v[0] = v; return r; }

template <int F, int MODE> __global__ void __launch_bounds__(128) k_edge(const u32 *__restrict__ in, u32 *__restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    constexpr int WI = MODE == M_ADD ? 4 : (MODE == M_SQRT || MODE == M_SWU) ? 1 : 2, WO = MODE == M_ADD ? 3 : 2;
    fe a[WI], r[WO];
    for (int j = 0; j < WI; ++j) a[j] = fe_to_mont<F>(fe_load(in + 8 * (WI * i + j)));
    for (int j = 0; j < WO; ++j) r[j] = fe_zero();
    bool flag = false;
    if constexpr (MODE == M_SQRT) flag = fe_sqrt<F>(a[0], r[1]);
    if constexpr (MODE == M_SWU) map_to_curve_simple_swu<F>(a[0], r[0], r[1]);
    if constexpr (MODE == M_ADD) flag = !h2c_iso_add<F>(a[0], a[1], a[2], a[3], r[0], r[1]);
    if constexpr (MODE == M_ISO) h2c_iso_map<F>(a[0], a[1], r[0], r[1]);
    if constexpr (MODE == M_PAIR) h2c_map_pair<F>(a[0], a[1], r[0], r[1]);
    for (int j = 0; j < WO; ++j) r[j] = fe_from_mont<F>(r[j]);
    if (MODE == M_SQRT) r[0] = fe_small(flag ? 1u : 0u);
    if (MODE == M_ADD) r[WO - 1] = fe_small(flag ? 1u : 0u);
    for (int j = 0; j < WO; ++j) fe_store(out + 8 * (WO * i + j), r[j]);
}

template <int F> static void launch(int mode, const u32 *in, u32 *out, size_t n) {
    const dim3 grid((unsigned)((n + 127) / 128)), block(128);
    switch (mode) {
        case M_SQRT: hipLaunchKernelGGL((k_edge<F, M_SQRT>), grid, block, 0, 0, in, out, n); break;
        case M_SWU: hipLaunchKernelGGL((k_edge<F, M_SWU>), grid, block, 0, 0, in, out, n); break;
        case M_ADD: hipLaunchKernelGGL((k_edge<F, M_ADD>), grid, block, 0, 0, in, out, n); break;
        case M_ISO: hipLaunchKernelGGL((k_edge<F, M_ISO>), grid, block, 0, 0, in, out, n); break;
        default: hipLaunchKernelGGL((k_edge<F, M_PAIR>), grid, block, 0, 0, in, out, n); break;
    }
}

int main(int argc, char **argv) {
    if (argc != 5) { fprintf(stderr, "usage: %s <sqrt|swu|add|iso|pair> <fp|fq> <in> <out>\n", argv[0]); return 2; }
    int mode = -1;
    for (int m = 0; m < M_COUNT; ++m) if (!strcmp(argv[1], kModes[m])) mode = m;
    const int field = !strcmp(argv[2], "fp") ? FP : !strcmp(argv[2], "fq") ? FQ : -1;
    if (mode < 0 || field < 0) { fprintf(stderr, "unknown mode or field\n"); return 2; }
    FILE *f = fopen(argv[3], "rb");
    if (!f) { perror(argv[3]); return 2; }
    std::vector<unsigned char> in;
    unsigned char buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) in.insert(in.end(), buf, buf + got);
    fclose(f);
    const size_t case_bytes = 32 * (size_t)kWordsIn[mode];
    if (in.empty() || in.size() % case_bytes || in.size() / case_bytes > ((size_t)1 << 20)) { fprintf(stderr, "bad input size %zu\n", in.size()); return 2; }
    const size_t n = in.size() / case_bytes, out_bytes = 32 * (size_t)kWordsOut[mode] * n;
    std::vector<unsigned char> out(out_bytes);
    u32 *d_in = nullptr, *d_out = nullptr;
    CK(hipMalloc(&d_in, in.size()));
    CK(hipMalloc(&d_out, out_bytes));
    CK(hipMemcpy(d_in, in.data(), in.size(), hipMemcpyHostToDevice));
    CK(hipMemset(d_out, 0xff, out_bytes));                       // a lane that stored nothing shows as 2^256 - 1, not as a value
    if (field == FP) launch<FP>(mode, d_in, d_out, n);
    else launch<FQ>(mode, d_in, d_out, n);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out.data(), d_out, out_bytes, hipMemcpyDeviceToHost));
    CK(hipFree(d_in));
    CK(hipFree(d_out));
    f = fopen(argv[4], "wb");
    if (!f) { perror(argv[4]); return 2; }
    const bool wrote = fwrite(out.data(), 1, out_bytes, f) == out_bytes;
    if (fclose(f) != 0 || !wrote) { fprintf(stderr, "short write to %s\n", argv[4]); return 2; }
    printf("%s %s: %zu cases\n", kModes[mode], argv[2], n);
    return 0;
}
