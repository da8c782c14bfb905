// Native parity + throughput check of the gfx950 field arithmetic against the C oracle.
// TEST CODE: links oracle/h2_oracle.c (allowed: tests may use the oracle as the checker).
// Build: hipcc --offload-arch=gfx950 -O3 tests/native/field_check.hip oracle/h2_oracle.c -o build/field_check
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#define H2_FIELD_EXPERIMENTS 1
#include "../../halo2_amd/csrc/field.cuh"
#include "../../halo2_amd/csrc/curve9.cuh"
#include "../../halo2_amd/csrc/curve9_wide.cuh"

extern "C" {
void orc_f_mul(int field, uint64_t *r, const uint64_t *a, const uint64_t *b);
void orc_f_add(int field, uint64_t *r, const uint64_t *a, const uint64_t *b);
void orc_f_sub(int field, uint64_t *r, const uint64_t *a, const uint64_t *b);
void orc_f_inv(int field, uint64_t *r, const uint64_t *a);
void orc_random_field(int field, uint64_t seed, uint64_t *out, size_t n);
void orc_from_mont(int field, uint64_t *a, size_t n);
void orc_to_mont(int field, uint64_t *a, size_t n);
void orc_point_mul(int curve, uint64_t *out_xyz, const uint64_t *p_xy, const uint64_t *k_canonical);
void orc_point_to_affine(int curve, uint64_t *out_xy, const uint64_t *in_xyz);
}
using namespace h2;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

// op: 0 mul_c, 1 mul_col, 2 mul(per-product asm), 3 add, 4 sub, 5 inv, 6 mul_blk
template <int F> __global__ void k_ops(const u32 *a, const u32 *b, u32 *out, int n, int op) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe x = fe_load(a + 8 * i), y = fe_load(b + 8 * i), r;
    switch (op) {
        case 0: r = fe_mul_c<F>(x, y); break;
        case 1: r = fe_mul_col<F>(x, y); break;
        case 2: r = fe_mul<F>(x, y); break;
        case 3: r = fe_add<F>(x, y); break;
        case 4: r = fe_sub<F>(x, y); break;
        case 6: r = fe_mul_blk<F>(x, y); break;
        case 7: r = fe_mul_sched<F>(x, y); break;
        default: r = fe_inv<F>(x); break;
    }
    fe_store(out + 8 * i, r);
}

// ---- lazy arithmetic (field.cuh "lazy reduction"): every result, made canonical, must equal the canonical computation.
// a, b arrive canonical; `ka`, `kb` in {0, 1, 2} pick the representative a + ka p / b + kb p (skipped when it would not be
// a legal lazy value, i.e. >= 2p + 2^200).  mode 0: mul, 1: sub, 2: is-zero of (a - b), 3: 300 dependent squarings + subs.
template <int F> __device__ fe add_kp(fe v, int k) {
    for (int r = 0; r < k; ++r) {
        u32 c = 0;
        for (int i = 0; i < 8; i++) { u32 co; v.v[i] = __builtin_addc(v.v[i], mod_limb<F>(i), c, &co); c = co; }
    }
    return v;
}
template <int F> __global__ void k_lazy(const u32 *a, const u32 *b, u32 *out, int n, int mode, int ka, int kb) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe x = fe_load(a + 8 * i), y = fe_load(b + 8 * i);
    // a value may only sit in [2p, 2p + d) if its residue is tiny: keep the representative legal
    const bool x_small = (x.v[7] | x.v[6] | x.v[5] | x.v[4]) == 0, y_small = (y.v[7] | y.v[6] | y.v[5] | y.v[4]) == 0;
    fe xl = add_kp<F>(x, (ka == 2 && !x_small) ? 1 : ka), yl = add_kp<F>(y, (kb == 2 && !y_small) ? 1 : kb);
    fe r;
    if (mode == 0) r = fe_reduce_lazy<F>(fe_mul_lazy<F>(xl, yl));
    else if (mode == 1) r = fe_reduce_lazy<F>(fe_sub_lazy<F>(xl, yl));
    else if (mode == 2) { r = fe_zero(); r.v[0] = fe_is_zero_lazy<F>(fe_sub_lazy<F>(xl, yl)) ? 1u : 0u; }
    else {
        fe u = xl, v = x;
        for (int it = 0; it < 300; ++it) {
            u = fe_sub_lazy<F>(fe_mul_lazy<F>(u, u), yl);      // u <- u^2 - y, lazily
            v = fe_sub<F>(fe_mulx<F>(v, v), y);                // canonically
        }
        r = fe_reduce_lazy<F>(u);
        if (!fe_eq(r, v)) r.v[0] ^= 0xdeadbeefu;               // flagged below as a mismatch against v
        else r = fe_zero();
    }
    fe_store(out + 8 * i, r);
}

template <int F, int IMPL> __global__ void __launch_bounds__(256) k_chain(const u32 *a, u32 *out, int iters) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    fe x = fe_load(a + 8 * (i & 1023)), y = fe_load(a + 8 * ((i + 7) & 1023));
    fe z = y, w = x;
    for (int it = 0; it < iters; ++it) {
        if (IMPL == 0) { x = fe_mul_c<F>(x, y); z = fe_mul_c<F>(z, w); }
        if (IMPL == 1) { x = fe_mul_col<F>(x, y); z = fe_mul_col<F>(z, w); }
        if (IMPL == 2) { x = fe_mul<F>(x, y); z = fe_mul<F>(z, w); }
        if (IMPL == 3) { x = fe_mul_blk<F>(x, y); z = fe_mul_blk<F>(z, w); }
        if (IMPL == 4) { x = fe_mul_sched<F>(x, y); z = fe_mul_sched<F>(z, w); }
    }
    fe_store(out + 8 * i, fe_add<F>(x, z));
}

// ---- the carry-free 9 x 29 layer (field9.cuh) against the C oracle.  Inputs / outputs cross in the reference's Montgomery form.
// op 0: mul   1: sqr   2: (a - b)^2 (a + b - 3a) on signed un-normalised limbs   3: a - b after a carry pass
// op 4: bridge round trip r256 -> M9 -> r256   5: plain-C multiplier (fe9_mul_c)   6: M9 table form (aff_to_m9 + unpack) times b
// op 8: fe9_dot2 (two products, one reduction)   9: fe9_sqr_minus (subtrahend in the upper columns of the square)
template <int F> __global__ void k_ops9(const u32 *a, const u32 *b, u32 *out, int n, int op) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const fe x = fe_load(a + 8 * i), y = fe_load(b + 8 * i);
    const fe9 x9 = fe9_from_r256<F>(x), y9 = fe9_from_r256<F>(y);
    fe r;
    switch (op) {
        case 0: r = fe9_to_r256<F>(fe9_mul<F>(x9, y9)); break;
        case 1: r = fe9_to_r256<F>(fe9_sqr<F>(x9)); break;
        case 2: r = fe9_to_r256<F>(fe9_mul<F>(fe9_sqr<F>(fe9_sub(x9, y9)), fe9_sub(fe9_add(x9, y9), fe9_add(fe9_dbl(x9), x9)))); break;
        case 3: r = fe9_to_r256<F>(fe9_norm(fe9_sub(x9, y9))); break;
        case 4: r = fe9_to_r256<F>(x9); break;
        case 5: r = fe9_to_r256<F>(fe9_mul_c<F>(x9, y9)); break;
        case 7: r = fe_redc<F>(x); break;                                  // = fe_from_mont: the sort kernels' canonicalisation
        case 8: r = fe9_to_r256<F>(fe9_dot2<F>(x9, y9, fe9_sub(x9, y9), fe9_sub(fe9_zero(), fe9_add(x9, y9)))); break;   // a b - (a - b)(a + b), signed limbs
        case 9: r = fe9_to_r256<F>(fe9_sqr_minus<F>(fe9_sub(x9, y9), fe9_add(fe9_dbl(x9), y9))); break;                   // (a - b)^2 - (2 a + b)
        default: {
            affine<F> pt{x, x};
            const aff9<F> q = aff9_unpack<F>(aff_to_m9<F>(pt));
            r = fe9_to_r256<F>(fe9_mul<F>(q.x, y9));
        }
    }
    fe_store(out + 8 * i, r);
}
// ---- quad-lane point doubling on the carry-free layer (curve9_wide.cuh) against the 8 x 32 one (curve_wide.cuh) ---------------
// mode 0: a chain of `reps` doublings from the affine point (a[i], b[i]) (the formulas are polynomial identities: the point need
// not lie on the curve).  mode 1: ONE doubling from a raw M9 state -- the recorded state whose Y^2 leaves the multiplier with
// limb 0 equal to 2^29 (the only limb value 4 * limb does not fit an i32 for; fe9_quadruple_norm).
template <int F> __global__ void k_dbl9_wide(const u32 *a, const u32 *b, const u32 *raw, u32 *out, int n, int reps, int mode) {
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) / kGroup;
    if (i >= n) return;
    xyzz<F> r;
    xyzz9<F> r9;
    if (mode == 0) {
        const affine<F> p{fe_load(a + 8 * i), fe_load(b + 8 * i)};
        r = xyzz_identity<F>();
        xyzz_madd<F>(r, p);
        r9 = xyzz9_from_r256_wide<F>(r);
    } else {
        r9 = xyzz9_load_raw<F>(raw);
        r = xyzz9_to_r256_wide<F>(r9);
    }
    for (int k = 0; k < reps; ++k) {
        r = xyzz_dbl_wide<F>(r);
        r9 = xyzz9_dbl_wide<F>(r9);
    }
    const xyzz<F> o = xyzz9_to_r256_wide<F>(r9);
    bool same = true;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        same = same && o.x.v[j] == r.x.v[j] && o.y.v[j] == r.y.v[j] && o.zz.v[j] == r.zz.v[j] && o.zzz.v[j] == r.zzz.v[j];
    if ((threadIdx.x & (kGroup - 1)) == 0) out[i] = same ? 0u : 1u;
}
__global__ void k_quadruple_norm(u32 *out) {
    fe9 a = fe9_zero();
    a.v[0] = 1 << 29;                                      // what a product may leave in limb 0
    for (int i = 1; i < 8; i++) a.v[i] = (i32)M29 - i;
    a.v[8] = -5;
    const fe9 got = fe9_quadruple_norm(a), want = fe9_norm(fe9_dbl(fe9_norm(fe9_dbl(fe9_norm(a)))));
    u32 bad = 0;
    for (int i = 0; i < 9; i++) bad |= (u32)(got.v[i] != want.v[i]);
    out[0] = bad;
}
template <int F> int run_wide9(const u32 *da, const u32 *db, int n) {
    static const u32 kState[36] = {     // Fq, M9 limbs of (X, Y, ZZ, ZZZ): doubling 221 of a 16-bit table chain, found on the device
        0x038d27b2, 0x05039a9d, 0x12356f7c, 0x15b60e05, 0x0faf35a4, 0x07a6a677, 0x08780ea0, 0x03734c88, 0x00079790,
        0x01198606, 0x150a0983, 0x15963169, 0x0228e707, 0x076b97cb, 0x15217f1f, 0x0be3beab, 0x1454604c, 0xffe0f2ac,
        0x0413c791, 0x16925096, 0x1558a0c2, 0x09ab6c99, 0x1f698236, 0x043fa20f, 0x1804ede6, 0x0404f056, 0x00394ee7,
        0x00ae9230, 0x090ab3d3, 0x0c3cf140, 0x1de44147, 0x0ac239cf, 0x12ae76e2, 0x0bd3b3ec, 0x1aa2ffd3, 0x00369c3d};
    u32 *draw, *dflag;
    CK(hipMalloc(&draw, sizeof(kState)));
    CK(hipMalloc(&dflag, 4 * (size_t)n));
    CK(hipMemcpy(draw, kState, sizeof(kState), hipMemcpyHostToDevice));
    std::vector<u32> flag(n);
    int fails = 0;
    for (int mode = 0; mode < (F == FQ ? 2 : 1); ++mode) {
        const int cnt = mode ? 1 : n, reps = mode ? 1 : 48;
        hipLaunchKernelGGL((k_dbl9_wide<F>), dim3((cnt * kGroup + 255) / 256), dim3(256), 0, 0, da, db, draw, dflag, cnt, reps, mode);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(flag.data(), dflag, 4 * (size_t)cnt, hipMemcpyDeviceToHost));
        int bad = 0;
        for (int i = 0; i < cnt; ++i) bad += flag[i] != 0;
        printf("field %d %-16s: %d/%d mismatches\n", F, mode ? "dbl9 wide 2^29" : "dbl9 wide chain", bad, cnt);
        fails += bad != 0;
    }
    hipLaunchKernelGGL(k_quadruple_norm, dim3(1), dim3(1), 0, 0, dflag);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(flag.data(), dflag, 4, hipMemcpyDeviceToHost));
    printf("field %d %-16s: %d/1 mismatches\n", F, "quadruple norm", (int)flag[0]);
    fails += flag[0] != 0;
    (void)hipFree(draw);
    (void)hipFree(dflag);
    return fails;
}
template <int F> int run_field9(const std::vector<uint64_t> &a, const std::vector<uint64_t> &b, const u32 *da, const u32 *db, u32 *dout, int n) {
    std::vector<uint64_t> got(4 * (size_t)n);
    const char *names[] = {"fe9 mul", "fe9 sqr", "fe9 signed chain", "fe9 sub+norm", "fe9 bridge", "fe9 mul_c", "fe9 table form", "fe_redc", "fe9 dot2", "fe9 sqr_minus"};
    int fails = 0;
    for (int op = 0; op < 10; ++op) {
        hipLaunchKernelGGL((k_ops9<F>), dim3((n + 255) / 256), dim3(256), 0, 0, da, db, dout, n, op);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(got.data(), dout, 32 * (size_t)n, hipMemcpyDeviceToHost));
        int bad = 0;
        for (int i = 0; i < n; ++i) {
            uint64_t w[4], t[4], u[4];
            const uint64_t *x = &a[4 * i], *y = &b[4 * i];
            if (op == 0 || op == 5 || op == 6) orc_f_mul(F, w, x, y);
            else if (op == 1) orc_f_mul(F, w, x, x);
            else if (op == 2) {
                orc_f_sub(F, t, x, y); orc_f_mul(F, t, t, t);                    // (a - b)^2
                orc_f_add(F, u, x, y); orc_f_sub(F, u, u, x); orc_f_sub(F, u, u, x); orc_f_sub(F, u, u, x);
                orc_f_mul(F, w, t, u);
            } else if (op == 3) orc_f_sub(F, w, x, y);
            else if (op == 7) { memcpy(w, x, 32); orc_from_mont(F, w, 1); }
            else if (op == 8) {
                orc_f_mul(F, w, x, y); orc_f_sub(F, t, x, y); orc_f_add(F, u, x, y); orc_f_mul(F, t, t, u); orc_f_sub(F, w, w, t);
            } else if (op == 9) {
                orc_f_sub(F, t, x, y); orc_f_mul(F, t, t, t); orc_f_add(F, u, x, x); orc_f_add(F, u, u, y); orc_f_sub(F, w, t, u);
            } else memcpy(w, x, 32);
            if (memcmp(w, &got[4 * i], 32)) { if (!bad) printf("  first mismatch %s idx %d\n", names[op], i); bad++; }
        }
        printf("field %d %-16s: %d/%d mismatches\n", F, names[op], bad, n);
        fails += bad;
    }
    return fails;
}

// ---- exceptional additions: every addition / doubling form on P + P, P - P and O, against the oracle's complete group law ----------
// All operands are multiples c G of the oracle's generator (affine, reference Montgomery form), so the expected sum is a table entry.
// One quad of lanes per case: the quad-lane forms need all four lanes, the one-lane forms run on each lane and lane 0 stores.
enum { XF_MADD9, XF_MADD9_HOT, XF_ADD9, XF_ADD9_WIDE, XF_DBL9_WIDE, XF_MADD, XF_MADD_LAZY, XF_ADD, XF_ADD_WIDE, XF_HOT_THEN, XF_MADD9_THEN, XF_COUNT };
// chain forms (64 steps from the identity, one palette point per step)
enum { XC_MADD9_HOT, XC_MADD9, XC_ADD9, XC_ADD9_WIDE, XC_MADD, XC_MADD_LAZY, XC_ADD, XC_ADD_WIDE, XC_COUNT };
static constexpr int kChainSteps = 64;

template <int F> __device__ xyzz<F> xc_rescaled(const affine<F> &p, const fe &lam) {      // (l^2 x, l^3 y, l^2, l^3)
    if (aff_is_identity(p)) return xyzz_identity<F>();
    const fe l2 = fe_sqr<F>(lam), l3 = fe_mulx<F>(l2, lam);
    return xyzz<F>{fe_mulx<F>(p.x, l2), fe_mulx<F>(p.y, l3), l2, l3};
}
template <int F> __device__ void xc_store(u32 *dst, const xyzz<F> &r) {
    const affine<F> a = xyzz_to_affine<F>(r);
    if ((threadIdx.x & (kGroup - 1)) == 0) { fe_store(dst, a.x); fe_store(dst + 8, a.y); }
}
template <int F> __device__ void xc_store9(u32 *dst, const xyzz9<F> &r) { xc_store<F>(dst, xyzz9_to_r256<F>(r)); }
// the operand bounds of curve9.cuh's header that fe9_maybe_zero_mod_p relies on: limbs 0..7 in [0, 2^29] and
// |value| < 2^258 (limb 8 in (-2^26, 2^26 - 1)) for X, |value| < 2^256 (|limb 8| < 2^24) for Y, ZZ, ZZZ
__device__ bool xc_limbs_ok(const fe9 &a, i32 top) {
    bool ok = a.v[8] > -top && a.v[8] < top - 1;
#pragma unroll
    for (int i = 0; i < 8; i++) ok = ok && a.v[i] >= 0 && a.v[i] <= (i32)(1u << 29);
    return ok;
}
template <int F> __device__ bool xc_acc_ok(const xyzz9<F> &a) {
    return xc_limbs_ok(a.x, 1 << 26) && xc_limbs_ok(a.y, 1 << 24) && xc_limbs_ok(a.zz, 1 << 24) && xc_limbs_ok(a.zzz, 1 << 24);
}
// the difference the filter sees, carried: |value| < 2^258 < 16 p
__device__ bool xc_diff_ok(const fe9 &d) { return xc_limbs_ok(fe9_norm(d), 1 << 26); }

// pts: per case A, B, A1, A2, B1, B2, C (A = A1 + A2, B = B1 + B2, C != O); lam: per case lambda_A, lambda_B (nonzero).
// mode bit 0: A is the output of two additions instead of a rescaled point; bit 1: the same for B (the XYZZ operand of the adds).
template <int F> __global__ void k_exc_pairs(const u32 *pts, const u32 *lam, const int *mode, u32 *out, int n) {
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) / kGroup;
    if (i >= n) return;
    affine<F> P[7];
    for (int j = 0; j < 7; ++j) P[j] = aff_load<F>(pts + 16 * (7 * (size_t)i + j));
    const fe la = fe_load(lam + 16 * (size_t)i), lb = fe_load(lam + 16 * (size_t)i + 8);
    const bool formed_a = mode[i] & 1, formed_b = mode[i] & 2;
    xyzz<F> A = xc_rescaled<F>(P[0], la), B = xc_rescaled<F>(P[1], lb);
    xyzz9<F> A9 = xyzz9_from_r256<F>(A), B9 = xyzz9_from_r256<F>(B);
    if (formed_a) {
        A = xyzz_identity<F>(); xyzz_madd<F>(A, P[2]); xyzz_madd<F>(A, P[3]);
        A9 = xyzz9_identity<F>(); xyzz9_madd<F>(A9, aff9_from_r256<F>(P[2])); xyzz9_madd<F>(A9, aff9_from_r256<F>(P[3]));
    }
    if (formed_b) {
        B = xyzz_identity<F>(); xyzz_madd<F>(B, P[4]); xyzz_madd<F>(B, P[5]);
        B9 = xyzz9_identity<F>(); xyzz9_madd<F>(B9, aff9_from_r256<F>(P[4])); xyzz9_madd<F>(B9, aff9_from_r256<F>(P[5]));
    }
    const aff9<F> b9 = aff9_from_r256<F>(P[1]), c9 = aff9_from_r256<F>(P[6]);
    const bool b_id = aff_is_identity(P[1]);
    u32 *o = out + 16 * (size_t)XF_COUNT * i;
    { xyzz9<F> r = A9; xyzz9_madd<F>(r, b9); xc_store9<F>(o + 16 * XF_MADD9, r); }
    { xyzz9<F> r = A9; if (!b_id) xyzz9_madd<F, true>(r, b9); xc_store9<F>(o + 16 * XF_MADD9_HOT, r); }       // HOT: q != O
    { xyzz9<F> r = A9; xyzz9_add<F>(r, B9); xc_store9<F>(o + 16 * XF_ADD9, r); }
    { xyzz9<F> r = A9; xyzz9_add_wide<F>(r, B9); xc_store9<F>(o + 16 * XF_ADD9_WIDE, r); }
    xc_store9<F>(o + 16 * XF_DBL9_WIDE, xyzz9_dbl_wide<F>(A9));
    { xyzz<F> r = A; xyzz_madd<F>(r, P[1]); xc_store<F>(o + 16 * XF_MADD, r); }
    { xyzz<F> r = A; xyzz_madd_lazy<F>(r, P[1]); xyzz_reduce_lazy<F>(r); xc_store<F>(o + 16 * XF_MADD_LAZY, r); }
    { xyzz<F> r = A; xyzz_add<F>(r, B); xc_store<F>(o + 16 * XF_ADD, r); }
    { xyzz<F> r = A; xyzz_add_wide<F>(r, B); xc_store<F>(o + 16 * XF_ADD_WIDE, r); }
    { xyzz9<F> r = A9; if (!b_id) xyzz9_madd<F, true>(r, b9); xyzz9_madd<F, true>(r, c9); xc_store9<F>(o + 16 * XF_HOT_THEN, r); }
    { xyzz9<F> r = A9; xyzz9_madd<F>(r, b9); xyzz9_madd<F>(r, c9); xc_store9<F>(o + 16 * XF_MADD9_THEN, r); }
}

// one quad per chain: every chain form adds the same 64 points (pts, no identity) from the identity; the XYZZ operands are rescaled
// by lam[t].  out: per chain, step and form the affine running sum; bad[chain]: bit f set when form f broke an operand bound.
template <int F> __global__ void k_exc_chains(const u32 *pts, const u32 *lam, u32 *out, u32 *bad, int n) {
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) / kGroup;
    if (i >= n) return;
    xyzz9<F> a9[4] = {xyzz9_identity<F>(), xyzz9_identity<F>(), xyzz9_identity<F>(), xyzz9_identity<F>()};
    xyzz<F> a[4] = {xyzz_identity<F>(), xyzz_identity<F>(), xyzz_identity<F>(), xyzz_identity<F>()};
    u32 flags = 0;
    for (int t = 0; t < kChainSteps; ++t) {
        const affine<F> p = aff_load<F>(pts + 16 * ((size_t)i * kChainSteps + t));
        const xyzz<F> q = xc_rescaled<F>(p, fe_load(lam + 8 * ((size_t)i * kChainSteps + t)));
        const xyzz9<F> q9 = xyzz9_from_r256<F>(q);
        const aff9<F> p9 = aff9_from_r256<F>(p);
        for (int f = XC_MADD9_HOT; f <= XC_MADD9; ++f)
            if (!xyzz9_is_identity(a9[f]) && !xc_diff_ok(fe9_sub(fe9_mul<F>(p9.x, a9[f].zz), a9[f].x))) flags |= 1u << f;
        for (int f = XC_ADD9; f <= XC_ADD9_WIDE; ++f)
            if (!xyzz9_is_identity(a9[f]) && !xc_diff_ok(fe9_sub(fe9_mul<F>(q9.x, a9[f].zz), fe9_mul<F>(a9[f].x, q9.zz)))) flags |= 1u << f;
        xyzz9_madd<F, true>(a9[XC_MADD9_HOT], p9);
        xyzz9_madd<F>(a9[XC_MADD9], p9);
        xyzz9_add<F>(a9[XC_ADD9], q9);
        xyzz9_add_wide<F>(a9[XC_ADD9_WIDE], q9);
        xyzz_madd<F>(a[XC_MADD - XC_MADD], p);
        xyzz_madd_lazy<F>(a[XC_MADD_LAZY - XC_MADD], p);
        xyzz_add<F>(a[XC_ADD - XC_MADD], q);
        xyzz_add_wide<F>(a[XC_ADD_WIDE - XC_MADD], q);
        u32 *o = out + 16 * (size_t)XC_COUNT * ((size_t)i * kChainSteps + t);
        for (int f = 0; f < 4; ++f) {
            if (!xyzz9_is_identity(a9[f]) && !xc_acc_ok(a9[f])) flags |= 1u << f;
            xc_store9<F>(o + 16 * f, a9[f]);
        }
        xyzz<F> lz = a[XC_MADD_LAZY - XC_MADD];
        xyzz_reduce_lazy<F>(lz);
        xc_store<F>(o + 16 * XC_MADD, a[0]);
        xc_store<F>(o + 16 * XC_MADD_LAZY, lz);
        xc_store<F>(o + 16 * XC_ADD, a[2]);
        xc_store<F>(o + 16 * XC_ADD_WIDE, a[3]);
    }
    if ((threadIdx.x & (kGroup - 1)) == 0) bad[i] = flags;
}

// fe9_maybe_zero_mod_p / fe9_is_zero_mod_p on signed limb vectors (9 x i32 each)
template <int F> __global__ void k_exc_filter(const i32 *limbs, u32 *out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe9 a;
    for (int j = 0; j < 9; ++j) a.v[j] = limbs[9 * (size_t)i + j];
    out[2 * (size_t)i] = fe9_maybe_zero_mod_p(a) ? 1u : 0u;
    out[2 * (size_t)i + 1] = fe9_is_zero_mod_p<F>(a) ? 1u : 0u;
}

template <int F> int run_exceptional() {
    const int R = 8 * kChainSteps + 16;                        // table of c G for |c| <= R
    const uint64_t P[2][4] = {{0x992d30ed00000001ULL, 0x224698fc094cf91bULL, 0, 0x4000000000000000ULL},
                              {0x8c46eb2100000001ULL, 0x224698fc0994a8ddULL, 0, 0x4000000000000000ULL}};
    std::vector<uint64_t> T(8 * (size_t)(2 * R + 1));
    auto tab = [&](int c) { return &T[8 * (size_t)(c + R)]; };
    {
        uint64_t g[8] = {0}, jac[12], k[4] = {0, 0, 0, 0}, zero[4] = {0, 0, 0, 0};
        memcpy(g, P[F], 32); g[0] -= 1; g[4] = 2;              // G = (-1, 2)
        orc_to_mont(F, g, 2);
        for (int c = 0; c <= R; ++c) {
            k[0] = (uint64_t)c;
            orc_point_mul(F, jac, g, k);
            orc_point_to_affine(F, tab(c), jac);
            memcpy(tab(-c), tab(c), 64);
            if (c) orc_f_sub(F, tab(-c) + 4, zero, tab(c) + 4);
        }
    }
    uint64_t rng = 0x9e3779b97f4a7c15ULL ^ (uint64_t)F;
    auto rnd = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    int fails = 0;
    // ---- pairs: A = a G, B = b G for a, b in [-8, 8], every operand form
    {
        std::vector<int> ca, cb, md;
        for (int a = -8; a <= 8; ++a)
            for (int b = -8; b <= 8; ++b)
                for (int m = 0; m < 4; ++m) { ca.push_back(a); cb.push_back(b); md.push_back(m); }
        const int n = (int)ca.size();
        std::vector<uint64_t> pts(8 * 7 * (size_t)n), lam(8 * (size_t)n), got(8 * (size_t)XF_COUNT * n);
        orc_random_field(F, 901 + F, lam.data(), 2 * (size_t)n);
        for (int i = 0; i < n; ++i) {
            const int a = ca[i], b = cb[i], a1 = (int)(rnd() % 17) - 8, b1 = (int)(rnd() % 17) - 8;
            const int parts[7] = {a, b, a1, a - a1, b1, b - b1, 1};
            for (int j = 0; j < 7; ++j) memcpy(&pts[8 * (7 * (size_t)i + j)], tab(parts[j]), 64);
            if (!(lam[8 * i] | lam[8 * i + 1] | lam[8 * i + 2] | lam[8 * i + 3])) lam[8 * i] = 7;
            if (!(lam[8 * i + 4] | lam[8 * i + 5] | lam[8 * i + 6] | lam[8 * i + 7])) lam[8 * i + 4] = 7;
        }
        u32 *dp, *dl, *dout; int *dm;
        CK(hipMalloc(&dp, 8 * pts.size())); CK(hipMalloc(&dl, 8 * lam.size())); CK(hipMalloc(&dout, 8 * got.size()));
        CK(hipMalloc(&dm, sizeof(int) * n));
        CK(hipMemcpy(dp, pts.data(), 8 * pts.size(), hipMemcpyHostToDevice));
        CK(hipMemcpy(dl, lam.data(), 8 * lam.size(), hipMemcpyHostToDevice));
        CK(hipMemcpy(dm, md.data(), sizeof(int) * n, hipMemcpyHostToDevice));
        hipLaunchKernelGGL((k_exc_pairs<F>), dim3((n * kGroup + 255) / 256), dim3(256), 0, 0, dp, dl, dm, dout, n);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(got.data(), dout, 8 * got.size(), hipMemcpyDeviceToHost));
        const char *names[XF_COUNT] = {"madd9", "madd9 HOT", "add9", "add9 wide", "dbl9 wide", "madd", "madd lazy", "add", "add wide",
                                       "HOT after rare", "madd9 after rare"};
        for (int f = 0; f < XF_COUNT; ++f) {
            int bad = 0, cnt = 0;
            for (int i = 0; i < n; ++i) {
                if ((f == XF_MADD9_HOT || f == XF_HOT_THEN) && cb[i] == 0) continue;                  // HOT: q is never O
                const int want = f == XF_DBL9_WIDE ? 2 * ca[i] : ca[i] + cb[i] + (f >= XF_HOT_THEN ? 1 : 0);
                ++cnt;
                if (memcmp(tab(want), &got[8 * ((size_t)XF_COUNT * i + f)], 64)) {
                    if (!bad) printf("  first mismatch %s: %d G + %d G (operand mode %d)\n", names[f], ca[i], cb[i], md[i]);
                    bad++;
                }
            }
            printf("field %d exc %-16s: %d/%d mismatches\n", F, names[f], bad, cnt);
            fails += bad;
        }
        (void)hipFree(dp); (void)hipFree(dl); (void)hipFree(dout); (void)hipFree(dm);
    }
    // ---- 64-step palette chains: steps that double the running sum (c = S) or cancel it (c = -S) whenever |S| <= 8
    {
        const int n = 512;
        std::vector<int> c(n * kChainSteps), sum(n * kChainSteps);
        for (int i = 0; i < n; ++i) {
            int s = 0;
            for (int t = 0; t < kChainSteps; ++t) {
                const int pick = (int)(rnd() % 3);
                int v = (int)(rnd() % 16) - 8;
                v += v >= 0;                                                                        // [-8, 8] without 0
                if (s != 0 && s >= -8 && s <= 8 && pick) v = pick == 1 ? s : -s;
                c[i * kChainSteps + t] = v;
                s += v;
                sum[i * kChainSteps + t] = s;
            }
        }
        std::vector<uint64_t> pts(8 * (size_t)n * kChainSteps), lam(4 * (size_t)n * kChainSteps), got(8 * (size_t)XC_COUNT * n * kChainSteps);
        std::vector<u32> flags(n);
        for (size_t j = 0; j < c.size(); ++j) memcpy(&pts[8 * j], tab(c[j]), 64);
        orc_random_field(F, 911 + F, lam.data(), (size_t)n * kChainSteps);
        for (size_t j = 0; j < c.size(); ++j)
            if (!(lam[4 * j] | lam[4 * j + 1] | lam[4 * j + 2] | lam[4 * j + 3])) lam[4 * j] = 7;
        u32 *dp, *dl, *dout, *dbad;
        CK(hipMalloc(&dp, 8 * pts.size())); CK(hipMalloc(&dl, 8 * lam.size())); CK(hipMalloc(&dout, 8 * got.size()));
        CK(hipMalloc(&dbad, 4 * (size_t)n));
        CK(hipMemcpy(dp, pts.data(), 8 * pts.size(), hipMemcpyHostToDevice));
        CK(hipMemcpy(dl, lam.data(), 8 * lam.size(), hipMemcpyHostToDevice));
        hipLaunchKernelGGL((k_exc_chains<F>), dim3((n * kGroup + 255) / 256), dim3(256), 0, 0, dp, dl, dout, dbad, n);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(got.data(), dout, 8 * got.size(), hipMemcpyDeviceToHost));
        CK(hipMemcpy(flags.data(), dbad, 4 * (size_t)n, hipMemcpyDeviceToHost));
        const char *names[XC_COUNT] = {"madd9 HOT", "madd9", "add9", "add9 wide", "madd", "madd lazy", "add", "add wide"};
        int rare = 0;
        for (int i = 0; i < n; ++i)
            for (int t = 1; t < kChainSteps; ++t) {
                const int s = sum[i * kChainSteps + t - 1], v = c[i * kChainSteps + t];
                rare += s == v || s == -v;
            }
        for (int f = 0; f < XC_COUNT; ++f) {
            int bad = 0, oob = 0;
            for (int i = 0; i < n; ++i) {
                oob += (flags[i] >> f) & 1;
                for (int t = 0; t < kChainSteps; ++t)
                    if (memcmp(tab(sum[i * kChainSteps + t]), &got[8 * ((size_t)XC_COUNT * (i * kChainSteps + t) + f)], 64)) {
                        if (!bad) printf("  first chain mismatch %s: chain %d step %d\n", names[f], i, t);
                        bad++;
                        break;
                    }
            }
            printf("field %d exc chain %-10s: %d/%d chains wrong, %d out of operand bounds (%d equal / opposite steps)\n", F, names[f], bad, n, oob, rare);
            fails += bad + oob;
        }
        (void)hipFree(dp); (void)hipFree(dl); (void)hipFree(dout); (void)hipFree(dbad);
    }
    // ---- the filter: k p for |k| <= 16 in several limb layouts (limbs below 2^31), and near misses k p + d
    {
        i32 p9[9];
        for (int i = 0; i < 9; ++i) {                          // p in 29-bit limbs
            const int bit = 29 * i, w = bit >> 6, s = bit & 63;
            uint64_t v = P[F][w] >> s;
            if (s > 35 && w + 1 < 4) v |= P[F][w + 1] << (64 - s);
            p9[i] = (i32)(v & M29);
        }
        std::vector<i32> limbs;
        std::vector<int> ks, ds;
        for (int k = -16; k <= 16; ++k)
            for (int d : {0, 1, -1, 16, -16, 17, -17, 1 << 28})
                for (int layout = 0; layout < 5; ++layout) {
                    int64_t v[9], carry = 0;
                    for (int i = 0; i < 9; ++i) {
                        const int64_t t = (int64_t)k * p9[i] + (i == 0 ? d : 0) + carry;
                        if (i < 8) { v[i] = t & M29; carry = t >> 29; } else v[i] = t;
                    }
                    if (layout == 1) { v[0] -= 1 << 29; v[1] += 1; }
                    if (layout == 2) for (int i = 0; i < 8; ++i) { v[i] += 1 << 29; v[i + 1] -= 1; }
                    if (layout == 3) for (int i = 0; i < 8; i += 2) { v[i] -= 1 << 29; v[i + 1] += 1; }
                    if (layout == 4) { v[0] += 1 << 30; v[1] -= 2; }
                    for (int i = 0; i < 9; ++i) limbs.push_back((i32)v[i]);
                    ks.push_back(k);
                    ds.push_back(d);
                }
        const int n = (int)ks.size();
        std::vector<u32> got(2 * (size_t)n);
        i32 *dl; u32 *dout;
        CK(hipMalloc(&dl, 4 * limbs.size())); CK(hipMalloc(&dout, 4 * got.size()));
        CK(hipMemcpy(dl, limbs.data(), 4 * limbs.size(), hipMemcpyHostToDevice));
        hipLaunchKernelGGL((k_exc_filter<F>), dim3((n + 255) / 256), dim3(256), 0, 0, dl, dout, n);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(got.data(), dout, 4 * got.size(), hipMemcpyDeviceToHost));
        int bad = 0;
        for (int i = 0; i < n; ++i) {
            // the independent checks are the d = 0 rows (k p must pass the filter) and the full test on every row; for d != 0 the
            // filter's expectation below restates its own formula (a near miss may pass the cheap filter, never the full test)
            const int64_t low = ks[i] + ds[i];                 // the value mod 2^29 (p = 1 mod 2^29)
            const u32 maybe = (u32)(((uint64_t)(low + 16) & M29) <= 32u);
            const bool full_ok = ks[i] >= -15 && ks[i] <= 15;  // fe9_is_zero_mod_p wants |value| < 2^258
            if (got[2 * i] != maybe || (full_ok && got[2 * i + 1] != (u32)(ds[i] == 0))) {
                if (!bad) printf("  first filter mismatch: k %d, d %d (maybe %u, zero %u)\n", ks[i], ds[i], got[2 * i], got[2 * i + 1]);
                bad++;
            }
        }
        printf("field %d exc %-16s: %d/%d mismatches\n", F, "zero filter", bad, n);
        fails += bad;
        (void)hipFree(dl); (void)hipFree(dout);
    }
    return fails;
}

template <int F> int run_field() {
    const int n = 1 << 14;
    std::vector<uint64_t> a(4 * n), b(4 * n), want(4 * n), got(4 * n);
    orc_random_field(F, 11 + F, a.data(), n);
    orc_random_field(F, 23 + F, b.data(), n);
    // edge cases: 0, 1 (canonical one, not Montgomery), p-1, equal operands
    const uint64_t P[2][4] = {{0x992d30ed00000001ULL, 0x224698fc094cf91bULL, 0, 0x4000000000000000ULL},
                              {0x8c46eb2100000001ULL, 0x224698fc0994a8ddULL, 0, 0x4000000000000000ULL}};
    memset(&a[0], 0, 32);
    memset(&a[4], 0, 32); a[4] = 1;
    memcpy(&a[8], P[F], 32); a[8] -= 1;
    memcpy(&b[8], P[F], 32); b[8] -= 1;
    memcpy(&a[12], &b[12], 32);
    memcpy(&b[16], P[F], 32); b[16] -= 1; memset(&a[16], 0, 32); a[16] = 1;
    u32 *da, *db, *dout;
    CK(hipMalloc(&da, 32 * n)); CK(hipMalloc(&db, 32 * n)); CK(hipMalloc(&dout, 32 * n));
    CK(hipMemcpy(da, a.data(), 32 * n, hipMemcpyHostToDevice));
    CK(hipMemcpy(db, b.data(), 32 * n, hipMemcpyHostToDevice));
    const char *names[] = {"mul_c", "mul_col", "mul_asm", "add", "sub", "inv", "mul_blk", "mul_sched"};
    int fails = 0;
    for (int op = 0; op < 8; ++op) {
        int cnt = op == 5 ? 256 : n;
        hipLaunchKernelGGL((k_ops<F>), dim3((cnt + 255) / 256), dim3(256), 0, 0, da, db, dout, cnt, op);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(got.data(), dout, 32 * cnt, hipMemcpyDeviceToHost));
        int bad = 0;
        for (int i = 0; i < cnt; ++i) {
            uint64_t w[4];
            if (op <= 2 || op >= 6) orc_f_mul(F, w, &a[4 * i], &b[4 * i]);
            else if (op == 3) orc_f_add(F, w, &a[4 * i], &b[4 * i]);
            else if (op == 4) orc_f_sub(F, w, &a[4 * i], &b[4 * i]);
            else orc_f_inv(F, w, &a[4 * i]);
            if (memcmp(w, &got[4 * i], 32)) { if (!bad) printf("  first mismatch op %s idx %d\n", names[op], i); bad++; }
        }
        printf("field %d %-8s: %d/%d mismatches\n", F, names[op], bad, cnt);
        fails += bad;
    }
    // lazy arithmetic against the canonical oracle results, every pair of representatives
    for (int mode = 0; mode < 4; ++mode)
        for (int ka = 0; ka < 3; ++ka)
            for (int kb = 0; kb < 3; ++kb) {
                hipLaunchKernelGGL((k_lazy<F>), dim3((n + 255) / 256), dim3(256), 0, 0, da, db, dout, n, mode, ka, kb);
                CK(hipDeviceSynchronize());
                CK(hipMemcpy(got.data(), dout, 32 * n, hipMemcpyDeviceToHost));
                int bad = 0;
                for (int i = 0; i < n; ++i) {
                    uint64_t w[4] = {0, 0, 0, 0};
                    if (mode == 0) orc_f_mul(F, w, &a[4 * i], &b[4 * i]);
                    else if (mode == 1) orc_f_sub(F, w, &a[4 * i], &b[4 * i]);
                    else if (mode == 2) w[0] = memcmp(&a[4 * i], &b[4 * i], 32) == 0;
                    if (memcmp(w, &got[4 * i], 32)) { if (!bad) printf("  first lazy mismatch mode %d reps (%d, %d) idx %d\n", mode, ka, kb, i); bad++; }
                }
                if (bad) printf("field %d lazy mode %d reps (%d, %d): %d/%d mismatches\n", F, mode, ka, kb, bad, n);
                fails += bad;
            }
    printf("field %d lazy mul / sub / zero-test / 300-step chain over 9 representative pairs: done\n", F);
    fails += run_field9<F>(a, b, da, db, dout, n);
    fails += run_wide9<F>(da, db, n);
    fails += run_exceptional<F>();
    CK(hipFree(da)); CK(hipFree(db)); CK(hipFree(dout));
    return fails;
}

template <int IMPL> int bench(const char *name, int blocks_per_cu) {
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    int blocks = prop.multiProcessorCount * blocks_per_cu;
    std::vector<uint64_t> a(4 * 1024);
    orc_random_field(0, 5, a.data(), 1024);
    u32 *da, *dout;
    CK(hipMalloc(&da, 32 * 1024)); CK(hipMalloc(&dout, (size_t)32 * blocks * 256));
    CK(hipMemcpy(da, a.data(), 32 * 1024, hipMemcpyHostToDevice));
    const int iters = 2000;
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    hipLaunchKernelGGL((k_chain<FP, IMPL>), dim3(blocks), dim3(256), 0, 0, da, dout, 10);
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0));
    hipLaunchKernelGGL((k_chain<FP, IMPL>), dim3(blocks), dim3(256), 0, 0, da, dout, iters);
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    double muls = (double)blocks * 256 * iters * 2;
    printf("%-8s waves/SIMD %d: %8.3f ms  %8.2f G modmul/s\n", name, blocks_per_cu, ms, muls / (ms * 1e-3) / 1e9);
    CK(hipFree(da)); CK(hipFree(dout));
    return 0;
}

int main() {
    int fails = run_field<FP>() + run_field<FQ>();
    for (int w : {1, 2, 4, 8}) {
        bench<1>("mul_col", w); bench<3>("mul_blk", w); bench<4>("mul_sched", w);
    }
    printf(fails ? "FIELD CHECK FAILED\n" : "FIELD CHECK OK\n");
    return fails ? 1 : 0;
}
