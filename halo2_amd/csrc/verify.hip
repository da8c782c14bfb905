// The verifier's one data-parallel vector: the challenge products of `Guard::use_challenges` (poly/commitment/verifier.rs:35-41,
// compute_s :156-172), summed over a batch of proofs with one coefficient each -- the g part of the accumulated MSM of
// `BatchVerifier` (plonk/verifier/batch.rs:79-127), and with batch = 1, coefficient 1 the s vector of `Guard::compute_g`.
//
//   out[j] (+)= sum_b coeffs[b] * prod_{i : bit i of j set} u_b[k-1-i],   0 <= j < 2^k
//
// One lane owns 2^kSBits consecutive indices; a workgroup of 256 lanes 2^(kSBits+8).  Per proof b the index bits split three ways:
//   bits >= kSBits+8  shared by the workgroup: coeffs[b] times their challenges, once per workgroup and proof (wpre);
//   bits kSBits..+7   the lane id: two 16-entry tables in LDS, one per nibble (the high one carries wpre), so the lane's prefix is
//                     ONE product H[lane >> 4] * A[lane & 15];
//   bits 0..kSBits-1  the lane's own 2^kSBits outputs, expanded from the prefix by doubling (2^kSBits - 1 products).
// So a lane pays 2^kSBits products and additions per proof for its 2^kSBits outputs -- one product per output, where the products
// of the definition cost k/2.  Challenges and coefficients come through LDS in chunks of kSChunk proofs, so any batch is one
// launch; the accumulators stay in VGPRs across the whole batch and every output is written once.
//
// Form: the challenges are uploaded in Montgomery form; a Montgomery product with them keeps the form of the other factor, so the
// coefficients (host-reduced, left in the caller's form) carry their form through to the output and `accumulate` is a plain add.
#include <vector>

#include "common.h"
#include "field.cuh"
#include "host_field.h"

namespace h2 {

static constexpr u32 kSBits = 3;                // indices per lane: 2^kSBits
static constexpr u32 kSLanes = 256;
static constexpr u32 kSChunk = 32;              // proofs per LDS chunk
static constexpr u32 kSEnt = 32 + kSBits;       // per proof: A[16], H[16], the kSBits low-bit challenges

template <int F>
__global__ void __launch_bounds__(256) s_combine(const u32 *__restrict__ ch, const u32 *__restrict__ coeff, u32 k, u32 batch,
                                                 u32 accumulate, u32 *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) u32 tab[kSChunk * kSEnt * 8];
    __shared__ __attribute__((aligned(16))) u32 wpre[kSChunk * 8];
    const u32 lane = threadIdx.x;
    const u32 wg = blockIdx.x;
    fe acc[1 << kSBits];
#pragma unroll
    for (u32 e = 0; e < (1u << kSBits); ++e) acc[e] = fe_zero();
    for (u32 c0 = 0; c0 < batch; c0 += kSChunk) {
        const u32 nc = batch - c0 < kSChunk ? batch - c0 : kSChunk;
        __syncthreads();                                   // the previous chunk's tables are read
        if (lane < nc) {                                   // the workgroup's prefix: coeff * challenges of index bits >= kSBits + 8
            const u32 b = c0 + lane;
            const u32 *u = ch + 8 * (size_t)b * k;
            fe w = fe_load(coeff + 8 * (size_t)b);
            for (u32 i = kSBits + 8; i < k; ++i)
                if ((wg >> (i - kSBits - 8)) & 1) w = fe_mulx<F>(w, fe_load(u + 8 * (k - 1 - i)));
            fe_store(wpre + 8 * lane, w);
        }
        __syncthreads();
        for (u32 task = lane; task < nc * kSEnt; task += kSLanes) {
            const u32 p = task / kSEnt, e = task % kSEnt;
            const u32 *u = ch + 8 * (size_t)(c0 + p) * k;
            fe v;
            if (e < 32) {                                  // A[e] (lane bits 0..3) or H[e - 16] (lane bits 4..7, times the prefix)
                const u32 first = kSBits + (e < 16 ? 0 : 4);
                v = e < 16 ? fe_one<F>() : fe_load(wpre + 8 * p);
                for (u32 m = 0; m < 4; ++m) {
                    const u32 i = first + m;               // index bits at or above k never occur in a stored output
                    if (((e >> m) & 1) && i < k) v = fe_mulx<F>(v, fe_load(u + 8 * (k - 1 - i)));
                }
            } else {
                const u32 i = e - 32;
                v = i < k ? fe_load(u + 8 * (k - 1 - i)) : fe_one<F>();
            }
            fe_store(tab + 8 * task, v);
        }
        __syncthreads();
        for (u32 p = 0; p < nc; ++p) {
            const u32 *t = tab + 8 * p * kSEnt;
            const fe mid = fe_mulx<F>(fe_load(t + 8 * (16 + (lane >> 4))), fe_load(t + 8 * (lane & 15)));
            const fe u0 = fe_load(t + 8 * 32), u1 = fe_load(t + 8 * 33), u2 = fe_load(t + 8 * 34);    // index bits 0, 1, 2
            const fe p4 = fe_mulx<F>(mid, u2), p2 = fe_mulx<F>(mid, u1);
            const fe p6 = fe_mulx<F>(p4, u1);
            acc[0] = fe_add<F>(acc[0], mid);
            acc[1] = fe_add<F>(acc[1], fe_mulx<F>(mid, u0));
            acc[2] = fe_add<F>(acc[2], p2);
            acc[3] = fe_add<F>(acc[3], fe_mulx<F>(p2, u0));
            acc[4] = fe_add<F>(acc[4], p4);
            acc[5] = fe_add<F>(acc[5], fe_mulx<F>(p4, u0));
            acc[6] = fe_add<F>(acc[6], p6);
            acc[7] = fe_add<F>(acc[7], fe_mulx<F>(p6, u0));
        }
    }
    static_assert(kSBits == 3, "the expansion above is written out for 8 outputs per lane");
    const u32 base = (wg * kSLanes + lane) << kSBits;
#pragma unroll
    for (u32 e = 0; e < (1u << kSBits); ++e) {
        const u32 j = base + e;
        if (j >> k) continue;
        u32 *o = out + 8 * (size_t)j;
        fe_store(o, accumulate ? fe_add<F>(fe_load(o), acc[e]) : acc[e]);
    }
}

struct VerifyContext {
    std::mutex mu;
    DevBuf stage;
    void release_all() { stage.release(); }
};
static StreamContexts<VerifyContext> g_verify_ctxs;
void verify_release_workspaces() { g_verify_ctxs.release_current_device(); }   // h2_trim

static bool s_combine_args_ok(int field, unsigned k, size_t batch, const uint64_t *challenges, const uint64_t *coeffs, int form,
                              int accumulate, const void *out) {
    return (field == H2_FP || field == H2_FQ) && (form == H2_FORM_CANONICAL || form == H2_FORM_MONTGOMERY) && k >= 1 && k <= 30 &&
           batch >= 1 && batch <= (1u << 24) && challenges && coeffs && out && (accumulate == 0 || accumulate == 1);
}

static int s_combine_launch(int field, unsigned k, size_t batch, const u64 *challenges, const u64 *coeffs, int form, int accumulate,
                            void *d_out, hipStream_t st) {
    // challenges -> Montgomery; coefficients reduced and left in the caller's form (see the header of this file)
    std::vector<u64> host(4 * batch * ((size_t)k + 1));
    u64 *hc = host.data(), *hk = hc + 4 * batch * k;
    for (size_t i = 0; i < batch * k; ++i) host_to_mont(field, hc + 4 * i, challenges + 4 * i, form);
    for (size_t b = 0; b < batch; ++b) {
        u64 m[4];
        host_to_mont(field, m, coeffs + 4 * b, form);
        if (form == H2_FORM_CANONICAL) host_from_mont(field, hk + 4 * b, m);
        else memcpy(hk + 4 * b, m, 32);
    }
    VerifyContext &cx = g_verify_ctxs.get(st);
    std::lock_guard<std::mutex> lk(cx.mu);
    int rc = cx.stage.reserve(host.size() * 8);
    if (rc != H2_OK) return rc;
    // stream-ordered after the previous launch that read the staging buffer; the pageable source is consumed when the call returns
    H2_HIP(hipMemcpyAsync(cx.stage.ptr, hc, host.size() * 8, hipMemcpyHostToDevice, st));
    const u32 *d_ch = cx.stage.as<u32>(), *d_co = d_ch + 8 * batch * k;
    const size_t per_wg = (size_t)kSLanes << kSBits;
    dim3 grid((unsigned)((((size_t)1 << k) + per_wg - 1) / per_wg)), block(kSLanes);
    if (field == H2_FP) hipLaunchKernelGGL((s_combine<FP>), grid, block, 0, st, d_ch, d_co, (u32)k, (u32)batch, (u32)accumulate, (u32 *)d_out);
    else hipLaunchKernelGGL((s_combine<FQ>), grid, block, 0, st, d_ch, d_co, (u32)k, (u32)batch, (u32)accumulate, (u32 *)d_out);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

}  // namespace h2

using namespace h2;

extern "C" int h2_ipa_s_combine_device(int field, unsigned k, size_t batch, const uint64_t *challenges, const uint64_t *coeffs, int form,
                                       int accumulate, void *d_out, void *stream) {
    if (!s_combine_args_ok(field, k, batch, challenges, coeffs, form, accumulate, d_out)) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    return s_combine_launch(field, k, batch, challenges, coeffs, form, accumulate, d_out, (hipStream_t)stream);
}

extern "C" int h2_ipa_s_combine(int field, unsigned k, size_t batch, const uint64_t *challenges, const uint64_t *coeffs, int form,
                                int accumulate, uint64_t *out) {
    if (!s_combine_args_ok(field, k, batch, challenges, coeffs, form, accumulate, out)) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    const size_t bytes = (size_t)32 << k;
    void *d = nullptr;
    H2_HIP(hipMalloc(&d, bytes));
    hipError_t e = accumulate ? hipMemcpy(d, out, bytes, hipMemcpyHostToDevice) : hipSuccess;
    if (e == hipSuccess) {
        rc = s_combine_launch(field, k, batch, challenges, coeffs, form, accumulate, d, 0);
        if (rc == H2_OK) e = hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost);
    }
    (void)hipFree(d);
    if (e != hipSuccess) { set_last_hip_error(e, __FILE__, __LINE__); return H2_ERR_HIP; }
    return rc;
}
