// Radix-2 NTT over the Pasta fields on gfx950: the host side -- twiddle cache, pass dispatch, ntt_run and the C entry points.
//
// Replaces the body of `best_fft` (halo2_proofs/src/arithmetic.rs:192-295) and the EvaluationDomain wrappers around it
// (poly/domain.rs:227-255, :303-325, :357-383).  The reference bit-reverses, builds a twiddle table omega^0..omega^(n/2-1) and runs
// log n decimation-in-time butterfly stages (recursively).  This implementation keeps EXACTLY that butterfly network (same pairs, same
// twiddle omega^(i * n/m) per pair), so outputs agree element for element for any omega -- but executes it as a few HBM passes of up to
// 10 stages each: the plan is ntt_plan.h, the kernels are ntt_pass.cuh, the design and its measurements DESIGN.md section 5.
#include <cstdlib>
#include <cstring>
#include <list>
#include <map>
#include <memory>
#include <vector>

#include "ntt_pass.cuh"
#include "host_field.h"

namespace h2 {

static feparam to_param(const u64 a[4]) {
    feparam p;
    memcpy(p.v, a, 32);
    return p;
}

// ---- host: twiddle cache ---------------------------------------------------------------------------
struct TwKey {
    int dev, field, L;
    int flavour;     // 0: omega^e in the reference's Montgomery form, 32 B each (also read by the curve-point FFT); 1: M9 raw limbs, 36 B
    u64 w[4];
    bool operator==(const TwKey &o) const {
        return dev == o.dev && field == o.field && L == o.L && flavour == o.flavour && memcmp(w, o.w, 32) == 0;
    }
    bool operator<(const TwKey &o) const {
        if (dev != o.dev) return dev < o.dev;
        if (field != o.field) return field < o.field;
        if (L != o.L) return L < o.L;
        if (flavour != o.flavour) return flavour < o.flavour;
        return memcmp(w, o.w, 32) < 0;
    }
};
struct TwEntry {
    void *d = nullptr;
    hipEvent_t ready = nullptr;
    ~TwEntry() {
        if (d) (void)hipFree(d);
        if (ready) (void)hipEventDestroy(ready);
    }
};
struct NttContext {
    std::mutex mu;
    std::map<TwKey, std::shared_ptr<TwEntry>> cache;
    std::list<TwKey> lru;
    size_t cache_bytes = 0;
    std::map<std::pair<int, hipStream_t>, DevBuf> tmp, stage;
    bool lds_raised[16][2][2][2][12] = {};   // a pass kernel's dynamic-LDS cap is raised once per (device, family, field, first, r)
};
static NttContext &ntt_ctx() {
    static NttContext c;
    return c;
}
static const size_t kTwCacheBytes = (size_t)6 << 30;  // HBM is 288 GB: keep tables around
void ntt_release_workspaces() {   // h2_trim: scratch vectors and cached twiddle tables (rebuilt on the next transform)
    NttContext &cx = ntt_ctx();
    std::lock_guard<std::mutex> lk(cx.mu);
    for (auto &kv : cx.tmp) kv.second.release();
    for (auto &kv : cx.stage) kv.second.release();
    cx.cache.clear();
    cx.lru.clear();
    cx.cache_bytes = 0;
}

// omega^e for e < n / 2: 32 B each, or (M9 flavour) stage-major, 2^L - 1 entries of 36 B = 72 B per omega^e
static size_t tw_count(int L) { return L >= 1 ? ((size_t)1 << (L - 1)) : 1; }
static size_t tw_bytes(int L, int flavour) { return tw_count(L) * (flavour ? 72 : 32); }
static Tw9 tw9_planes(const void *d, int L) {   // the three planes of an M9 table: limbs 0-3 | 4-7 | 8
    const uint4 *a = (const uint4 *)d, *b = a + 2 * tw_count(L);
    return Tw9{a, b, (const u32 *)(b + 2 * tw_count(L))};
}

// returns the device table omega^0..omega^(n/2-1); builds it on `st` when missing
static int get_twiddles(NttContext &cx, int field, int L, const u64 omega_m[4], hipStream_t st, std::shared_ptr<TwEntry> &out,
                        int flavour = 0) {
    TwKey key;
    (void)hipGetDevice(&key.dev);
    key.field = field;
    key.L = L;
    key.flavour = flavour;
    memcpy(key.w, omega_m, 32);
    auto it = cx.cache.find(key);
    if (it != cx.cache.end()) {
        cx.lru.remove(key);
        cx.lru.push_front(key);
        out = it->second;
        // order this stream behind the build
        H2_HIP(hipStreamWaitEvent(st, out->ready, 0));
        debug_count(DBG_TWIDDLE_HITS);
        return H2_OK;
    }
    const size_t count = tw_count(L);
    auto ent = std::make_shared<TwEntry>();
    H2_HIP(hipMalloc(&ent->d, tw_bytes(L, flavour)));
    H2_HIP(hipEventCreateWithFlags(&ent->ready, hipEventDisableTiming));
    u32 T = (u32)std::min<size_t>(count, 1u << 16);
    u64 step[4];
    memcpy(step, omega_m, 32);
    for (u32 s = 1; s < T; s <<= 1) host_mul(field, step, step, step);  // omega^T, T a power of two
    dim3 grid((T + 255) / 256), block(256);
    if (flavour) {
        const Tw9 t9 = tw9_planes(ent->d, L);
        uint4 *pa = (uint4 *)t9.a, *pb = (uint4 *)t9.b;
        u32 *pc = (u32 *)t9.c;
        if (field == H2_FP) hipLaunchKernelGGL((ntt_twiddles9<FP>), grid, block, 0, st, pa, pb, pc, to_param(omega_m), to_param(step), T, count, L);
        else hipLaunchKernelGGL((ntt_twiddles9<FQ>), grid, block, 0, st, pa, pb, pc, to_param(omega_m), to_param(step), T, count, L);
    } else if (field == H2_FP)
        hipLaunchKernelGGL((ntt_twiddles<FP>), grid, block, 0, st, (u32 *)ent->d, to_param(omega_m), to_param(step), T, count);
    else
        hipLaunchKernelGGL((ntt_twiddles<FQ>), grid, block, 0, st, (u32 *)ent->d, to_param(omega_m), to_param(step), T, count);
    H2_HIP(hipGetLastError());
    H2_HIP(hipEventRecord(ent->ready, st));
    cx.cache[key] = ent;
    cx.lru.push_front(key);
    debug_count(DBG_TWIDDLE_BUILT);
    cx.cache_bytes += tw_bytes(L, flavour);
    while (cx.cache_bytes > kTwCacheBytes && cx.lru.size() > 1) {
        TwKey old = cx.lru.back();
        cx.lru.pop_back();
        auto o = cx.cache.find(old);
        if (o != cx.cache.end()) {
            // entries still referenced by in-flight work stay alive through the shared_ptr held by the caller
            H2_HIP(hipEventSynchronize(o->second->ready));
            H2_HIP(hipDeviceSynchronize());
            cx.cache_bytes -= tw_bytes(old.L, old.flavour);
            cx.cache.erase(o);
        }
    }
    out = ent;
    return H2_OK;
}

int ntt_twiddle_table(int field, int L, const uint64_t omega_mont[4], hipStream_t st, const uint32_t **d_tw) {
    NttContext &cx = ntt_ctx();
    std::lock_guard<std::mutex> lk(cx.mu);
    std::shared_ptr<TwEntry> tw;
    int rc = get_twiddles(cx, field, L, omega_mont, st, tw);
    if (rc != H2_OK) return rc;
    *d_tw = (const uint32_t *)tw->d;   // stays alive in the cache (evicted only beyond 6 GiB of tables)
    return H2_OK;
}

// ---- host: switches, dispatch, ntt_run ---------------------------------------------------------------
// The laboratory's switches, read once per process (ab_env: a constant null in the product, where the defaults hold): H2_NTT_FE9=0
// runs the 8 x 32 kernel at every size, H2_NTT_MAXR / _LOGT / _LOGT_FIRST / _LDS are the plan's knobs.
struct NttSwitches { bool fe9; NttKnobs knobs; };
static NttSwitches ntt_read_switches() {
    auto in_range = [](const char *e, int lo, int hi, int dflt) { const int v = e ? atoi(e) : dflt; return v >= lo && v <= hi ? v : dflt; };
    NttSwitches s;
    const char *e = ab_env("H2_NTT_FE9");
    s.fe9 = !(e && atoi(e) == 0);
    s.knobs.maxr = in_range(ab_env("H2_NTT_MAXR"), 1, 12, 10);
    s.knobs.logT = in_range(ab_env("H2_NTT_LOGT"), 0, 5, 3);
    s.knobs.logT_first = in_range(ab_env("H2_NTT_LOGT_FIRST"), 0, 5, -1);
    s.knobs.lds = (u32)in_range(ab_env("H2_NTT_LDS"), 32768, 131072, 131072);
    return s;
}

// the pass kernels by [field][first][r - 1]: R is a compile-time parameter, 2 x 2 x 12 instantiations per family
using PassFn = void (*)(const u32 *, u32 *, const u32 *, PassArgs);
using Pass9Fn = void (*)(const u32 *, u32 *, Tw9, PassArgs);
#define NTT_PASS_ROW(K, F, FIRST)                                                                                                   \
    {K<F, 1, FIRST>, K<F, 2, FIRST>, K<F, 3, FIRST>, K<F, 4, FIRST>, K<F, 5, FIRST>, K<F, 6, FIRST>, K<F, 7, FIRST>, K<F, 8, FIRST>, \
     K<F, 9, FIRST>, K<F, 10, FIRST>, K<F, 11, FIRST>, K<F, 12, FIRST>}
#define NTT_PASS_TABLE(K) {{NTT_PASS_ROW(K, FP, false), NTT_PASS_ROW(K, FP, true)}, {NTT_PASS_ROW(K, FQ, false), NTT_PASS_ROW(K, FQ, true)}}
static const PassFn kPass[2][2][12] = NTT_PASS_TABLE(ntt_pass);
static const Pass9Fn kPass9[2][2][12] = NTT_PASS_TABLE(ntt_pass9);

// callers hold cx.mu
static int enqueue_pass(NttContext &cx, int field, const NttPlan &P, const NttPassPlan &pp, const PassArgs &A, hipStream_t st,
                        const u32 *src, u32 *dst, const void *tw) {
    const PassFn fn = kPass[field][pp.first][pp.r - 1];
    const Pass9Fn fn9 = kPass9[field][pp.first][pp.r - 1];
    int dev = 0;
    (void)hipGetDevice(&dev);
    bool &raised = cx.lds_raised[dev & 15][P.use_fe9][field][pp.first][pp.r - 1];     // per DEVICE (the attribute is): a process driving several GPUs sets it on each
    if (!raised) {
        H2_HIP(hipFuncSetAttribute(P.use_fe9 ? (const void *)fn9 : (const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   P.use_fe9 ? (int)kNttLds9Max : 131072));
        raised = true;
    }
    if (P.use_fe9) hipLaunchKernelGGL(fn9, dim3(pp.tiles), dim3(pp.threads), pp.lds9, st, src, dst, tw9_planes(tw, A.L), A);
    else hipLaunchKernelGGL(fn, dim3(pp.tiles), dim3(pp.threads), pp.lds, st, src, dst, (const u32 *)tw, A);
    return H2_OK;
}

struct NttJob {
    int field;
    unsigned L;
    const void *d_in;   // first-pass source (n_in valid elements)
    void *d_out;        // final destination (2^L elements)
    size_t n_in;
    int load_mode, store_mode;
    u64 omega[4];       // Montgomery
    u64 lk0[4], lk1[4];           // load multipliers (Montgomery)
    u64 sk0[4], sk1[4], sk2[4];   // store multipliers (Montgomery)
    int plan = 0;                 // 0: fewest passes (one transform owns the chip); 1: small tiles, for concurrent transforms
};

// The first pass is out of place (its store is a transposition), later passes run in place and the last one lands in d_out: between
// the passes the vector is d_out itself, or for an in-place call the scratch vector.  (A single workgroup owns all of a one-pass vector.)
static void pass_buffers(const NttPassPlan &pp, const NttPlan &P, const NttJob &J, void *tmp, const void *&src, void *&dst) {
    void *between = P.needs_scratch ? tmp : J.d_out;
    src = pp.first ? J.d_in : between;
    dst = pp.last ? J.d_out : between;
}

static int ntt_run(const NttJob &J, hipStream_t st) {
    NttContext &cx = ntt_ctx();
    std::lock_guard<std::mutex> lk(cx.mu);
    const int L = (int)J.L;
    if (L == 0) {
        if (J.d_in != J.d_out) H2_HIP(hipMemcpyAsync(J.d_out, J.d_in, 32, hipMemcpyDeviceToDevice, st));
        if (J.store_mode) {
            if (J.field == H2_FP) hipLaunchKernelGGL((ntt_scale1<FP>), dim3(1), dim3(64), 0, st, (u32 *)J.d_out, to_param(J.sk0));
            else hipLaunchKernelGGL((ntt_scale1<FQ>), dim3(1), dim3(64), 0, st, (u32 *)J.d_out, to_param(J.sk0));
        }
        return H2_OK;
    }
    static const NttSwitches sw = ntt_read_switches();
    NttPlan P;
    int rc = ntt_plan(L, J.plan, J.d_in == J.d_out, sw.fe9, sw.knobs, &P);
    if (rc != H2_OK) return rc;
    std::shared_ptr<TwEntry> tw;
    if ((rc = get_twiddles(cx, J.field, L, J.omega, st, tw, P.use_fe9 ? 1 : 0)) != H2_OK) return rc;
    void *tmp = nullptr;
    if (P.needs_scratch) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        DevBuf &tb = cx.tmp[std::make_pair(dev, st)];
        if ((rc = tb.reserve((size_t)32 << L)) != H2_OK) return rc;
        tmp = tb.ptr;
    }
    for (int i = 0; i < P.passes; ++i) {
        const NttPassPlan &pp = P.pass[i];
        PassArgs A;
        memset(&A, 0, sizeof A);
        A.L = L; A.s0 = pp.s0; A.r = pp.r; A.logT = pp.logT;
        A.first = pp.first; A.last = pp.last; A.n_in = J.n_in;
        if (pp.first) {
            A.load_mode = J.load_mode;
            A.lk0 = to_param(J.lk0);
            A.lk1 = to_param(J.lk1);
        }
        if (pp.last) {
            A.store_mode = J.store_mode;
            A.k0 = to_param(J.sk0);
            A.k1 = to_param(J.sk1);
            A.k2 = to_param(J.sk2);
        }
        const void *src;
        void *dst;
        pass_buffers(pp, P, J, tmp, src, dst);
        prof_begin(PROF_NTT_PASS, st);
        if ((rc = enqueue_pass(cx, J.field, P, pp, A, st, (const u32 *)src, (u32 *)dst, tw->d)) != H2_OK) return rc;
        prof_end(PROF_NTT_PASS, st);
    }
    H2_HIP(hipGetLastError());
    return H2_OK;
}

static bool bad_field(int field, int form) {
    return (field != H2_FP && field != H2_FQ) || (form != H2_FORM_CANONICAL && form != H2_FORM_MONTGOMERY);
}

static int job_ntt(NttJob &J, int field, void *d_a, unsigned log_n, const u64 *omega, int form) {
    memset(&J, 0, sizeof J);
    J.field = field;
    J.L = log_n;
    J.d_in = d_a;
    J.d_out = d_a;
    J.n_in = (size_t)1 << log_n;
    host_to_mont(field, J.omega, omega, form);
    return H2_OK;
}

}  // namespace h2

using namespace h2;

extern "C" int h2_ntt_device(int field, void *d_a, unsigned log_n, const uint64_t *omega, int form, void *stream) {
    if (bad_field(field, form) || !d_a || !omega || log_n > 32) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    NttJob J;
    job_ntt(J, field, d_a, log_n, omega, form);
    return ntt_run(J, (hipStream_t)stream);
}

extern "C" int h2_ifft_device(int field, void *d_a, unsigned log_n, const uint64_t *omega_inv, const uint64_t *divisor,
                              int form, void *stream) {
    if (bad_field(field, form) || !d_a || !omega_inv || !divisor || log_n > 32) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    NttJob J;
    job_ntt(J, field, d_a, log_n, omega_inv, form);
    J.store_mode = 1;
    host_to_mont(field, J.sk0, divisor, form);
    return ntt_run(J, (hipStream_t)stream);
}

// ---- independent column transforms in one call (plonk/prover.rs:111-117, 322-327): forked over internal streams with the
// small-tile plan so that they share the chip, joined on the caller's stream
namespace {
struct NttBatchStreams {
    std::mutex mu;
    std::vector<hipStream_t> s;
    std::vector<hipEvent_t> done;
    hipEvent_t fork = nullptr;
};
NttBatchStreams &ntt_batch_streams() {
    static NttBatchStreams b[16];
    int dev = 0;
    (void)hipGetDevice(&dev);
    return b[dev & 15];
}
int ntt_batch(int field, void *const *d_a, size_t count, unsigned log_n, const uint64_t *omega, const uint64_t *divisor, int form,
              hipStream_t user) {
    NttBatchStreams &bs = ntt_batch_streams();
    std::lock_guard<std::mutex> lk(bs.mu);
    const size_t want = std::min<size_t>(3, count);
    while (bs.s.size() < want) {
        hipStream_t st;
        hipEvent_t ev;
        H2_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        H2_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        bs.s.push_back(st);
        bs.done.push_back(ev);
    }
    if (!bs.fork) H2_HIP(hipEventCreateWithFlags(&bs.fork, hipEventDisableTiming));
    H2_HIP(hipEventRecord(bs.fork, user));
    for (size_t i = 0; i < want; ++i) H2_HIP(hipStreamWaitEvent(bs.s[i], bs.fork, 0));
    int rc = H2_OK;
    for (size_t i = 0; i < count && rc == H2_OK; ++i) {
        if (!d_a[i]) return H2_ERR_ARGS;
        NttJob J;
        job_ntt(J, field, d_a[i], log_n, omega, form);
        if (divisor) {
            J.store_mode = 1;
            host_to_mont(field, J.sk0, divisor, form);
        }
        J.plan = want > 1 ? 1 : 0;
        rc = ntt_run(J, bs.s[i % want]);
    }
    for (size_t i = 0; i < want; ++i) {
        H2_HIP(hipEventRecord(bs.done[i], bs.s[i]));
        H2_HIP(hipStreamWaitEvent(user, bs.done[i], 0));
    }
    return rc;
}
}  // namespace

extern "C" int h2_ntt_batch_device(int field, void *const *d_a, size_t count, unsigned log_n, const uint64_t *omega, int form, void *stream) {
    if (bad_field(field, form) || !d_a || !omega || log_n > 32) return H2_ERR_ARGS;
    if (!count) return H2_OK;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    return ntt_batch(field, d_a, count, log_n, omega, nullptr, form, (hipStream_t)stream);
}

extern "C" int h2_ifft_batch_device(int field, void *const *d_a, size_t count, unsigned log_n, const uint64_t *omega_inv,
                                    const uint64_t *divisor, int form, void *stream) {
    if (bad_field(field, form) || !d_a || !omega_inv || !divisor || log_n > 32) return H2_ERR_ARGS;
    if (!count) return H2_OK;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    return ntt_batch(field, d_a, count, log_n, omega_inv, divisor, form, (hipStream_t)stream);
}

extern "C" int h2_coeff_to_extended_device(int field, const void *d_a, void *d_out, unsigned k, unsigned ext_k,
                                           const uint64_t *g_coset, const uint64_t *g_coset_inv,
                                           const uint64_t *extended_omega, int form, void *stream) {
    if (bad_field(field, form) || !d_a || !d_out || d_a == d_out || !g_coset || !g_coset_inv || !extended_omega || ext_k > 32 ||
        k > ext_k)
        return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    NttJob J;
    job_ntt(J, field, d_out, ext_k, extended_omega, form);
    J.d_in = d_a;
    J.n_in = (size_t)1 << k;
    J.load_mode = 1;
    host_to_mont(field, J.lk0, g_coset, form);
    host_to_mont(field, J.lk1, g_coset_inv, form);
    return ntt_run(J, (hipStream_t)stream);
}

extern "C" int h2_extended_to_coeff_device(int field, void *d_a, unsigned ext_k, const uint64_t *g_coset,
                                           const uint64_t *g_coset_inv, const uint64_t *extended_omega_inv,
                                           const uint64_t *extended_ifft_divisor, int form, void *stream) {
    if (bad_field(field, form) || !d_a || !g_coset || !g_coset_inv || !extended_omega_inv || !extended_ifft_divisor || ext_k > 32)
        return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    NttJob J;
    job_ntt(J, field, d_a, ext_k, extended_omega_inv, form);
    J.store_mode = 2;
    // a[i] * divisor * {1, zeta^2, zeta}[i % 3]   (domain.rs:316, into_coset = false)
    u64 div[4], z[4], zi[4];
    host_to_mont(field, div, extended_ifft_divisor, form);
    host_to_mont(field, z, g_coset, form);
    host_to_mont(field, zi, g_coset_inv, form);
    memcpy(J.sk0, div, 32);
    host_mul(field, J.sk1, div, zi);
    host_mul(field, J.sk2, div, z);
    return ntt_run(J, (hipStream_t)stream);
}

// ---- divide_by_vanishing_poly (poly/domain.rs:329-348): a[i] *= t_evaluations[i mod nt], k_mul_periodic ------------
extern "C" int h2_divide_by_vanishing_poly_device(int field, void *d_a, unsigned ext_k, const uint64_t *t_evaluations, size_t nt, int form,
                                                  void *stream) {
    if (bad_field(field, form) || !d_a || !t_evaluations || nt == 0 || nt > 4096 || ext_k > 32) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    NttContext &cx = ntt_ctx();
    std::lock_guard<std::mutex> lk(cx.mu);
    int dev = 0;
    (void)hipGetDevice(&dev);
    DevBuf &tb = cx.stage[std::make_pair(dev * 4 + 2, st)];
    if ((rc = tb.reserve(nt * 32)) != H2_OK) return rc;
    std::vector<u64> tm(nt * 4);
    for (size_t i = 0; i < nt; ++i) host_to_mont(field, &tm[4 * i], t_evaluations + 4 * i, form);   // Montgomery factors work for either data form
    H2_HIP(hipStreamSynchronize(st));   // the small table buffer is reused across calls
    H2_HIP(hipMemcpyAsync(tb.ptr, tm.data(), nt * 32, hipMemcpyHostToDevice, st));
    H2_HIP(hipStreamSynchronize(st));   // tm goes out of scope
    const size_t n = (size_t)1 << ext_k;
    dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (field == H2_FP) hipLaunchKernelGGL((k_mul_periodic<FP>), grid, block, 0, st, (u32 *)d_a, tb.as<u32>(), n, (u32)nt);
    else hipLaunchKernelGGL((k_mul_periodic<FQ>), grid, block, 0, st, (u32 *)d_a, tb.as<u32>(), n, (u32)nt);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

// ---- host-pointer variants: stage through a per-stream device buffer --------------------------------
namespace {
int stage_buffer(size_t bytes, int slot, void *&d) {
    NttContext &cx = ntt_ctx();
    std::lock_guard<std::mutex> lk(cx.mu);
    int dev = 0;
    (void)hipGetDevice(&dev);
    // slot-indexed staging buffers live beside the tmp buffers, keyed by a pseudo-stream
    DevBuf &b = cx.stage[std::make_pair(dev * 4 + slot, (hipStream_t) nullptr)];
    const int rc = b.reserve(bytes);
    d = b.ptr;
    return rc;
}
std::mutex g_host_mu;  // host-pointer calls share staging buffers: serialise them
// copy `in` up, run call(d_in, d_out) on the null stream, copy `out` back and wait; d_in is d_out unless the call is out of place
template <typename Call> int run_staged(const void *in, size_t in_bytes, void *out, size_t out_bytes, bool out_of_place, Call call) {
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    std::lock_guard<std::mutex> lk(g_host_mu);
    void *d_out = nullptr, *d_in = nullptr;
    if ((rc = stage_buffer(out_bytes, 0, d_out)) != H2_OK) return rc;
    if (!out_of_place) d_in = d_out;
    else if ((rc = stage_buffer(in_bytes, 1, d_in)) != H2_OK) return rc;
    H2_HIP(hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, 0));
    if ((rc = call(d_in, d_out)) != H2_OK) return rc;
    H2_HIP(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, 0));
    H2_HIP(hipStreamSynchronize(0));
    return H2_OK;
}
}  // namespace

extern "C" int h2_ntt(int field, uint64_t *a, unsigned log_n, const uint64_t *omega, int form) {
    if (bad_field(field, form) || !a || !omega || log_n > 32) return H2_ERR_ARGS;
    const size_t bytes = (size_t)32 << log_n;
    return run_staged(a, bytes, a, bytes, false, [&](void *d, void *) { return h2_ntt_device(field, d, log_n, omega, form, nullptr); });
}

extern "C" int h2_ifft(int field, uint64_t *a, unsigned log_n, const uint64_t *omega_inv, const uint64_t *divisor, int form) {
    if (bad_field(field, form) || !a || !omega_inv || !divisor || log_n > 32) return H2_ERR_ARGS;
    const size_t bytes = (size_t)32 << log_n;
    return run_staged(a, bytes, a, bytes, false, [&](void *d, void *) { return h2_ifft_device(field, d, log_n, omega_inv, divisor, form, nullptr); });
}

extern "C" int h2_coeff_to_extended(int field, const uint64_t *a, uint64_t *out, unsigned k, unsigned ext_k,
                                    const uint64_t *g_coset, const uint64_t *g_coset_inv, const uint64_t *extended_omega,
                                    int form) {
    if (bad_field(field, form) || !a || !out || !g_coset || !g_coset_inv || !extended_omega || ext_k > 32 || k > ext_k)
        return H2_ERR_ARGS;
    return run_staged(a, (size_t)32 << k, out, (size_t)32 << ext_k, true, [&](void *d_in, void *d_out) {
        return h2_coeff_to_extended_device(field, d_in, d_out, k, ext_k, g_coset, g_coset_inv, extended_omega, form, nullptr);
    });
}

extern "C" int h2_divide_by_vanishing_poly(int field, uint64_t *a, unsigned ext_k, const uint64_t *t_evaluations, size_t nt, int form) {
    if (bad_field(field, form) || !a || !t_evaluations || nt == 0 || nt > 4096 || ext_k > 32) return H2_ERR_ARGS;
    const size_t bytes = (size_t)32 << ext_k;
    return run_staged(a, bytes, a, bytes, false,
                      [&](void *d, void *) { return h2_divide_by_vanishing_poly_device(field, d, ext_k, t_evaluations, nt, form, nullptr); });
}

extern "C" int h2_extended_to_coeff(int field, uint64_t *a, unsigned ext_k, const uint64_t *g_coset,
                                    const uint64_t *g_coset_inv, const uint64_t *extended_omega_inv,
                                    const uint64_t *extended_ifft_divisor, int form) {
    if (bad_field(field, form) || !a || !g_coset || !g_coset_inv || !extended_omega_inv || !extended_ifft_divisor || ext_k > 32)
        return H2_ERR_ARGS;
    const size_t bytes = (size_t)32 << ext_k;
    return run_staged(a, bytes, a, bytes, false, [&](void *d, void *) {
        return h2_extended_to_coeff_device(field, d, ext_k, g_coset, g_coset_inv, extended_omega_inv, extended_ifft_divisor, form, nullptr);
    });
}
