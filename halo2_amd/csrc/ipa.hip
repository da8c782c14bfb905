// Inner-product-argument round kernels: the per-round work of
// `commitment::create_proof` (halo2_proofs/src/poly/commitment/prover.rs:100-142) that is not an MSM.
//
//   h2_generator_collapse   parallel_generator_collapse (:154-166):  g'[i] = g_lo[i] + [u_j] * g_hi[i], normalised to
//                           affine -- n / 2^(j+1) FULL 255-bit scalar multiplications per round, an order of
//                           magnitude more group operations per proof than one commit.  The challenge is the same
//                           for every lane, so the host splits it once with the curve endomorphism
//                           phi(x, y) = (zeta x, y) = [lambda](x, y):  u = k1 + k2 lambda, |k1|, |k2| < 2^129, and
//                           the NAFs of k1 and k2 drive a divergence-free JOINT double-and-add over P and phi(P):
//                           ~130 doublings + ~87 mixed adds instead of 255 + 85.  One lane per point for large
//                           rounds; the last rounds (<= 2^15 points, pure latency) run one point per quad of lanes
//                           (curve_wide.cuh).  One Fermat inversion per point normalises.
//   h2_fold_scalars         the `p'` / `b` collapse (:128-131):  a[i] += a[i + half] * factor.
//
// Both keep their vectors on the device across rounds (d_* variants), removing 2k host round trips per proof.
#include "common.h"
#include "host_field.h"
#include "ipa_kernels.cuh"
#include "ipa_recode.h"
#include "msm_internal.cuh"      // bases_refill_device, bases_register_device_internal, pair_subdigits_apply (msm_table.hip)

namespace h2 {

struct IpaContext {
    std::mutex mu;
    DevBuf naf, stage, stab;
    // the round loop (h2_ipa_rounds_device): its own lock (held for the whole argument; the launches it makes take `mu`),
    // device scratch { <p'_hi, b_lo>, <p'_lo, b_hi>, L_j, R_j } and the pinned landing pad of L_j, R_j
    std::mutex rounds_mu;
    DevBuf rounds, gprime, rstab;      // rstab: the round loop's two s tables (the single-round entry point keeps `stab`)
    void *rounds_host = nullptr;
    h2_bases_t gp_handle = 0;          // the table of the collapsed generators, kept between arguments (rebuilt in place while its shape repeats)
    size_t gp_n = 0;
    int gp_curve = -1;
    // the whole argument (h2_open_device / h2_open): b, the round loop's column(s), the landing places of host vectors, a few words
    // { s(x_3), p(x_3), the S commitment, its blind }, a pinned landing pad, and a side stream for what does not wait for xi
    std::mutex open_mu;
    DevBuf open_b, open_col, open_s, open_p, open_small;
    void *open_host = nullptr;
    hipStream_t open_side = nullptr, open_side2 = nullptr;
    hipEvent_t open_ev = nullptr, open_ev2 = nullptr;
    hipEvent_t open_land[4] = {nullptr, nullptr, nullptr, nullptr}, open_fixed = nullptr, open_parts = nullptr;     // the S commitment by ranges (open_impl)
    void release_all() {
        for (DevBuf *b : {&naf, &stage, &stab}) b->release();
        // h2_trim must not take the round loop's scratch from under a running argument (which holds rounds_mu for its whole
        // length and takes `mu` inside: try, never wait -- the lock order is the other way round there)
        std::unique_lock<std::mutex> rl(rounds_mu, std::try_to_lock);
        if (!rl.owns_lock()) return;
        for (DevBuf *b : {&rounds, &gprime, &rstab}) b->release();
        if (gp_handle) {
            (void)h2_bases_free(gp_handle);
            debug_count(DBG_IPA_TABLE_FREED);
        }
        gp_handle = 0;
        if (rounds_host) (void)hipHostFree(rounds_host);
        rounds_host = nullptr;
        std::unique_lock<std::mutex> ol(open_mu, std::try_to_lock);      // (as above: never under a running argument)
        if (!ol.owns_lock()) return;
        for (DevBuf *b : {&open_b, &open_col, &open_s, &open_p, &open_small}) b->release();
        if (open_host) (void)hipHostFree(open_host);
        open_host = nullptr;
        for (hipEvent_t *e : {&open_ev, &open_ev2, &open_land[0], &open_land[1], &open_land[2], &open_land[3], &open_fixed, &open_parts}) {
            if (*e) (void)hipEventDestroy(*e);
            *e = nullptr;
        }
        for (hipStream_t *s : {&open_side, &open_side2}) {
            if (*s) (void)hipStreamDestroy(*s);
            *s = nullptr;
        }
    }
};
static StreamContexts<IpaContext> g_ipa_ctxs;
void ipa_release_workspaces() { g_ipa_ctxs.release_current_device(); }   // h2_trim

static int scalar_field_of(int curve) { return curve == H2_PALLAS ? H2_FQ : H2_FP; }
static int base_field_of(int curve) { return curve == H2_PALLAS ? H2_FP : H2_FQ; }
static fe to_fe(const u64 m[4]) {
    fe f;
    memcpy(f.v, m, 32);
    return f;
}

// .to_affine() of `count` <= 2 Jacobian points (12 limbs each, Montgomery) into xy (8 limbs each) with ONE inversion: the running
// products of the Z's, host_inv, back-multiplication.  false (nothing written): some Z is zero.
static bool host_to_affine(int bf, const u64 *jac, int count, u64 *xy) {
    u64 prod[2][4], inv[4], zi[4], i2[4], i3[4];
    for (int i = 0; i < count; ++i) {
        const u64 *z = jac + 12 * i + 8;
        if (host_is_zero(z)) return false;
        if (i) host_mul(bf, prod[i], prod[i - 1], z);
        else memcpy(prod[0], z, 32);
    }
    host_inv(bf, inv, prod[count - 1]);
    for (int i = count - 1; i >= 0; --i) {
        const u64 *pt = jac + 12 * i;
        memcpy(zi, inv, 32);
        if (i) {
            host_mul(bf, zi, inv, prod[i - 1]);      // 1 / z_i = (z_0 .. z_i)^-1 (z_0 .. z_(i-1))
            host_mul(bf, inv, inv, pt + 8);          // (z_0 .. z_(i-1))^-1
        }
        host_mul(bf, i2, zi, zi);
        host_mul(bf, i3, i2, zi);
        host_mul(bf, xy + 8 * i, pt, i2);
        host_mul(bf, xy + 8 * i + 4, pt + 4, i3);
    }
    return true;
}

static int collapse_launch(int curve, void *d_g, size_t half, const u64 *u, int form, hipStream_t st) {
    IpaContext &cx = g_ipa_ctxs.get(st);
    std::lock_guard<std::mutex> lk(cx.mu);
    const int sf = scalar_field_of(curve), bf = base_field_of(curve);      // the challenge lives in the scalar field
    u64 canon[4];
    if (form == H2_FORM_MONTGOMERY) host_from_mont(sf, canon, u);
    else memcpy(canon, u, 32);
    int8_t naf[2 * 264];
    memset(naf, 0, sizeof naf);
    int top = glv_recode(sf, canon, naf, naf + 264);
    int rc = cx.naf.reserve(sizeof naf);
    if (rc != H2_OK) return rc;
    // the digit buffer belongs to this (device, stream): the copy is stream-ordered after the previous collapse that read
    // it, and hipMemcpyAsync from pageable memory has consumed `naf` when it returns
    H2_HIP(hipMemcpyAsync(cx.naf.ptr, naf, sizeof naf, hipMemcpyHostToDevice, st));
    const int8_t *d1 = cx.naf.as<int8_t>(), *d2 = d1 + 264;
    const bool wide = half <= 32768;      // few points: latency-bound, one point per quad of lanes
    dim3 grid((unsigned)(((wide ? half * kGroup : half) + 255) / 256)), block(256);
    const bool canonical = form == H2_FORM_CANONICAL;
    if (canonical) H2_FIELD_LAUNCH(bf, ipa_to_mont, dim3((unsigned)((half * 4 + 255) / 256)), block, 0, st, (u32 *)d_g, half * 4, 1);
    if (wide) H2_FIELD_LAUNCH(bf, ipa_collapse_wide, grid, block, 0, st, (u32 *)d_g, (u32)half, d1, d2, top);
    else H2_FIELD_LAUNCH(bf, ipa_collapse, grid, block, 0, st, (u32 *)d_g, (u32)half, d1, d2, top);
    if (canonical) H2_FIELD_LAUNCH(bf, ipa_to_mont, dim3((unsigned)((half * 2 + 255) / 256)), block, 0, st, (u32 *)d_g, half * 2, 0);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

static int round_scalars_launch(int field, const void *d_p, unsigned k, unsigned j, const u64 *challenges, int form, void *d_cl,
                                void *d_cr, hipStream_t st) {
    IpaContext &cx = g_ipa_ctxs.get(st);
    std::lock_guard<std::mutex> lk(cx.mu);
    u64 um[32 * 4];
    for (unsigned r = 0; r < j; ++r) host_to_mont(field, um + 4 * r, challenges + 4 * r, form);
    int rc = cx.stage.reserve(32 * 32);
    if (rc == H2_OK) rc = cx.stab.reserve(((size_t)32 << j));
    if (rc != H2_OK) return rc;
    // stream-ordered after the previous round's kernels that read the staging buffer; pageable source consumed on return
    if (j) H2_HIP(hipMemcpyAsync(cx.stage.ptr, um, 32 * j, hipMemcpyHostToDevice, st));
    dim3 block(256), gs((unsigned)((((size_t)1 << j) + 255) / 256)), gc((unsigned)((((size_t)1 << k) + 255) / 256));
    H2_FIELD_LAUNCH(field, ipa_s_table, gs, block, 0, st, cx.stab.as<u32>(), cx.stage.as<u32>(), j);
    H2_FIELD_LAUNCH(field, ipa_round_scalars, gc, block, 0, st, (const u32 *)d_p, cx.stab.as<u32>(), k, j, (u32 *)d_cl, (u32 *)d_cr);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

}  // namespace h2

using namespace h2;

extern "C" int h2_generator_collapse_device(int curve, void *d_g_xy, size_t half, const uint64_t *challenge, int form, void *stream) {
    if ((curve != H2_PALLAS && curve != H2_VESTA) || (form != H2_FORM_CANONICAL && form != H2_FORM_MONTGOMERY) || !challenge ||
        (half && !d_g_xy) || half > (1u << 30))
        return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!half) return H2_OK;
    return collapse_launch(curve, d_g_xy, half, challenge, form, (hipStream_t)stream);
}

extern "C" int h2_generator_collapse(int curve, uint64_t *g_xy, size_t half, const uint64_t *challenge, int form) {
    if ((curve != H2_PALLAS && curve != H2_VESTA) || (form != H2_FORM_CANONICAL && form != H2_FORM_MONTGOMERY) || !challenge ||
        (half && !g_xy) || half > (1u << 30))
        return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!half) return H2_OK;
    void *d = nullptr;
    H2_HIP(hipMalloc(&d, half * 128));
    hipError_t e = hipMemcpy(d, g_xy, half * 128, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        rc = collapse_launch(curve, d, half, challenge, form, 0);
        if (rc == H2_OK) e = hipMemcpy(g_xy, d, half * 64, hipMemcpyDeviceToHost);
    }
    (void)hipFree(d);
    if (e != hipSuccess) { set_last_hip_error(e, __FILE__, __LINE__); return H2_ERR_HIP; }
    return rc;
}

static int fold_launch(int field, void *d_a, size_t half, const u64 *factor, int form, hipStream_t st) {
    u64 fm[4];
    host_to_mont(field, fm, factor, form);     // a Montgomery factor works for data in either form
    H2_FIELD_LAUNCH(field, ipa_fold, dim3((unsigned)((half + 255) / 256)), dim3(256), 0, st, (u32 *)d_a, (u32)half, to_fe(fm));
    H2_HIP(hipGetLastError());
    return H2_OK;
}

extern "C" int h2_fold_scalars_device(int field, void *d_a, size_t half, const uint64_t *factor, int form, void *stream) {
    if ((field != H2_FP && field != H2_FQ) || (form != H2_FORM_CANONICAL && form != H2_FORM_MONTGOMERY) || !factor || (half && !d_a) ||
        half > (1u << 30))
        return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!half) return H2_OK;
    return fold_launch(field, d_a, half, factor, form, (hipStream_t)stream);
}

extern "C" int h2_fold_scalars(int field, uint64_t *a, size_t half, const uint64_t *factor, int form) {
    if ((field != H2_FP && field != H2_FQ) || (form != H2_FORM_CANONICAL && form != H2_FORM_MONTGOMERY) || !factor || (half && !a) ||
        half > (1u << 30))
        return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    if (!half) return H2_OK;
    void *d = nullptr;
    H2_HIP(hipMalloc(&d, half * 64));
    hipError_t e = hipMemcpy(d, a, half * 64, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        rc = fold_launch(field, d, half, factor, form, 0);
        if (rc == H2_OK) e = hipMemcpy(a, d, half * 32, hipMemcpyDeviceToHost);
    }
    (void)hipFree(d);
    if (e != hipSuccess) { set_last_hip_error(e, __FILE__, __LINE__); return H2_ERR_HIP; }
    return rc;
}

extern "C" int h2_ipa_round_scalars_device(int field, const void *d_p, unsigned k, unsigned j, const uint64_t *challenges, int form,
                                           void *d_cl, void *d_cr, void *stream) {
    if ((field != H2_FP && field != H2_FQ) || (form != H2_FORM_CANONICAL && form != H2_FORM_MONTGOMERY) || k < 1 || k > 30 || j >= k ||
        (j && !challenges) || !d_p || !d_cl || !d_cr)
        return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    return round_scalars_launch(field, d_p, k, j, challenges, form, d_cl, d_cr, (hipStream_t)stream);
}

// ---- the round loop (h2_ipa_rounds_device) ------------------------------------------------------------------------------------------
// What is fixed while the loop runs: the argument's part (the entry point fills it), then what belongs to ONE registered basis (ipa_rounds_impl)
struct RoundLoop {
    int sf, bf;
    hipStream_t st;
    u32 *p, *b;                        // p' and b, folded in place
    fe z;
    h2_ipa_write_point_fn write_point;
    h2_ipa_squeeze_fn squeeze;
    void *user;
    unsigned k, rounds;                // over this basis: 2^k coefficients, `rounds` rounds
    size_t n;
    h2_bases_t basis;
    bool paired;
    const u64 *rands;                  // the rounds' blinds, two per round
    u32 *col_l, *col_r;                // the round's scalars over the generators (paired: one merged column)
    u32 *vl, *vr, *bl, *br;            // the rows behind the generators': both inner products times z, both blinds
    u32 *d_lr, *d_partial, *stab[2];   // scratch: L_j and R_j, the inner products' partial sums, this round's s table and the next one's
    u64 *lr;                           // the pinned landing pad of L_j, R_j
};

// both inner products' partial sums and the round's scalars in one launch, the sums and the tail rows in a second
static int round_enqueue_prep(const RoundLoop &R, unsigned j) {
    const dim3 gp(2 * kIpBlocks + (unsigned)((R.n + 255) / 256));
    H2_FIELD_LAUNCH(R.sf, ipa_round_prep, gp, dim3(256), 0, R.st, (const u32 *)R.p, (const u32 *)R.b, (const u32 *)R.stab[j & 1], R.k, j, R.d_partial,
                    R.col_l, R.col_r);
    H2_FIELD_LAUNCH(R.sf, ipa_round_finish, dim3(1), dim3(256), 0, R.st, (const u32 *)R.d_partial, R.z, to_fe(R.rands + 8 * j), to_fe(R.rands + 8 * j + 4),
                    R.vl, R.vr, R.bl, R.br);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

// L_j and R_j: one paired commit or a commit of two columns, then 192 bytes to the landing pad
static int round_commit(const RoundLoop &R, unsigned j) {
    int rc;
    if (R.paired) {
        rc = h2_commit_pair_device(R.basis, R.col_l, R.n + 4, R.k - j - 1, H2_FORM_MONTGOMERY, H2_OUT_JACOBIAN, R.d_lr, R.st);
    } else {
        const void *cols[2] = {R.col_l, R.col_r};
        void *outs[2] = {R.d_lr, R.d_lr + 24};
        rc = h2_commit_batch_device(R.basis, cols, 2, R.n + 2, nullptr, nullptr, H2_FORM_MONTGOMERY, H2_OUT_JACOBIAN, outs, R.st);
    }
    if (rc != H2_OK) return rc;
    H2_HIP(hipMemcpyAsync(R.lr, R.d_lr, 192, hipMemcpyDeviceToHost, R.st));
    H2_HIP(hipStreamSynchronize(R.st));
    return H2_OK;
}

// .to_affine() of both points with one inversion (prover.rs:116-117), the transcript (:121-124) and the challenge's inverse (:125)
static int round_absorb(const RoundLoop &R, u64 *u, u64 *u_inv) {
    u64 xy[16];
    if (!host_to_affine(R.bf, R.lr, 2, xy)) {
        set_last_error_msg("h2_ipa_rounds_device: L_j or R_j is the point at infinity, which a transcript cannot absorb");
        return H2_ERR_ARGS;
    }
    int rc;
    if ((rc = R.write_point(R.user, xy)) != H2_OK || (rc = R.write_point(R.user, xy + 8)) != H2_OK || (rc = R.squeeze(R.user, u)) != H2_OK) return rc;
    if (host_is_zero(u)) {
        set_last_error_msg("h2_ipa_rounds_device: zero challenge");       // the reference unwraps the inverse (:125)
        return H2_ERR_ARGS;
    }
    host_inv(R.sf, u_inv, u);
    return H2_OK;
}

// the two folds (:128-133) and the next round's s table in one launch
static int round_enqueue_fold(const RoundLoop &R, unsigned j, const u64 *u, const u64 *u_inv) {
    const size_t half = (size_t)1 << (R.k - j - 1);
    const u32 fold_blocks = (u32)((half + 255) / 256), s_count = j + 1 < R.rounds ? 2u << j : 0u;
    H2_FIELD_LAUNCH(R.sf, ipa_round_fold, dim3(fold_blocks + (s_count + 255) / 256), dim3(256), 0, R.st, R.p, R.b, (u32)half, fold_blocks, to_fe(u_inv), to_fe(u),
                    (const u32 *)R.stab[j & 1], R.stab[(j + 1) & 1], s_count);
    H2_HIP(hipGetLastError());
    return H2_OK;
}

// `rounds` rounds over ONE registered basis; R arrives with the argument's part filled.  The caller holds cx.rounds_mu.
static int ipa_rounds_impl(IpaContext &cx, RoundLoop R, unsigned k, unsigned rounds, h2_bases_t basis, int paired, const uint64_t *rands, void *d_column_l,
                           void *d_column_r, uint64_t *challenges_out, uint64_t *c_out, uint64_t *f_acc) {
    int rc;
    if ((rc = cx.rounds.reserve(64 + 192 + (size_t)2 * kIpBlocks * 32)) != H2_OK) return rc;
    const size_t tab_words = (size_t)8 << (rounds ? rounds - 1 : 0);          // s_j has 2^j entries, j < rounds
    if ((rc = cx.rstab.reserve(2 * tab_words * 4)) != H2_OK) return rc;         // two tables: a round reads one, its fold writes the next
    if (!cx.rounds_host) H2_HIP(hipHostMalloc(&cx.rounds_host, 256, hipHostMallocDefault));
    const size_t n = (size_t)1 << k;
    u32 *d_ip = cx.rounds.as<u32>(), *cl = (u32 *)d_column_l, *cr = paired ? cl : (u32 *)d_column_r;
    R.k = k, R.rounds = rounds, R.n = n, R.basis = basis, R.paired = paired != 0, R.rands = rands;
    R.col_l = cl, R.col_r = cr;
    R.vl = cl + 8 * n, R.vr = paired ? cl + 8 * (n + 1) : cr + 8 * n;
    R.bl = paired ? cl + 8 * (n + 2) : cl + 8 * (n + 1), R.br = paired ? cl + 8 * (n + 3) : cr + 8 * (n + 1);
    R.d_lr = d_ip + 16, R.d_partial = d_ip + 64, R.stab[0] = cx.rstab.as<u32>(), R.stab[1] = R.stab[0] + tab_words;
    R.lr = (u64 *)cx.rounds_host;
    H2_HIP(hipMemcpyAsync(R.stab[0], kHostField[R.sf].one, 32, hipMemcpyHostToDevice, R.st));      // s_0 = [1]
    u64 challenges[32 * 4];
    for (unsigned j = 0; j < rounds; ++j) {
        u64 *u = challenges + 4 * j, u_inv[4], t[4];
        if ((rc = round_enqueue_prep(R, j)) != H2_OK || (rc = round_commit(R, j)) != H2_OK || (rc = round_absorb(R, u, u_inv)) != H2_OK ||
            (rc = round_enqueue_fold(R, j, u, u_inv)) != H2_OK)
            return rc;
        host_mul(R.sf, t, rands + 8 * j, u_inv);                                                          // :140-141
        host_add(R.sf, f_acc, f_acc, t);
        host_mul(R.sf, t, rands + 8 * j + 4, u);
        host_add(R.sf, f_acc, f_acc, t);
    }
    if (rounds == k) {                   // p' has collapsed to the scalar c (:146)
        H2_HIP(hipMemcpyAsync(R.lr, R.p, 32, hipMemcpyDeviceToHost, R.st));
        H2_HIP(hipStreamSynchronize(R.st));
        memcpy(c_out, R.lr, 32);
    }
    if (challenges_out) memcpy(challenges_out, challenges, 32 * (size_t)rounds);
    return H2_OK;
}

// ---- the switch to the collapsed generators ---------------------------------------------------------------------------------------------
static bool keep_gp_table() {      // H2_IPA_KEEP_TABLE=0: register / free per argument (A/B)
    static const bool keep = [] { const char *e = ab_env("H2_IPA_KEEP_TABLE"); return !(e && e[0] == '0'); }();
    return keep;
}

// The table of G'_J for this context: G'_J read off `basis` (h2_ipa_collapsed_generators_device) with u and w behind it, then the table kept from
// the last argument refilled in place while its shape repeats, or a new one registered.  *hj: the handle (cx.gp_handle).
static int collapsed_table(IpaContext &cx, int curve, unsigned k, unsigned J, h2_bases_t basis, const u64 *challenges, const uint64_t *uw_xy, bool pair2,
                           hipStream_t st, h2_bases_t *hj) {
    const size_t nj = (size_t)1 << (k - J), tail = pair2 ? 4 : 2;
    int rc;
    if ((rc = cx.gprime.reserve((nj + tail) * 64)) != H2_OK) return rc;
    char *d_g = cx.gprime.as<char>();
    if ((rc = h2_ipa_collapsed_generators_device(basis, k, J, challenges, H2_FORM_MONTGOMERY, d_g, st)) != H2_OK) return rc;
    u64 tails[4 * 8];                                                 // u, u, w, w  or  u, w
    for (size_t t = 0; t < tail; ++t) memcpy(tails + 8 * t, uw_xy + 8 * (pair2 ? t / 2 : t), 64);
    H2_HIP(hipMemcpyAsync(d_g + nj * 64, tails, tail * 64, hipMemcpyHostToDevice, st));
    H2_HIP(hipStreamSynchronize(st));                                // the registration reads the points on the null stream
    if (cx.gp_handle && (!keep_gp_table() || cx.gp_curve != curve || cx.gp_n != nj + tail)) {
        (void)h2_bases_free(cx.gp_handle);
        cx.gp_handle = 0;
        debug_count(DBG_IPA_TABLE_FREED);
    }
    if (cx.gp_handle) {
        if ((rc = bases_refill_device(cx.gp_handle, d_g, nj + tail, H2_FORM_MONTGOMERY)) != H2_OK) return rc;
        debug_count(DBG_IPA_TABLE_REFILLED);
    } else {
        // rounds over a small table are sub-digit paired commits, which read an ENDOMORPHISM table as well: 8 x 16 doublings in its chain instead
        // of 15 x 16 -- the chain is what the table costs (0.77 ms of 240 dependent doublings at 2^14 points).  H2_IPA_GLV_TABLE=0: the plain table (A/B).
        static const bool glv_env = [] { const char *e = ab_env("H2_IPA_GLV_TABLE"); return !(e && e[0] == '0'); }();
        const bool glv = glv_env && pair2 && pair_subdigits_apply(nj + tail);
        if ((rc = bases_register_device_internal(curve, d_g, nj + tail, H2_FORM_MONTGOMERY, &cx.gp_handle, glv)) != H2_OK) return rc;
        cx.gp_curve = curve;
        cx.gp_n = nj + tail;
        debug_count(DBG_IPA_TABLE_REGISTERED);
    }
    *hj = cx.gp_handle;
    return H2_OK;
}

// Retention: the table (16 rows x gp_n x 64 B) stays with this (device, stream) context for the next argument of the same shape -- up to
// 2^17 points (128 MiB); beyond that, and with H2_IPA_KEEP_TABLE=0, it goes back at the END of the call.  h2_trim releases what is kept.
// (ipa_rounds_impl synchronised the stream before returning c and f to the host, so nothing is reading the table any more.)
static void collapsed_table_retain(IpaContext &cx) {
    if (keep_gp_table() && cx.gp_n <= ((size_t)1 << 17) + 4) return;
    (void)h2_bases_free(cx.gp_handle);
    cx.gp_handle = 0;
    debug_count(DBG_IPA_TABLE_FREED);
}

// The round loop of `commitment::create_proof` (poly/commitment/prover.rs:104-142) as ONE call: per round the inner products,
// the L_j / R_j scalars over the original generators, their commit(s), the two points to the transcript, the challenge, and the
// p' / b folds.  The host is touched once per round (192 bytes of L_j, R_j in Jacobian form land in pinned memory; the
// normalisation -- one shared inversion -- and the challenge's inverse are microseconds of 64-bit host arithmetic), through
// the caller's transcript: `write_point` receives the affine point (8 x u64, Montgomery), `squeeze` returns the challenge
// scalar (4 x u64, Montgomery) -- the two TranscriptWrite methods the reference's loop uses (:121-124).
// With switch_rounds = J > 0 the first J rounds run over `basis` (the original generators), then G'_J is read off its table
// (h2_ipa_collapsed_generators_device), registered as a table of its own next to u and w, and the remaining k - J rounds run as a
// (k - J)-round argument over it: a round over the original generators costs a full-size commit whatever j, a round over G'_J a
// commit of 2^(k-J) points.
// Measured (profiles/r04_opening_switch_sweep.txt, ms per argument): k = 16: J = 2 8.8 / 1 9.3; k = 18: J = 4 10.7 / 3 11.6; k = 19: 5 13.4 / 4 13.6;
// k = 20: 5 19.5 / 6 20.0 / 4 21.2; k = 21: 6 31.8 / 5 32.2; k = 22: 5 58.2 / 6 59.8 / 4 61.5 / 8 66.1 -- a table of 2^14 points up to k = 19, then
// five rounds: every further round over the original generators costs a full 2^k commit, a larger G' only its registration.
// Round 5: rounds over a table of up to 2^16 points are paired commits with 8-bit sub-digits (msm.hip, pair_subdigit_launch: 0.20 ms at 2^14
// points against 0.245 at 2^15 and 0.26 for the general form at either), which moves k = 20 to a 2^14-point table as well: J = 6 16.8 ms, J = 5
// 16.9-17.4, the general form 17.6-17.7 either way (profiles/r05_pair_subdigits.txt).  k = 21 keeps 6 rounds, k >= 22 five.
extern "C" unsigned h2_ipa_default_switch_rounds(unsigned k, int paired) {
    if (!paired || k < 16 || k > 26 || h2_commit_window_bits(((size_t)1 << k) + 4) != 16) return 0;
    return k <= 20 ? k - 14 : k == 21 ? 6 : 5;
}

extern "C" int h2_ipa_rounds_device(int curve, unsigned k, unsigned switch_rounds, h2_bases_t basis, int paired, void *d_p, void *d_b,
                                    const uint64_t *z, const uint64_t *rands, const uint64_t *uw_xy, void *d_column_l, void *d_column_r,
                                    h2_ipa_write_point_fn write_point, h2_ipa_squeeze_fn squeeze, void *user, uint64_t *c_out,
                                    uint64_t *f_out, void *stream) {
    if ((curve != H2_PALLAS && curve != H2_VESTA) || k < 1 || k > 30 || !d_p || !d_b || !z || !rands || !d_column_l || !write_point ||
        !squeeze || !c_out || !f_out || (!paired && !d_column_r))
        return H2_ERR_ARGS;
    // everything that can be refused is refused HERE, before round 0 writes L_0 / R_0 into the caller's transcript and folds p' / b:
    // the read-out of the collapsed generators (h2_ipa_collapsed_generators_device) takes a 16-bit table over g || u || u || w || w
    size_t basis_n = 0;
    int basis_c = 0, basis_curve = -1;
    if ((h2_bases_info(basis, &basis_n, &basis_c, &basis_curve)) != H2_OK) return H2_ERR_HANDLE;
    if (basis_curve != curve || basis_n < ((size_t)1 << k)) return H2_ERR_ARGS;
    const bool can_switch = paired && basis_c == 16 && k <= 26 && basis_n == ((size_t)1 << k) + 4;
    unsigned J = switch_rounds == H2_IPA_SWITCH_DEFAULT ? (can_switch ? h2_ipa_default_switch_rounds(k, paired) : 0) : switch_rounds;
    if (J && (!can_switch || J >= k || J > 12 || !uw_xy)) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    IpaContext &cx = g_ipa_ctxs.get(st);
    std::lock_guard<std::mutex> lk(cx.rounds_mu);
    RoundLoop R{};
    R.sf = scalar_field_of(curve), R.bf = base_field_of(curve), R.st = st, R.p = (u32 *)d_p, R.b = (u32 *)d_b, R.z = to_fe(z);
    R.write_point = write_point, R.squeeze = squeeze, R.user = user;
    u64 f_acc[4] = {0, 0, 0, 0}, challenges[12 * 4];
    if (!J) {
        rc = ipa_rounds_impl(cx, R, k, k, basis, paired, rands, d_column_l, d_column_r, nullptr, c_out, f_acc);
        if (rc == H2_OK) memcpy(f_out, f_acc, 32);
        return rc;
    }
    if ((rc = ipa_rounds_impl(cx, R, k, J, basis, 1, rands, d_column_l, nullptr, challenges, c_out, f_acc)) != H2_OK) return rc;
    const size_t nj = (size_t)1 << (k - J);
    const bool pair2 = h2_commit_pair_supported(nj + 4) != 0;
    h2_bases_t hj = 0;
    if ((rc = collapsed_table(cx, curve, k, J, basis, challenges, uw_xy, pair2, st, &hj)) != H2_OK) return rc;
    // the columns of the second phase fit in the first phase's scratch (2 (nj + 2) <= 2^k + 4)
    void *col_r = pair2 ? nullptr : (void *)((char *)d_column_l + 32 * (nj + 2));
    rc = ipa_rounds_impl(cx, R, k - J, k - J, hj, pair2 ? 1 : 0, rands + 8 * J, d_column_l, col_r, nullptr, c_out, f_acc);
    if (rc == H2_OK) memcpy(f_out, f_acc, 32);
    collapsed_table_retain(cx);
    return rc;
}

// the same with p' and b in host memory (copied in; the folded vectors are not copied back: only c and f leave the argument)
extern "C" int h2_ipa_rounds(int curve, unsigned k, unsigned switch_rounds, h2_bases_t basis, int paired, const uint64_t *p, const uint64_t *b,
                             const uint64_t *z, const uint64_t *rands, const uint64_t *uw_xy, h2_ipa_write_point_fn write_point,
                             h2_ipa_squeeze_fn squeeze, void *user, uint64_t *c_out, uint64_t *f_out) {
    if (k < 1 || k > 30 || !p || !b) return H2_ERR_ARGS;
    int rc = ensure_device();
    if (rc != H2_OK) return rc;
    const size_t n = (size_t)1 << k, col = (n + 4) * 32;
    char *d = nullptr;
    H2_HIP(hipMalloc((void **)&d, 2 * n * 32 + 2 * col));
    hipError_t e = hipMemcpy(d, p, n * 32, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + n * 32, b, n * 32, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        rc = h2_ipa_rounds_device(curve, k, switch_rounds, basis, paired, d, d + n * 32, z, rands, uw_xy, d + 2 * n * 32, d + 2 * n * 32 + col,
                                  write_point, squeeze, user, c_out, f_out, nullptr);
    (void)hipFree(d);
    if (e != hipSuccess) { set_last_hip_error(e, __FILE__, __LINE__); return H2_ERR_HIP; }
    return rc;
}

// ---- the whole opening argument: poly::commitment::prover::create_proof (prover.rs:26-151) as ONE call -----------------------------
// What a Rust shim replaces is the function, not its loop: the caller draws the randomness (n + 1 + 2k scalars in the reference's
// order, :45-47, :53, :111-112) and owns the transcript; everything between is here.  With the round loop alone native
// (h2_ipa_rounds) the C++ host mirror spent 68-71 ms on a k = 20 argument whose device work is 18: two host Horner evaluations
// of 2^20 coefficients and five 32 MiB vectors across PCIe between host-pointer calls.  Here the vectors cross once (h2_open) or
// not at all (h2_open_device), the constant-coefficient corrections (:51, :72) are one-lane kernels instead of host round trips,
// and what does not depend on xi -- b = powers of x_3 (:86-97) and v -- runs while the host normalises and hashes the S
// commitment.  v: P'(x_3) = xi s(x_3) + p(x_3) with s(x_3) = 0 EXACTLY after :51 (field arithmetic), so v = p(x_3) is
// evaluated before xi exists and p' is never read a second time.  Same bytes as the reference for the same randomness
// (tests/test_gpu_opening.py).
struct OpenArgs {
    int curve;
    unsigned k;
    h2_bases_t g_basis, opening_basis;
    int paired;
    unsigned switch_rounds;
    const uint64_t *uw_xy;
    const void *d_p;                  // p_poly: resident, or
    const uint64_t *host_p;           //         in host memory (it lands in cx.open_p)
    const uint64_t *p_blind, *x3;
    void *d_s;                        // s_poly: resident (overwritten with P'), or
    const uint64_t *host_s;           //         in host memory (d_s is then its landing place, cx.open_s)
    const uint64_t *s_blind, *rands;
    h2_ipa_write_point_fn write_point;
    h2_ipa_squeeze_fn squeeze;
    void *user;
    uint64_t *c_out, *f_out;
    hipStream_t st;
    int sf;                           // (open_checked) the scalar field and n = 2^k
    size_t n;
};
// cx.open_small in words: s(x_3), v = p(x_3), the S commitment, its blind; (by ranges) the quarters' evaluations, 4 x 8, and their shares of the commitment, 4 x 24
enum { kOpenSAt = 0, kOpenV = 8, kOpenCommit = 16, kOpenBlind = 40, kOpenEv = 64, kOpenPart = 128 };

// the context's scratch, and its streams and events where this is their first use; nothing is enqueued yet
static int open_prepare(IpaContext &cx, const OpenArgs &a, bool by_ranges) {
    const size_t n = a.n;
    int rc;
    if ((rc = cx.open_b.reserve(n * 32)) != H2_OK || (rc = cx.open_col.reserve((2 * n + 8) * 32)) != H2_OK || (rc = cx.open_small.reserve(1024)) != H2_OK) return rc;
    if (!cx.open_host) H2_HIP(hipHostMalloc(&cx.open_host, 256, hipHostMallocDefault));
    if (!cx.open_ev) H2_HIP(hipEventCreateWithFlags(&cx.open_ev, hipEventDisableTiming));
    if (!cx.open_ev2) H2_HIP(hipEventCreateWithFlags(&cx.open_ev2, hipEventDisableTiming));
    if (!cx.open_side) H2_HIP(hipStreamCreateWithFlags(&cx.open_side, hipStreamNonBlocking));
    if (!by_ranges) return H2_OK;
    if (!cx.open_side2) H2_HIP(hipStreamCreateWithFlags(&cx.open_side2, hipStreamNonBlocking));
    for (hipEvent_t *e : {&cx.open_land[0], &cx.open_land[1], &cx.open_land[2], &cx.open_land[3], &cx.open_fixed, &cx.open_parts})
        if (!*e) H2_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return H2_OK;
}

// s_poly gets its root at x_3 (:49-51) and is committed to (:56), BY RANGES:
// The fresh coefficients come from the caller's rng, i.e. from HOST memory: 32 MiB across PCIe at k = 20 (0.9 ms) in front of a 1.1 ms commit.
// Cut into four quarters that cross from the top down: quarter r's share of the commitment (h2_commit_range_device over its columns of the
// table) starts as soon as it has landed, on one of two side streams, while the next quarter crosses; every quarter is evaluated at x_3 on the
// way (as a polynomial in its own index).  The quarter with the constant coefficient crosses LAST: s(x_3) = sum_r x_3^(r n / 4) ev_r is known a
// kernel later, the coefficient is fixed, that quarter is committed with the blind, and the four shares are added.  Behind the last byte: one
// quarter-size commit instead of a whole one.
static int open_commit_s_ranges(IpaContext &cx, const OpenArgs &a) {
    const int sf = a.sf;
    const size_t q = a.n / 4;
    hipStream_t st = a.st, sides[2] = {cx.open_side, cx.open_side2};
    u32 *small = cx.open_small.as<u32>(), *d_commit = small + kOpenCommit, *d_blind = small + kOpenBlind, *d_ev = small + kOpenEv, *d_part = small + kOpenPart;
    int rc;
    H2_HIP(hipMemcpyAsync(d_blind, a.s_blind, 32, hipMemcpyHostToDevice, st));
    u64 xq[4], xp[4][4];                                    // x_3^(n / 4) by squaring, then its first three powers
    memcpy(xq, a.x3, 32);
    for (unsigned i = 0; i + 2 < a.k; ++i) host_mul(sf, xq, xq, xq);
    memcpy(xp[1], xq, 32);
    host_mul(sf, xp[2], xq, xq);
    host_mul(sf, xp[3], xp[2], xq);
    for (int r = 3; r >= 0; --r) {
        char *dst = (char *)a.d_s + (size_t)r * q * 32;
        H2_HIP(hipMemcpyAsync(dst, (const char *)a.host_s + (size_t)r * q * 32, q * 32, hipMemcpyHostToDevice, st));
        if ((rc = h2_eval_polynomial_device(sf, dst, q, a.x3, H2_FORM_MONTGOMERY, d_ev + 8 * r, st)) != H2_OK) return rc;
        if (r == 0) {
            H2_FIELD_LAUNCH(sf, ipa_fix_s0, dim3(1), dim3(64), 0, st, (u32 *)a.d_s, (const u32 *)d_ev, to_fe(xp[1]), to_fe(xp[2]), to_fe(xp[3]));
            H2_HIP(hipGetLastError());
        }
        H2_HIP(hipEventRecord(cx.open_land[r], st));
        hipStream_t sd = sides[r & 1];
        H2_HIP(hipStreamWaitEvent(sd, cx.open_land[r], 0));
        if ((rc = h2_commit_range_device(a.g_basis, dst, (size_t)r * q, q, r == 0 ? d_blind : nullptr, H2_FORM_MONTGOMERY, H2_OUT_JACOBIAN, d_part + 24 * r,
                                         sd)) != H2_OK)
            return rc;
    }
    // the four shares meet on the first side stream (quarter 0 ran on it last; the other stream's two are awaited)
    H2_HIP(hipEventRecord(cx.open_parts, sides[1]));
    H2_HIP(hipStreamWaitEvent(sides[0], cx.open_parts, 0));
    if ((rc = h2_points_sum_device(a.curve, d_part, 4, H2_FORM_MONTGOMERY, H2_OUT_JACOBIAN, d_commit, sides[0])) != H2_OK) return rc;
    H2_HIP(hipMemcpyAsync(cx.open_host, d_commit, 96, hipMemcpyDeviceToHost, sides[0]));
    H2_HIP(hipEventRecord(cx.open_ev, sides[0]));
    return H2_OK;
}

// the same WHOLE: one upload (a host s_poly), one evaluation, one commit, all on `st`
static int open_commit_s_whole(IpaContext &cx, const OpenArgs &a) {
    const int sf = a.sf;
    const size_t n = a.n;
    hipStream_t st = a.st;
    u32 *small = cx.open_small.as<u32>(), *d_s_at = small + kOpenSAt, *d_commit = small + kOpenCommit, *d_blind = small + kOpenBlind;
    int rc;
    if (!a.host_p) {
        // a resident p_poly may have been produced on the caller's stream: the side stream (b and v) waits for what is on `st` NOW --
        // recorded before the evaluation and the commitment of s_poly are enqueued, so that it runs beside them, not behind them
        H2_HIP(hipEventRecord(cx.open_ev2, st));
        H2_HIP(hipStreamWaitEvent(cx.open_side, cx.open_ev2, 0));
    }
    if (a.host_s) H2_HIP(hipMemcpyAsync(a.d_s, a.host_s, n * 32, hipMemcpyHostToDevice, st));
    if ((rc = h2_eval_polynomial_device(sf, a.d_s, n, a.x3, H2_FORM_MONTGOMERY, d_s_at, st)) != H2_OK) return rc;
    H2_FIELD_LAUNCH(sf, ipa_sub_at0, dim3(1), dim3(64), 0, st, (u32 *)a.d_s, (const u32 *)d_s_at);
    H2_HIP(hipGetLastError());
    H2_HIP(hipMemcpyAsync(d_blind, a.s_blind, 32, hipMemcpyHostToDevice, st));
    if ((rc = h2_commit_device(a.g_basis, a.d_s, n, nullptr, d_blind, H2_FORM_MONTGOMERY, H2_OUT_JACOBIAN, d_commit, st)) != H2_OK) return rc;
    H2_HIP(hipMemcpyAsync(cx.open_host, d_commit, 96, hipMemcpyDeviceToHost, st));
    H2_HIP(hipEventRecord(cx.open_ev, st));
    return H2_OK;
}

// beside the commit and the host's part, on `side`: p_poly's way in (a host vector; *d_p is where it lands), b = the powers of x_3 and v = p(x_3)
static int open_b_and_v(IpaContext &cx, const OpenArgs &a, hipStream_t side, const void **d_p) {
    int rc;
    if (a.host_p) {
        if ((rc = cx.open_p.reserve(a.n * 32)) != H2_OK) return rc;
        H2_HIP(hipMemcpyAsync(cx.open_p.ptr, a.host_p, a.n * 32, hipMemcpyHostToDevice, side));
        *d_p = cx.open_p.ptr;
    }
    if ((rc = h2_powers_device(a.sf, a.x3, a.n, H2_FORM_MONTGOMERY, cx.open_b.ptr, side)) != H2_OK) return rc;
    if ((rc = h2_eval_polynomial_device(a.sf, *d_p, a.n, a.x3, H2_FORM_MONTGOMERY, cx.open_small.as<u32>() + kOpenV, side)) != H2_OK) return rc;
    H2_HIP(hipEventRecord(cx.open_ev2, side));
    return H2_OK;
}

// the S commitment has landed: .to_affine() (:56), the transcript (:57), xi (:62) and z (:66)
static int open_absorb_s(IpaContext &cx, const OpenArgs &a, u64 *xi, u64 *z) {
    H2_HIP(hipEventSynchronize(cx.open_ev));
    u64 xy[8];
    if (!host_to_affine(base_field_of(a.curve), (const u64 *)cx.open_host, 1, xy)) {
        set_last_error_msg("h2_open: the commitment to s_poly is the point at infinity, which a transcript cannot absorb");
        return H2_ERR_ARGS;
    }
    int rc;
    if ((rc = a.write_point(a.user, xy)) == H2_OK && (rc = a.squeeze(a.user, xi)) == H2_OK) rc = a.squeeze(a.user, z);
    return rc;
}

// P' = P - [v] G_0 + [xi] S (:70-73), in place on s_poly, behind b and v; then the rounds
static int open_rounds(IpaContext &cx, const OpenArgs &a, const void *d_p, const u64 *xi, const u64 *z) {
    const int sf = a.sf;
    const size_t n = a.n;
    int rc;
    H2_HIP(hipStreamWaitEvent(a.st, cx.open_ev2, 0));
    if ((rc = h2_scale_add_device(sf, a.d_s, xi, d_p, n, H2_FORM_MONTGOMERY, a.st)) != H2_OK) return rc;
    H2_FIELD_LAUNCH(sf, ipa_sub_at0, dim3(1), dim3(64), 0, a.st, (u32 *)a.d_s, (const u32 *)(cx.open_small.as<u32>() + kOpenV));
    H2_HIP(hipGetLastError());
    u64 f0[4], t[4], f_delta[4];
    host_mul(sf, t, a.s_blind, xi);                                                                      // :74-78
    host_add(sf, f0, t, a.p_blind);
    char *col = cx.open_col.as<char>();
    rc = h2_ipa_rounds_device(a.curve, a.k, a.switch_rounds, a.opening_basis, a.paired, a.d_s, cx.open_b.ptr, z, a.rands, a.uw_xy, col,
                              a.paired ? nullptr : col + (n + 4) * 32, a.write_point, a.squeeze, a.user, a.c_out, f_delta, a.st);
    if (rc == H2_OK) host_add(sf, a.f_out, f0, f_delta);
    return rc;
}

// The stages in order.  ONE exit: whichever stage fails, the side streams -- which may still be reading the caller's p_poly and writing this context's
// scratch -- are joined before the caller hears of it.  The success path has no such wait: h2_ipa_rounds_device ends synchronised behind everything.
static int open_impl(IpaContext &cx, const OpenArgs &a) {
    static const bool ranges_env = [] { const char *e = ab_env("H2_OPEN_S_RANGES"); return !(e && e[0] == '0'); }();      // 0: one upload, one commit (A/B)
    // (with p_poly in host memory too -- h2_open -- the calling thread is the bottleneck either way: 96 MiB of pageable copies through one thread, and every launch
    // between two of them is PCIe idle time; measured there the quarters LOSE a millisecond to one upload + one commit, so they serve the resident p_poly only)
    const bool by_ranges = a.host_s && !a.host_p && ranges_env && a.k >= 16;
    int rc = open_prepare(cx, a, by_ranges);
    if (rc != H2_OK) return rc;           // (nothing enqueued)
    // b and v run on the side stream, or (S commitment by ranges: the side streams carry its shares) on `st` itself, which has only moved and
    // evaluated the quarters so far
    hipStream_t side = by_ranges ? a.st : cx.open_side;
    const void *d_p = a.d_p;
    u64 xi[4], z[4];
    rc = by_ranges ? open_commit_s_ranges(cx, a) : open_commit_s_whole(cx, a);
    if (rc == H2_OK) rc = open_b_and_v(cx, a, side, &d_p);
    if (rc == H2_OK) rc = open_absorb_s(cx, a, xi, z);
    if (rc == H2_OK) rc = open_rounds(cx, a, d_p, xi, z);
    if (rc != H2_OK) {
        (void)hipStreamSynchronize(cx.open_side);
        if (cx.open_side2) (void)hipStreamSynchronize(cx.open_side2);
    }
    return rc;
}

// What the three entry points share: the checks -- what can be refused is refused before the S commitment reaches the caller's transcript --, the
// context's lock, the landing place of a host s_poly, the argument
static int open_checked(OpenArgs a) {
    if ((a.curve != H2_PALLAS && a.curve != H2_VESTA) || a.k < 1 || a.k > 30 || !a.p_blind || !a.x3 || !a.s_blind || !a.rands || !a.write_point || !a.squeeze ||
        !a.c_out || !a.f_out || (!a.d_p && !a.host_p) || (!a.d_s && !a.host_s) ||
        (a.d_p && a.d_p == a.d_s))                     // (s_poly is overwritten with P' while p_poly is still being read)
        return H2_ERR_ARGS;
    a.sf = scalar_field_of(a.curve), a.n = (size_t)1 << a.k;
    size_t gn = 0, on = 0;
    int gc = -1, oc = -1, rc;
    if (h2_bases_info(a.g_basis, &gn, nullptr, &gc) != H2_OK || h2_bases_info(a.opening_basis, &on, nullptr, &oc) != H2_OK) return H2_ERR_HANDLE;
    if (gc != a.curve || oc != a.curve || gn != a.n || on != a.n + (a.paired ? 4 : 2)) return H2_ERR_ARGS;
    if (h2_bases_blind_base_set(a.g_basis) != 1) return H2_ERR_ARGS;             // Params::w must be installed (h2_bases_set_blind_base)
    if ((rc = ensure_device()) != H2_OK) return rc;
    IpaContext &cx = g_ipa_ctxs.get(a.st);
    std::lock_guard<std::mutex> lk(cx.open_mu);
    if (a.host_s) {
        if ((rc = cx.open_s.reserve(a.n * 32)) != H2_OK) return rc;
        a.d_s = cx.open_s.ptr;
    }
    return open_impl(cx, a);
}

extern "C" int h2_open_device(int curve, unsigned k, h2_bases_t g_basis, h2_bases_t opening_basis, int paired, unsigned switch_rounds,
                              const uint64_t *uw_xy, const void *d_p_poly, const uint64_t *p_blind, const uint64_t *x3, void *d_s_poly,
                              const uint64_t *s_blind, const uint64_t *rands, h2_ipa_write_point_fn write_point, h2_ipa_squeeze_fn squeeze,
                              void *user, uint64_t *c_out, uint64_t *f_out, void *stream) {
    return open_checked(OpenArgs{curve, k, g_basis, opening_basis, paired, switch_rounds, uw_xy, d_p_poly, nullptr, p_blind, x3, d_s_poly, nullptr, s_blind, rands,
                                 write_point, squeeze, user, c_out, f_out, (hipStream_t)stream});
}

// p_poly resident, the fresh s_poly where a host rng leaves it: its quarters cross PCIe inside the call and are committed as they land
extern "C" int h2_open_device_host_s(int curve, unsigned k, h2_bases_t g_basis, h2_bases_t opening_basis, int paired, unsigned switch_rounds,
                                     const uint64_t *uw_xy, const void *d_p_poly, const uint64_t *p_blind, const uint64_t *x3, const uint64_t *s_poly,
                                     const uint64_t *s_blind, const uint64_t *rands, h2_ipa_write_point_fn write_point, h2_ipa_squeeze_fn squeeze,
                                     void *user, uint64_t *c_out, uint64_t *f_out, void *stream) {
    return open_checked(OpenArgs{curve, k, g_basis, opening_basis, paired, switch_rounds, uw_xy, d_p_poly, nullptr, p_blind, x3, nullptr, s_poly, s_blind, rands,
                                 write_point, squeeze, user, c_out, f_out, (hipStream_t)stream});
}

// the same from host vectors (what `&Polynomial<C::Scalar, Coeff>` and a Vec of fresh randomness are): both cross PCIe once, p_poly
// beside the commitment to s_poly; nothing is copied back
extern "C" int h2_open(int curve, unsigned k, h2_bases_t g_basis, h2_bases_t opening_basis, int paired, unsigned switch_rounds,
                       const uint64_t *uw_xy, const uint64_t *p_poly, const uint64_t *p_blind, const uint64_t *x3, const uint64_t *s_poly,
                       const uint64_t *s_blind, const uint64_t *rands, h2_ipa_write_point_fn write_point, h2_ipa_squeeze_fn squeeze, void *user,
                       uint64_t *c_out, uint64_t *f_out) {
    return open_checked(OpenArgs{curve, k, g_basis, opening_basis, paired, switch_rounds, uw_xy, nullptr, p_poly, p_blind, x3, nullptr, s_poly, s_blind, rands,
                                 write_point, squeeze, user, c_out, f_out, nullptr});
}
