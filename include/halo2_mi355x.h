/*
 * halo2_mi355x.h -- C ABI of libhalo2_mi355x.so: the MI355X (gfx950) implementation of the
 * halo2_proofs prover hot path (Pasta MSM + NTT).
 *
 * The reference (zcash/halo2, halo2_proofs 0.3.2) has no FFI seam of its own (`#![deny(unsafe_code)]`,
 * halo2_proofs/src/lib.rs:9).  The narrowest seam is the pair of free functions every MSM and FFT in
 * the crate funnels through -- `best_multiexp` (halo2_proofs/src/arithmetic.rs:143) and `best_fft`
 * (arithmetic.rs:192) -- plus the EvaluationDomain / Params wrappers directly above them.  Each entry
 * point below names the reference function whose body it replaces.  INTEGRATION.md shows the Rust
 * `extern "C"` block and shim a maintainer would add.
 *
 * Conventions
 *   field element : 4 x uint64_t little-endian limbs (32 bytes).
 *   affine point  : {x, y} = 8 x uint64_t (64 bytes); the identity is all-zero.
 *   Jacobian point: {X, Y, Z} = 12 x uint64_t (96 bytes); identity has Z = 0.  x = X/Z^2, y = Y/Z^3.
 *   `form`        : H2_FORM_MONTGOMERY -- limbs are in Montgomery form, R = 2^256: exactly the bytes a
 *                   Rust `Vec<Fp>` / `Vec<EpAffine>` holds in memory (zero-copy from pasta_curves);
 *                   H2_FORM_CANONICAL -- limbs are the canonical integer (`to_repr()` / `from_repr()`),
 *                   reachable from 100 % safe Rust.  Applies to inputs and outputs alike.
 *   curve id      : H2_PALLAS (coordinates in Fp, scalars in Fq) / H2_VESTA (coordinates in Fq, scalars Fp).
 *   field id      : H2_FP / H2_FQ.
 *   pointers      : `const uint64_t *` arguments named h_* / plain are HOST memory, borrowed for the call;
 *                   `d_*` arguments are DEVICE (HBM) pointers on the current HIP device.  The library never
 *                   frees or retains caller memory (registered bases are copied to the device).
 *   return value  : H2_OK or an H2_ERR_* code; never aborts.  The reference panics on bad lengths
 *                   (arithmetic.rs:144, :205); the Rust shim turns H2_ERR_ARGS back into a panic.
 *   threading     : all entry points are thread-safe and re-entrant (internal per-device lock).
 *   results       : bit-exact with the reference as group / field elements: canonical affine (x, y) of
 *                   an MSM and every canonical NTT output element are identical to the CPU path's.
 */
#ifndef HALO2_MI355X_H
#define HALO2_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define H2_OK 0
#define H2_ERR_ARGS 1   /* bad argument (null pointer, length mismatch, log_n out of range, bad id) */
#define H2_ERR_HIP 2    /* a HIP runtime call failed; see h2_last_error() */
#define H2_ERR_NODEV 3  /* no gfx950 device / HIP runtime unavailable */
#define H2_ERR_HANDLE 4 /* unknown or freed handle */
#define H2_ERR_DECODE 5 /* a compressed point does not decode (where pasta_curves' from_bytes returns None) */
#define H2_ERR_LOOKUP 6 /* permute_expression_pair: an input value does not occur in the table (Error::ConstraintSystemFailure) */
#define H2_ERR_PEER 7   /* a split multiexp / commit: ANOTHER rank failed its range; no result is written (a partial sum would be a wrong point) */
#define H2_ERR_NOTFOUND 8 /* h2_ecc_fixed_tables_device: a window has no z below z_limit (find_zs_and_us returns None) */

#define H2_FP 0
#define H2_FQ 1
#define H2_PALLAS 0
#define H2_VESTA 1
#define H2_FORM_CANONICAL 0
#define H2_FORM_MONTGOMERY 1
#define H2_OUT_JACOBIAN 0 /* 12 limbs, what `best_multiexp` returns (`C::Curve`) */
#define H2_OUT_AFFINE 1   /* 8 limbs, what `to_affine()` / `batch_normalize` would give */

typedef uint64_t h2_bases_t; /* opaque handle to a device-resident basis (Params::g / g_lagrange) */

/* ---- library ------------------------------------------------------------------------------ */
int h2_device_count(void);
/* The HIP device current on the calling thread (what registrations and launches will use), or -1 without a device. */
int h2_current_device(void);
/* Binds the calling thread to `device` (hipSetDevice) and warms the per-device context. */
int h2_init(int device);
/* Human-readable description of the last failure on this thread (static storage). */
const char *h2_last_error(void);
/* Returns the library's cached device scratch (per-stream multiexp / NTT workspaces, twiddle tables) of the current
 * device to the allocator after a device-wide synchronise.  Registered bases stay.  A long-lived prover that used many
 * streams calls this between phases; everything is re-created on demand. */
int h2_trim(void);
/* Window width the MSM would use for n points (informational; the result does not depend on it). */
int h2_msm_window_bits(size_t n);
/* The same for a registered basis of n points (h2_bases_register / h2_commit); h2_commit_pair_device: see h2_commit_pair_supported. */
int h2_commit_window_bits(size_t n);
/* 1 if h2_commit_pair_device accepts a registered basis of n points (n >= 8192 and the sort geometry fits), else 0. */
int h2_commit_pair_supported(size_t n);
/* Tuning knobs (never change results).  "msm_lane_fraction" in (0.05, 1]: share of the resident wave slots
 * one bucket-accumulation launch claims; < 1 lets commits issued on other streams overlap it (default 1).
 * "host_commit_chunk": scalars per range of h2_commit's pipelined transfer (0 = default 2^18 = 8 MiB). */
int h2_set_option(const char *key, double value);

/* ---- MSM: replaces best_multiexp (halo2_proofs/src/arithmetic.rs:143-180) -------------------- */
/* out = sum_i scalars[i] * bases[i].  n may be 0 (identity).  `out_kind` selects 12- or 8-limb output. */
int h2_msm(int curve, const uint64_t *scalars, const uint64_t *bases_xy, size_t n, int form,
           int out_kind, uint64_t *out);

/* Params::{new,read} keep `g` / `g_lagrange` for the life of the Params (poly/commitment.rs:26-33):
 * register them once, commit many times. */
int h2_bases_register(int curve, const uint64_t *bases_xy, size_t n, int form, h2_bases_t *handle);
/* the same from `n` affine points already in device memory (work that produces them must have completed) */
int h2_bases_register_device(int curve, const void *d_bases_xy, size_t n, int form, h2_bases_t *handle);
/* the same with the table's window width chosen by the caller (0 = the library's choice, as h2_bases_register; 4 .. 20, wider
 * than 16 only where the two-pass sort fits: H2_ERR_ARGS otherwise).  h2_commit_column_window_bits(n) is the width to ask for
 * when the table only serves independent column commits (Params::g / g_lagrange): 17 bits from 2^18 points on -- a scalar has
 * 15 digits instead of 16 -- which h2_commit_pair_device and h2_ipa_collapsed_generators_device do not take. */
int h2_bases_register_ex(int curve, const uint64_t *bases_xy, size_t n, int form, int window_bits, h2_bases_t *handle);
int h2_commit_column_window_bits(size_t n);
/* `Params::w` (poly/commitment.rs:26-33): installs the multiples of the affine point w_xy as the blind column of the handle's
 * table.  Compared by content with what the handle holds: the same point is a no-op, a different one waits for the device to
 * drain (commits with the old w may be in flight), installs it and returns when the column is complete.  Host pointer, blocking. */
int h2_bases_set_blind_base(h2_bases_t handle, const uint64_t *w_xy, int form);
/* What a handle holds: the number of registered points, the window width of its table, its curve (any pointer may be NULL). */
int h2_bases_info(h2_bases_t handle, size_t *n, int *window_bits, int *curve);
/* 1 if the handle has a blind base installed (h2_bases_set_blind_base, or a w_xy presented to a commit), 0 if not, a negative
 * status for a dead handle.  The rank-independent precondition of a blinded commit that is split over GPUs: every rank checks it
 * BEFORE entering the exchange step, so that either all ranks fail or none waits in a collective for one that never arrives. */
int h2_bases_blind_base_set(h2_bases_t handle);
int h2_bases_free(h2_bases_t handle);

/* replaces Params::commit / commit_lagrange (halo2_proofs/src/poly/commitment.rs:119-150):
 * out = sum_{i<n} scalars[i]*g[i] + blind*w.  The reference copies poly+blind and g+w into fresh
 * (n+1)-vectors per call; here g stays on the device and (w, blind) ride along.  `w_xy` / `blind`
 * may both be NULL for a plain MSM over the first n registered bases (IPA rounds,
 * poly/commitment/prover.rs:107-108); `blind` alone uses the handle's blind base (h2_bases_set_blind_base); a `w_xy` is compared
 * by content with it and installed first when it differs.  The column crosses PCIe in ranges that are committed as they land
 * (copy stream + two compute streams), so the transfer runs beside the bucket arithmetic. */
int h2_commit(h2_bases_t g, const uint64_t *scalars, size_t n, const uint64_t *w_xy,
              const uint64_t *blind, int form, int out_kind, uint64_t *out);

/* ---- NTT: replaces best_fft (halo2_proofs/src/arithmetic.rs:192-295) ------------------------- */
/* In place, natural order in and out: a[j] <- sum_i a[i] * omega^(i*j), n = 2^log_n, 0 <= log_n <= 32
 * (device memory permitting).  Reproduces the reference's butterfly network exactly, so the output
 * matches the CPU path for ANY omega, including the non-root omega of benches/fft.rs:17. */
int h2_ntt(int field, uint64_t *a, unsigned log_n, const uint64_t *omega, int form);

/* replaces EvaluationDomain::ifft (halo2_proofs/src/poly/domain.rs:375-383; lagrange_to_coeff :227):
 * best_fft with omega_inv, then every element times `divisor` (fused into the last pass). */
int h2_ifft(int field, uint64_t *a, unsigned log_n, const uint64_t *omega_inv, const uint64_t *divisor,
            int form);

/* replaces EvaluationDomain::coeff_to_extended (poly/domain.rs:241-255, :357-373):
 * out[i] = a[i] * {1, zeta, zeta^2}[i % 3] for i < 2^k, zero-extended to 2^ext_k, forward NTT with
 * extended_omega.  `a` has 2^k elements, `out` 2^ext_k (may not alias). */
int h2_coeff_to_extended(int field, const uint64_t *a, uint64_t *out, unsigned k, unsigned ext_k,
                         const uint64_t *g_coset, const uint64_t *g_coset_inv,
                         const uint64_t *extended_omega, int form);

/* replaces EvaluationDomain::extended_to_coeff (poly/domain.rs:303-325): inverse NTT of size 2^ext_k,
 * times extended_ifft_divisor, then a[i] *= {1, zeta^2, zeta}[i % 3].  In place; the caller truncates
 * to n*(degree-1) as the reference does (:321-322). */
int h2_extended_to_coeff(int field, uint64_t *a, unsigned ext_k, const uint64_t *g_coset,
                         const uint64_t *g_coset_inv, const uint64_t *extended_omega_inv,
                         const uint64_t *extended_ifft_divisor, int form);

/* replaces EvaluationDomain::divide_by_vanishing_poly (poly/domain.rs:329-348): a[i] *= t_evaluations[i mod nt]
 * over the extended domain (nt = 2^(ext_k - k) <= 4096 inverse vanishing-polynomial values, host memory). */
int h2_divide_by_vanishing_poly(int field, uint64_t *a, unsigned ext_k, const uint64_t *t_evaluations,
                                size_t nt, int form);

/* ---- device-resident variants (data already in HBM; `stream` is a hipStream_t or NULL) -------- */
/* Same contracts as above with device pointers; asynchronous on `stream`; outputs land in device
 * memory.  Used by batched provers and by bench.py (inputs resident in HBM before timing starts).
 * "Asynchronous on `stream`" is an ordering promise: everything a call enqueues runs behind what `stream` already holds and has
 * finished before anything enqueued on `stream` afterwards runs, work on the library's own streams included; no other stream and
 * no device-wide synchronise is needed around a call (tests/test_gpu_stream_order.py).  It is not a promise that the host never
 * waits: the entry points that say "synchronises `stream`" do, and so does h2_divide_by_vanishing_poly_device, which stages its nt
 * factors through a small per-stream buffer and waits for `stream` before and after that copy. */
int h2_msm_device(int curve, const void *d_scalars, const void *d_bases_xy, size_t n, int form,
                  int out_kind, void *d_out, void *stream);
/* Blind base: `Params::w` is a field of `Params`, fixed for its life (poly/commitment.rs:26-33, :102-103), and here a property of
 * the HANDLE: h2_bases_set_blind_base installs its multiples as one more column of the registered table.  A commit that passes
 * `d_blind` and NO `d_w_xy` uses that column (H2_ERR_ARGS if none was ever installed).  A commit may still present a `d_w_xy`:
 * its 64 BYTES -- never its address -- are compared with the installed point by one small kernel on `stream`, and only a
 * different point rebuilds the column (and becomes the handle's blind base); commits that use the old w on other streams
 * must have completed by then.  d_w_xy without d_blind: H2_ERR_ARGS.  Both NULL: no blind term. */
int h2_commit_device(h2_bases_t g, const void *d_scalars, size_t n, const void *d_w_xy,
                     const void *d_blind, int form, int out_kind, void *d_out, void *stream);
/* The commit restricted to registered bases [first, first + n): d_scalars[i] multiplies base first + i; d_blind (optional) adds
 * blind * (the handle's blind base).  One range of a commit split over GPUs or over the chunks of a host transfer. */
int h2_commit_range_device(h2_bases_t g, const void *d_scalars, size_t first, size_t n, const void *d_blind, int form,
                           int out_kind, void *d_out, void *stream);
/* TWO commits from one column over a registered basis of n points: column i < n - 4 feeds output (i >> pair_shift) & 1, the last
 * four columns feed outputs 0, 1, 0, 1.  This is one round of the opening argument written over the original generators
 * (poly/commitment/prover.rs:107-114): L_j and R_j have disjoint supports in g, so they share the scalar column produced by
 * h2_ipa_round_scalars_device (pass the same buffer for d_cl and d_cr), and the basis g || u || u || w || w carries the
 * [value z] U and [rand] W terms of each.  d_out: output 0 then output 1 (2 x 12 or 2 x 8 limbs).  n >= 8192. */
int h2_commit_pair_device(h2_bases_t g, const void *d_scalars, size_t n, unsigned pair_shift, int form, int out_kind,
                          void *d_out, void *stream);
/* `count` independent commits over one registered basis -- the column commits of a prover phase
 * (plonk/prover.rs:93-101, 301-313; vanishing/prover.rs:96-108).  d_scalars[i] / d_blinds[i] / d_outs[i] are
 * device pointers held in HOST arrays.  The library picks the faster of two forms by size and count: the COLUMN-BATCHED form --
 * one sort / accumulate / fold launch set for up to eight columns at a time, the column a grid dimension; a single group runs on
 * `stream` itself, several alternate over two internal streams -- or one commit per column spread over three internal streams
 * (many full-size columns: one column's sort / fold beside another's accumulate); either way the work is joined on `stream`.
 * d_blinds NULL: no blind term; d_blinds without d_w_xy: the handle's blind base; a d_w_xy is content-checked once, on
 * `stream`, as for h2_commit_device. */
int h2_commit_batch_device(h2_bases_t g, const void *const *d_scalars, size_t count, size_t n,
                           const void *d_w_xy, const void *const *d_blinds, int form, int out_kind,
                           void *const *d_outs, void *stream);
/* `count` independent multiexps over caller-supplied bases (e.g. the L_j / R_j pair of one opening-argument round,
 * halo2_proofs/src/poly/commitment/prover.rs:107-108), overlapped on internal streams and joined on `stream`.
 * Arrays of `count` device pointers / lengths; argument meaning per entry as h2_msm_device. */
int h2_msm_batch_device(int curve, const void *const *d_scalars, const void *const *d_bases_xy, const size_t *n,
                        size_t count, int form, int out_kind, void *const *d_outs, void *stream);
int h2_ntt_device(int field, void *d_a, unsigned log_n, const uint64_t *omega, int form, void *stream);
int h2_ifft_device(int field, void *d_a, unsigned log_n, const uint64_t *omega_inv,
                   const uint64_t *divisor, int form, void *stream);
/* `count` independent transforms of one size (the column FFTs of a prover phase, halo2_proofs/src/plonk/prover.rs:111-117,
 * 322-327) in one call: overlapped on internal streams, joined on `stream`.  d_a: array of `count` device pointers; each
 * vector is transformed in place as by h2_ntt_device / h2_ifft_device. */
int h2_ntt_batch_device(int field, void *const *d_a, size_t count, unsigned log_n, const uint64_t *omega, int form,
                        void *stream);
int h2_ifft_batch_device(int field, void *const *d_a, size_t count, unsigned log_n, const uint64_t *omega_inv,
                         const uint64_t *divisor, int form, void *stream);
int h2_coeff_to_extended_device(int field, const void *d_a, void *d_out, unsigned k, unsigned ext_k,
                                const uint64_t *g_coset, const uint64_t *g_coset_inv,
                                const uint64_t *extended_omega, int form, void *stream);
int h2_extended_to_coeff_device(int field, void *d_a, unsigned ext_k, const uint64_t *g_coset,
                                const uint64_t *g_coset_inv, const uint64_t *extended_omega_inv,
                                const uint64_t *extended_ifft_divisor, int form, void *stream);

int h2_divide_by_vanishing_poly_device(int field, void *d_a, unsigned ext_k, const uint64_t *t_evaluations,
                                       size_t nt, int form, void *stream);

/* Sum of `count` Jacobian points laid out contiguously (12 limbs each, Montgomery) -> one Jacobian
 * point.  The local step after the 96-byte all-gather of a range-split MSM (one partial per GPU). */
int h2_points_sum(int curve, const uint64_t *points_xyz, size_t count, uint64_t *out_xyz);
/* The same over device memory, asynchronous on `stream`; `form` applies to inputs and output, `out_kind` as for h2_msm. */
int h2_points_sum_device(int curve, const void *d_points_xyz, size_t count, int form, int out_kind, void *d_out, void *stream);

/* ---- several GPUs (no counterpart in the reference, whose create_proof is one process) ----------- */
/* The `count` independent column commits of a prover phase (plonk/prover.rs:93-101, 301-313; vanishing/prover.rs:96-108)
 * spread over `ndev` devices from ONE process: column i goes to devices[i % ndev], which holds handles[i % ndev] -- the same
 * bases registered once per device (h2_init(dev) + h2_bases_register on each).  Host columns in, host points out; one host
 * thread and three streams per device, no collective (a result is one point).  Blocking. */
int h2_commit_batch_multi(const h2_bases_t *handles, const int *devices, int ndev, const uint64_t *const *scalars,
                          size_t count, size_t n, const uint64_t *w_xy, const uint64_t *const *blinds, int form,
                          int out_kind, uint64_t *const *outs);
/* ONE multiexp (best_multiexp, arithmetic.rs:143) cut into ndev contiguous point ranges, one per device; the ndev partial
 * points (96 bytes each) are brought to devices[0] and added there.  Host pointers, blocking. */
int h2_msm_split_multi(int curve, const uint64_t *scalars, const uint64_t *bases_xy, size_t n, const int *devices,
                       int ndev, int form, int out_kind, uint64_t *out);
/* The same split for the one-process-per-GPU model: RCCL (bound with dlopen at first use) carries the exchange step.
 * Rank 0 calls h2_rccl_unique_id and hands the 128 bytes to the other ranks by whatever means its launcher offers
 * (a broadcast of its process group, MPI, a file); every rank then calls h2_rccl_init(id, rank, world) with its GPU current.
 * h2_msm_split_rccl_device: every rank passes the same device-resident problem; rank r multiplies points
 * [n r / world, n (r + 1) / world), ONE ncclAllGather of a 128-byte slot per rank (the 96-byte partial + a status word), and
 * every rank writes the total to d_out.  A rank whose range fails still enters the exchange with its status set: it returns its
 * own error and EVERY other rank returns H2_ERR_PEER -- nobody hangs, nobody sums the partials that did arrive.  The status read-back
 * synchronises `stream` once per call (the sum itself is enqueued behind it). */
int h2_rccl_unique_id(uint8_t id_out[128]);
int h2_rccl_init(const uint8_t id[128], int rank, int world);
int h2_rccl_finalize(void);
int h2_msm_split_rccl_device(int curve, const void *d_scalars, const void *d_bases_xy, size_t n, int form,
                             int out_kind, void *d_out, void *stream);
/* The same exchange for a commit over REGISTERED bases (Params::commit, an opening-argument round; BASELINE configs[4]'s
 * "RCCL-summed final commit"): every rank holds the table and the column, rank r commits table columns
 * [n r / world, n (r + 1) / world), the last rank carries the blind term (the handle's blind base), ONE ncclAllGather (128-byte
 * slots: partial + status, as above -- H2_ERR_PEER on every rank when any rank failed), every rank writes the total to d_out. */
int h2_commit_split_rccl_device(h2_bases_t g, const void *d_scalars, size_t n, const void *d_blind, int form, int out_kind,
                                void *d_out, void *stream);

/* ---- IPA round kernels (next to the MSMs inside commitment::create_proof) ----------------------- */
/* replaces parallel_generator_collapse (halo2_proofs/src/poly/commitment/prover.rs:154-166):
 * g holds 2*half affine points; on return g[i] = g[i] + [challenge] * g[half + i] for i < half, affine
 * (the caller truncates to `half`, :137).  `challenge` is a scalar-field element in `form`. */
int h2_generator_collapse(int curve, uint64_t *g_xy, size_t half, const uint64_t *challenge, int form);
int h2_generator_collapse_device(int curve, void *d_g_xy, size_t half, const uint64_t *challenge, int form,
                                 void *stream);
/* replaces the p' / b collapse loop (prover.rs:128-131): a[i] += a[half + i] * factor for i < half. */
int h2_fold_scalars(int field, uint64_t *a, size_t half, const uint64_t *factor, int form);
int h2_fold_scalars_device(int field, void *d_a, size_t half, const uint64_t *factor, int form, void *stream);
/* The scalars of round j's L_j / R_j multiexps (prover.rs:107-108) over the ORIGINAL generators instead of the collapsed
 * G': after j collapses G'[i] = sum_h s_j(h) * G[i + h * 2^(k-j)], where s_j(h) is the product of the challenges u_r, r < j,
 * selected by the bits of h (bit j-1-r <-> u_r; the products compute_s builds for the verifier, verifier.rs:156-172).  So with
 * m = h * 2^(k-j) + i and half = 2^(k-j-1):
 *     L_j = <p'_hi, G'_lo> = sum_m cl[m] * G[m],   cl[m] = p'[half + i] * s_j(h) for i <  half, else 0
 *     R_j = <p'_lo, G'_hi> = sum_m cr[m] * G[m],   cr[m] = p'[i - half] * s_j(h) for i >= half, else 0
 * Both become commits over a registered G (h2_commit_batch_device): every round costs two half-empty registered multiexps,
 * and the generator collapse (prover.rs:136-137, 2^(k-j-1) scalar multiplications per round) is never needed.
 * d_p: the current p' (2^(k-j) elements); challenges: u_0 .. u_{j-1} (host, `form`; may be NULL when j = 0);
 * d_cl, d_cr: 2^k elements each, in the form of d_p.  1 <= k <= 30, j < k. */
int h2_ipa_round_scalars_device(int field, const void *d_p, unsigned k, unsigned j, const uint64_t *challenges, int form,
                                void *d_cl, void *d_cr, void *stream);
/* Guard::use_challenges summed over a batch (poly/commitment/verifier.rs:35-41, compute_s :156-172; plonk/verifier/batch.rs:79-127):
 *   out[j] (+)= sum_{b < batch} coeffs[b] * prod_{i : bit i of j set} challenges[b*k + (k-1-i)],   0 <= j < 2^k
 * i.e. the sum of coeffs[b] * compute_s(u_b, 1).  challenges: batch*k scalars (proof-major, u_0..u_{k-1} in transcript order),
 * coeffs: batch scalars, both host memory in `form`; out / d_out: 2^k scalars in `form`.  accumulate = 0 overwrites, 1 adds.
 * 1 <= k <= 30, 1 <= batch <= 2^24.  With batch = 1 and coefficient 1 this is the s vector of Guard::compute_g (:22-33). */
int h2_ipa_s_combine(int field, unsigned k, size_t batch, const uint64_t *challenges, const uint64_t *coeffs, int form,
                     int accumulate, uint64_t *out);
int h2_ipa_s_combine_device(int field, unsigned k, size_t batch, const uint64_t *challenges, const uint64_t *coeffs, int form,
                            int accumulate, void *d_out, void *stream);
/* The whole round loop of commitment::create_proof (prover.rs:104-142) in one call, p' and b resident: per round the two inner
 * products (:109-110), the L_j / R_j scalars over the original generators (above), their commit, the two points to the
 * transcript (:121-122), the challenge and its inverse (:124-125), the p' / b folds (:128-133) and the blind bookkeeping
 * (:140-141).  The host is visited once per round -- L_j and R_j (192 bytes) land in pinned memory, are normalised with one
 * shared inversion and handed to the caller's transcript through the two TranscriptWrite methods the loop uses:
 *     write_point(user, xy)  the affine point, 8 x u64 Montgomery; returns H2_OK or an error the call passes on
 *     squeeze(user, out)     the next challenge scalar, 4 x u64 Montgomery, into out
 * Everything here is Montgomery form (the working form of resident vectors).
 *   paired != 0: `basis` is a registered g || u || u || w || w (2^k + 4 points; h2_commit_pair_supported) and each
 *                round is ONE h2_commit_pair_device over d_column_l (2^k + 4 scalars of scratch); d_column_r unused
 *   paired == 0: `basis` is a registered g || u || w (2^k + 2 points), each round two commits (h2_commit_batch_device) over
 *                d_column_l / d_column_r (2^k + 2 scalars of scratch each): any table size
 * d_p: p' (2^k scalars, folded in place; c_out receives the final p'[0]);  d_b: b, likewise;  z: the challenge of :66;
 * rands: l_0, r_0, l_1, r_1, ... (2k scalars, the order the reference draws them, :111-112);
 * f_out: sum_j (l_j u_j^-1 + r_j u_j), the amount the synthetic blinding factor grows by (:140-141).
 * switch_rounds = J > 0 (paired only, J < k, J <= 12, 16-bit window table): after J rounds the argument leaves the original
 *   generators -- G'_J is read off the table (h2_ipa_collapsed_generators_device), registered next to u and w (uw_xy: u then w,
 *   host, affine Montgomery) as a table of 2^(k-J) points, and the remaining rounds run over it: a round over the original
 *   generators costs a full-size commit whatever j, a round over G'_J a small one.  0 = never; H2_IPA_SWITCH_DEFAULT = the
 *   library's choice (h2_ipa_default_switch_rounds: from k = 16 on the rounds that leave a table of 2^14 points up to k = 20, six rounds at
 *   k = 21, five beyond).  Same L_j, R_j, so the same proof bytes.
 * Returns H2_ERR_ARGS if an L_j / R_j is the point at infinity or a challenge is zero (the reference errors / panics).
 * h2_ipa_rounds: the same with p' and b in host memory (copied in; only c and f leave the argument). */
#define H2_IPA_SWITCH_DEFAULT 0xFFFFFFFFu
typedef int (*h2_ipa_write_point_fn)(void *user, const uint64_t *xy);
typedef int (*h2_ipa_squeeze_fn)(void *user, uint64_t *challenge);
unsigned h2_ipa_default_switch_rounds(unsigned k, int paired);
int h2_ipa_rounds_device(int curve, unsigned k, unsigned switch_rounds, h2_bases_t basis, int paired, void *d_p, void *d_b,
                         const uint64_t *z, const uint64_t *rands, const uint64_t *uw_xy, void *d_column_l, void *d_column_r,
                         h2_ipa_write_point_fn write_point, h2_ipa_squeeze_fn squeeze, void *user, uint64_t *c_out,
                         uint64_t *f_out, void *stream);
int h2_ipa_rounds(int curve, unsigned k, unsigned switch_rounds, h2_bases_t basis, int paired, const uint64_t *p, const uint64_t *b,
                  const uint64_t *z, const uint64_t *rands, const uint64_t *uw_xy, h2_ipa_write_point_fn write_point,
                  h2_ipa_squeeze_fn squeeze, void *user, uint64_t *c_out, uint64_t *f_out);
/* replaces poly::commitment::prover::create_proof (halo2_proofs/src/poly/commitment/prover.rs:26-151) -- the whole opening
 * argument for p_poly at x_3 -- as ONE call: the function a Rust shim swaps, with the caller keeping what is the caller's (its rng
 * and its transcript).  Everything is Montgomery form.
 *   g_basis        Params::g registered with Params::w installed (h2_bases_set_blind_base): the commitment to s_poly (:56)
 *   opening_basis  g || u || u || w || w (paired != 0) or g || u || w (paired == 0), as for h2_ipa_rounds_device; switch_rounds,
 *                  uw_xy: as there
 *   p_poly         the 2^k coefficients (:41), read only;  p_blind (:38), x3 (:39): one scalar each (host)
 *   s_poly         2^k fresh random scalars, s_blind one more, rands the 2k blinds l_0, r_0, l_1, ... -- C::Scalar::random in the
 *                  order the reference draws them (:45-47, :53, :111-112).  h2_open_device overwrites d_s_poly (it becomes p' and is
 *                  folded in place); h2_open reads s_poly and p_poly from host memory, once each, and writes nothing back
 *   write_point    receives the commitment to s_poly (:57), then L_j, R_j per round (:121-122); squeeze yields xi (:62), z (:66),
 *                  then u_j per round (:124) -- the TranscriptWrite calls of the function, in its order
 *   c_out, f_out   the two scalars the caller writes last (:146-148): the final p'[0] and the synthetic blinding factor
 * The constant-coefficient corrections (:51, :72) happen on the device; b (:86-97) and v run beside the commitment to s_poly
 * (v = p_poly(x_3): s_poly(x_3) is exactly zero after :51).  Scratch (b, the round column, landing places for host vectors)
 * belongs to the (device, stream) context and goes back with h2_trim.  Same proof bytes as the reference for the same
 * randomness.  Errors: as h2_ipa_rounds_device; H2_ERR_ARGS also when g_basis has no blind base or a table has the wrong size --
 * all of that before anything reaches the transcript. */
int h2_open_device(int curve, unsigned k, h2_bases_t g_basis, h2_bases_t opening_basis, int paired, unsigned switch_rounds,
                   const uint64_t *uw_xy, const void *d_p_poly, const uint64_t *p_blind, const uint64_t *x3, void *d_s_poly,
                   const uint64_t *s_blind, const uint64_t *rands, h2_ipa_write_point_fn write_point, h2_ipa_squeeze_fn squeeze,
                   void *user, uint64_t *c_out, uint64_t *f_out, void *stream);
/* p_poly resident in HBM, the fresh s_poly where a host rng leaves it (what a prover that keeps its polynomials on the device has at this point):
 * s_poly crosses PCIe inside the call, in quarters, each committed as it lands (from k = 16 on). */
int h2_open_device_host_s(int curve, unsigned k, h2_bases_t g_basis, h2_bases_t opening_basis, int paired, unsigned switch_rounds,
                          const uint64_t *uw_xy, const void *d_p_poly, const uint64_t *p_blind, const uint64_t *x3, const uint64_t *s_poly,
                          const uint64_t *s_blind, const uint64_t *rands, h2_ipa_write_point_fn write_point, h2_ipa_squeeze_fn squeeze,
                          void *user, uint64_t *c_out, uint64_t *f_out, void *stream);
int h2_open(int curve, unsigned k, h2_bases_t g_basis, h2_bases_t opening_basis, int paired, unsigned switch_rounds,
            const uint64_t *uw_xy, const uint64_t *p_poly, const uint64_t *p_blind, const uint64_t *x3, const uint64_t *s_poly,
            const uint64_t *s_blind, const uint64_t *rands, h2_ipa_write_point_fn write_point, h2_ipa_squeeze_fn squeeze, void *user,
            uint64_t *c_out, uint64_t *f_out);
/* The generators after `rounds` collapses, without collapsing: G'[i] = sum_{h < 2^rounds} s(h) * G[i + h * 2^(k-rounds)] for
 * i < 2^(k-rounds), s(h) the challenge products of h2_ipa_round_scalars_device, read off the registered table of `basis` (its
 * first 2^k points are G; the table must use 16-bit windows, h2_commit_window_bits) as 2^(k-rounds) multiexps that share their
 * scalars: every 16-bit table digit as two signed 8-bit sub-digits, ~28 * 2^k mixed additions plus 512 full additions per output
 * for the bucket weights, no sort (csrc/msm.hip, ipa_readout_*).  With h2_bases_register_device this is how
 * h2_ipa_rounds_device moves to a 2^rounds times smaller table after its first rounds.
 * challenges: u_0 .. u_{rounds-1} in `form` (host); d_out_xy: 2^(k-rounds) affine points, Montgomery form.  rounds <= 12. */
int h2_ipa_collapsed_generators_device(h2_bases_t basis, unsigned k, unsigned rounds, const uint64_t *challenges, int form,
                                       void *d_out_xy, void *stream);

/* ---- the Fiat-Shamir transcript (host side) ------------------------------------------------------- */
/* replaces Blake2bWrite<_, C, Challenge255<C>> (halo2_proofs/src/transcript.rs:150-198, 286-296) for callers that want the
 * round loop above to stay in native code: BLAKE2b-512 personalised "Halo2-Transcript"; points are absorbed as canonical
 * (x, y) and written compressed (x with the sign of y in the top bit), scalars canonical little-endian; a challenge is the
 * digest of a copy of the state reduced from 512 bits into the curve's scalar field.  Inputs and challenges are Montgomery
 * limbs; `jacobian` != 0: the point is (X, Y, Z), 12 limbs, and is normalised first (the prover's .to_affine()).  Writing the
 * point at infinity returns H2_ERR_ARGS (the reference returns an io::Error, :209-214).  Host arithmetic only. */
typedef uint64_t h2_transcript_t;
int h2_transcript_new(int curve, h2_transcript_t *t);
int h2_transcript_free(h2_transcript_t t);
int h2_transcript_common_point(h2_transcript_t t, const uint64_t *point, int jacobian);
int h2_transcript_write_point(h2_transcript_t t, const uint64_t *point, int jacobian);
int h2_transcript_common_scalar(h2_transcript_t t, const uint64_t *scalar);
int h2_transcript_write_scalar(h2_transcript_t t, const uint64_t *scalar);
int h2_transcript_squeeze_challenge(h2_transcript_t t, uint64_t *challenge);
/* the bytes written so far (the proof): *len always receives their count, out is filled when cap >= *len */
int h2_transcript_bytes(h2_transcript_t t, uint8_t *out, size_t cap, size_t *len);
/* write_point / squeeze of h2_ipa_rounds_device over such a transcript: pass these with user = (void *)(uintptr_t)t */
int h2_transcript_cb_write_point(void *user, const uint64_t *xy);
int h2_transcript_cb_squeeze(void *user, uint64_t *challenge);

/* ---- Params set-up: Lagrange basis by an FFT over curve points -------------------------------- */
/* replaces the point FFT + 2^-k scaling + batch_normalize of Params::new
 * (halo2_proofs/src/poly/commitment.rs:77-100): out[j] = 2^-k * sum_i alpha_inv^(i*j) * g[i], affine, where
 * alpha_inv is the inverse 2^k-th root of unity of the curve's scalar field.  g and out hold 2^k points.
 * The device variant allocates its scratch per call and synchronises `stream` before it frees it: it returns with out complete. */
int h2_lagrange_basis(int curve, const uint64_t *g_xy, uint64_t *out_xy, unsigned k, int form);
int h2_lagrange_basis_device(int curve, const void *d_g_xy, void *d_out_xy, unsigned k, int form, void *stream);

/* ---- polynomial helpers between the commits and the transforms ------------------------------- */
/* Each replaces one O(n) field loop of the prover so a column can stay in HBM from witness to opening.
 * Vectors are n contiguous 32-byte elements in `form`; single field elements (`point`, `x`, `init`) are
 * host pointers in `form`; the *_device variants take device pointers for vectors and results. */
/* eval_polynomial (halo2_proofs/src/arithmetic.rs:298-303): out = sum_i poly[i] * point^i. */
int h2_eval_polynomial(int field, const uint64_t *poly, size_t n, const uint64_t *point, int form, uint64_t *out);
int h2_eval_polynomial_device(int field, const void *d_poly, size_t n, const uint64_t *point, int form, void *d_out,
                              void *stream);
/* compute_inner_product (arithmetic.rs:308-318): out = sum_i a[i] * b[i]; both vectors have n elements
 * (the reference panics on a length mismatch; the caller passes one n). */
int h2_inner_product(int field, const uint64_t *a, const uint64_t *b, size_t n, int form, uint64_t *out);
int h2_inner_product_device(int field, const void *d_a, const void *d_b, size_t n, int form, void *d_out, void *stream);
/* kate_division (arithmetic.rs:322-341): out[0 .. n-2] = quotient of a(X) by (X - point), remainder dropped.
 * n >= 1 (the reference underflows on an empty input); out must not alias a. */
int h2_kate_division(int field, const uint64_t *a, size_t n, const uint64_t *point, int form, uint64_t *out);
int h2_kate_division_device(int field, const void *d_a, size_t n, const uint64_t *point, int form, void *d_out, void *stream);
/* the `b` vector of the opening argument (poly/commitment/prover.rs:90-97): out[i] = x^i, i < n. */
int h2_powers(int field, const uint64_t *x, size_t n, int form, uint64_t *out);
int h2_powers_device(int field, const uint64_t *x, size_t n, int form, void *d_out, void *stream);
/* `s_poly * xi + p_poly` (poly/commitment/prover.rs:70): a[i] = a[i] * x + b[i]. */
int h2_scale_add(int field, uint64_t *a, const uint64_t *x, const uint64_t *b, size_t n, int form);
int h2_scale_add_device(int field, void *d_a, const uint64_t *x, const void *d_b, size_t n, int form, void *stream);
/* ff::BatchInvert as the grand products use it (plonk/permutation/prover.rs:118, plonk/lookup/prover.rs:297):
 * a[i] = 1 / a[i]; zeros are left zero. */
int h2_batch_invert(int field, uint64_t *a, size_t n, int form);
int h2_batch_invert_device(int field, void *d_a, size_t n, int form, void *stream);
/* batch_invert_assigned (halo2_proofs/src/poly.rs:135-180; plonk/keygen.rs:221, plonk/prover.rs:291): out[i] = num[i] / den[i] with
 * x / 0 = 0; a denominator equal to one stays out of the inversion, as the reference's Trivial values do.  den == NULL: every value is
 * trivial, out = num.  All columns of a proof go concatenated into one call (n_total elements).  out may alias num. */
int h2_assigned_to_field(int field, const uint64_t *num, const uint64_t *den, uint64_t *out, size_t n_total, int form);
int h2_assigned_to_field_device(int field, const void *d_num, const void *d_den, void *d_out, size_t n_total, int form, void *stream);
/* the running product of a permutation / lookup argument (plonk/permutation/prover.rs:147-153,
 * plonk/lookup/prover.rs:318-326): z[0] = init, z[i] = z[i-1] * m[i-1] for 0 < i < n.  m holds at least
 * n - 1 factors; z has n elements and must not alias m. */
int h2_grand_product(int field, const uint64_t *m, size_t n, const uint64_t *init, int form, uint64_t *z);
int h2_grand_product_device(int field, const void *d_m, size_t n, const uint64_t *init, int form, void *d_z, void *stream);

/* ---- selector compression (plonk/circuit/compress_selectors.rs:51-227), the parts that scale with the circuit ---- */
/* Activations are bit-packed: selector s owns the n_words = ceil(n / 32) words bits[s * n_words ...], row r is bit r % 32 of word
 * r / 32, bits past n are zero.  All pointers are device pointers.
 * h2_selector_conflicts_device: the exclusion matrix of `process` (:103-124) -- out[i * S + j] = 1 where selectors i and j are
 * both enabled on some row, else 0; symmetric, zero diagonal; S = n_selectors bytes per row.
 * h2_selector_combine_device: the combination assignments (:180-213) -- out_columns is n_columns vectors of n field elements
 * (Montgomery form), out_columns[c][r] = root_of_selector[s] for the one selector s with column_of_selector[s] == c that is
 * enabled on row r, else 0 (the conflict matrix guarantees there is at most one). */
int h2_selector_conflicts_device(const uint32_t *bits, size_t n_selectors, size_t n_words, uint8_t *out, void *stream);
int h2_selector_combine_device(int field, const uint32_t *bits, const uint32_t *root_of_selector, const uint32_t *column_of_selector,
                               size_t n_selectors, size_t n, void *out_columns, size_t n_columns, void *stream);

/* ---- expression evaluation between the coset FFTs and the quotient iFFT ----------------------- */
/* poly::Evaluator::evaluate (halo2_proofs/src/poly/evaluator.rs:129-228): one expression tree over registered
 * polynomials, evaluated element by element in a single kernel.  The tree arrives flattened in post-order as 32-bit
 * words `op | operand << 8`:
 *   H2_EV_POLY   operand = polynomial index; the NEXT word is the signed element shift (rotation * 1 for the Lagrange
 *                basis, * 2^(extended_k - k) for the extended basis; must be 0 in the coefficient basis, evaluator.rs:519).
 *                |shift| <= 2^log_len: the read wraps modulo the length, a shift of exactly the length is the identity as in
 *                the reference (Polynomial::get_chunk_of_rotated_helper asserts k <= len), a larger one is H2_ERR_ARGS
 *   H2_EV_CONST  operand = constant index (Ast::ConstantTerm)      H2_EV_LINEAR  operand = constant index (Ast::LinearTerm:
 *                value consts[c] * omega^i; the caller folds ZETA into the constant for the extended basis, :590-600)
 *   H2_EV_ADD, H2_EV_MUL (element-wise; Lagrange and extended bases, as in the reference: evaluator.rs:370-418), H2_EV_SCALE operand = constant index,
 *   H2_EV_MULADD operand = constant index of the base: one fold step acc * base + term of Ast::DistributePowers (:186-196)
 * basis: 0 coefficient, 1 Lagrange, 2 extended Lagrange.  consts: n_consts field elements, d_polys: n_polys device
 * vectors of 2^log_len elements, all in MONTGOMERY form (products of canonical-form data would not be canonical).
 * omega: the domain's (extended) root of unity, needed only when the program has a LINEAR node.  Stack depth <= 9. */
#define H2_EV_POLY 1
#define H2_EV_CONST 2
#define H2_EV_LINEAR 3
#define H2_EV_ADD 4
#define H2_EV_MUL 5
#define H2_EV_SCALE 6
#define H2_EV_MULADD 7
int h2_evaluate_device(int field, int basis, const uint32_t *program, size_t n_words, const uint64_t *consts, size_t n_consts,
                       const void *const *d_polys, size_t n_polys, unsigned log_len, const uint64_t *omega, void *d_out,
                       void *stream);

/* ---- lookup argument: the data-dependent step (plonk/lookup/prover.rs:557-647) ----------------------------------- */
/* `Vec<F>::sort()` as the prover uses it (:574): ascending by canonical value, in place.  n need not be a power of two. */
int h2_sort_device(int field, void *d_a, size_t n, int form, void *stream);
/* replaces permute_expression_pair over the `n` usable rows (the caller appends the blinding rows, :624-627):
 * permuted_input = the input values sorted ascending; permuted_table[i] = permuted_input[i] on the first row of every run
 * of equal input values, and the table values not consumed that way -- ascending -- on the repeated rows taken from the
 * last one up (the reference pops them off the end of its list, :617-622).  Returns H2_ERR_LOOKUP when an input value does
 * not occur in the table (Error::ConstraintSystemFailure, :609-611).  Synchronises `stream` (the status has to reach the
 * host).  Inputs are not modified; outputs hold n elements each and may not alias the inputs. */
int h2_permute_expression_pair_device(int field, const void *d_input, const void *d_table, size_t n, int form,
                                      void *d_permuted_input, void *d_permuted_table, void *stream);

/* ---- dev::MockProver::verify over device columns (halo2_proofs/src/dev.rs:576-904) ------------------------------- */
/* Finding failures is the RESULT of these three calls, not an error: they return H2_OK and leave bit planes (one bit per row,
 * row r = bit r % 64 of 64-bit word r / 64, ceil(2^log_len / 64) words per plane) and exact counts (uint32) in device memory.
 * None of them synchronises `stream`: the caller reads the counts back (one small copy) and fetches a plane only when its count
 * is not zero.  Planes and counts are overwritten, not accumulated.
 *
 * h2_check_expressions_device: n_programs programs in the bytecode of h2_evaluate_device (Lagrange basis; program p is the words
 * [prog_offsets[p], prog_offsets[p + 1]) of `programs`, all sharing `consts`), each evaluated at every one of the 2^log_len rows
 * with the poison tracking of dev.rs:104-156.  poly_is_advice[i] != 0 marks a registered vector as an advice column: its cell is
 * Poison where the row it is read at (after rotation, modulo the length) is >= usable_rows.  Negation (a SCALE) and ADD propagate
 * poison; MUL and SCALE turn Poison into Real(0) when the other factor is Real(0) / the constant 0.  H2_EV_MULADD b is
 * SCALE b of the accumulator, then ADD.  H2_EV_LINEAR is refused (a lowered gate has no such term); everything else is validated as
 * h2_evaluate_device validates a Lagrange-basis program (|shift| <= 2^log_len, stack depth <= 9).
 *   d_nonzero_bits, d_poison_bits: n_programs planes each; bit set where the program gives Real(x != 0) / Poison
 *   d_counts: 2 * n_programs uint32: set bits of program p's non-zero plane at [2p], of its poison plane at [2p + 1]
 *   d_values: null, or n_programs device vectors of 2^log_len elements that receive program p's value (Montgomery; 0 where poisoned) */
int h2_check_expressions_device(int field, const uint32_t *programs, const size_t *prog_offsets, size_t n_programs, const uint64_t *consts,
                                size_t n_consts, const void *const *d_polys, const uint8_t *poly_is_advice, size_t n_polys, unsigned log_len,
                                size_t usable_rows, void *d_nonzero_bits, void *d_poison_bits, void *d_counts, void *const *d_values,
                                void *stream);
/* Exact tuple membership (dev.rs:709-833): input row r < usable_rows fails iff (inputs[0][r], ..., inputs[w-1][r]) does not occur
 * among the tuples (tables[0][t], ..., tables[w-1][t]), t < usable_rows.  Tuples of canonical values are compared exactly; a
 * component whose bit is set in its poison plane (d_*_poison[c], layout above; a null plane = never poisoned) is one more value,
 * equal only to itself.  Vectors hold n >= usable_rows elements in `form`; any w >= 1.
 *   d_fail_bits: one plane of ceil(n / 64) words (rows >= usable_rows clear);  d_count: one uint32 */
int h2_lookup_check_device(int field, const void *const *d_inputs, const void *const *d_input_poison, const void *const *d_tables,
                           const void *const *d_table_poison, size_t w, size_t n, size_t usable_rows, int form, void *d_fail_bits,
                           void *d_count, void *stream);
/* Copy constraints (dev.rs:835-881): cell (c, r) of n_columns vectors of 2^log_len elements must equal the cell
 * d_mapping[c * 2^log_len + r] = c' * 2^log_len + r' (int64).  A cell of a column with column_is_advice[c] != 0 in a row
 * >= usable_rows is poisoned: equal to itself only.  A mapping entry outside the table fails its cell.
 *   d_fail_bits: n_columns planes;  d_counts: n_columns uint32 */
int h2_permutation_check_device(int field, const void *const *d_columns, const uint8_t *column_is_advice, size_t n_columns,
                                const void *d_mapping, unsigned log_len, size_t usable_rows, int form, void *d_fail_bits, void *d_counts,
                                void *stream);
/* Are the cells that enabled gates query assigned by the region that enabled them (dev.rs:581-641: CellNotAssigned and
 * InstanceCellNotAssigned)?  Host memory in, host memory out, synchronous, like h2_points_sum: the records come from a circuit's
 * synthesis on the host and the answer is read there.  2^log_len rows; a plane is a fixed or advice column, n_planes of them.
 *   ranges: n_ranges x (plane, first row, count, region): region `region` assigned `count` cells of the plane from `first row` on
 *   instance_lens: the number of values given for each of the n_instance instance columns; a cell past them is Padding
 *   event_rows / event_regions: every enabling of a selector, (absolute row, region), grouped by selector: those of selector s are
 *     [selector_offsets[s], selector_offsets[s + 1]); n_selectors + 1 offsets from 0
 *   pair_selector / pair_cell_offsets: n_pairs (gate, selector the gate queries) pairs; pair p checks, at every event of selector
 *     pair_selector[p], the cells [pair_cell_offsets[p], pair_cell_offsets[p + 1]) of `cells`; n_pairs + 1 offsets from 0
 *   cells: x (column code, rotation as int32); a column code is a plane index or 0x80000000 | instance column.  The cell of an
 *     event in row r lies in row (r + rotation) mod 2^log_len; a plane cell fails unless the event's region assigned it, an
 *     instance cell fails when its row is >= instance_lens[column]
 *   counts: n_pairs exact numbers of failing cells
 *   records: the first max_records failures in the order (pair, event, cell) as (pair, event index within its selector, cell index
 *     within its pair); *n_records of them are written
 *   n_conflicts: assignments that found their cell held by another region (no floor planner lets two regions share a cell; the
 *     answer means what the reference's means only when this is 0)
 * H2_ERR_ARGS, with every output untouched: a null pointer for an array that is not empty or for n_records / n_conflicts /
 * the offsets, log_len > 30, a range past 2^log_len, a plane >= n_planes, an event row >= 2^log_len, offsets that decrease or do
 * not start at 0, a selector, instance column or plane out of range, a total of range cells >= 2^32. */
int h2_cells_assigned_check(unsigned log_len, size_t n_planes, const uint32_t *ranges, size_t n_ranges, const uint64_t *instance_lens,
                            size_t n_instance, const uint32_t *event_rows, const uint32_t *event_regions, const size_t *selector_offsets,
                            size_t n_selectors, const uint32_t *pair_selector, const size_t *pair_cell_offsets, size_t n_pairs,
                            const uint32_t *cells, uint64_t *counts, uint32_t *records, size_t max_records, size_t *n_records,
                            uint64_t *n_conflicts);

/* ---- compressed points: the URS file and proof encoding --------------------------------------- */
/* pasta_curves `to_bytes` as Params::write uses it (halo2_proofs/src/poly/commitment.rs:169-181) and write_point
 * (transcript.rs:183-187): out[32 i ..] = x little-endian with the parity of y in bit 255; identity = 32 zero bytes.
 * Input: n affine points in `form`. */
int h2_points_compress(int curve, const uint64_t *xy, size_t n, int form, uint8_t *out_bytes);
int h2_points_compress_device(int curve, const void *d_xy, size_t n, int form, void *d_out_bytes, void *stream);
/* `from_bytes` as Params::read uses it (commitment.rs:184-205): one base-field square root per point.  Returns
 * H2_ERR_DECODE if any encoding is invalid (x >= p, x^3 + 5 not a square, or (0, odd)); those entries are zeroed.
 * The device variant synchronises `stream` to learn the verdict. */
int h2_points_decompress(int curve, const uint8_t *bytes, size_t n, int form, uint64_t *out_xy);
int h2_points_decompress_device(int curve, const void *d_bytes, size_t n, int form, void *d_out_xy, void *stream);

/* ---- hash-to-curve: `C::CurveExt::hash_to_curve(domain_prefix)` as Params::new calls it (poly/commitment.rs:52-62, :102-104) ---- */
/* out[i] = hash_to_curve(domain_prefix)(message i), affine; `count` messages of `msg_len` (<= 64) bytes each, contiguous.  The map
 * is pasta_curves' (BLAKE2b-512 XMD, simplified SWU on iso-Pallas / iso-Vesta, 3-isogeny: Zcash protocol specification 5.4.9.8);
 * Params::new(k) is count = 2^k messages {0, i as LE u32} plus {1} for w and {2} for u with the prefix "Halo2-Parameters". */
int h2_hash_to_curve(int curve, const char *domain_prefix, const uint8_t *msgs, size_t msg_len, size_t count, int form,
                     uint64_t *out_xy);
int h2_hash_to_curve_device(int curve, const char *domain_prefix, const void *d_msgs, size_t msg_len, size_t count,
                            int form, void *d_out_xy, void *stream);

/* ---- measurement aid (no reference counterpart) ------------------------------------------------ */
/* When enabled, the library brackets its dominant kernels with HIP events on the launching stream.
 * h2_profile_read drains them: slot 0 = MSM bucket accumulation, 1 = NTT passes (sum over the passes
 * of one transform counts as several launches), 2 = MSM recode+sort, 3 = MSM reduce+combine. */
#define H2_PROF_MSM_ACCUMULATE 0
#define H2_PROF_NTT_PASS 1
#define H2_PROF_MSM_SORT 2
#define H2_PROF_MSM_REDUCE 3
/* on = 1: every slot records; on = 2: only the dominant kernels (H2_PROF_MSM_ACCUMULATE, H2_PROF_NTT_PASS) -- an event pair costs the
 * launching stream ~10 us, and bench.py's timed region wants the accumulate's duration without paying for the sort's and the fold's;
 * on = 0: off. */
int h2_profile_enable(int on);
int h2_profile_read(int slot, double *total_ms, uint64_t *launches);
/* The same, plus `busy_ms`: the length of the union of the launch intervals since h2_profile_enable(1).  With launches
 * issued on several streams overlapping on the device, total_ms counts shared time once per launch; busy_ms is the time
 * the device spent on the kernel, so busy_ms / launches never exceeds the wall time per launch. */
int h2_profile_read_busy(int slot, double *total_ms, double *busy_ms, uint64_t *launches);
/* Profiling (h2_profile_enable(1) or (2)) and the timeline (H2_TIMELINE=1) never change a result, but they DO change the algorithm of a
 * generic multiexp (h2_msm_device without a registered basis): from 65536 scalars on every such call takes the plain two-pass sort
 * (H2_MSM_PATH_TWO_PASS below; the endomorphism split inside the sort), never the grouped form or the slice split, so that the
 * bracketed stages are the ones a single stream runs. */

/* The form the last generic multiexp (h2_msm_device / h2_msm_batch_device without a registered basis) enqueued on `stream` of the
 * current device took.  Host-side bookkeeping of the call that enqueued it: no device work, no synchronisation.  The calls of
 * h2_msm_batch_device run on the library's streams; the last of them is also recorded for the caller's `stream`.
 *   path         H2_MSM_PATH_*:
 *                ONE_PASS           one-pass counting sort (below 65536 scalars)
 *                TWO_PASS           two-pass sort, one accumulate (65536 .. 2^18 scalars; every size from 65536 under profiling / timeline)
 *                SLICE_SPLIT        two-pass sort, the upper and lower window slices accumulated in turn (sizes the grouped form declines)
 *                GROUPED_LATENCY    grouped form, a lone call: `groups` groups on the library's own streams (2^18 + 1 .. 5120255 scalars)
 *                GROUPED_THROUGHPUT grouped form, another stream's generic multiexp in flight: one group on `stream` (up to 2560127 scalars)
 *   groups       accumulate launches over disjoint window slices (1 for one pass / two pass, 2 for the slice split)
 *   acc_lanes    the largest lane count (threads) of the call's bucket-accumulation launches
 *   window_bits  the window width c
 * Any output pointer may be NULL.  H2_ERR_ARGS when no generic multiexp has been enqueued on that stream (the query creates nothing). */
#define H2_MSM_PATH_ONE_PASS 1
#define H2_MSM_PATH_TWO_PASS 2
#define H2_MSM_PATH_SLICE_SPLIT 3
#define H2_MSM_PATH_GROUPED_LATENCY 4
#define H2_MSM_PATH_GROUPED_THROUGHPUT 5
int h2_msm_last_path(void *stream, int *path, int *groups, unsigned *acc_lanes, int *window_bits);
/* The same for commits over a REGISTERED basis (h2_commit*, h2_commit_range_device, h2_commit_pair_device, h2_commit_batch_device):
 * what the last one enqueued on `stream` of the current device decided before it launched anything, and which caller form wrapped it.
 * Host-side bookkeeping: no device work, no synchronisation.  h2_commit (host memory) has no stream: it records on stream NULL, the last
 * range's plan (add_only = 1) with fold_only / wide_reduce taken from the fold the ranges share.  h2_commit_batch_device records the
 * last group's (or column's) plan on the caller's `stream` whatever stream of the library ran it.
 *   caller        H2_COMMIT_CALLER_*:
 *                 DIRECT          h2_commit_device / h2_commit_range_device (and the library's own commits)
 *                 HOST_RANGE      h2_commit, one range
 *                 HOST_PIPELINED  h2_commit, `caller_count` ranges (add_only) and one fold (fold_only)
 *                 BATCH_COLUMNS   h2_commit_batch_device, `caller_count` column-batched groups of cols_first .. cols_last columns
 *                 BATCH_FORK      h2_commit_batch_device, one commit per column over `caller_count` columns
 *                 PAIR_TWO_PASS   h2_commit_pair_device, two bucket slices behind the two-pass sort
 *                 PAIR_SUBDIGIT   h2_commit_pair_device, the 8-bit sub-digit form (only c, W, m, T, lane_div, pair, lanes are filled)
 *   empty         1: nothing to sum, the identity was written and nothing else is filled; 2: an empty range of a host commit
 *   lanes         lanes of the accumulate kernel the device holds at once (T never exceeds it)
 *   c, W, m       window bits, digits per scalar, scalars incl. the blind;  K columns of the launch set;  T lanes of the accumulate,
 *                 which aims at lane_div entries per lane
 *   use_sort2     two-pass sort (s2_lowb low bucket bits per pass-1 bin, s2_nh bins, s2_side: the 16-bit side array, s2_s1_scalars
 *                 scalars per pass-1 workgroup, s2_bins_form: pass 2 as one launch), else the one-pass sort
 *   max_big       oversized pass-2 bins the chunked kernels take (0: their launches are skipped);  zero_in_sort: pass 2 clears the buckets
 *   fold9         the carry-free fold, else the 8 x 32 finisher;  wide_reduce: row / column sums in front of the 8 x 32 fold
 *   pair, joined, add_only, fold_only: two outputs from one column; the columns' sorted lists form one; a range that stops at its
 *                 buckets; the fold of buckets summed by such ranges
 * H2_ERR_ARGS when `out` is NULL or no registered commit has been enqueued on that stream (the query creates nothing). */
#define H2_COMMIT_CALLER_DIRECT 1
#define H2_COMMIT_CALLER_HOST_RANGE 2
#define H2_COMMIT_CALLER_HOST_PIPELINED 3
#define H2_COMMIT_CALLER_BATCH_COLUMNS 4
#define H2_COMMIT_CALLER_BATCH_FORK 5
#define H2_COMMIT_CALLER_PAIR_TWO_PASS 6
#define H2_COMMIT_CALLER_PAIR_SUBDIGIT 7
typedef struct h2_commit_plan {
    uint32_t caller, caller_count, cols_first, cols_last;
    uint32_t empty, lanes;
    uint32_t c, W, m, K, T, lane_div;
    uint32_t use_sort2, s2_lowb, s2_nh, s2_side, s2_s1_scalars, s2_bins_form, max_big, zero_in_sort;
    uint32_t fold9, wide_reduce, pair, joined, add_only, fold_only;
} h2_commit_plan_t;
int h2_commit_last_plan(void *stream, h2_commit_plan_t *out);
/* What the library did with the state it keeps BETWEEN calls, as process-wide counters that only rise (every device and stream together).
 * Host-side bookkeeping: no device work, no synchronisation, no effect on any result; a test reads them before and after a call to prove
 * which arm the call took.
 *   devbuf_epoch             (re)allocations and releases of the grow-only workspaces of every unit (what a captured graph is keyed by)
 *   host_msm_plain           h2_msm calls through the range pipeline (from 2^19 host points) that enqueued plain launches
 *   host_msm_captured        ... that captured the launch graphs of their shape (such a call replays them as well)
 *   host_msm_replayed        ... that replayed captured graphs
 *   host_msm_graphs_dropped  sets of captured graphs destroyed that a call could have replayed: another shape, a moved buffer, h2_trim
 *   ipa_table_registered     the opening argument's table of collapsed generators: registered anew,
 *   ipa_table_refilled       refilled in place (curve and size repeat on the stream),
 *   ipa_table_freed          freed (another curve or size, above 2^17 points at the end of the call, h2_trim)
 *   twiddle_built            twiddle tables built into the NTT's cache (the curve-point FFT shares it); twiddle_hits: look-ups it answered
 * H2_ERR_ARGS when `out` is NULL. */
typedef struct h2_debug_counters {
    uint64_t devbuf_epoch;
    uint64_t host_msm_plain, host_msm_captured, host_msm_replayed, host_msm_graphs_dropped;
    uint64_t ipa_table_registered, ipa_table_refilled, ipa_table_freed;
    uint64_t twiddle_built, twiddle_hits;
} h2_debug_counters_t;
int h2_debug_counters(h2_debug_counters_t *out);
/* ENVIRONMENT.  libhalo2_mi355x.so reads ONE environment variable, the diagnostic H2_TIMELINE below; it never changes a result (it does
 * change the form of a large generic multiexp, see above).  Every A/B switch and sweep knob of the experiments behind DESIGN_LOG.md is compiled out of this library (csrc/common.h,
 * ab_env()) and lives only in the laboratory build of the same sources (`make -C halo2_amd/csrc ab` -> build/ab/libhalo2_mi355x_ab.so)
 * that the A/B parity tests and bench/tools load; tests/test_abi_and_host.py holds the shipped binary to that.
 *
 * With H2_TIMELINE=1 in the environment every commit stamps the device clock (100 MHz) as its sort, accumulate
 * and reduce stages become runnable; this drains up to `cap` {clock, (stream id << 8) | stage} pairs, stage
 * 1 = sort, 2 = accumulate, 3 = reduce, 4 = done.  Returns the pair count, or -1 when the timeline is off. */
int h2_debug_timeline(unsigned long long *out, unsigned cap);

/* ---- Poseidon P128Pow5T3 (halo2_poseidon: width 3, rate 2, R_F = 8, R_P = 56, S-box x^5), batched ---- */
/* All pointers are device pointers; every element is 4 x u64 Montgomery limbs; one lane per permutation / message.  The constants
 * are those halo2_amd/poseidon_spec.py generates (csrc/poseidon_consts.inc).  Bad arguments -- an unknown field, a null pointer
 * with a nonzero count, a count above 2^30 -- return H2_ERR_ARGS before anything touches the device; a count of 0 launches nothing.
 *
 * h2_poseidon_permute_device: d_states holds n states of 3 elements, d_out receives the n permuted states.  d_out may be d_states
 * (in place); any other overlap is not allowed. */
int h2_poseidon_permute_device(int field, const void *d_states, size_t n, void *d_out, void *stream);
/* h2_poseidon_hash_device: the reference's Hash<_, P128Pow5T3, ConstantLength<len>, 3, 2> of n messages of `len` elements each
 * (d_messages: n * len elements, message after message).  The state starts as (0, 0, len * 2^64); two elements are added to words 0
 * and 1 per permutation, the last block zero-padded; d_out[i] is word 0 after the last permutation of message i.  len = 0,
 * len >= 2^32 and n * len > 2^40 are H2_ERR_ARGS.  d_out must not overlap d_messages. */
int h2_poseidon_hash_device(int field, const void *d_messages, size_t n, size_t len, void *d_out, void *stream);
/* h2_poseidon_trace_device: the Pow5 chip's witness (halo2_gadgets poseidon/pow5.rs) of `count` permutations of the states in
 * d_states (3 elements each).  d_columns is ONE buffer of 4 vectors of 37 * count elements, one after the other: state0, state1,
 * state2, partial_sbox.  Rows 37 i .. 37 i + 36 of the state vectors belong to permutation i: row 0 the input, rows 1-4 the state
 * after full rounds 0-3, rows 5-32 after each pair of partial rounds, rows 33-36 after full rounds 60-63 (row 36 is the output).
 * Rows 37 i + 4 .. 37 i + 31 of partial_sbox hold (state0 + rc)^5 of the first round of that row's pair, before the MDS; its other
 * rows are zero.  Every one of the 4 * 37 * count elements is written.  d_columns must not overlap d_states. */
int h2_poseidon_trace_device(int field, const void *d_states, size_t count, void *d_columns, void *stream);

/* ---- Poseidon for any specification (halo2_poseidon Spec<F, T, RATE>: width 2 .. 12, S-box x^5), batched ---- */
/* The three entry points above with the width, the rate and the round counts taken at run time (csrc/poseidon_spec.hip); at
 * (3, 2, 8, 56) with P128Pow5T3's constants they give the same bytes.  The caller fills the descriptor.  d_constants is the CALLER's
 * device buffer of Montgomery elements (4 x u64 each): (full_rounds + partial_rounds) * width round constants, round after round,
 * then the width * width entries of the MDS matrix, row-major.  The library keeps no device memory for these calls -- no cached
 * table, no workspace -- and every launch goes on `stream`, which travels in the descriptor as an FFT plan carries its stream: the
 * calls are asynchronous on it and ordered by it alone, and d_constants must be complete on it.
 *
 * H2_ERR_ARGS before anything touches the device: a null spec; an unknown field; a width outside 2 .. H2_POSEIDON_MAX_WIDTH; a rate
 * outside 1 .. width - 1; full_rounds odd or below 2; full_rounds + partial_rounds above 1024; a null buffer (d_constants included)
 * with a nonzero count; a count above 2^30.  A count of 0 launches nothing. */
#define H2_POSEIDON_MAX_WIDTH 12
typedef struct h2_poseidon_spec {
    int field;                                   /* H2_FP or H2_FQ */
    unsigned width, rate, full_rounds, partial_rounds;
    const void *d_constants;
    void *stream;
} h2_poseidon_spec_t;
/* h2_poseidon_spec_permute_device: d_states holds n states of `width` elements, d_out receives the n permuted states.  d_out may be
 * d_states (in place); any other overlap is not allowed. */
int h2_poseidon_spec_permute_device(const h2_poseidon_spec_t *spec, const void *d_states, size_t n, void *d_out);
/* h2_poseidon_spec_hash_device: Hash<_, S, ConstantLength<len>, T, RATE> of n messages of `len` elements each (d_messages: n * len
 * elements, message after message).  The state starts as zeros with len * 2^64 in word `rate`; `rate` elements are added to words
 * 0 .. rate - 1 per permutation, the last block zero-padded; d_out[i] is word 0 after the last permutation of message i.  len = 0,
 * len >= 2^32 and n * len > 2^40 are H2_ERR_ARGS.  d_out must not overlap d_messages. */
int h2_poseidon_spec_hash_device(const h2_poseidon_spec_t *spec, const void *d_messages, size_t n, size_t len, void *d_out);
/* h2_poseidon_spec_trace_device: the witness of Pow5Chip<F, WIDTH, RATE> for `count` permutations; an odd partial_rounds is
 * H2_ERR_ARGS (the chip lays two partial rounds on a row).  With rows = full_rounds + partial_rounds / 2 + 1, d_columns is ONE buffer of
 * width + 1 vectors of rows * count elements, one after the other: state0 .. state(width - 1), partial_sbox.  Rows rows * i ..
 * rows * i + rows - 1 of the state vectors belong to permutation i: row 0 the input, rows 1 .. full_rounds / 2 the state after the
 * first full rounds, one row after each pair of partial rounds, then the last full rounds, the output on row rows - 1.  The
 * partial_sbox cell of a partial row holds (state0 + rc)^5 of the first round of that row's pair, before the MDS; its other rows
 * are zero.  Every one of the (width + 1) * rows * count elements is written.  d_columns must not overlap d_states. */
int h2_poseidon_spec_trace_device(const h2_poseidon_spec_t *spec, const void *d_states, size_t count, void *d_columns);

/* ---- Sinsemilla over Pallas (Zcash protocol specification 5.4.1.9; K = 10, C = 253), batched ---- */
/* One lane per message.  q_xy is the domain's Q in HOST memory; d_table the 1024 points S(j) = hash_to_curve("z.cash:SinsemillaS")
 * (j as 4 bytes LE) in device memory; both Montgomery affine (8 limbs a point).  Every addition is the specification's INCOMPLETE
 * addition: a message whose chain Acc <- (Acc + S(m_i)) + Acc meets equal or opposite operands (or starts from the identity) gets
 * d_status[i] = 1 (one byte per message; the reference's bottom) where every other message gets 0.
 *
 * h2_sinsemilla_hash_device: d_words holds n messages of `words` uint16 each, message after message; only the low 10 bits of a word
 * are read.  d_out_xy[i] is the Montgomery affine hash point of message i, zeros where d_status[i] = 1.  words = 0 returns Q;
 * words > 253, n > 2^30 or a null pointer with n > 0 are H2_ERR_ARGS. */
int h2_sinsemilla_hash_device(const void *d_words, size_t n, size_t words, const uint64_t *q_xy, const void *d_table, void *d_out_xy,
                              void *d_status, void *stream);
/* h2_sinsemilla_merkle_layer_device: MerkleCRH (specification 5.4.1.3) of n pairs: d_pairs holds n times (left, right), Montgomery
 * elements; message i is the 52 words  layer (10 bits) || left (255 bits) || right (255 bits), low bits first, cut on the lane.
 * d_out_x[i] is the x coordinate of its hash (Montgomery), zero where d_status[i] = 1.  layer >= 1024 is H2_ERR_ARGS.  d_out_x must
 * not overlap d_pairs. */
int h2_sinsemilla_merkle_layer_device(unsigned layer, const void *d_pairs, size_t n, const uint64_t *q_xy, const void *d_table,
                                      void *d_out_x, void *d_status, void *stream);
/* h2_sinsemilla_trace_device: the witness of SinsemillaChip::hash_message (halo2_gadgets sinsemilla/chip/hash_to_point.rs) for `count`
 * messages of one piece structure.  d_pieces: count * n_pieces CANONICAL field elements, message after message; piece k supplies
 * num_words[k] (1 .. 25, host memory) words, its low bits first; the sum of num_words is at most 253.  Each message takes
 * rows = sum(num_words) + 1 rows.  d_columns is ONE buffer of 5 vectors of rows * count Montgomery elements, one after the other,
 * in the order of the chip's advice columns: x_a, x_p, bits, lambda_1, lambda_2; rows i * rows .. (i + 1) * rows - 1 belong to
 * message i.  A word row holds the accumulator's x before the round, the x of S(word), the running sum z = piece >> 10 j of the
 * j-th word of its piece, and the two slopes; the last row holds the hash's x in x_a, its y in lambda_1, zeros elsewhere.  Every
 * element is written.  The rows of a message with d_status[i] = 1 are not a witness (a vanished denominator inverts to 0, as the
 * reference's Assigned does).  Scratch (32 bytes per row of at most 2^20 rows at a time) belongs to the (device, stream) context
 * and goes back with h2_trim.  Bad arguments are H2_ERR_ARGS. */
int h2_sinsemilla_trace_device(const void *d_pieces, size_t count, const uint32_t *num_words, size_t n_pieces, const uint64_t *q_xy,
                               const void *d_table, void *d_columns, void *d_status, void *stream);

/* ---- Variable-base scalar multiplication over Pallas (halo2_gadgets ecc/chip/mul.rs), batched ---- */
/* One lane per multiplication.  Points are Montgomery affine (8 limbs), the identity is (0, 0).
 *
 * h2_ecc_mul_device: n independent products d_out_xy[i] = [k_i] P_i (nothing is summed).  d_scalars holds n CANONICAL integers of 4
 * limbs, any value below 2^255 (bit 255 is ignored).  Complete: every scalar and base, the identity among them, gives the group's
 * answer.  d_status[i] (one byte) is 1 where P_i is neither the identity nor on the curve (the product of such a base is not
 * defined), 0 elsewhere.  n > 2^30 or a null pointer with n > 0 are H2_ERR_ARGS.
 *
 * h2_ecc_mul_trace_device: the witness of mul::Config::assign for `count` pairs (P_i, alpha_i), alpha a Montgomery element of Fp.
 * d_columns is ONE buffer of 10 vectors of 137 * count Montgomery elements, the chip's advice columns 0 .. 9 one after the other; rows
 * 137 i .. 137 i + 136 hold the region "variable-base scalar mul" of multiplication i: row 0 the complete addition P + P, rows 1 - 128
 * the two incomplete halves side by side over the bits of k = alpha + t_q (not reduced, most significant first), rows 129 - 134 the
 * three complete iterations, rows 135 - 136 the last bit; a cell the reference leaves unassigned is zero.  The product's coordinates
 * are columns 2 and 3 of row 136.  d_aux holds 16 Montgomery elements per multiplication, the overflow check's witnesses:
 * s = alpha + k_254 2^130, the 14 running sums s >> 10 j (j = 0 .. 13) of its range check, eta = inv0(z_130).  d_status[i] = 1 where a
 * denominator of the incomplete range vanished or P_i is the identity (for a point of the curve neither happens): those rows are
 * not a witness.  Scratch (32 bytes per element, 253 elements per multiplication, at most 2^23 elements at a time) belongs to the (device, stream) context and goes back
 * with h2_trim.  Bad arguments are H2_ERR_ARGS. */
int h2_ecc_mul_device(const void *d_bases_xy, const void *d_scalars, size_t n, void *d_out_xy, void *d_status, void *stream);
int h2_ecc_mul_trace_device(const void *d_bases_xy, const void *d_alphas, size_t count, void *d_columns, void *d_aux, void *d_status,
                            void *stream);

/* ---- Fixed-base scalar multiplication over Pallas (halo2_gadgets ecc/chip/constants.rs, mul_fixed.rs, mul_fixed/full_width.rs) ---- */
/* A fixed base B has four tables over its 3-bit windows; num_windows is 85 (NUM_WINDOWS) or 22 (NUM_WINDOWS_SHORT), any value from 2 to
 * 85 is accepted, another is H2_ERR_ARGS.  Points are Montgomery affine (8 limbs), the identity is (0, 0).
 *
 * h2_ecc_fixed_tables_device: compute_window_table, compute_lagrange_coeffs and find_zs_and_us of the base base_xy (HOST memory, 8
 * limbs) in one call; the four outputs are device buffers.  d_points: num_windows * 8 points, [w][k] = [(k + 2) 8^w]B for
 * w < num_windows - 1 and [k 8^w - sum_{j<w} 2^(3j+1)]B for the last window.  d_lagrange: num_windows * 8 Montgomery coefficients,
 * [w][c] the coefficient of X^c of the polynomial of degree 7 through (k, x(points[w][k])), k = 0 .. 7.  d_z: num_windows uint64, the
 * SMALLEST z >= 0 such that for all eight y of the window z + y is a square or zero and z - y is neither.  d_u: num_windows * 8
 * Montgomery elements with u^2 = y + z; the reference does not pin which root: it is the one this library's Tonelli-Shanks
 * (field_sqrt.cuh, fe_sqrt) returns, zero for zero.  z_limit is the exclusive bound on the candidates, 0 for the reference's
 * 1000 * 2^16; a window without a z below it makes the call return H2_ERR_NOTFOUND (the reference's None): d_points and d_lagrange
 * are then complete, d_z holds 2^64 - 1 for each such window and d_u is not written.  A base that is the identity, off the curve
 * or not reduced, and a null pointer, are H2_ERR_ARGS.  The search runs in rounds of 2^15 candidates per unfinished window and the
 * host reads the minima back after each, so the call returns with the stream idle and the tables complete.  Scratch (under 100 KB)
 * belongs to the (device, stream) context and goes back with h2_trim.
 *
 * h2_ecc_mul_fixed_device: n products d_out_xy[i] = [k_i]B from d_points, one lane each.  d_scalars holds n CANONICAL integers of 4
 * limbs of which only the low 3 * num_windows bits are read (any value below 2^255 at 85 windows, as h2_ecc_mul_device).  The sum is
 * the reference's, sum_{w < nw-1} points[w][k_w] + points[nw-1][k_(nw-1)], its last addition complete: k = 0 gives (0, 0).  n > 2^30
 * or a null pointer with n > 0 are H2_ERR_ARGS.
 *
 * h2_ecc_mul_fixed_trace_device: the witness of mul_fixed::Config::assign_region_inner for `count` scalars (as above), and of the
 * complete addition full_width::Config::assign closes with.  d_columns is ONE buffer of 6 vectors of num_windows * count Montgomery
 * elements, the chip's advice columns 0 .. 5 one after the other: x_p, y_p, x_qr, y_qr, window, u.  Rows num_windows i .. belong to
 * multiplication i; row w holds points[w][k_w] in x_p, y_p, k_w in window, u[w][k_w] in u; rows 1 .. nw-2 hold the accumulator before
 * the row's incomplete addition in x_qr, y_qr, row nw-1 the accumulator after the last one, and row 0 zeros there (the reference
 * assigns nothing).  Every element is written.  d_aux holds 11 Montgomery elements per multiplication: the complete addition's row
 * x_p, y_p (the last window's point), x_qr, y_qr (the accumulator), lambda, alpha, beta, gamma, delta (add.rs), then the product's x
 * and y.  Scratch (32 bytes per element, num_windows - 2 elements per multiplication, at most 2^23 elements at a time: 101 067
 * multiplications of 85 windows a chunk) belongs to the (device, stream) context and goes back with h2_trim.  Bad arguments are
 * H2_ERR_ARGS. */
int h2_ecc_fixed_tables_device(const uint64_t *base_xy, unsigned num_windows, uint64_t z_limit, void *d_points, void *d_lagrange, void *d_z,
                               void *d_u, void *stream);
int h2_ecc_mul_fixed_device(const void *d_points, unsigned num_windows, const void *d_scalars, size_t n, void *d_out_xy, void *stream);
int h2_ecc_mul_fixed_trace_device(const void *d_points, const void *d_u, unsigned num_windows, const void *d_scalars, size_t count,
                                  void *d_columns, void *d_aux, void *stream);

/* ---- Sinsemilla commitments and hashing from a private point (halo2_gadgets src/sinsemilla.rs CommitDomain; specification 5.4.8.4) ---- */
/* The conventions are those of the Sinsemilla and fixed-base entries above: Montgomery affine points of 8 limbs, the identity (0, 0),
 * one lane per message.  n or count above 2^30, words > 253 and a null pointer with n > 0 are H2_ERR_ARGS.
 *
 * h2_sinsemilla_hash_from_device: h2_sinsemilla_hash_device with the initial point of message i read from d_q_xy[i] (device memory, n
 * points): the reference's hash_to_point_with_private_init.  d_status[i] = 1 and a zero point where the chain meets an exceptional
 * addition or Q_i is the identity.
 *
 * h2_sinsemilla_commit_device: d_out_xy[i] = SinsemillaHashToPoint(Q, M_i) + [r_i]R in one launch.  Exactly one of q_xy (HOST memory, one Q
 * shared by all messages) and d_q_xy (device memory, one Q per message) is non-null; anything else is H2_ERR_ARGS.  d_r_points is the
 * 85 * 8 window table of R as h2_ecc_fixed_tables_device writes it; d_scalars holds n CANONICAL integers of 4 limbs read as
 * h2_ecc_mul_fixed_device reads them (255 bits, not reduced).  The final addition is the group's: M = [r]R gives the double,
 * M = -[r]R gives (0, 0) with status 0, r = 0 gives M.  d_status[i] = 1 and a zero point mean only that the HASH is bottom.
 *
 * h2_sinsemilla_trace_from_device: the witness of hash_message_with_private_init, and of a hash from a public Q on a chip configured
 * with allow_init_from_private_point (sinsemilla/chip/hash_to_point.rs:117-121, :179-182), for `count` messages of one piece
 * structure (d_pieces, num_words, n_pieces as h2_sinsemilla_trace_device) from the points d_q_xy[i] (device memory).  Each message
 * takes rows = sum(num_words) + 2 rows of the five columns x_a, x_p, bits, lambda_1, lambda_2: row 0 holds y_Q in x_p and zeros in
 * the other four (the reference assigns nothing there), rows 1 .. are the rows h2_sinsemilla_trace_device writes from Q_i.  Every
 * element is written.  Scratch (32 bytes per row but the first, at most 2^20 / rows messages at a time) belongs to the (device,
 * stream) context and goes back with h2_trim.
 *
 * h2_ecc_add_trace_device: n complete additions P_i + Q_i (ecc/chip/add.rs), each with its witness row.  d_aux holds 11 Montgomery
 * elements per addition in the order of h2_ecc_mul_fixed_trace_device's d_aux: x_p, y_p, x_qr, y_qr, lambda, alpha, beta, gamma,
 * delta, then the sum's x and y; the inverses are inv0 (zero for zero).  Every branch is covered: P + P, P + (-P), either operand or
 * both the identity.  d_aux must not overlap the inputs. */
int h2_sinsemilla_hash_from_device(const void *d_words, size_t n, size_t words, const void *d_q_xy, const void *d_table, void *d_out_xy,
                                   void *d_status, void *stream);
int h2_sinsemilla_commit_device(const void *d_words, size_t n, size_t words, const uint64_t *q_xy, const void *d_q_xy, const void *d_table,
                                const void *d_r_points, const void *d_scalars, void *d_out_xy, void *d_status, void *stream);
int h2_sinsemilla_trace_from_device(const void *d_pieces, size_t count, const uint32_t *num_words, size_t n_pieces, const void *d_q_xy,
                                    const void *d_table, void *d_columns, void *d_status, void *stream);
int h2_ecc_add_trace_device(const void *d_p_xy, const void *d_q_xy, size_t n, void *d_aux, void *stream);

/* ---- The K = 10 lookup range check (halo2_gadgets utilities/lookup_range_check.rs), its witness in bulk ---- */
/* One lane per OUTPUT ROW.  `field` is H2_FP or H2_FQ.  d_values holds `count` CANONICAL field elements of 4 limbs, as
 * h2_sinsemilla_trace_device takes its pieces; every output is a Montgomery element, the form of a cell.  d_status (one byte per value)
 * may be null.  count = 0 succeeds without a launch; count > 2^30 or a null d_values or d_rows with count > 0 are H2_ERR_ARGS.
 *
 * h2_range_check_trace_device: the running sums of LookupRangeCheck::range_check.  d_rows holds count * (num_words + 1) elements; rows
 * i (num_words + 1) .. i (num_words + 1) + num_words are z_0 .. z_W of value i, z_j = value >> 10 j as an integer: the reference's
 * z_{j+1} = (z_j - a_j) / 2^10 exactly, a_j being the j-th 10-bit word (the difference is a multiple of 2^10 below p).  d_status[i] = 1
 * where z_W != 0, i.e. value >= 2^(10 num_words), else 0; the rows are written either way (a non-strict check uses them).  num_words
 * outside 1 .. 25 (25 * 10 <= 254, the field's capacity) is H2_ERR_ARGS.
 *
 * h2_short_range_check_trace_device: the three rows of LookupRangeCheck::short_range_check.  d_rows holds 3 * count elements; rows 3 i,
 * 3 i + 1, 3 i + 2 are value, value * 2^(10 - num_bits) IN THE FIELD (a value above 10 bits still gets the product the gate "Short
 * lookup bitshift" checks) and the constant 2^-num_bits.  d_status[i] = 1 where the canonical value >= 2^num_bits, else 0.  The 4- and
 * 5-bit checks of LookupRangeCheck4_5BConfig consume rows 3 i alone; the same three rows are written regardless.  num_bits > 10 is
 * H2_ERR_ARGS. */
int h2_range_check_trace_device(int field, const void *d_values, size_t count, unsigned num_words, void *d_rows, void *d_status,
                                void *stream);
int h2_short_range_check_trace_device(int field, const void *d_values, size_t count, unsigned num_bits, void *d_rows, void *d_status,
                                      void *stream);

/* ---- Sinsemilla Merkle paths over Pallas (halo2_gadgets sinsemilla/merkle.rs, merkle/chip.rs, utilities/cond_swap.rs), batched ---- */
/* n paths of `depth` layers each (csrc/merkle_path.hip).  The caller fills the descriptor: q_xy is the domain's Q in HOST memory and
 * d_table the 1024 points S(j) in device memory, both Montgomery affine as the Sinsemilla entry points above take them.  The library
 * keeps NO device memory for these calls -- no workspace, no cached table -- and every launch goes on `stream`, which travels in the
 * descriptor as h2_poseidon_spec_t carries its stream: the calls are asynchronous on it and ordered by it alone, and every input must
 * be complete on it.  No two buffers of a call may overlap.
 *
 * H2_ERR_ARGS before anything touches the device: a null descriptor; a depth outside 1 .. 32 (the reference's leaf_pos is a u32);
 * n * depth above 2^30 (what h2_sinsemilla_trace_device accepts as its count); a null buffer with n > 0 (for the walk q_xy, always,
 * and d_table; the trace reads neither); for the trace layer_lo >= layer_hi or layer_hi > depth.  n = 0 launches nothing. */
typedef struct h2_merkle_paths {
    unsigned depth;                              /* 1 .. 32 */
    const uint64_t *q_xy;                        /* the domain's Q, HOST memory, Montgomery affine */
    const void *d_table;                         /* the 1024 points S(j), device memory */
    void *stream;
} h2_merkle_paths_t;
/* h2_sinsemilla_merkle_paths_device: the walk of MerklePath::calculate_root, one lane per path, ONE launch for all layers.  d_leaves:
 * n Montgomery elements; d_siblings: n * depth Montgomery elements, path after path, the sibling of layer 0 (the leaf's) first;
 * d_positions: n uint32_t.  d_nodes receives n * (depth + 1) Montgomery elements, path after path: node 0 is the leaf, node l + 1 =
 * MerkleCRH(l, left, right) with (left, right) = (sibling_l, node_l) where bit l of the position is set and (node_l, sibling_l)
 * where it is not, node `depth` the root.  d_status receives n * depth bytes: d_status[path * depth + l] = 1 where the chain of layer l
 * has no value (incomplete addition met equal or opposite operands), 0 elsewhere; node l + 1 is then 0 and the walk goes on from 0,
 * as the reference's test fold does.  Every element of d_nodes and every byte of d_status is written. */
int h2_sinsemilla_merkle_paths_device(const h2_merkle_paths_t *paths, const void *d_leaves, const void *d_siblings, const void *d_positions,
                                      size_t n, void *d_nodes, void *d_status);
/* h2_sinsemilla_merkle_trace_device: what MerkleChip::hash_layer and CondSwapChip::swap assign outside the 53-row hash region, for the
 * layers [layer_lo, layer_hi) of every path; d_nodes, d_siblings, d_positions as above (d_nodes as the walk wrote it).  With
 * layers = layer_hi - layer_lo there are count = n * layers items, item t = path * layers + (l - layer_lo).  With left and right the
 * CANONICAL values of the swapped pair, the three pieces are
 *     a = l | left[0..240) << 10,   b = left[240..250) | b_1 << 10 | b_2 << 15,   c = right[5..255),
 *     b_1 = left[250..255),  b_2 = right[0..5),  z1_a = a >> 10,  z1_b = b >> 10.
 * d_out is ONE buffer of 23 * count elements, whole column vectors one after the other (offsets in elements):
 *     [0, 5 count)          the swap rows, five vectors of count Montgomery elements: a (the node), b (the sibling), a_swapped
 *                           (left), b_swapped (right), swap (0 or 1)
 *     [5 count, 8 count)    the pieces, Montgomery: a, b, c of item t at 3 t, 3 t + 1, 3 t + 2
 *     [8 count, 18 count)   the rows of "Check piece decomposition", five vectors of 2 count Montgomery elements, the chip's advice
 *                           columns 0 .. 4: rows 2 t and 2 t + 1 of item t hold (a, z1_a), (b, z1_b), (c, b_1), (left, b_2), (right, l)
 *     [18 count, 21 count)  the pieces again as CANONICAL limbs: the (count, 3, 4) d_pieces of h2_sinsemilla_trace_device, whose
 *                           piece structure is 25, 2, 25 words
 *     [21 count, 23 count)  b_1, then b_2, count CANONICAL elements each: the values of the two 5-bit range checks
 * Every element is written. */
int h2_sinsemilla_merkle_trace_device(const h2_merkle_paths_t *paths, const void *d_nodes, const void *d_siblings, const void *d_positions,
                                      size_t n, unsigned layer_lo, unsigned layer_hi, void *d_out);

/* ---- Fixed-base multiplication by a running sum (halo2_gadgets ecc/chip/mul_fixed/short.rs, mul_fixed/base_field_elem.rs), batched ---- */
/* `count` multiplications over one base's tables, one lane each (csrc/ecc_fixed_sum.hip): the witness of the two fixed-base forms whose
 * scalar is decomposed by a running sum in the `window` column.  The caller fills the descriptor: d_points and d_u are the base's
 * tables as h2_ecc_fixed_tables_device writes them at num_windows windows, d_scratch is device memory of the CALLER's, 32 bytes per
 * element, for the inverses of the accumulators' denominators: num_windows - 2 elements per multiplication, and
 * scratch_elems / (num_windows - 2) multiplications go through per chunk, so any capacity from num_windows - 2 up gives the same
 * bytes.  The library keeps NO device memory for these calls and every launch goes on `stream`, which travels in the descriptor as
 * h2_merkle_paths_t carries its stream: the calls are asynchronous on it and ordered by it alone, every input must be complete on it,
 * and the scratch is free again once the call's work on the stream is done.  No two buffers of a call may overlap.
 *
 * The inputs are `count` CANONICAL elements of 4 limbs below p.  d_columns is ONE buffer of 6 vectors of (num_windows + 1) * count
 * Montgomery elements, the chip's advice columns 0 .. 5 one after the other: x_p, y_p, x_qr, y_qr, window, u.  Rows
 * (num_windows + 1) i .. belong to multiplication i.  Row w < num_windows holds points[w][k_w] in x_p, y_p and u[w][k_w] in u, and in
 * x_qr, y_qr what h2_ecc_mul_fixed_trace_device writes there: zeros on row 0, the accumulator before the row's addition on the others,
 * on row num_windows - 1 the one the complete addition starts from.  `window` holds the running sum: z_0 is the input and
 * z_(w+1) = (z_w - k_w) / 8 in Fp on rows 0 .. num_windows.  Row num_windows holds z_(num_windows) in `window` and zeros in the other
 * five.  Every element is written.
 *
 * h2_ecc_mul_fixed_short_trace_device (num_windows = 22): k_w is bits 3w .. 3w+2 of the LOW 64 bits of the magnitude, window 21 bit
 * 63 alone (decompose_word(magnitude, 64, 3)).  A magnitude below 2^64 has z_w = magnitude >> 3w and z_22 = 0; from 2^64 up the
 * recurrence is still the field's, z_22 != 0, and the circuit's constant constraint fails as the reference's negative tests expect.
 * d_signs holds `count` canonical elements.  d_aux holds 12 Montgomery elements per multiplication: the 11 of
 * h2_ecc_add_trace_device for (the last window's point) + (the accumulator), then the signed y: -y where the sign is p - 1, y for
 * every other sign, valid or not (short.rs:178-184); the identity's 0 stays 0.
 *
 * h2_ecc_mul_fixed_base_field_trace_device (num_windows = 85): k_w is bits 3w .. 3w+2 of the 255-bit alpha and z_85 = 0.  d_aux holds
 * 15 elements per multiplication: the same 11, then alpha_0' = alpha - (alpha >> 252) 2^252 + 2^130 - t_p (t_p = p - 2^254),
 * alpha_1 = alpha[252..254) and alpha_2 = alpha[254], Montgomery, and alpha_0' once more as CANONICAL limbs, the d_values of
 * h2_range_check_trace_device.
 *
 * H2_ERR_ARGS before anything touches the device: a null descriptor; a num_windows that is not the entry point's; count above 2^30;
 * with count > 0 a null buffer or scratch_elems < num_windows - 2.  count = 0 launches nothing. */
typedef struct h2_ecc_fixed_sum {
    unsigned num_windows;                        /* 22 for the short form, 85 for the base-field form */
    const void *d_points;                        /* num_windows * 8 points, as h2_ecc_fixed_tables_device writes them */
    const void *d_u;                             /* num_windows * 8 roots, likewise */
    void *d_scratch;                             /* the CALLER's device memory, 32 bytes per element */
    size_t scratch_elems;                        /* >= num_windows - 2 */
    void *stream;
} h2_ecc_fixed_sum_t;
int h2_ecc_mul_fixed_short_trace_device(const h2_ecc_fixed_sum_t *d, const void *d_magnitudes, const void *d_signs, size_t count,
                                        void *d_columns, void *d_aux);
int h2_ecc_mul_fixed_base_field_trace_device(const h2_ecc_fixed_sum_t *d, const void *d_alphas, size_t count, void *d_columns,
                                             void *d_aux);

#ifdef __cplusplus
}
#endif
#endif /* HALO2_MI355X_H */
