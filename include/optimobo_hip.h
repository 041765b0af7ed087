/*
 * optimobo_hip.h — C-ABI of liboptimobo_hip.so, the MI355X (gfx950) hot path of
 * OptiMOBO's acquisition maximisation.
 *
 * The reference (aje220/OptiMOBO v0.2.1) is pure Python: its "boundary" is duck typing, not
 * an FFI.  Each entry point below replaces one arithmetic site of the reference (cited
 * file:line, relative to the reference root) and is bound from Python with ctypes
 * (optimobo_amd/_lib.py; INTEGRATION.md shows the binding a maintainer would add).
 *
 * Conventions
 *   - Every array argument named *_dev is a DEVICE pointer owned by the caller (e.g. a torch
 *     tensor's data_ptr()); fp64, C-contiguous.  Small fixed-size vectors (reference point,
 *     weights, bounds, scalarisation parameters) are HOST pointers read during the call.
 *   - Calls are asynchronous on the context's stream (omb_set_stream), except omb_argmax,
 *     omb_synchronize and omb_timing_read, which synchronise.  Device memory is allocated by
 *     omb_create, omb_set_gp, the omb_plan_* calls (geometry) and the fused-chain calls
 *     (workspace, grown on demand); a grow synchronises the stream first.
 *   - Return 0 (OMB_OK) on success or a negative OMB_E* code; omb_last_error() describes the
 *     last failure.  No C++ exception crosses the ABI.
 *   - One context per device; a context is not thread-safe; different contexts are
 *     independent.
 *   - Posterior moments are laid out objective-major: mu_dev[o * ld + i], var_dev likewise.
 */
#ifndef OPTIMOBO_HIP_H
#define OPTIMOBO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OMB_ABI_VERSION 1
#define OMB_MAX_OBJ 8      /* objectives held by one context */
#define OMB_MAX_DIM 256    /* n_var.  Up to 64 the fused / register-fragment kernels; 65..256 the wide path
                              (DP 128 / 256: GEMM-tiled cross terms over 16-dim slabs, the dense posterior) */
#define OMB_MAX_TRAIN 1024 /* n_train handled by the fused posterior kernel */
#define OMB_MAX_TRAIN_DENSE 16384 /* n_train of the GEMM-based posterior path used above OMB_MAX_TRAIN */
#define OMB_HVI_PATHS_CHUNK 262144 /* candidates per pass of the fused chain under an omb_plan_hvi_paths plan */
#define OMB_NONDOM_SETS 16         /* point sets of one omb_nondominated call */
#define OMB_NONDOM_POINTS 16777216 /* points per set of omb_nondominated (2^24) */
#define OMB_HV_POINTS 1024         /* kept rows per set of omb_hypervolume / omb_hypervolume_contrib */
#define OMB_HV_MAX_WORK 274877906944LL /* point tests (cells × kept rows × variants) of one such call (2^38) */

enum {
  OMB_OK = 0,
  OMB_EINVAL = -1,   /* bad argument */
  OMB_EHIP = -2,     /* HIP runtime error */
  OMB_ENOMEM = -3,   /* device allocation failed */
  OMB_ESTATE = -4,   /* objective not set (omb_set_gp) */
  OMB_EUNSUP = -5,   /* size outside what the kernels support */
  OMB_ENOTPD = -6    /* matrix not positive definite (Cholesky), even with the allowed jitter */
};

enum { OMB_KERNEL_MATERN52 = 0, OMB_KERNEL_RBF = 1 };
enum { OMB_EHVI_REFERENCE = 0, OMB_EHVI_TEXTBOOK = 1, OMB_EHVI_SIGMA = 2 };
enum { OMB_EI_PLAIN = 0, OMB_EI_PARETO = 1, OMB_EI_CONSTRAINED = 2 };

/* Scalarisation ids (optimobo/scalarisations.py:37-397) and their params[] layout. */
enum {
  OMB_SCAL_WS = 0,    /* WeightedSum                       params: -            */
  OMB_SCAL_TCH = 1,   /* Tchebicheff                       params: -            */
  OMB_SCAL_ATCH = 2,  /* AugmentedTchebicheff              params: alpha        */
  OMB_SCAL_MTCH = 3,  /* ModifiedTchebicheff               params: alpha        */
  OMB_SCAL_EWC = 4,   /* ExponentialWeightedCriterion      params: p            */
  OMB_SCAL_WN = 5,    /* WeightedNorm                      params: p            */
  OMB_SCAL_WPO = 6,   /* WeightedPower                     params: p            */
  OMB_SCAL_WPR = 7,   /* WeightedProduct                   params: -            */
  OMB_SCAL_PBI = 8,   /* PBI                               params: theta        */
  OMB_SCAL_IPBI = 9,  /* IPBI                              params: theta        */
  OMB_SCAL_QPBI = 10, /* QPBI                              params: theta, alpha, H */
  OMB_SCAL_APD = 11   /* APD                               params: FE, FE_max, gamma */
};

typedef struct omb_ctx omb_ctx;

int omb_abi_version(void);

/* Create a context on HIP device `device` (own non-blocking stream). */
int omb_create(int device, omb_ctx** out);
int omb_destroy(omb_ctx* ctx);
/* Run subsequent calls on `hip_stream` (a hipStream_t, e.g. torch's current stream;
 * NULL is the HIP null stream).  omb_use_own_stream restores the context's own stream. */
int omb_set_stream(omb_ctx* ctx, void* hip_stream);
int omb_use_own_stream(omb_ctx* ctx);
int omb_synchronize(omb_ctx* ctx);
const char* omb_last_error(const omb_ctx* ctx);

/* Device fault word.  The fused posterior kernel's waves hand K* chunks to each other through
 * LDS counters; every wait is bounded (by default 2^22 polls).  A wait that runs out — which
 * only a broken invariant can cause — marks the context's fault word (pinned host memory) and
 * lets the kernel finish.  The next call on the context that enters the library (and
 * omb_synchronize after its sync) then returns OMB_EHIP once, describing the fault: the moments
 * and acquisition values computed since the previous report are invalid.
 * The same bound limits the fused Cholesky steps' wait for the diagonal block (omb_cholesky,
 * omb_posterior_samples, the GP fit above n = 128): running out returns OMB_EHIP from that call.
 * omb_debug_set(ctx, OMB_DEBUG_SPIN_LIMIT, polls) changes the bound (tests force the path with 0).
 * omb_debug_set(ctx, OMB_DEBUG_COV_TABLE, 1) builds K(X, X) / K(X*, X*) (GP-fit state, posterior covariance) with
 * the posterior kernels' table-driven Matern transform instead of the polynomial exp (a parity check of that
 * transform near r = 0; default 0).
 * omb_debug_set(ctx, OMB_DEBUG_FUSED_CHAIN, m) picks how omb_eval_argmax[_sobol] with an EHVI-2D plan runs the
 * acquisition and the arg-max: 0 the EHVI launch, then the arg-max's passes; 1 one launch (the last workgroup at
 * an agent-scope ticket reduces: the ticket's same-address atomics serialise, 23 vs 13.5 µs at config 2);
 * 2 the EHVI launch reducing to one pair per workgroup, then the arg-max's second pass.  Bit-identical pair.
 * omb_debug_set(ctx, OMB_DEBUG_ARGMAX_PASSES, 1) runs the arg-max as one launch (the last workgroup to finish
 * reduces the per-workgroup pairs) instead of two (default 2: config 2 measured 719.6 vs 719.5 M candidates/s,
 * gpurun_out/r04_l; bit-identical pair).
 * omb_debug_set(ctx, OMB_DEBUG_CHOL_MODE, m) picks the Cholesky schedule of omb_cholesky / omb_posterior_samples /
 * omb_gp_fit_state: 0 auto (default: where A fits the persistent launch's 32-bit buffer offsets, the whole
 * factorisation in one persistent launch; else 1),
 * 1 one launch per step, 2 the same as 0; m + 4 runs schedule m with every cross-workgroup hand-off
 * an agent-scope release / acquire pair (the HIP memory model's guarantee; the default form — sc1 payloads, a vmcnt
 * wait and relaxed flags — is measured valid on gfx950), bitwise the same factor as schedule m; m + 8 has the persistent
 * launch's workers apply every trailing update as its own task instead of batching the far tiles' updates,
 * again bitwise the same factor.
 * omb_debug_set(ctx, OMB_DEBUG_TIMING_STRIDE, s) records omb_timing's events on every s-th chain only (default 1;
 * omb_timing_read then averages over the recorded chains), so that a timed loop carries fewer event records. *
 * Value 7 (round 5's OMB_DEBUG_POSTERIOR_PERSIST, a persistent-ring posterior kernel measured 2-5% slower at every
 * configuration) is retired: the library has one posterior kernel per shape, and omb_debug_set(ctx, 7, ·) fails.
 * omb_debug_set(ctx, OMB_DEBUG_COV_FUSED, 0) builds the posterior covariance as K(X*, X*) then the VᵀV update (two
 * launches) instead of one SYRK with K(X*, X*) in its epilogue (default 1; the same matrix to the ulp).
 * omb_debug_set(ctx, OMB_DEBUG_SELECT_SEQ, 1) makes omb_thompson_select walk the samples in order for B ≤ 64 too
 * (default 0: the picks in parallel rounds to their fixed point; the same picks).
 * omb_debug_set(ctx, OMB_DEBUG_SYRK_GLDS, 0) builds the posterior covariance's SYRK with the register-staged two-slab
 * pipeline instead of the three-stage direct-to-LDS one (default 1 where n_train % 16 = 0 and N is even; the same
 * matrix bit for bit).
 * omb_debug_set(ctx, OMB_DEBUG_BOXES_KD, 1) runs omb_ehvi_boxes_k / an omb_plan_ehvi_boxes_k plan with one wavefront
 * per candidate (omb_ehvi_boxes' kernel, instantiated for every k) where 9·k·C ≤ 8192, instead of the
 * candidate-blocked kernel (default 0; the same per-box products, another order of the sum: equal to rounding).
 * omb_debug_set(ctx, OMB_DEBUG_POSTERIOR_ALL_VAR, 1) makes the fused chain (omb_eval, omb_eval_argmax[_sobol]) compute
 * σ² of every objective of the plan.  By default (0) the chain's posterior computes σ² only of the objectives whose
 * variance the planned acquisition loads — objective 0 alone for reference-mode EHVI-2D, Monte-Carlo EHVI, expected
 * decomposition and the plain / Pareto EI, whose reference uses σ²₀ for every objective; all of them for the other
 * plans — and μ of the rest without the triangular product V = L⁻¹K*.  Values and arg-max pairs are bit-identical
 * either way; omb_posterior and omb_eval_grad always compute every σ².
 * omb_debug_set(ctx, OMB_DEBUG_POSTERIOR_MEAN_KERNEL, m) picks where μ of those masked objectives is computed when
 * n_var ≤ 8 and some n_train > 128: 1 (default) in a small kernel of its own (one wavefront per 16 candidates, no LDS
 * ring, no barriers) launched after the posterior kernel, which then covers the unmasked objectives only; 2 the same
 * kernel launched before it; 0 inside the posterior launch, by its mean-only workgroups.  μ is bit-identical.
 * omb_debug_set(ctx, OMB_DEBUG_PATHS_LIBCOS, 1) evaluates the sample paths' features (omb_paths_set, omb_paths_eval)
 * with the device library's cosine instead of the kernel's own reduction (default 0): the baseline the kernel's
 * cosine is measured against (tools/paths_timing.py); values agree to the cosines' rounding.
 * omb_debug_set(ctx, OMB_DEBUG_HVI_PATHS_CHUNK, c) sets the candidates per pass of the fused chain under an
 * omb_plan_hvi_paths plan (default OMB_HVI_PATHS_CHUNK; 0: one pass over all N, whose workspace is the whole
 * (k·S, N) matrix of path values).  Values and arg-max pairs are bit-identical for every c.
 * omb_debug_set(ctx, OMB_DEBUG_ARGMAX_PRUNE, m) picks how omb_eval_argmax[_sobol] runs under a reference-mode EHVI-2D
 * plan with s00 > 0, s01 > 0 and a sorted non-dominated front, no constraint or log modifier, n_var ≤ 8 and
 * n_train > 128: 1 (default) in two phases from 2^16 candidates on — the means of both objectives and from them an
 * upper bound of the acquisition for every candidate, the full posterior and the acquisition for the seed (the
 * candidate with the largest bound in each run of 256 consecutive candidates), and then only for the candidates
 * whose bound reaches the seed's best value; 3 the same at any batch size; 2 the earlier order at any batch size — the
 * seed is every 16th candidate, evaluated before the bound of the rest; 0 the dense chain.  The arg-max pair is
 * bit-identical.
 * omb_debug_set(ctx, OMB_DEBUG_ARGMAX_SCREEN, m) picks where that two-phase path takes the means its bound reads: 1
 * (default) from omb_posterior_screen's fp32-transform means with their margins folded into the bound as intervals, the
 * fp64 mean of objective 1 then computed only for the seed sample and the survivors; 0 from fp64 means of both
 * objectives for every candidate (for a model so ill-conditioned that the margins keep everything).  The arg-max pair
 * is bit-identical: only the fp64 kernels' values reach it.
 * omb_debug_set(ctx, OMB_DEBUG_ARGMAX_STAGED, m) picks the order of that path where the seed comes from the bound
 * (OMB_DEBUG_ARGMAX_PRUNE 1 or 3) and the screen is on: 1 (default) staged — the screen of objective 1 alone for every
 * candidate, a bound from it that holds for any mean of objective 0, the seed (the smallest screened mean of objective 1
 * in each run of 256 candidates) and a first list by that bound, and objective 0's screen and the full bound only for
 * that list; 0 both objectives' screen and the full bound for every candidate.  The staged order wins where objective 1's mean rules most candidates out; where objective 0 decides
 * (the first list keeps most of the batch) it costs an extra pass over the list — measured 1.9 % behind 0 at 2^20
 * candidates with the flagship's two objectives swapped, where the list keeps 83 % (8.4 % before the first list was
 * drawn by a cut, OMB_DEBUG_ARGMAX_CUT) — and 0 is the order to use.  The
 * arg-max pair is bit-identical (omb_argmax_stage_stats reports the lists' sizes).
 * omb_debug_set(ctx, OMB_DEBUG_ARGMAX_CUT, m) picks how the staged order draws that first list: 1 (default) by one
 * cut — objective 1's bound decreases in its one argument, the low end of the screened mean, so one workgroup solves
 * bound(m*) = the seed's best value once per call and a candidate is dropped where its low end is at least m*; 0 by
 * evaluating the bound for every candidate.  The lists agree but for candidates whose bound lies within 1e-7 of the
 * seed's best value, and the arg-max pair is bit-identical (omb_argmax_cut_stats reports m*). */
enum {
  OMB_DEBUG_SPIN_LIMIT = 1,
  OMB_DEBUG_COV_TABLE = 2,
  OMB_DEBUG_FUSED_CHAIN = 3,
  OMB_DEBUG_ARGMAX_PASSES = 4,
  OMB_DEBUG_CHOL_MODE = 5,
  OMB_DEBUG_TIMING_STRIDE = 6,
  OMB_DEBUG_COV_FUSED = 8,
  OMB_DEBUG_SELECT_SEQ = 9,
  OMB_DEBUG_SYRK_GLDS = 10,
  OMB_DEBUG_BOXES_KD = 11,
  OMB_DEBUG_POSTERIOR_ALL_VAR = 12,
  OMB_DEBUG_POSTERIOR_MEAN_KERNEL = 13,
  OMB_DEBUG_PATHS_LIBCOS = 14,
  OMB_DEBUG_HVI_PATHS_CHUNK = 15,
  OMB_DEBUG_ARGMAX_PRUNE = 16,
  OMB_DEBUG_ARGMAX_SCREEN = 17,
  OMB_DEBUG_ARGMAX_STAGED = 18,
  OMB_DEBUG_ARGMAX_CUT = 19
};
int omb_debug_set(omb_ctx* ctx, int what, int64_t value);

/* Fitted-GP state of objective `obj` — replaces the fitted GPy model
 * (GPRegression + Matern52(ARD) with noise fixed to 0, optimisers.py:223-231).
 *   X_dev     (n, d)  training inputs, unscaled
 *   lengthscale_host (d) ARD lengthscales ℓ;  variance = σ_f²
 *   alpha_dev (n)     woodbury vector (K + 1e-8 I)^-1 y
 *   Linv_dev  (n, n)  row-major inverse of the lower Cholesky factor of K + 1e-8 I.  Only the diagonal and the
 *                     entries below it are read: what lies above the diagonal (the other half of an in-place LAPACK
 *                     dpotrf / dtrtri result, say) is ignored by every consumer — posterior, covariance, gradients,
 *                     sample paths, append — which all see zeros there.
 * The context packs this into its own layout (Lp: MFMA-fragment order) on its stream. */
int omb_set_gp(omb_ctx* ctx, int obj, int kernel, int n, int d, const double* X_dev,
               const double* lengthscale_host, double variance, const double* alpha_dev,
               const double* Linv_dev);

/* K(X_train, X*) block of objective `obj` (GPy Stationary._scaled_dist + Matern52.K_of_r,
 * the first half of model.predict at util_functions.py:156): K_dev (n, N) row-major. */
int omb_kernel_block(omb_ctx* ctx, int obj, const double* Xc_dev, int64_t N, double* K_dev);

/* Posterior μ, σ² of objectives 0..n_obj-1 at N candidates Xc_dev (N, d)
 * (GPy PosteriorExact._raw_predict via model.predict, util_functions.py:155-158):
 * mu_dev/var_dev (n_obj, N).  Fused K-block generation + FP64-MFMA L^-1 K* + reductions for
 * n_train ≤ OMB_MAX_TRAIN; above it (≤ OMB_MAX_TRAIN_DENSE) candidate chunks go through the K block,
 * an FP64-MFMA GEMM V = L^-1 K* and a column reduction. */
int omb_posterior(omb_ctx* ctx, int n_obj, const double* Xc_dev, int64_t N, double* mu_dev,
                  double* var_dev);

/* Screened posterior mean of objectives 0..n_obj-1 at N candidates (n_var ≤ 8): mu_out_dev (n_obj, N) is μ̃, the mean
 * with the kernel transform of the fp64 squared distance evaluated in fp32 (native square root and exponential) and
 * summed in fp64 against the fp64 woodbury vector; eps_out_dev (n_obj, N) is a rigorous margin, |μ̃ − μ| ≤ ε against
 * omb_posterior's μ, finite and positive for finite inputs.  About half the cost of the fp64 mean; the arg-max chain's
 * two-phase path prunes with it (OMB_DEBUG_ARGMAX_SCREEN). */
int omb_posterior_screen(omb_ctx* ctx, const double* Xc_dev, int64_t N, int n_obj, double* mu_out_dev,
                          double* eps_out_dev);

/* omb_posterior_screen of objective `obj` alone for the candidates idx_dev[0 .. *count_dev − 1] (int32 indices into the
 * N candidates, *count_dev ≤ N, both on the device): μ̃ and ε go to mu_dev[idx], eps_dev[idx] (N each, the objective's
 * own row) with the bits omb_posterior_screen gives them; unlisted slots are left alone.  The staged arg-max path's
 * second screen (OMB_DEBUG_ARGMAX_STAGED). */
int omb_posterior_screen_list(omb_ctx* ctx, const double* Xc_dev, int64_t N, const int32_t* idx_dev,
                               const int32_t* count_dev, int obj, double* mu_dev, double* eps_dev);

/* EHVI for 2 objectives (util_functions.py:136-167 + EHVI_2D_aux :81-128).
 *   pf_sorted_dev (P, 2): Pareto front sorted by f2 ascending (util_functions.py:98)
 *   r_host (2): reference (max) point;  s00, s01: np.cov(cache) entries (per-solve constants)
 *   mode OMB_EHVI_REFERENCE: σA = σ²0·s00, σB = σ²0·s01, last stripe omitted (bug-compatible)
 *   mode OMB_EHVI_TEXTBOOK : σA = sqrt(σ²0), σB = sqrt(σ²1), all P+1 stripes (exact EHVI)
 *   mode OMB_EHVI_SIGMA    : var_dev holds (σA, σB) directly — EHVI_2D_aux(PF, r, μ, σ) itself */
int omb_ehvi2d(omb_ctx* ctx, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
               const double* pf_sorted_dev, int P, const double* r_host, double s00, double s01,
               int mode, double* out_dev);

/* EHVI_3D reference Monte-Carlo form (util_functions.py:170-214):
 *   out = mean_s max(0, Π_j(r_j − s_j) − hv_pf),  s = cache·sqrt(σ²0) + μ (util_functions.py:217-237)
 * raised_dev (N, int32, may be NULL) is set to 1 where pygmo's hypervolume would raise
 * (a sample outside the reference box); out is NaN there. */
int omb_ehvi3d_mc(omb_ctx* ctx, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
                  const double* cache_dev, int M, const double* r_host, double hv_pf, double* out_dev,
                  int32_t* raised_dev);
/* The same Monte-Carlo EHVI for any 2 ≤ k ≤ OMB_MAX_OBJ objectives (omb_ehvi3d_mc is k = 3): the
 * reference calls EHVI_3D for every n_obj != 2 (optimisers.py:245-248), and EHVI_3D's per-sample volume
 * is pygmo's k-D hypervolume([s]).compute(r) = Π_{j<k}(r_j − s_j) (util_functions.py:205-206; the 3-term
 * product of :204 is overwritten).  cache_dev (M, k) row-major, r_host (k), hv_pf = HV(PF, r) in k-D;
 * k·M ≤ 8192 (the cache is staged in LDS). */
int omb_ehvi_mc(omb_ctx* ctx, int k, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
                const double* cache_dev, int M, const double* r_host, double hv_pf, double* out_dev,
                int32_t* raised_dev);

/* Exact ("textbook") EHVI for k = 2 or 3 objectives — the exact value the Monte-Carlo
 * EHVI_3D (util_functions.py:170-214) estimates — from a disjoint box decomposition of the
 * non-dominated region (optimobo_amd.pareto.box_decomposition):
 *   coords_dev (k, C) f64: per objective a sorted grid [-inf, front values..., r_j] (padded)
 *   boxes_dev  (B, 2k) uint16: [lo_0, hi_0, lo_1, hi_1, ...] grid indices of each box
 *   EHVI = Σ_b Π_j E[(hi_j − max(Y_j, lo_j))⁺],  Y_j ~ N(μ_j, σ²_j) independent.
 * One wavefront per candidate; 9·k·C ≤ 8192 (grid and per-wave Φ/φ tables in LDS). */
int omb_ehvi_boxes(omb_ctx* ctx, int k, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
                   const double* coords_dev, int C, const uint16_t* boxes_dev, int B, double* out_dev);

/* The same exact EHVI for any 2 ≤ k ≤ OMB_MAX_OBJ objectives and box lists of up to 2^24 boxes (the k ≥ 4
 * decompositions of optimobo_amd.pareto.box_decomposition hold 10^3..10^5): arguments as omb_ehvi_boxes, boxes_dev
 * 4-byte aligned.  One workgroup per 8 (4, 2, 1: as the LDS budget allows) candidates tabulates their Φ/φ at the
 * k·C grid coordinates; each lane then reads a box's indices once from global memory and accumulates every
 * candidate's product; fixed-order reduction, so a candidate's value does not depend on N or on its place in the
 * batch.  Per box the product is omb_ehvi_boxes' term for term; the order of the sum over boxes differs.
 *   OMB_EINVAL  k outside [2, OMB_MAX_OBJ], B < 1, null or misaligned pointers
 *   OMB_EUNSUP  C < 2 or 3·k·C + 2·k + 4 > 8192 (one candidate's tables in 64 KiB of LDS), B > 2^24
 * Indices are not checked here (the list is on the device): omb_plan_ehvi_boxes_k checks them. */
int omb_ehvi_boxes_k(omb_ctx* ctx, int k, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
                     const double* coords_dev, int C, const uint16_t* boxes_dev, int B, double* out_dev);

/* Hypervolume improvement of N points over the front behind the same box decomposition — the σ → 0 limit of the exact
 * EHVI, and what a Thompson batch scores a joint posterior draw with:
 *   out_dev[i] = HVI(y_i) = Σ_b Π_j (hi_bj − max(y_ij, lo_bj))⁺
 * y_dev is objective-major like μ everywhere else: row j starts at y_dev + j·ld, point i is column i (ld ≥ N).
 * coords_dev (k, C) and boxes_dev (B, 2k) are exactly omb_ehvi_boxes_k's (leading −∞ column, uint16 index pairs,
 * 4-byte aligned).  One lane per point; LDS holds the k·C grid doubles alone, the box list (up to 2^24 boxes) is
 * streamed in list order.  The sum runs in slices of 1024 boxes, the slices added in slice order, so a point's value
 * is bitwise the same whatever N, its column or the launch shape (a small batch gives every slice a workgroup row of
 * its own and adds the stored sums in the same order).  Asynchronous on the context's stream.
 *   a NaN coordinate: NaN for that point; y_j ≥ r_j (+∞ included): exactly 0; −∞: inf or NaN
 *   OMB_EINVAL  k outside [2, OMB_MAX_OBJ], N < 0, B < 1, a null pointer, a pointer off its alignment (8 bytes; the
 *               box list 4), ld < N
 *   OMB_EUNSUP  C < 2, k·C > 8192 (the grid in 64 KiB of LDS), B > 2^24
 * in that order; N = 0 returns OMB_OK and writes nothing.  Indices are not checked (the list is on the device); one
 * past the grid reads the grid's last coordinate. */
int omb_hvi_boxes(omb_ctx* ctx, int k, const double* y_dev, int64_t ld, int64_t N, const double* coords_dev, int C,
                  const uint16_t* boxes_dev, int B, double* out_dev);

/* The mean hypervolume improvement over S sampled fronts: the Monte-Carlo integrand of the noisy EHVI (Daulton et al.
 * 2021) and, at k = 1, of the noisy EI (Letham et al. 2019), everything minimised.  Posterior sample path s
 * (omb_paths_set) evaluated at the training inputs gives a draw of the latent values there, hence a front (k = 1: a
 * best value b_s) and a box decomposition of its own; the same path at candidate i is jointly distributed with it:
 *   t_s(i) = Σ_{b in list s} Π_j (hi_bj − max(y_{j,s,i}, lo_bj))⁺,   out_dev[i] = ((…((0 + t_0) + t_1) + …) + t_{S−1}) / S
 * y_dev is omb_paths_eval's output: path s of objective j is row j·S + s, pitch ld ≥ N.  List s is rows
 * box_off_host[s] .. box_off_host[s+1] of boxes_dev (box_off_host: S + 1 HOST ints from 0; (box_off[S], 2k) uint16
 * index pairs, 4-byte aligned), over the grid coords_dev + s·k·C — the S grids (S, k, C), each with a leading −∞
 * column and padded with its last coordinate exactly like one omb_hvi_boxes grid.  At k = 1 list s is the single box
 * (−∞, b_s]: t_s = (b_s − y)⁺.  t_s is bitwise omb_hvi_boxes' value of list s on rows {j·S + s} (slices of 1024 boxes
 * counted from the list's own start, added in slice order); the paths are added in path order from 0.0 and the sum
 * divided once by S, unfused.  One lane per candidate; LDS holds the current path's k·C grid doubles; no atomics; a
 * candidate's value is bitwise the same whatever N, its column or the launch shape (a small batch gives every path a
 * workgroup row of its own and adds the stored t_s in the same order).  1 ≤ S ≤ 16: one path install.  Asynchronous.
 *   a NaN coordinate in any path: NaN for that candidate; y_j ≥ r_j in every path: exactly 0
 *   OMB_EINVAL  k outside [1, OMB_MAX_OBJ], S outside [1, 16], N < 0, a null grid / box list / offsets, offsets not
 *               increasing from 0 (an empty list included), a null y / out with N > 0, a pointer off its alignment
 *               (8 bytes; the box list 4), ld < N
 *   OMB_EUNSUP  C < 2, k·C > 8192 (one grid in 64 KiB of LDS), box_off[S] > 2^24
 * in that order; N = 0 returns OMB_OK and writes nothing.  Indices are not checked (the lists are on the device); one
 * past the grid reads the grid's last coordinate.  omb_hvi_boxes itself stays k ≥ 2. */
int omb_hvi_paths(omb_ctx* ctx, int k, int S, const double* y_dev, int64_t ld, int64_t N, const double* coords_dev,
                  int C, const int32_t* box_off_host, const uint16_t* boxes_dev, double* out_dev);
/* omb_hvi_paths with its gradient through the paths.  y_dev and dy_dev are omb_paths_grad's two outputs at the same
 * pitch ld (dy_dev[((j·S + s)·d + l)·ld + i] = ∂y_{j,s,i}/∂x_l, d = n_var in [1, 64]):
 *   ∂t_s/∂y_j = −Σ_b 1[lo_bj < y_j < hi_bj] Π_{l≠j} (hi_bl − max(y_l, lo_bl))⁺      (k = 1: −1[y < b_s])
 *   ∂t_s/∂x   = Σ_j ∂t_s/∂y_j · dy[j·S + s], j ascending;   ∂out/∂x = ((…(0 + ∂t_0) + …) + ∂t_{S−1}) / S
 * The inequalities are strict: a value exactly on a grid coordinate takes derivative 0 for that factor.  The sum over
 * boxes runs in omb_hvi_paths' slices of 1024 boxes from the list's own start, added in slice order.
 *   out_dev (N)               bitwise omb_hvi_paths' value
 *   grad_dev[l·ld + i]        ∂out_i/∂x_l
 *   t_dev (S, ld), tgrad_dev (S, d, ld)   the per-path t_s and ∂t_s/∂x; both NULL or both set
 * One lane per candidate walks a path's list (a workgroup row per path, the path's grid in LDS), one lane per
 * (candidate, dimension) chains and averages; no atomics; a candidate's results are bitwise the same whatever N, its
 * column or the launch shape.  Where the value is NaN every gradient entry of the candidate is NaN (per path: where
 * t_s is); where y_j ≥ r_j in every path every entry is exactly 0.  Asynchronous; the context's workspace is grown
 * on demand (a grow synchronises first).
 *   OMB_EINVAL  omb_hvi_paths' own, in its order; then d outside [1, 64], a NULL dy / grad with N > 0, exactly one of
 *               t_dev / tgrad_dev NULL, one of the four off its 8-byte alignment
 *   OMB_EUNSUP  omb_hvi_paths' own
 * N = 0 returns OMB_OK and writes nothing.  Plans are untouched: under omb_plan_hvi_paths omb_eval_grad stays
 * OMB_EUNSUP. */
int omb_hvi_paths_grad(omb_ctx* ctx, int k, int S, int d, const double* y_dev, const double* dy_dev, int64_t ld,
                       int64_t N, const double* coords_dev, int C, const int32_t* box_off_host,
                       const uint16_t* boxes_dev, double* out_dev, double* grad_dev, double* t_dev,
                       double* tgrad_dev);
/* omb_hvi_paths under constraints through sample paths (everything minimised, g ≤ 0 feasible).  y_dev is
 * omb_paths_eval's output over k + n_con slots: the objectives are slots 0..k−1, the constraint models slots
 * k..k+n_con−1, path s of slot o at row o·S + s, pitch ld.  Per path s and candidate i:
 *   ω(g)  = 1[g ≤ 0]                                                            eta = 0
 *         = 1/(1 + e^{g/η}) for g ≤ 0,  e^{−g/η}/(1 + e^{−g/η}) for g > 0         eta > 0 (a smoothed indicator)
 *   w_s   = ((1·ω(g_{0,s,i}))·ω(g_{1,s,i}))·…   in constraint order
 *   u_s   = t_s·w_s (one multiplication, unfused), exactly 0.0 where w_s == 0.0;  t_s bitwise omb_hvi_paths' t_s
 *   out_dev[i] = ((…((0 + u_0) + u_1) + …) + u_{S−1}) / S
 * flags = OMB_CON_VIOLATION (eta = 0 only): where w_s == 0, u_s = −((0 + max(g_0, 0)) + max(g_1, 0) + …) < 0, so a
 * feasible candidate (u_s ≥ 0) ranks above every infeasible one and the least total violation leads the infeasible
 * ones.  A NaN among the k + n_con values of path s makes u_s, and so out_dev[i], NaN; no other candidate is
 * affected.  At n_con = 0 out_dev is bitwise omb_hvi_paths'.  u_dev (S, ld), when not NULL, takes every u_s (row s,
 * pitch ld); out_dev (N) may then be NULL.  One lane per candidate as omb_hvi_paths; a wavefront whose candidates all
 * have w_s == 0 walks no box of list s, which changes no bit; no atomics; a candidate's values are bitwise the same
 * whatever N, its column or the launch shape.  Asynchronous.
 *   omb_hvi_paths' refusals, in its order (a NULL out_dev is not one of them here); then
 *   OMB_EINVAL  n_con < 0, eta negative or not finite, flag bits other than OMB_CON_VIOLATION, that flag with eta > 0,
 *               out_dev and u_dev both NULL with N > 0, u_dev off its 8-byte alignment
 *   OMB_EUNSUP  k + n_con > OMB_MAX_OBJ
 * N = 0 returns OMB_OK and writes nothing. */
#define OMB_CON_VIOLATION 1u
int omb_hvi_paths_con(omb_ctx* ctx, int k, int S, int n_con, const double* y_dev, int64_t ld, int64_t N,
                      const double* coords_dev, int C, const int32_t* box_off_host, const uint16_t* boxes_dev,
                      double eta, unsigned flags, double* out_dev, double* u_dev);

/* The non-dominated points of S independent point sets (everything minimised): the Pareto set of the posterior mean
 * over a candidate set (S = 1: the (k, N) layout of mu_dev) or of every sample path over it.  y_dev has omb_paths_eval's
 * layout: coordinate j of point i of set s is y_dev[(j·S + s)·ld + i].  a dominates b when a_j ≤ b_j for every j and
 * a_j < b_j for some j, in IEEE comparisons:
 *   mask_dev[s·ldm + i] = 1 when no point of set s dominates i and no coordinate of i is NaN, else 0   (i < N)
 *   count_dev[s]        = the number of ones in row s
 * Duplicates are all kept; −0.0 equals +0.0; ±∞ are ordinary values; a point with a NaN dominates nobody; k = 1 keeps
 * every occurrence of the minimum.  Mask bytes at columns ≥ N are not written.  A sieve (omb_pareto.hip): tile passes
 * drop, workgroup by workgroup, the points that another point of the same 1024 dominates and append the survivors to
 * a list (a slot counter with atomics: the order of a list changes no result), the final pass tests every remaining
 * survivor against all of them.  Filtering against survivors alone is exact (dominance on NaN-free points is a strict
 * partial order), so the mask is a function of the set alone: bitwise the same whatever ld, ldm, the launch shape and
 * the order of the lists.  N²·k comparisons at worst (every point non-dominated).
 * SYNCHRONISES: the survivor counts are read back after every tile pass (at most 4) to size the next launch; the
 * final pass is asynchronous.  Scratch is a context buffer grown on demand (8 bytes per point and set at most).
 * Touches no plan, no GP state and no paths.
 *   OMB_EINVAL  k outside [1, OMB_MAX_OBJ], S outside [1, OMB_NONDOM_SETS], N < 0, ld < N or ldm < N, a NULL
 *               count_dev, a NULL y_dev / mask_dev with N > 0, y_dev or count_dev off 8-byte alignment — in this order
 *   OMB_EUNSUP  N > OMB_NONDOM_POINTS
 * N = 0 returns OMB_OK and writes count_dev[s] = 0 only. */
int omb_nondominated(omb_ctx* ctx, int k, int S, const double* y_dev, int64_t ld, int64_t N, uint8_t* mask_dev,
                     int64_t ldm, int64_t* count_dev);
/* The sieve of the last omb_nondominated call on this context: *rounds_host its tile passes (0 before any call, at
 * most 4) and survivors_host[r] (5 entries; those past *rounds_host are 0) the largest set's survivors after pass r —
 * what the final pass then tested against itself is the last of them.  Host values; nothing is launched. */
int omb_nondominated_stats(omb_ctx* ctx, int64_t* survivors_host, int* rounds_host);

/* The exact hypervolume (everything minimised) that each of S independent point sets dominates below the reference
 * point r_host (k host doubles).  y_dev and mask_dev have omb_nondominated's layout: coordinate j of point i of set s
 * is y_dev[(j·S + s)·ld + i], and row i belongs to set s when mask_dev[s·ldm + i] != 0 (mask_dev NULL: every row, ldm
 * is then only checked against N).  A row is KEPT when every coordinate is finite and < r_j: NaN, ±∞ and y_j ≥ r_j
 * drop it.  The set need not be non-dominated: dominated rows, duplicates and ties change nothing.
 *   hv_dev[s] = the hypervolume of set s; 0.0 for a set with no kept row
 * A grid sweep (omb_hypervolume.hip): objectives 0..k-3 are cut at the kept rows' distinct values, and
 * every cell's weight times the area of the 2-D staircase of the rows that reach it is summed — exact arithmetic on
 * exactly the dominated region, cells × kept rows point tests, every addition of positive terms, in a tree whose
 * shape depends on the cell count alone: the result is bitwise the same whatever ld, ldm, S, the set's slot, the order
 * of the rows and the number of dropped rows.
 * SYNCHRONISES: the kept count and the grid sizes are read back once to size the second launch.  Scratch is a context
 * buffer grown on demand.  Touches no plan, no GP state and no paths.
 *   OMB_EINVAL  k outside [1, OMB_MAX_OBJ], S outside [1, OMB_NONDOM_SETS], N < 0, ld < N or ldm < N, a NULL r_host or
 *               a non-finite r_j, a NULL hv_dev, a NULL y_dev with N > 0, y_dev or hv_dev off 8-byte alignment — in
 *               this order
 *   OMB_EUNSUP  N > OMB_NONDOM_POINTS; then, after the first launch, a set with more than OMB_HV_POINTS kept rows; then
 *               Σ_s cells_s × kept_s above OMB_HV_MAX_WORK
 * A refused call writes nothing to hv_dev.  N = 0 returns OMB_OK and writes hv_dev[s] = 0.0. */
int omb_hypervolume(omb_ctx* ctx, int k, int S, const double* y_dev, int64_t ld, int64_t N, const uint8_t* mask_dev,
                    int64_t ldm, const double* r_host, double* hv_dev);
/* One set (y_dev (k, N) at pitch ld, mask_dev N bytes or NULL) and what every row adds to it:
 *   hv_dev[0]      = HV(set), as omb_hypervolume gives it, bit for bit
 *   contrib_dev[i] = HV(set) − HV(set without row i) for a kept row i, 0.0 for a dropped or masked-out row   (i < N)
 * Both hypervolumes are sums over the whole set's grid in the same tree, so a row whose removal changes no cell's
 * staircase — a duplicate, a row that another kept row dominates — gets exactly 0.0, not a rounding of it; the other
 * rows' values carry the rounding of both sums (about 2·(n + k + 48)·2^-53·HV at worst).  cells × kept × (kept + 1) point
 * tests.  SYNCHRONISES like omb_hypervolume.
 *   OMB_EINVAL  omb_hypervolume's (S = 1, ldm = N), a NULL contrib_dev where a NULL hv_dev is refused, contrib_dev off
 *               8-byte alignment with the other two
 *   OMB_EUNSUP  N > OMB_NONDOM_POINTS; more than OMB_HV_POINTS kept rows; cells × kept × (kept + 1) above OMB_HV_MAX_WORK
 * A refused call writes nothing to either output.  N = 0 returns OMB_OK and writes hv_dev[0] = 0.0 only. */
int omb_hypervolume_contrib(omb_ctx* ctx, int k, const double* y_dev, int64_t ld, int64_t N, const uint8_t* mask_dev,
                            const double* r_host, double* hv_dev, double* contrib_dev);
/* The last omb_eval_argmax[_sobol] call on this context (OMB_DEBUG_ARGMAX_PRUNE): stats_host[0] = 1 if it took the
 * two-phase path, 0 if the dense chain; [1] the candidates of its seed (⌈N/256⌉, or ⌈N/16⌉ under the value 2); [2]
 * the candidates past the seed whose bound kept them.  [2] is stored by the call's kernels: it is that call's once
 * its result has been waited for.  All 0 after a dense call.  Host values; nothing is launched and nothing is waited for. */
int omb_argmax_prune_stats(omb_ctx* ctx, int64_t* stats_host);
/* The same call's staged order (OMB_DEBUG_ARGMAX_STAGED): stats_host[0] = 1 if it took it; [1] the candidates past the
 * seed that objective 1's bound kept (list A); [2] those of them that the full bound kept (list B, omb_argmax_prune_stats'
 * [2]).  [1] and [2] are stored by the call's kernels, as above.  All 0 otherwise. */
int omb_argmax_stage_stats(omb_ctx* ctx, int64_t* stats_host);
/* The same call's cut (OMB_DEBUG_ARGMAX_CUT): stats_host[0] = 1 if the staged order drew its first list by the cut;
 * [1] m*, the smallest value found whose bound lies below [2] τ₀, the seed's best value (+∞: nothing could be
 * dropped); [3] the bound at m* (NaN where m* is +∞).  [1] to [3] are stored by the call's kernels, as above.  All 0
 * otherwise. */
int omb_argmax_cut_stats(omb_ctx* ctx, double* stats_host);

/* Hypervolume-based PoI of EMO (emo.py:176-228): cells_dev (C, 2, 2) [upper, lower]. */
int omb_hvpoi(omb_ctx* ctx, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
              const double* cells_dev, int C, double* out_dev);

/* expected_decomposition (util_functions.py:285-327) for k objectives:
 *   cache_dev (M, k); weights/ideal/max host (k); params_host per OMB_SCAL_* (may be NULL). */
int omb_expdec(omb_ctx* ctx, int k, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
               const double* cache_dev, int M, int scal_id, const double* params_host,
               const double* weights_host, const double* ideal_host, const double* max_host,
               double agg_min, double* out_dev);

/* Expected improvement (optimisers.py:325-344 with var_eps = 0; parego.py:126-145 and
 * keep.py:118-137 with var_eps = 1e-6). */
int omb_ei(omb_ctx* ctx, const double* mu_dev, const double* var_dev, int64_t N, double best,
           double var_eps, double* out_dev);
/* EI and its products with further models, over k posterior rows (row o at mu_dev + o·ld):
 *   OMB_EI_PLAIN       k = 1   EI(μ0, σ²0 + var_eps)                              (= omb_ei)
 *   OMB_EI_PARETO      k = 2   μ1 · EI(μ0, σ²0 + var_eps), var_eps = 1e-6 in the reference:
 *                              KEEP.pareto_expected_improvement (keep.py:118-151), row 1 = the
 *                              Pareto-membership model
 *   OMB_EI_CONSTRAINED k ≥ 2   EI(μ0, σ²0 + var_eps) · Π_{c=1}^{k-1} Φ(−μc / sqrt(σ²c + pof_eps)),
 *                              var_eps = 0, pof_eps = 1e-5 in the reference:
 *                              ParEGO_C2.consraint_ei (cparego.py:450-496), rows 1.. = constraints */
int omb_ei_ext(omb_ctx* ctx, int kind, int k, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
               double best, double var_eps, double pof_eps, double* out_dev);

/* Probability of feasibility over c rows of constraint-model moments (row j at mu_dev + j·ld; feasible is g ≤ 0):
 *   z_j = (0 − μ_j) / sqrt(σ²_j + pof_eps),   F = (((1·Φ(z_0))·Φ(z_1))…·Φ(z_{c−1})),   out = acq · F
 * (acq_dev NULL: out = F; out_dev may be acq_dev).  z and the multiplication order are OMB_EI_CONSTRAINED's, so
 * omb_ei weighted here has that kind's bits.  A NaN acquisition value stays NaN; σ²_j + pof_eps < 0 gives NaN, as in
 * OMB_EI_CONSTRAINED (σ² is not clamped).  1 ≤ c ≤ OMB_MAX_OBJ; OMB_EINVAL for c outside it, a null pointer with
 * N > 0, ld < N with c > 1, or pof_eps negative or not finite (nothing is written); N = 0 is OMB_OK and touches
 * nothing.  Asynchronous. */
int omb_feasibility(omb_ctx* ctx, int c, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
                    double pof_eps, const double* acq_dev /* may be NULL */, double* out_dev);

/* ---- Log-space acquisitions (Ament et al. 2023).  The linear values above are exactly 0.0 in fp64 where the
 * improvement lies more than ~38 σ away (Φ and φ underflow; EI's h(γ) = γΦ(γ) + φ(γ) is 0.0 at γ = −39): over such a
 * region the arg-max returns the lowest index and every gradient is 0.  The logarithms below are finite there and
 * keep their slope.  All three are written on
 *   log h(t):  the direct log above t = −1;  −t²/2 − log√(2π) + log T(t) below, T = h/φ = 1 + t·R(t),
 *              R = Φ/φ = sqrt(π/2)·erfcx(−t/√2);  the asymptotic series of T in 1/t² below t = −30
 *   log Φ(t):  log1p(−Φ(−t)) above 0;  the direct log down to −1;  −t²/2 + log(erfcx(−t/√2)/2) below
 * and agree with a 60-digit reference to a few 1e-16 of max(1, |value|).  Edge rules: a NaN moment gives
 * NaN for that candidate only; −inf and NaN never win the arg-max.  Asynchronous. */
/* log EI over omb_ei_ext's arguments, σ and γ formed exactly as there:
 *   OMB_EI_PLAIN        log σ + log h(γ)
 *   OMB_EI_CONSTRAINED  … + Σ_{c=1}^{k-1} log Φ(−μc / sqrt(σ²c + pof_eps))    (bitwise omb_log_feasibility over PLAIN)
 * σ = 0 gives −inf (the log of omb_ei's 0), σ² + var_eps < 0 NaN.  Checks, in this order: omb_ei_ext's on
 * (kind, k, var_eps, pof_eps); OMB_EUNSUP for OMB_EI_PARETO (μ₁·EI has no logarithm where μ₁ ≤ 0); omb_ei_ext's on
 * the pointers, ld and N. */
int omb_log_ei(omb_ctx* ctx, int kind, int k, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
               double best, double var_eps, double pof_eps, double* out_dev);
/* log of the exact EHVI: arguments, checks and limits are omb_ehvi_boxes_k's (2 ≤ k ≤ OMB_MAX_OBJ, boxes 4-byte
 * aligned).  With lh = log h((coordinate − μ_j)/σ_j):
 *   L_b = Σ_j [lh_hi + log(1 − e^(lh_lo − lh_hi))],   out = Σ_j log σ_j + logsumexp_b L_b
 * (a lower index at the −∞ column contributes lh_hi alone).  The sum over boxes has one fixed order and no atomics:
 * a candidate's value does not depend on N or its column.  σ²_j ≤ 0 gives NaN (the linear kernel: NaN below 0; at
 * exactly 0 the log form is −inf + inf — take the log of omb_hvi_boxes, the σ → 0 limit). */
int omb_log_ehvi_boxes(omb_ctx* ctx, int k, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
                       const double* coords_dev, int C, const uint16_t* boxes_dev, int B, double* out_dev);
/* out = acq + log F over omb_feasibility's arguments and checks (acq_dev NULL: out = log F; out_dev may be acq_dev):
 * log F = ((0 + log Φ(z_0)) + log Φ(z_1)) + …, z_j and the order over j as there.  Finite where F is 0.0. */
int omb_log_feasibility(omb_ctx* ctx, int c, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
                        double pof_eps, const double* acq_dev /* may be NULL */, double* out_dev);

/* Max-value entropy search (MES, Wang & Jegelka 2017; over k objectives MESMO, Belakaria et al. 2019), everything
 * minimised.  ystar_dev (k, S): the minimum of objective j under posterior sample s (omb_paths_min).  With
 * σ_j = sqrt(σ²_j) and γ_js = (μ_j − y*_js)/σ_j:
 *   out = Σ_j [ (Σ_s a(γ_js)) / S ],   a(γ) = γφ(γ)/(2Φ(γ)) − log Φ(γ)   (≥ 0, decreasing in γ),
 * both sums in index order, unfused; a on the tail ratios Φ/φ and h/φ below 0, finite where Φ underflows.
 * α over k posterior rows (row j at mu_dev + j·ld).  1 ≤ k ≤ OMB_MAX_OBJ, 1 ≤ S ≤ 64.
 * OMB_EINVAL: k or S outside its range, N < 0, a null pointer with N > 0, ld < N with k > 1.  N = 0: OMB_OK, nothing
 * written.  ystar is not inspected (it is on the device): a NaN y* gives NaN.  σ²_j ≤ 0 or a NaN moment gives NaN for
 * that candidate only.  Asynchronous. */
int omb_mes(omb_ctx* ctx, int k, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
            const double* ystar_dev, int S, double* out_dev);

/* Arg-max over vals_dev (N): lowest index among maxima, NaN and -inf never win
 * (replaces scipy differential_evolution(lambda x: -acq(x)), optimisers.py:87,118).
 * result_dev (2 doubles, device): {best value, best index + offset (as double)};
 * index -1 when nothing qualifies.  Asynchronous. */
int omb_argmax_dev(omb_ctx* ctx, const double* vals_dev, int64_t N, int64_t offset, double* result_dev);
/* Same, synchronising and returning to host. */
int omb_argmax(omb_ctx* ctx, const double* vals_dev, int64_t N, int64_t offset, double* best_val,
               int64_t* best_idx);

/* ---------------------------------------------------------------------------------------
 * Fused chain.  One BO iteration of the reference calls
 *   differential_evolution(lambda x: -acq(x, models, ...), bounds)      (optimisers.py:87,118)
 * where acq is fixed for the iteration.  Here the acquisition and its per-iteration geometry
 * are uploaded once as a *plan* (HOST pointers, copied into context-owned device memory; the
 * call synchronises the stream first), then each candidate batch is one call that runs
 * posterior (objectives 0..k-1) → acquisition → arg-max on the stream, with the moments in a
 * context-owned workspace (grown on demand).  Setting a plan replaces the previous one; a
 * failed plan call leaves no plan (OMB_ESTATE from the eval calls).
 * ------------------------------------------------------------------------------------- */
/* util_functions.EHVI / EHVI_2D_aux (k = 2): as omb_ehvi2d, pf_sorted_host (P, 2). */
int omb_plan_ehvi2d(omb_ctx* ctx, const double* pf_sorted_host, int P, const double* r_host, double s00,
                    double s01, int mode);
/* util_functions.EHVI_3D reference Monte-Carlo form (k = 3): as omb_ehvi3d_mc, cache_host (M, 3). */
int omb_plan_ehvi3d_mc(omb_ctx* ctx, const double* cache_host, int M, const double* r_host, double hv_pf);
/* EHVI_3D's Monte-Carlo form for k objectives (2 ≤ k ≤ OMB_MAX_OBJ): as omb_ehvi_mc, cache_host (M, k). */
int omb_plan_ehvi_mc(omb_ctx* ctx, int k, const double* cache_host, int M, const double* r_host, double hv_pf);
/* Exact EHVI (k = 2, 3): as omb_ehvi_boxes, coords_host (k, C), boxes_host (B, 2k). */
int omb_plan_ehvi_boxes(omb_ctx* ctx, int k, const double* coords_host, int C, const uint16_t* boxes_host, int B);
/* Exact EHVI (2 ≤ k ≤ OMB_MAX_OBJ): as omb_ehvi_boxes_k, coords_host (k, C), boxes_host (B, 2k).  The list is on
 * the host here, so every box is checked: a grid index ≥ C, or a lower index ≥ its upper index, is OMB_EINVAL
 * (and leaves no plan). */
int omb_plan_ehvi_boxes_k(omb_ctx* ctx, int k, const double* coords_host, int C, const uint16_t* boxes_host, int B);
/* EMO hypervolume-based PoI (k = 2): as omb_hvpoi, cells_host (C, 2, 2). */
int omb_plan_hvpoi(omb_ctx* ctx, const double* cells_host, int C);
/* expected_decomposition (k objectives): as omb_expdec, cache_host (M, k). */
int omb_plan_expdec(omb_ctx* ctx, int k, const double* cache_host, int M, int scal_id, const double* params_host,
                    const double* weights_host, const double* ideal_host, const double* max_host, double agg_min);
/* Expected improvement of objective 0 (k = 1): as omb_ei. */
int omb_plan_ei(omb_ctx* ctx, double best, double var_eps);
/* EI family over objectives 0..k-1: as omb_ei_ext. */
int omb_plan_ei_ext(omb_ctx* ctx, int kind, int k, double best, double var_eps, double pof_eps);

/* omb_mes as a plan of the fused chain over objectives 0..k-1 (σ² of every one of them is read); ystar_host (k, S) is
 * checked: a non-finite entry is OMB_EINVAL and leaves no plan.  omb_eval_grad is analytic on it:
 *   ∂α/∂μ_j = (1/S) Σ_s a'(γ_js)/σ_j,  ∂α/∂σ²_j = (1/S) Σ_s a'(γ_js)·(−γ_js)/(2σ²_j),  a'(γ) = −(q/2)(1 + γ² + γq),
 * q = φ/Φ.  omb_plan_constraints applies as to every plan; omb_plan_log answers OMB_EUNSUP. */
int omb_plan_mes(omb_ctx* ctx, int k, int S, const double* ystar_host);

/* omb_hvi_paths as a plan of the fused chain over objectives 0..k-1: coords_host (S, k, C), box_off_host (S + 1),
 * boxes_host (box_off[S], 2k), all on the host and held to omb_hvi_paths' checks; every list's indices are checked
 * as omb_plan_ehvi_boxes_k checks its list (OMB_EINVAL, no plan left).  Under this plan the chain's posterior stage is
 * the evaluation of the installed sample paths: [Sobol →] omb_paths_eval(0..k-1) → omb_hvi_paths → [arg-max], in
 * passes of OMB_HVI_PATHS_CHUNK candidates, so the workspace holds (k·S, chunk) path values, not (k·S, N); values are
 * bitwise omb_paths_eval → omb_hvi_paths on the same points, whatever the chunk.  omb_timing's "posterior" interval
 * is the path evaluation (with several passes it ends after the last pass's, and so holds the earlier passes'
 * acquisition launches).  Before anything is launched the eval calls return OMB_ESTATE, naming omb_paths_set, when an
 * objective of 0..k-1 has no GP, has no paths, or holds another number of paths than the plan's S — omb_set_gp,
 * omb_gp_fit_state and omb_gp_append drop an objective's paths, so a plan over a changed state is refused, never
 * evaluated; omb_paths_eval's OMB_EUNSUP (n_var > 64, n_train > OMB_MAX_TRAIN_DENSE) applies.  omb_eval_grad returns
 * OMB_EUNSUP (no analytic gradient through the paths), as do omb_plan_log and omb_plan_constraints with n_con > 0 (the
 * weight would need a posterior of the constraint slots, which this chain does not compute); each names the plan and
 * leaves it as it was. */
int omb_plan_hvi_paths(omb_ctx* ctx, int k, int S, const double* coords_host, int C, const int32_t* box_off_host,
                       const uint16_t* boxes_host);
/* omb_hvi_paths_con (no flag) as a plan of the fused chain: omb_plan_hvi_paths' arguments and checks, then
 * omb_hvi_paths_con's for n_con and eta.  The chain runs [Sobol →] omb_paths_eval(0..k+n_con−1) →
 * omb_hvi_paths_con → [arg-max] in passes of OMB_HVI_PATHS_CHUNK candidates (OMB_DEBUG_HVI_PATHS_CHUNK applies); the
 * workspace holds ((k + n_con)·S, chunk) path values; values are bitwise omb_paths_eval → omb_hvi_paths_con,
 * whatever the chunk.  The OMB_ESTATE rule of omb_plan_hvi_paths covers all k + n_con slots.  The plan carries its
 * own constraints: omb_plan_constraints with n_con > 0, omb_plan_log and omb_eval_grad return OMB_EUNSUP on it, as on
 * omb_plan_hvi_paths. */
int omb_plan_hvi_paths_con(omb_ctx* ctx, int k, int S, int n_con, double eta, const double* coords_host, int C,
                           const int32_t* box_off_host, const uint16_t* boxes_host);

/* Inequality constraints on the plan that is set (g ≤ 0 feasible).  From here on omb_eval, omb_eval_argmax,
 * omb_eval_argmax_sobol and omb_eval_grad also compute the posterior (μ and σ²) of context slots k..k+n_con−1 — the
 * constraint models, set like objectives with omb_set_gp / omb_gp_fit_state — and multiply the acquisition by their
 * probability of feasibility (omb_feasibility's F at pof_eps) before the arg-max.  The objectives' σ² stay as the
 * plan needs them.  Every omb_plan_* call starts a new plan and so clears the constraints: set them after the plan.
 * n_con = 0 clears them.  OMB_ESTATE with no plan; OMB_EINVAL for n_con < 0 or pof_eps negative or not finite;
 * OMB_EUNSUP for k + n_con > OMB_MAX_OBJ; a failed call leaves the plan and its constraints as they were.  A
 * constraint slot with no GP is OMB_ESTATE from the eval calls, as for an objective.  With OMB_DEBUG_FUSED_CHAIN 1
 * or 2 a constrained EHVI-2D plan takes the plain chain (the same pair).  omb_eval_grad keeps the gradient of
 * every plan that has one (the product rule over a·F; finite where F underflows to 0) and its NaN-row rule.
 * σ²_j + pof_eps < 0 gives NaN there as well. */
int omb_plan_constraints(omb_ctx* ctx, int n_con, double pof_eps);

/* The plan that is set returns the logarithm of its acquisition (on = 1) or the acquisition itself (on = 0, what
 * every omb_plan_* call starts with: a new plan clears the flag).  Plans with a log form: omb_plan_ei,
 * omb_plan_ei_ext with OMB_EI_PLAIN or OMB_EI_CONSTRAINED (omb_log_ei's value), omb_plan_ehvi_boxes and
 * omb_plan_ehvi_boxes_k (omb_log_ehvi_boxes' value, one kernel for both).  It may come before or after
 * omb_plan_constraints; with both, the chain adds log F (omb_log_feasibility) in place of the multiplication by F.
 * The posterior's variance mask is the linear plan's.  Errors, in this order, each leaving the plan as it was:
 * OMB_ESTATE with no plan; OMB_EINVAL for `on` outside {0, 1}; OMB_EUNSUP, naming the plan, for Pareto EI, EHVI-2D
 * (any mode), Monte-Carlo EHVI, HV-PoI, expected decomposition, max-value entropy search and the sampled-front
 * improvement (omb_plan_hvi_paths).
 * omb_eval_grad on a log plan: log EI (plain or constrained, with or without omb_plan_constraints) is analytic —
 *   ∂/∂μ = −ρ/(σ + 1e-10),  ∂/∂σ² = (1/σ − ρ·γ/(σ + 1e-10))/(2σ),  ρ = Φ(γ)/h(γ) = R/T for γ < 0,
 *   a constraint row: ∂ log Φ(z)/∂z = φ(z)/Φ(z) = 1/R(z) times ∂z/∂μ, ∂z/∂σ² —
 * finite and non-zero where the linear gradient is 0; the NaN-row rule is kept.  The log exact EHVI returns
 * OMB_EUNSUP, writes nothing and leaves the plan set. */
int omb_plan_log(omb_ctx* ctx, int on);

/* Scrambled Sobol' candidates generated on the device (replaces the host-side sampling that
 * feeds the maximiser; same sequence as scipy.stats.qmc.Sobol, which the reference uses for
 * its MC cache at optimisers.py:121-141).  sv_host (d, bits) and shift_host (d) are the
 * engine's scrambled direction numbers and digital shift (scipy: Sobol._sv, Sobol._shift);
 * point i of the engine, mapped to the box, is
 *   x_ij = lo_j + u_ij (hi_j − lo_j),  u_ij = (shift_j ⊕ ⨁_{b ∈ gray(i)} sv_jb) · 2^-bits,
 * bit-identical to numpy's `lo + U * (hi - lo)` on scipy's U.  bits ≤ 32, d ≤ OMB_MAX_DIM. */
int omb_set_sobol(omb_ctx* ctx, int d, int bits, const uint32_t* sv_host, const uint32_t* shift_host,
                  const double* lo_host, const double* hi_host);
/* Points start .. start+N-1 → X_dev (N, d). */
int omb_sobol(omb_ctx* ctx, int64_t start, int64_t N, double* X_dev);

/* Acquisition values of the plan at candidates Xc_dev (N, d) → vals_dev (N). */
int omb_eval(omb_ctx* ctx, const double* Xc_dev, int64_t N, double* vals_dev);
/* posterior → plan → arg-max: result_dev = {best value, best index + offset} (see omb_argmax_dev). */
int omb_eval_argmax(omb_ctx* ctx, const double* Xc_dev, int64_t N, int64_t offset, double* result_dev);
/* Same over the Sobol' points start .. start+N-1 generated into the workspace; the index in
 * result_dev is the Sobol index (offset = start). */
int omb_eval_argmax_sobol(omb_ctx* ctx, int64_t start, int64_t N, double* result_dev);

/* ---------------------------------------------------------------------------------------
 * Gradients with respect to a candidate (closed forms; no finite differences).  With k_i = k(x, X_i) and
 * s_ij = (x_j − X_ij)/ℓ_j²:  ∂k_i/∂x_j = g_i·s_ij,  g_i = −(5/3)σ_f²(1 + √5 r_i)e^{−√5 r_i} (Matern-5/2; finite at
 * r = 0) or −k_i (RBF);  ∂μ/∂x_j = Σ_i α_i g_i s_ij;  ∂σ²/∂x_j = −2 Σ_i w_i g_i s_ij,  w = L⁻ᵀ(L⁻¹k) (two products
 * with the dense L⁻¹, no explicit K⁻¹).  σ² is not clamped, so the gradient is that of the unclamped expression.
 * n_train ≤ OMB_MAX_TRAIN_DENSE, n_var ≤ OMB_MAX_DIM, both kernels, N ≥ 0 (N = 0 is OMB_OK and touches nothing).
 * The workspace (K*, V, w: (n_obj + 2)·n_train doubles per candidate, in passes of at most 512 MiB) is grown on
 * demand; a grow synchronises the stream first.  Fixed-order sums: a candidate's gradient does not depend on N or
 * on its place in the batch.  Asynchronous.
 * ------------------------------------------------------------------------------------- */
/* μ, σ² as omb_posterior, plus ∂μ_o/∂x and ∂σ²_o/∂x at every candidate:
 * dmu_dev, dvar_dev (n_obj, N, d) row-major.  mu_dev / var_dev (n_obj, N) may not be NULL. */
int omb_posterior_grad(omb_ctx* ctx, int n_obj, const double* Xc_dev, int64_t N, double* mu_dev, double* var_dev,
                       double* dmu_dev, double* dvar_dev);
/* Plan's acquisition value and its gradient w.r.t. the candidate: vals_dev (N), grad_dev (N, d).
 * vals_dev is bitwise omb_eval's.  Plans with a gradient: omb_plan_ei, omb_plan_ei_ext (every kind),
 * omb_plan_ehvi2d (OMB_EHVI_REFERENCE: σA = σ²0·s00, σB = σ²0·s01, last stripe omitted — differentiated as it is;
 * OMB_EHVI_TEXTBOOK), omb_plan_ehvi_boxes, omb_plan_ehvi_boxes_k.  The Monte-Carlo EHVI, expected-decomposition
 * and HV-PoI plans (piecewise in the candidate) and EHVI-2D's OMB_EHVI_SIGMA mode return OMB_EUNSUP, write
 * nothing and leave the plan set; no plan is OMB_ESTATE, as for omb_eval.  Where the value is NaN, every gradient
 * entry of that candidate is NaN; no other candidate is affected.  Under omb_plan_log: see there (log EI is
 * differentiated, the log exact EHVI is OMB_EUNSUP). */
int omb_eval_grad(omb_ctx* ctx, const double* Xc_dev, int64_t N, double* vals_dev, double* grad_dev);

/* Device timing of the fused chain (HIP events on the context's stream), up to 4096 chains.
 * omb_timing(ctx, level): 0 off; 1 the posterior stage only (2 events per chain); 2 every
 * stage (5 events; each record costs a few µs of GPU time).  omb_timing_read synchronises
 * and returns the summed milliseconds of {Sobol generation, posterior, acquisition, arg-max}
 * (0 for stages not recorded) over the chains recorded since the last read, and their count.
 * Changing the level discards unread records. */
int omb_timing(omb_ctx* ctx, int enable);
int omb_timing_read(omb_ctx* ctx, double* stage_ms /* [4] */, int64_t* chains);

/* ---------------------------------------------------------------------------------------
 * Thompson sampling — TuRBO's candidate scoring (turbo.py:75-117 create_candidates,
 * turbo.py:142-153 / 365-383 candidate selection).  The reference draws `batch_size` joint
 * samples with GPy's GP.posterior_samples(X_cand, size) (turbo.py:114): a full posterior
 * covariance (PosteriorExact._raw_predict, full_cov=True) and numpy's multivariate_normal
 * (SVD).  Here: Σ on FP64 MFMA, a blocked Cholesky of Σ + jitter·I, samples μ + L z.
 * ------------------------------------------------------------------------------------- */
/* μ (N) and the full symmetric posterior covariance cov_dev (N, N) of objective `obj` at Xc_dev
 * (N, d):  Σ = K(X*, X*) − (L⁻¹K*)ᵀ(L⁻¹K*)  (GPy _raw_predict(full_cov=True) + σ_n² = 0).
 * N ≤ 32768.  Asynchronous. */
int omb_posterior_cov(omb_ctx* ctx, int obj, const double* Xc_dev, int64_t N, double* mu_dev, double* cov_dev);
/* In-place lower Cholesky factor of A + jitter·I (A_dev (N, N) row-major with leading dimension
 * lda; the lower triangle is read and overwritten, the upper triangle is left untouched —
 * LAPACK dpotrf('L') on the row-major lower triangle).  Synchronises; *info = 0 on success,
 * else the 1-based column of the first non-positive pivot (dpotrf's info). */
int omb_cholesky(omb_ctx* ctx, double* A_dev, int64_t N, int64_t lda, double jitter, int* info);
/* B joint posterior samples of objective `obj` at Xc_dev (N, d) (GPy posterior_samples_f):
 *   Y_dev (B, N) row b = μ + L z_b,  L = chol(Σ + j I),  Zt_dev (B, N) standard normals z_b.
 * Try t = 0 .. max_tries-1 uses j = jitter_rel · σ_f² · 10^t until the factorisation succeeds
 * (OMB_ENOTPD otherwise); *jitter_used (may be NULL) receives the j used.  Synchronises.  When the call fails after
 * the draws were queued (OMB_ENOTPD, or OMB_EHIP from a factor wait that ran out), Y_dev is filled with NaN. */
int omb_posterior_samples(omb_ctx* ctx, int obj, const double* Xc_dev, int64_t N, const double* Zt_dev, int B,
                          double jitter_rel, int max_tries, double* Y_dev, double* jitter_used);
/* Greedy selection of TuRBO_1.select_candidates (turbo.py:142-153) / TuRBO_M._select_candidates
 * (turbo.py:365-383): for b = 0 .. B-1, idx_dev[b] = np.argmin over row b of Y_dev (B, N)
 * (first NaN, else the lowest index among minima), every earlier pick reading as +inf
 * (the reference sets y_cand[pick, :] = inf).  N ≤ 2^18.  Y is not modified.  Asynchronous. */
int omb_thompson_select(omb_ctx* ctx, const double* Y_dev, int B, int64_t N, int64_t* idx_dev);

/* ---------------------------------------------------------------------------------------
 * Posterior sample paths: draws that are functions (pathwise conditioning, Matheron's rule; Wilson et al. 2020,
 * "Efficiently sampling functions from Gaussian process posteriors"):
 *     f_s(x) = φ(x)ᵀ w_s + k(x, X) v_s,   φ_i(x) = sqrt(2σ_f²/m)·cos(ω̃_i·(x/ℓ) + b_i),
 *     v_s = α − K_y⁻¹(Φ(X) w_s + ε_s),    ε_s = sqrt(σ_n² + 1e-8)·z_s.
 * S paths at N points cost O(N·(m + n)·S); nothing is N × N, nothing is factorised (no OMB_ENOTPD), and the paths can
 * be evaluated again anywhere.  omb_set_gp, omb_gp_fit_state and a successful omb_gp_append on an objective drop its
 * paths (omb_paths_eval then returns OMB_ESTATE); plans and GP states are never touched by either call.
 * The cosine is accurate (below 2 ulp of 1, absolute) for arguments |ω̃_i·(x/ℓ) + b_i| ≤ 2^20; a caller who draws
 * frequencies keeps them inside that range over the box of x (optimobo_amd.paths.draw_path_inputs does).
 * n_var ≤ 64 and n_train ≤ OMB_MAX_TRAIN_DENSE; both kernels.
 * ------------------------------------------------------------------------------------- */
/* Install S posterior sample paths of objective obj (1 ≤ S ≤ 16, 1 ≤ m ≤ 65536).  HOST pointers, copied
 * like a plan's geometry (the call synchronises the stream first):
 *   omega_host (m, d) frequencies of x/ℓ;  phase_host (m);  w_host (m, S) standard normals;
 *   z_host (n_train, S) standard normals or NULL (ε = 0);  noise = the σ_n² the state was factorised with.
 * Device: U = Φ(X)·w·sqrt(2σ_f²/m) + sqrt(noise + 1e-8)·z;  V = α − L⁻ᵀ(L⁻¹U)  (dense L⁻¹, existing GEMMs).
 * Refusals, in this order: OMB_EINVAL for obj, S or m outside its range, a null omega / phase / w, noise negative or
 * not finite; OMB_ESTATE for an objective that is not set; OMB_EUNSUP for n_var > 64 or n_train >
 * OMB_MAX_TRAIN_DENSE.  A failed call leaves the objective without paths. */
int omb_paths_set(omb_ctx* ctx, int obj, int S, int m, const double* omega_host, const double* phase_host,
                  const double* w_host, const double* z_host, double noise);
/* out_dev[(o·S + s)·ld + i] = f_{o,s}(Xc_i), objectives 0..n_obj-1 (all with the same S), Xc_dev (N, d), ld ≥ N.
 * Asynchronous.  N = 0 is OMB_OK and writes nothing.  A value is a function of the point and the installed state
 * alone: bitwise the same whatever N and the point's position in Xc.
 * Refusals, in this order: OMB_EINVAL for n_obj outside [1, OMB_MAX_OBJ], N < 0, ld < N, a null pointer with N > 0;
 * OMB_ESTATE for an objective that is not set, has no paths or another S than objective 0; OMB_EUNSUP as above. */
int omb_paths_eval(omb_ctx* ctx, int n_obj, const double* Xc_dev, int64_t N, int64_t ld, double* out_dev);
/* omb_paths_eval's values and the paths' gradients with respect to the candidate,
 *   ∂f_s/∂x_j = −(1/ℓ_j) Σ_i w_is·sqrt(2σ_f²/m)·ω̃_ij·sin(ω̃_i·(x/ℓ) + b_i) + Σ_r v_rs·g_r·(x_j − X_rj)/ℓ_j²,
 * g_r = −(5/3)σ_f²(1 + √5 r)e^{−√5 r} (Matern-5/2; finite at r = 0) or −k_r (RBF); x_j − X_rj is formed as a
 * difference first, so a candidate on a training row stays accurate.
 *   out_dev[(o·S + s)·ld + i]            bitwise omb_paths_eval's
 *   grad_dev[((o·S + s)·d + j)·ld + i]   ∂f_{o,s}/∂x_j at Xc_i (the candidate index innermost)
 * The evaluation kernel's wave with one more accumulator per input dimension, the dimensions in groups of 8 (one
 * pass over the tiles per group), a fixed tile order and no atomics: an entry is bitwise the same whatever N, the
 * point's column and the launch grid.  A NaN coordinate makes that candidate's entries NaN, nobody else's.
 * Asynchronous; N = 0 is OMB_OK and writes nothing.  Limits and refusals are omb_paths_eval's, in its order; a NULL
 * grad_dev with N > 0 is OMB_EINVAL where a NULL out_dev is. */
int omb_paths_grad(omb_ctx* ctx, int n_obj, const double* Xc_dev, int64_t N, int64_t ld, double* out_dev,
                   double* grad_dev);
/* res_dev[(o·S + s)·2 + {0, 1}] = { min_i f_{o,s}(Xc_i), the lowest such i + offset (as double) }, objectives
 * 0..n_obj-1: omb_paths_eval's tile loop with the minimum taken in its epilogue, so the (n_obj·S, N) matrix never
 * exists.  The value is bitwise the minimum of omb_paths_eval's row.  Every comparison is "smaller value, else lower
 * index" (no atomics): the pair does not depend on the launch grid.  NaN never wins; N = 0 or an all-NaN row gives
 * {+inf, −1}.  Asynchronous; the context's partials buffer is grown on demand (a grow synchronises first).  Limits
 * and refusals are omb_paths_eval's, in its order (res_dev takes out_dev's place and may not be NULL even at N = 0). */
int omb_paths_min(omb_ctx* ctx, int n_obj, const double* Xc_dev, int64_t N, int64_t offset, double* res_dev);

/* ---------------------------------------------------------------------------------------
 * ParEGO / KEEP evolutionary acquisition search (parego.py:223-271, keep.py:240-292): the
 * reference's steady-state GA over a temporary population (20: mutants of archive members + Latin
 * hypercube points), 1,000 generations of binary tournaments without replacement (parego.py:78-111),
 * simulated binary crossover (:58-75) and ×1.05 / ×0.95 mutation (:37-56), the child replacing the
 * first parent unless the parent is strictly fitter; the proposal is the best individual seen at the
 * start of any generation (initially `lower` with fitness 0).  Fitness of objective 0's model:
 *   OMB_EA_EI         EI(μ0, σ = sqrt(σ²0 + var_eps))                  ParEGO (var_eps 1e-6)
 *   OMB_EA_PARETO_EI  μ1 · EI(μ0, ...) with objective 1 the Pareto-membership model   KEEP
 * The random draws come as a tape replayed on the host in the reference's call order (see
 * optimobo_amd/ea.py): sel_dev (iters, 4) int32 — tournament 1's random.sample over range(1, P),
 * tournament 2's over range(1, P − 1) (indices into the population without the first winner; the
 * caller guarantees these ranges); cross_dev (iters) int8 crossover flags; beta_dev (iters, d) the
 * crossover β per gene; mut_dev (iters, d) int8 mutation codes (0 none, 1 ×1.05, 2 ×0.95).
 * pop_dev (P, d), lower_dev / upper_dev (d), out_dev (d + 1) = best x, best fitness.  3 ≤ P ≤ 32,
 * n_train ≤ 2048.  One workgroup runs the search.  Asynchronous. */
enum { OMB_EA_EI = 0, OMB_EA_PARETO_EI = 1 };
int omb_ea_search(omb_ctx* ctx, int mode, double best, double var_eps, const double* pop_dev, int P, int iters,
                  const int32_t* sel_dev, const int8_t* cross_dev, const double* beta_dev, const int8_t* mut_dev,
                  const double* lower_dev, const double* upper_dev, double* out_dev);

/* ---------------------------------------------------------------------------------------
 * GP fit on the device — GPy GPRegression(X, y, Matern52(d, ARD=True)) with the noise variance
 * fixed (optimisers.py:223-231 and every other driver's fit) or free (the *_noise entries): exact inference
 * with GPy's jitchol
 * (Ky = K + (σ_n² + 1e-8) I; on failure + mean(diag Ky)·1e-6·10^t, t < 5), the log marginal
 * likelihood and its gradient for the hyperparameter search.  X_dev (n, d), y_dev (n) device.
 * ------------------------------------------------------------------------------------- */
/* *lml = log p(y | X, θ) = −½ yᵀα − Σ log L_ii − ½ n log 2π;  grad_host (d + 1) = ∂ lml / ∂(log σ_f²,
 * log ℓ_1 .. log ℓ_d);  *jitter_used (may be NULL) = jitchol's extra jitter.  n ≤ 16384.
 * Synchronises.  OMB_ENOTPD when even the jittered matrix is not positive definite. */
int omb_gp_lml_grad(omb_ctx* ctx, int kernel, int n, int d, const double* X_dev, const double* y_dev,
                    const double* lengthscale_host, double variance, double noise, double* lml, double* grad_host,
                    double* jitter_used);
/* k ≤ 4 GPs on the same inputs at once (the drivers fit one GP per objective on the same X;
 * optimisers.py:186): problem p has targets y_dev[p] (device pointer, n), lengthscales
 * lengthscale_host[p·d .. p·d + d − 1] and variance_host[p]; its results go to lml[p], grad_host[p·(d+1) ..],
 * jitter_used[p] (may be NULL) and status[p] (OMB_OK or OMB_ENOTPD, per problem: one non-positive-definite
 * problem does not fail the others).  Each problem's results are exactly omb_gp_lml_grad's: for n ≤ 128
 * and n_var ≤ 8 they run as one launch (one workgroup each) and one synchronisation, otherwise one after
 * another through omb_gp_lml_grad.  Replaces GPy
 * model.optimize's per-objective evaluations (optimisers.py:231).  Returns OMB_OK unless an argument or the
 * device call fails. */
int omb_gp_lml_grad_batch(omb_ctx* ctx, int kernel, int k, int n, int d, const double* X_dev,
                          const double* const* y_dev, const double* lengthscale_host, const double* variance_host,
                          double noise, double* lml, double* grad_host, double* jitter_used, int* status);
/* The same evaluation with the noise variance as a free parameter (GPy's default for GPRegression; the
 * reference's drivers fix it at 0).  With Ky = K + (σ_n² + 1e-8 + jitter) I,
 *     ∂ lml / ∂ log σ_n² = ½ tr((ααᵀ − Ky⁻¹) σ_n² I) = ½ σ_n² (αᵀα − tr Ky⁻¹),
 * taken at the jitter jitchol ended on (what GPy's formula does with its L).  The kernels of omb_gp_lml_grad
 * leave αᵀα and tr Ky⁻¹ beside their other sums in the same launches, so the two calls cost the same and
 * share every other result bit for bit.
 * As omb_gp_lml_grad; grad_host (d + 2): the d + 1 entries of omb_gp_lml_grad, then ∂ lml / ∂ log σ_n²
 * (exactly 0 at noise = 0).  Synchronises. */
int omb_gp_lml_grad_noise(omb_ctx* ctx, int kernel, int n, int d, const double* X_dev, const double* y_dev,
                          const double* lengthscale_host, double variance, double noise, double* lml,
                          double* grad_host, double* jitter_used);
/* As omb_gp_lml_grad_batch with a noise variance per problem: noise_host (k), grad_host k·(d + 2), problem p's
 * entries at grad_host[p·(d+2) ..].  The same argument checks, limits (n ≤ 16384, k ≤ 4), per-problem status and
 * choice between one launch and one problem after another; every problem's results are exactly its own
 * omb_gp_lml_grad_noise's.  Synchronises. */
int omb_gp_lml_grad_noise_batch(omb_ctx* ctx, int kernel, int k, int n, int d, const double* X_dev,
                                const double* const* y_dev, const double* lengthscale_host,
                                const double* variance_host, const double* noise_host, double* lml,
                                double* grad_host, double* jitter_used, int* status);
/* Fit the exact-inference state of objective `obj` on the device (Cholesky, L⁻¹, α) and install
 * it as omb_set_gp would — the device replacement for the host O(n³) factorisation. */
int omb_gp_fit_state(omb_ctx* ctx, int obj, int kernel, int n, int d, const double* X_dev, const double* y_dev,
                     const double* lengthscale_host, double variance, double noise, double* jitter_used);

/* ---------------------------------------------------------------------------------------
 * Conditioning an installed state on more observations without a refit (sequential-greedy batch proposals with
 * the Kriging believer; incremental conditioning on real observations between hyperparameter refits).
 * Per point, with k = K(X, x), mu = k'alpha, v = L^-1 k, delta^2 = variance + noise + 1e-8 - v'v, w = L^-T v and
 * zeta = (y - mu)/delta:  L^-1' = [[L^-1, 0], [-w'/delta, 1/delta]],  alpha' = [alpha - w zeta/delta ; zeta/delta],
 * X' = [X ; x] -- two mat-vecs over the dense L^-1, O(n^2); fixed-order sums, bitwise repeatable.
 * ------------------------------------------------------------------------------------- */
/* Condition the installed state of objective obj on q more observations, one after another (point j sees points < j):
 * Xnew_dev (q, d); ynew_dev (q) or NULL = Kriging believer (y_j = the posterior mean at x_j when it is appended);
 * noise = the sigma_n^2 the state was factorised with (plus any jitchol jitter the caller knows of);
 * mu_out_dev (q, may be NULL) receives that posterior mean of every point, var_out_dev (q, may be NULL) its delta^2_j.
 * All or nothing: on any failure the installed state is what it was.  Synchronises.
 *   OMB_ESTATE  objective not set
 *   OMB_EINVAL  q < 1, null Xnew_dev, negative or non-finite noise
 *   OMB_EUNSUP  n_train + q > OMB_MAX_TRAIN_DENSE
 *   OMB_ENOTPD  a delta^2 that is not positive and finite (a duplicate of a training point at zero noise can round
 *               below the jitter); omb_last_error names the 1-based index of the point
 * A plan that is set stays set (plans hold acquisition geometry, not GP state). */
int omb_gp_append(omb_ctx* ctx, int obj, int q, const double* Xnew_dev, const double* ynew_dev, double noise,
                  double* mu_out_dev, double* var_out_dev);

#ifdef __cplusplus
}
#endif

#endif /* OPTIMOBO_HIP_H */
