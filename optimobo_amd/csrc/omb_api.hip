// C-ABI of liboptimobo_hip.so (declared in include/optimobo_hip.h): context, GP state,
// argument validation and dispatch to the kernels.  No exception crosses this boundary.
#include <math.h>
#include <cmath>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <new>
#include <string>
#include <vector>

#include "omb_internal.h"

using namespace omb;

struct ObjState {
  bool set = false;
  int n = 0, d = 0, DP = 0, R = 0, n_pad = 0, kind = 0;
  double variance = 0.0;
  double* buf = nullptr;  // one allocation: Xs | xsq | alpha | ls | Lp | Ld | Xf | X
  size_t cap = 0;         // bytes
  const double* Ld = nullptr;  // dense row-major L⁻¹ (n, n): the full-covariance path's GEMM operand
  const double* Xraw = nullptr;  // unscaled inputs (n, d) and the host ℓ: what omb_gp_append packs the grown state from
  double ls[OMB_MAX_DIM] = {};
  GPDev dev{};
  // posterior sample paths over this state (omb_paths_set): path_S = 0 when none are installed.  One allocation:
  // Of | Wf | Vf | z | F | U | T | G (the last five: omb_paths_set's workspace, sized for 16 paths)
  int path_S = 0, path_MT = 0;
  double* pbuf = nullptr;
  size_t pcap = 0;       // bytes
  const double* path_Of = nullptr;
  const double* path_Wf = nullptr;
  const double* path_Vf = nullptr;
};

// One acquisition request.  A describe_* function validates the scalar arguments and fills everything but geo / boxes;
// a stand-alone entry then points those at the caller's device arrays, an omb_plan_* entry uploads the host geometry
// and points them at ctx->geo (the fused chain's plan).  launch_acq / launch_acq_grad run it.
enum PlanKind { PLAN_NONE = 0, PLAN_EHVI2D, PLAN_EHVI_MC, PLAN_EHVI_BOXES, PLAN_HVPOI, PLAN_EXPDEC, PLAN_EI, PLAN_MES,
                PLAN_HVI_PATHS, PLAN_HVI_PATHS_CON };

struct Plan {
  int kind = PLAN_NONE;
  int k = 0;                    // objectives the acquisition reads (posterior of 0..k-1)
  unsigned var_mask = 0;        // bit o: the plan's kernel loads σ² of objective o (the others' is never computed)
  int P = 0, M = 0, C = 0, B = 0, mode = 0;
  int S = 0;                    // PLAN_MES: sampled minima per objective (geo: ystar (k, S)); PLAN_HVI_PATHS: paths
  int32_t box_off[kPathsMaxS + 1] = {};   // PLAN_HVI_PATHS: list s is rows box_off[s]..box_off[s+1] of boxes (geo: the
                                          // S grids (S, k, C))
  // PLAN_HVI_PATHS_CON: slots k..k+path_con-1 are constraint models read through their sample paths, weighted by
  // omb_hvi_paths_con's w_s at path_eta with path_flags (the plan entry sets none)
  int path_con = 0;
  double path_eta = 0;
  unsigned path_flags = 0;
  double r[OMB_MAX_OBJ] = {};
  double s00 = 0, s01 = 0, hv = 0, best = 0, var_eps = 0, pof_eps = 0;
  int ei_kind = OMB_EI_PLAIN;
  ScalParams sp{};
  const double* geo = nullptr;  // pf / cache / coords / cells on the device
  const uint16_t* boxes = nullptr;
  bool boxes_kd = false;        // PLAN_EHVI_BOXES set by omb_plan_ehvi_boxes_k: the k-D kernel
  // omb_plan_constraints: context slots k..k+n_con-1 are constraint models, the acquisition is weighted by their
  // probability of feasibility (σ² of every one of them is computed: their bits are not in var_mask, which covers
  // the objectives only, and never in the chain's var_skip)
  int n_con = 0;
  double con_eps = 0;
  // omb_plan_log: the value is the logarithm of the acquisition (PLAN_EI plain / constrained, PLAN_EHVI_BOXES), and the
  // constraints' weight is added as log F.  var_mask is the linear plan's.
  bool log = false;
  // omb_plan_ehvi2d: the arg-max chain may prune by the upper bound of DESIGN §29 — OMB_EHVI_REFERENCE, s00 > 0,
  // s01 > 0, every number finite and the stripes' f1 non-increasing from r0 (a sorted non-dominated front)
  bool prune_ok = false;
};

// A device buffer that the context owns and grow_dev enlarges on demand.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;  // bytes
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

struct omb_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string err;
  ObjState obj[OMB_MAX_OBJ];
  double* partials = nullptr;  // argmax pass-1 output
  double* result_dev = nullptr;
  double* result_host = nullptr;  // pinned
  int* info_host = nullptr;       // pinned: the Cholesky status read back by run_cholesky / chol_wait
  // fused chain
  Plan plan;
  DevBuf geo;             // plan geometry
  void* stage = nullptr;  // pinned host staging of uploads
  size_t stage_cap = 0;
  DevBuf work;            // mu | var | vals | raised | X of the fused chain
  void* sob = nullptr;    // device: packed Sobol state (fixed capacity)
  int sob_d = 0, sob_bits = 0;
  // timing of the fused chain: 5 events per chain (level 2) or 2 around the posterior (level 1)
  int timing = 0;
  int timing_stride = 1;     // OMB_DEBUG_TIMING_STRIDE: events on every stride-th chain only
  int64_t timing_calls = 0;  // chains since omb_timing
  std::vector<hipEvent_t> ev;
  size_t ev_used = 0;
  // workspaces, each its own allocation (several are live at once: work with gws, tws with ichol)
  DevBuf tws;    // Thompson sampling: K* | V | μ | σ² | Σ
  DevBuf ichol;  // Cholesky info + step counters
  DevBuf sws;    // Thompson selection: per-sample sorted heads (select_sort_kernel)
  DevBuf ews;    // evolutionary search: L0⁻¹ transposed
  DevBuf fws;    // GP fit: Ky | L⁻¹ | Ky⁻¹ | scratch
  DevBuf dws;    // dense posterior path (n_train > OMB_MAX_TRAIN): K* | V chunk
  DevBuf gws;    // gradient chain (omb_posterior_grad / omb_eval_grad): ∂a/∂μ | ∂a/∂σ² | K* | V | w per objective
  DevBuf aws;    // omb_gp_append: the bordered state (AppendWs)
  DevBuf hws;    // omb_hvi_boxes: the slices' sums of a small batch (hvi_ws_doubles)
  DevBuf pws;    // omb_paths_min: the first launch's per-workgroup (value, index) pairs
  DevBuf nws;    // omb_nondominated: slot counters | final-pass counts | the first survivor list (S, N)
  DevBuf nws2;   // omb_nondominated: the second survivor list (S, survivors of the first pass)
  DevBuf prws;   // the arg-max chain's two-phase path: lists, flags, counts and pairs (PruneWs)
  DevBuf vws;    // omb_hypervolume: header | totals | one HvSet per set
  DevBuf vws2;   // omb_hypervolume: the cells' partial sums and their reduction's scratch
  // omb_argmax_prune_stats: whether the last arg-max chain took the two-phase path, its seed sample, and the survivor
  // count its scan kernel stores (pinned, device-mapped)
  int prune_taken = 0;
  int64_t prune_seed = 0;
  int64_t* prune_stats_host = nullptr;
  int64_t* prune_stats_dev = nullptr;
  // omb_argmax_stage_stats: whether it took the staged order; |A| is prune_stats_host[1], |B| is [0]
  int stage_taken = 0;
  // omb_argmax_cut_stats: whether the staged order took objective 1's bound as a cut; m*, τ₀ and
  // ubm1(m*) are the bits in prune_stats_host[2..4]
  int cut_taken = 0;
  int nd_rounds = 0;                              // omb_nondominated_stats: the last call's tile passes
  int64_t nd_survivors[kNdMaxRounds + 1] = {};    // and the largest set's survivors after each
  // device fault word (pinned, mapped host memory): kernels mark it, enter() reports it
  int* fault_host = nullptr;
  int* fault_dev = nullptr;
  // GP-fit results (omb_gp_lml_grad): pinned, host-mapped; the one-workgroup kernel stores into it
  // directly (no D2H copy on the per-evaluation path), the blocked path copies into it
  double* fit_host = nullptr;
  double* fit_dev = nullptr;
  // omb_debug_set's switches (kDebugSwitches): ints, the on/off ones 0 or 1
  int spin_limit = kDefaultSpinLimit;
  int cov_table = 0;    // OMB_DEBUG_COV_TABLE
  int cov_fused = 1;    // OMB_DEBUG_COV_FUSED: K(X*, X*) in the covariance SYRK's epilogue
  int syrk_glds = 1;    // OMB_DEBUG_SYRK_GLDS: the covariance SYRK's direct-to-LDS operand pipeline
  int fused_chain = 0;  // OMB_DEBUG_FUSED_CHAIN: 0 EHVI-2D then the arg-max's passes, 1 one ticketed launch, 2 EHVI
                        // with the per-workgroup pairs, then the arg-max's second pass
  bool argmax_one_pass = false;  // OMB_DEBUG_ARGMAX_PASSES: 1 (one launch) or 2 (default: measured level)
  int chol_mode = kCholPersistent;   // OMB_DEBUG_CHOL_MODE (value & 3): 1 per-step launches, else persistent
  int chol_acq_rel = 0;          // OMB_DEBUG_CHOL_MODE (value & 4): release / acquire hand-offs
  int chol_single = 0;           // OMB_DEBUG_CHOL_MODE (value & 8): every trailing update its own task
  int select_seq = 0;            // OMB_DEBUG_SELECT_SEQ: the sequential greedy walk for B ≤ 64 too
  int boxes_kd_wave = 0;         // OMB_DEBUG_BOXES_KD: omb_ehvi_boxes_k by one wavefront per candidate where that fits
  int paths_libcos = 0;          // OMB_DEBUG_PATHS_LIBCOS: the sample paths' features through the library cosine
  int hvi_paths_chunk = (int)kHviPathsChunk;   // OMB_DEBUG_HVI_PATHS_CHUNK: candidates per pass of a sampled-front chain
  int posterior_all_var = 0;     // OMB_DEBUG_POSTERIOR_ALL_VAR: the chain computes σ² of every objective
  int posterior_mean_kernel = kMeanKernelAfter;   // OMB_DEBUG_POSTERIOR_MEAN_KERNEL: masked objectives' μ in a launch of its own
  int argmax_prune = 1;          // OMB_DEBUG_ARGMAX_PRUNE: 0 dense, 1 two-phase (seed by bound) from kPruneMinN
                                 // candidates, 2 the strided seed at any N, 3 the seed by bound at any N
  int argmax_staged = 1;         // OMB_DEBUG_ARGMAX_STAGED: 1 objective 1's screen and bound first, 0 §31's order
  int argmax_screen = 1;         // OMB_DEBUG_ARGMAX_SCREEN: the two-phase path's bound from 1 the fp32 screen, 0 fp64 means
  int argmax_cut = 1;            // OMB_DEBUG_ARGMAX_CUT: the staged order's first list by 1 one cut on μ̃₁ − ε₁, 0 ubm1 per candidate
};

namespace {

int fail(omb_ctx* ctx, int code, const char* fmt, ...) {
  if (ctx) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    ctx->err = buf;
  }
  return code;
}

int hip_fail(omb_ctx* ctx, hipError_t e, const char* where) {
  return fail(ctx, OMB_EHIP, "%s: %s", where, hipGetErrorString(e));
}

#define OMB_HIP(ctx, call)                                   \
  do {                                                       \
    hipError_t e_ = (call);                                  \
    if (e_ != hipSuccess) return hip_fail(ctx, e_, #call);   \
  } while (0)

// Reports (once) a fault a kernel marked since the last report.
int check_fault(omb_ctx* ctx) {
  const int f = __atomic_exchange_n(ctx->fault_host, 0, __ATOMIC_ACQ_REL);
  if (f & kFaultSpin)
    return fail(ctx, OMB_EHIP, "posterior kernel: an LDS counter-ring wait exceeded %d polls; the posterior "
                "moments (and acquisition values) computed since the previous call are invalid", ctx->spin_limit);
  return OMB_OK;
}

int enter(omb_ctx* ctx) {
  if (!ctx) return OMB_EINVAL;
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
  return check_fault(ctx);
}

// GPArgs of the posterior launches: zeroed, with the context's fault word and spin bound.
void init_args(omb_ctx* ctx, GPArgs* args) {
  memset(args, 0, sizeof(*args));
  args->fault = ctx->fault_dev;
  args->spin_limit = ctx->spin_limit;
}

// GP state of objectives 0..n_obj-1, all set, sharing d.
int gather_gp(omb_ctx* ctx, int n_obj, GPArgs* args, int* max_R) {
  if (n_obj < 1 || n_obj > OMB_MAX_OBJ) return fail(ctx, OMB_EINVAL, "n_obj=%d outside [1, %d]", n_obj, OMB_MAX_OBJ);
  init_args(ctx, args);
  *max_R = 0;
  for (int o = 0; o < n_obj; ++o) {
    const ObjState& s = ctx->obj[o];
    if (!s.set) return fail(ctx, OMB_ESTATE, "objective %d has no GP state (call omb_set_gp)", o);
    if (s.d != ctx->obj[0].d) return fail(ctx, OMB_EINVAL, "objectives disagree on n_var (%d vs %d)", s.d, ctx->obj[0].d);
    if (s.kind != ctx->obj[0].kind) return fail(ctx, OMB_EINVAL, "objectives disagree on kernel kind");
    args->gp[o] = s.dev;
    if (s.R > *max_R) *max_R = s.R;
  }
  args->d = ctx->obj[0].d;
  args->DP = ctx->obj[0].DP;
  return OMB_OK;
}

// The context's error sink for the host-only checks (omb_host.cpp).
std::string* E(omb_ctx* ctx) { return ctx ? &ctx->err : nullptr; }

// ---- ctx-owned buffers
int grow_dev(omb_ctx* ctx, DevBuf& b, size_t bytes, const char* what) {
  if (bytes <= b.cap) return OMB_OK;
  OMB_HIP(ctx, hipStreamSynchronize(ctx->stream));  // queued kernels may still read the old buffer
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
  if (hipMalloc(&b.p, bytes) != hipSuccess) return fail(ctx, OMB_ENOMEM, "hipMalloc(%zu) for %s", bytes, what);
  b.cap = bytes;
  return OMB_OK;
}

// Pinned staging for a host→device upload of `bytes`; the previous upload is complete on return.
int stage_begin(omb_ctx* ctx, size_t bytes, void** host) {
  OMB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (bytes > ctx->stage_cap) {
    if (ctx->stage) (void)hipHostFree(ctx->stage);
    ctx->stage = nullptr;
    ctx->stage_cap = 0;
    if (hipHostMalloc(&ctx->stage, bytes, hipHostMallocDefault) != hipSuccess)
      return fail(ctx, OMB_ENOMEM, "hipHostMalloc(%zu) for staging", bytes);
    ctx->stage_cap = bytes;
  }
  *host = ctx->stage;
  return OMB_OK;
}

// ---- one description per acquisition: describe_* validates the scalars and fills the Plan (geo / boxes stay unset)
// bits 0..k-1
unsigned all_objectives(int k) { return k >= 32 ? ~0u : (1u << k) - 1u; }

int describe_ehvi2d(omb_ctx* ctx, int P, const double* r, double s00, double s01, int mode, Plan* pl) {
  int rc = check_ehvi2d(E(ctx), P, r, mode);
  if (rc) return rc;
  pl->kind = PLAN_EHVI2D;
  pl->k = 2;
  // ehvi2d_kernel / ehvi2d_argmax_kernel: reference mode passes 0 for σ²₁ (σ²₀ serves both objectives)
  pl->var_mask = mode == OMB_EHVI_REFERENCE ? 1u : 3u;
  pl->P = P;
  pl->mode = mode;
  pl->r[0] = r[0];
  pl->r[1] = r[1];
  pl->s00 = s00;
  pl->s01 = s01;
  return OMB_OK;
}

int describe_ehvi_mc(omb_ctx* ctx, int k, int M, const double* r, double hv_pf, Plan* pl) {
  int rc = check_ehvi_mc(E(ctx), k, M, r);
  if (rc) return rc;
  pl->kind = PLAN_EHVI_MC;
  pl->k = k;
  pl->var_mask = 1u;   // ehvi_mc_kernel: σ²₀ for every objective
  pl->M = M;
  for (int j = 0; j < k; ++j) pl->r[j] = r[j];
  pl->hv = hv_pf;
  return OMB_OK;
}

// kd: omb_ehvi_boxes_k / omb_plan_ehvi_boxes_k (the k-D kernel, any 2 ≤ k ≤ OMB_MAX_OBJ), else k = 2, 3
int describe_boxes(omb_ctx* ctx, bool kd, int k, int C, int B, Plan* pl) {
  int rc = kd ? check_boxes_k(E(ctx), k, C, B) : check_boxes(E(ctx), k, C, B);
  if (rc) return rc;
  pl->kind = PLAN_EHVI_BOXES;
  pl->boxes_kd = kd;
  pl->k = k;
  pl->var_mask = all_objectives(k);
  pl->C = C;
  pl->B = B;
  return OMB_OK;
}

int describe_hvpoi(omb_ctx* ctx, int C, Plan* pl) {
  int rc = check_hvpoi(E(ctx), C);
  if (rc) return rc;
  pl->kind = PLAN_HVPOI;
  pl->k = 2;
  pl->var_mask = 3u;
  pl->C = C;
  return OMB_OK;
}

int describe_expdec(omb_ctx* ctx, int k, int M, int scal_id, const double* params, const double* weights,
                    const double* ideal, const double* max_point, double agg_min, Plan* pl) {
  int rc = build_scal(E(ctx), k, M, scal_id, params, weights, ideal, max_point, agg_min, &pl->sp);
  if (rc) return rc;
  pl->kind = PLAN_EXPDEC;
  pl->k = k;
  pl->var_mask = 1u;   // expdec_kernel: σ²₀ for every objective
  pl->M = M;
  return OMB_OK;
}

int describe_ei(omb_ctx* ctx, int kind, int k, double best, double var_eps, double pof_eps, Plan* pl) {
  int rc = check_ei(E(ctx), kind, k, var_eps, pof_eps);
  if (rc) return rc;
  pl->kind = PLAN_EI;
  pl->ei_kind = kind;
  pl->k = k;
  // ei_kernel: EI of objective 0; the Pareto kind multiplies by μ₁, the constrained kind reads every σ²
  pl->var_mask = kind == OMB_EI_CONSTRAINED ? all_objectives(k) : 1u;
  pl->best = best;
  pl->var_eps = var_eps;
  pl->pof_eps = pof_eps;
  return OMB_OK;
}

// omb_mes / omb_plan_mes (the stand-alone entry's y* is on the device and is not inspected; the plan entry checks its
// host copy before it installs it)
int describe_mes(omb_ctx* ctx, int k, int S, Plan* pl) {
  int rc = check_mes(E(ctx), k, S, nullptr, nullptr, 0, 0, nullptr, nullptr);
  if (rc) return rc;
  pl->kind = PLAN_MES;
  pl->k = k;
  pl->var_mask = all_objectives(k);   // mes_kernel: γ_js over every σ_j
  pl->S = S;
  return OMB_OK;
}

// omb_hvi_paths / omb_plan_hvi_paths: every argument of the stand-alone entry; the plan entry passes y = out = null,
// N = 0 and its host arrays.  The offsets are kept in the Plan (the launch takes them from the host).
int describe_hvi_paths(omb_ctx* ctx, int k, int S, const void* y, int64_t ld, int64_t N, const void* coords, int C,
                       const int32_t* box_off, const void* boxes, const void* out, Plan* pl) {
  int rc = check_hvi_paths(E(ctx), k, S, y, ld, N, coords, C, box_off, boxes, out);
  if (rc) return rc;
  pl->kind = PLAN_HVI_PATHS;
  pl->k = k;
  pl->var_mask = 0u;   // no posterior moment is read: the chain evaluates the paths instead
  pl->S = S;
  pl->C = C;
  for (int s = 0; s <= kPathsMaxS; ++s) pl->box_off[s] = box_off[s < S ? s : S];
  return OMB_OK;
}

// omb_hvi_paths_con / omb_plan_hvi_paths_con: describe_hvi_paths' description with the constraint slots behind it.
int describe_hvi_paths_con(omb_ctx* ctx, int k, int S, int n_con, const void* y, int64_t ld, int64_t N,
                           const void* coords, int C, const int32_t* box_off, const void* boxes, double eta,
                           unsigned flags, const void* out, const void* u, Plan* pl) {
  int rc = check_hvi_paths_con(E(ctx), k, S, n_con, y, ld, N, coords, C, box_off, boxes, eta, flags, out, u);
  if (rc) return rc;
  // every check of describe_hvi_paths has passed (a null out aside, which it never reads)
  if ((rc = describe_hvi_paths(ctx, k, S, nullptr, 0, 0, coords, C, box_off, boxes, nullptr, pl))) return rc;
  pl->kind = PLAN_HVI_PATHS_CON;
  pl->path_con = n_con;
  pl->path_eta = eta;
  pl->path_flags = flags;
  return OMB_OK;
}

// The described sampled-front improvement over path values y ((k [+ path_con])·S rows at pitch ld), N > 0: the only
// place that launches hvi_paths_kernel / hvi_paths_con_kernel (the stand-alone entries and the chain's chunks).
// u: omb_hvi_paths_con's per-path output (PLAN_HVI_PATHS_CON only).
int run_hvi_paths(omb_ctx* ctx, const Plan& pl, const double* y, int64_t ld, int64_t N, double* out, const char* where,
                  double* u = nullptr) {
  const int64_t wsd = hvi_paths_ws_doubles(N, pl.S);
  int rc;
  if (wsd && (rc = grow_dev(ctx, ctx->hws, sizeof(double) * (size_t)wsd, "HVI path workspace"))) return rc;
  double* ws = wsd ? ctx->hws.as<double>() : nullptr;
  hipError_t e = pl.kind == PLAN_HVI_PATHS_CON
                     ? launch_hvi_paths_con(ctx->stream, pl.k, pl.S, pl.path_con, y, ld, N, pl.geo, pl.C, pl.boxes,
                                            pl.box_off, pl.path_eta, (pl.path_flags & OMB_CON_VIOLATION) != 0, out, u, ws)
                     : launch_hvi_paths(ctx->stream, pl.k, pl.S, y, ld, N, pl.geo, pl.C, pl.boxes, pl.box_off, out, ws);
  if (e != hipSuccess) return hip_fail(ctx, e, where);
  return OMB_OK;
}

// omb_ehvi_boxes_k's kernel: candidate-blocked, or (OMB_DEBUG_BOXES_KD = 1, where its tables fit) the baseline
hipError_t launch_boxes_k(omb_ctx* ctx, int k, const double* mu, const double* var, int64_t ld, int64_t N,
                          const double* coords, int C, const uint16_t* boxes, int B, double* out) {
  if (ctx->boxes_kd_wave && 9 * (int64_t)k * C <= kMaxLdsDoubles)
    return launch_ehvi_boxes_wave(ctx->stream, k, mu, var, ld, N, coords, C, boxes, B, out);
  return launch_ehvi_boxes_kd(ctx->stream, k, mu, var, ld, N, coords, C, boxes, B, out);
}

// The described acquisition over the moments (k, N) at row pitch ld: the only switch that launches value kernels.
// raised: Monte-Carlo EHVI's per-candidate flags.  (Every Plan comes from a describe_*: no other kind exists.)
hipError_t launch_acq(omb_ctx* ctx, const Plan& pl, const double* mu, const double* var, int64_t ld, int64_t N,
                      double* out, int32_t* raised) {
  hipStream_t st = ctx->stream;
  switch (pl.kind) {
    case PLAN_EHVI2D:
      return launch_ehvi2d(st, mu, var, ld, N, pl.geo, pl.P, pl.r[0], pl.r[1], pl.s00, pl.s01, pl.mode, out);
    case PLAN_EHVI_MC:
      return launch_ehvi_mc(st, pl.k, mu, var, ld, N, pl.geo, pl.M, pl.r, pl.hv, out, raised);
    case PLAN_EHVI_BOXES:
      if (pl.log) return launch_log_ehvi_boxes(st, pl.k, mu, var, ld, N, pl.geo, pl.C, pl.boxes, pl.B, out);
      return pl.boxes_kd ? launch_boxes_k(ctx, pl.k, mu, var, ld, N, pl.geo, pl.C, pl.boxes, pl.B, out)
                         : launch_ehvi_boxes(st, pl.k, mu, var, ld, N, pl.geo, pl.C, pl.boxes, pl.B, out);
    case PLAN_HVPOI:
      return launch_hvpoi(st, mu, var, ld, N, pl.geo, pl.C, out);
    case PLAN_EXPDEC:
      return launch_expdec(st, pl.sp, mu, var, ld, N, pl.geo, pl.M, out);
    case PLAN_EI:
      if (pl.log) return launch_log_ei(st, pl.ei_kind, pl.k, mu, var, ld, N, pl.best, pl.var_eps, pl.pof_eps, out);
      return launch_ei(st, pl.ei_kind, pl.k, mu, var, ld, N, pl.best, pl.var_eps, pl.pof_eps, out);
    case PLAN_MES:
      return launch_mes(st, pl.k, mu, var, ld, N, pl.geo, pl.S, out);
    default:
      return hipErrorInvalidValue;
  }
}

// ∂a/∂μ | ∂a/∂σ² (k, N) of the described acquisition over the moments at row pitch N: the only switch that launches
// gradient kernels, and the only place that knows which plans have no analytic gradient.  With dadm == nullptr it
// launches nothing and answers only that question (omb_eval_grad asks before it looks at the GP state).
int launch_acq_grad(omb_ctx* ctx, const Plan& pl, const double* mu, const double* var, int64_t N, double* dadm,
                    double* dadv) {
  hipStream_t st = ctx->stream;
  const char* unsup = nullptr;
  hipError_t e = hipSuccess;
  switch (pl.kind) {
    case PLAN_EHVI2D:
      if (pl.mode == OMB_EHVI_SIGMA) unsup = "EHVI-2D in OMB_EHVI_SIGMA mode";
      else if (dadm)
        e = launch_ehvi2d_grad(st, mu, var, N, N, pl.geo, pl.P, pl.r[0], pl.r[1], pl.s00, pl.s01, pl.mode, dadm, dadv);
      break;
    case PLAN_EHVI_BOXES:
      if (pl.log) unsup = "log exact EHVI";   // a box-sum gradient in log space: not yet
      else if (dadm) e = launch_ehvi_boxes_grad(st, pl.k, mu, var, N, N, pl.geo, pl.C, pl.boxes, pl.B, dadm, dadv);
      break;
    case PLAN_EI:
      if (dadm && pl.log)
        e = launch_log_ei_grad(st, pl.ei_kind, pl.k, mu, var, N, N, pl.best, pl.var_eps, pl.pof_eps, dadm, dadv);
      else if (dadm)
        e = launch_ei_grad(st, pl.ei_kind, pl.k, mu, var, N, N, pl.best, pl.var_eps, pl.pof_eps, dadm, dadv);
      break;
    case PLAN_MES:
      if (dadm) e = launch_mes_grad(st, pl.k, mu, var, N, N, pl.geo, pl.S, dadm, dadv);
      break;
    case PLAN_EHVI_MC: unsup = "Monte-Carlo EHVI"; break;
    case PLAN_EXPDEC: unsup = "expected decomposition"; break;
    case PLAN_HVPOI: unsup = "HV-PoI"; break;
    case PLAN_HVI_PATHS: unsup = "sampled-front improvement (noisy EHVI / EI)"; break;
    case PLAN_HVI_PATHS_CON: unsup = "constrained sampled-front improvement (noisy EHVI / EI)"; break;
    default:
      return fail(ctx, OMB_ESTATE, "corrupt plan");
  }
  if (unsup) return fail(ctx, OMB_EUNSUP, "the %s plan has no analytic gradient", unsup);
  if (e != hipSuccess) return hip_fail(ctx, e, "acquisition gradient");
  return OMB_OK;
}

// A stand-alone entry's tail, after its checks: the description over the caller's device geometry and moments.
int run_acq(omb_ctx* ctx, Plan& pl, const double* geo_dev, const uint16_t* boxes_dev, const double* mu,
            const double* var, int64_t ld, int64_t N, double* out, int32_t* raised, const char* where) {
  if (N == 0) return OMB_OK;
  pl.geo = geo_dev;
  pl.boxes = boxes_dev;
  hipError_t e = launch_acq(ctx, pl, mu, var, ld, N, out, raised);
  if (e != hipSuccess) return hip_fail(ctx, e, where);
  return OMB_OK;
}

// A plan entry's head: an invalid request leaves no plan behind.
int plan_enter(omb_ctx* ctx) {
  int rc = enter(ctx);
  if (rc == OMB_OK) ctx->plan = Plan();
  return rc;
}

// A plan entry's tail, after its checks: the host spans a | b through the pinned staging into ctx->geo, and the
// description, pointed at them, becomes the context's plan.
int install_plan(omb_ctx* ctx, Plan& pl, const void* a, size_t abytes, const void* b = nullptr, size_t bbytes = 0) {
  void* h = nullptr;
  int rc = stage_begin(ctx, abytes + bbytes, &h);
  if (rc) return rc;
  memcpy(h, a, abytes);
  if (bbytes) memcpy(static_cast<char*>(h) + abytes, b, bbytes);
  if ((rc = grow_dev(ctx, ctx->geo, abytes + bbytes, "plan geometry"))) return rc;
  OMB_HIP(ctx, hipMemcpyAsync(ctx->geo.p, h, abytes + bbytes, hipMemcpyHostToDevice, ctx->stream));
  pl.geo = ctx->geo.as<const double>();
  if (bbytes) pl.boxes = reinterpret_cast<const uint16_t*>(ctx->geo.as<const char>() + abytes);
  ctx->plan = pl;
  return OMB_OK;
}

// Posterior of objectives 0..n_obj-1 (their state in args.gp, dense L⁻¹ in Ld[o]): the fused kernel
// when every n_train fits it, else per objective and candidate chunk K block → V = L⁻¹K* (GEMM) →
// column reduction.

hipError_t posterior_any(omb_ctx* ctx, const GPArgs& args, const double* const* Ld, int n_obj, int max_R,
                         const double* Xc, int64_t N, double* mu, double* var) {
  // the fused kernel keeps the candidates' B fragments in registers: n_var ≤ 64 (kMaxFusedDP)
  if (16 * max_R <= OMB_MAX_TRAIN && args.DP <= kMaxFusedDP)
    return launch_posterior(ctx->stream, args, n_obj, max_R, Xc, N, mu, var, ctx->posterior_mean_kernel);
  // the dense path ignores args.var_skip: it computes σ² of every objective
  for (int o = 0; o < n_obj; ++o) {
    const int64_t n = args.gp[o].n;
    int64_t Nc = (int64_t)(((size_t)256 << 20) / (16 * (size_t)n));   // K* and V chunks of 128 MiB each
    Nc = Nc < 256 ? 256 : (Nc / 256) * 256;
    if (Nc > N) Nc = N;
    if (grow_dev(ctx, ctx->dws, sizeof(double) * 2 * (size_t)n * Nc, "dense posterior workspace"))
      return hipErrorOutOfMemory;
    double* Kst = ctx->dws.as<double>();
    double* V = Kst + (size_t)n * Nc;
    for (int64_t c0 = 0; c0 < N; c0 += Nc) {
      const int64_t nc = (N - c0) < Nc ? (N - c0) : Nc;
      hipError_t e = launch_kernel_block(ctx->stream, args, o, Xc + c0 * args.d, nc, Kst);
      if (e == hipSuccess) e = launch_gemm_ltri_nn(ctx->stream, n, nc, 1.0, Ld[o], n, Kst, nc, 0.0, V, nc);
      if (e == hipSuccess)
        e = launch_post_colreduce(ctx->stream, Kst, V, n, nc, args.gp[o].alpha, args.gp[o].variance,
                                  mu + (int64_t)o * N + c0, var + (int64_t)o * N + c0);
      if (e != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

void gather_Ld(omb_ctx* ctx, int n_obj, const double** Ld) {
  for (int o = 0; o < n_obj; ++o) Ld[o] = ctx->obj[o].Ld;
}

// A sampled-front plan's state checks, before anything is launched, and its path arguments: every slot of
// 0..k-1 (and the constraint slots behind them under PLAN_HVI_PATHS_CON) holds a GP and exactly the plan's S sample paths (install_gp drops them, so a plan over a changed state is
// refused here, never evaluated), within omb_paths_eval's limits.
int chain_paths(omb_ctx* ctx, const Plan& pl, PathArgs* pa) {
  PathsObjInfo info[OMB_MAX_OBJ];
  for (int o = 0; o < OMB_MAX_OBJ; ++o) {
    const ObjState& s = ctx->obj[o];
    info[o] = PathsObjInfo{s.set ? 1 : 0, s.d, s.n, s.path_S};
  }
  const int slots = pl.k + pl.path_con;
  for (int o = 0; o < slots; ++o) {
    const ObjState& s = ctx->obj[o];
    if (!s.set)
      return fail(ctx, OMB_ESTATE, "objective %d has no GP state (call omb_set_gp, then omb_paths_set)", o);
    if (s.path_S < 1) return fail(ctx, OMB_ESTATE, "objective %d has no sample paths (call omb_paths_set)", o);
    if (s.path_S != pl.S)
      return fail(ctx, OMB_ESTATE, "objective %d holds %d sample paths, the plan has %d fronts (call omb_paths_set)",
                  o, s.path_S, pl.S);
  }
  int rc = check_paths_eval(E(ctx), slots, nullptr, 0, 0, nullptr, info);   // what is left: omb_paths_eval's OMB_EUNSUP
  if (rc) return rc;
  for (int o = 0; o < slots; ++o) {
    const ObjState& s = ctx->obj[o];
    pa->o[o] = PathObj{s.dev, s.path_Of, s.path_Wf, s.path_Vf, s.path_MT, s.R, s.path_S, 0};
  }
  pa->d = ctx->obj[0].d;
  pa->DP = ctx->obj[0].DP;
  return OMB_OK;
}

// Batch sizes of the arg-max chain's two-phase path.  Below 2^16 candidates the dense step is a sixteenth of config
// 3's or less (0.34 ms at n_train 512) and the path's nine extra launches are a tenth of that or more; the lists hold
// 32-bit indices.
constexpr int64_t kPruneMinN = 1 << 16;
constexpr int64_t kPruneMaxN = 1ll << 30;

// The fused chain: [Sobol →] posterior(0..k-1) → planned acquisition → [arg-max].  Under a sampled-front plan
// (PLAN_HVI_PATHS) the posterior stage is the evaluation of the installed sample paths, in passes of Nc candidates.  The posterior computes σ² of the
// objectives in the plan's var_mask only (the others' slots of the workspace keep whatever they held); all_var (the
// gradient chain, which reads every σ² afterwards, and OMB_DEBUG_POSTERIOR_ALL_VAR) computes all of them.
int run_chain(omb_ctx* ctx, const double* Xc, bool sobol, int64_t start, int64_t N, int64_t offset, double* vals_out,
              double* result_dev, bool all_var = false, double* acq_raw = nullptr) {
  int rc = enter(ctx);
  if (rc) return rc;
  const Plan& pl = ctx->plan;
  if (pl.kind == PLAN_NONE) return fail(ctx, OMB_ESTATE, "no acquisition plan (call an omb_plan_* function)");
  if (N < 0) return fail(ctx, OMB_EINVAL, "N=%lld < 0", (long long)N);
  // the posterior stage is the evaluation of the sample paths (of the path_con constraint slots too)
  const bool paths = pl.kind == PLAN_HVI_PATHS || pl.kind == PLAN_HVI_PATHS_CON;
  PathArgs pa{};
  if (paths && (rc = chain_paths(ctx, pl, &pa))) return rc;
  GPArgs args;
  int max_R = 0;
  if ((rc = gather_gp(ctx, pl.k + pl.n_con + pl.path_con, &args, &max_R))) return rc;
  if (!all_var && !ctx->posterior_all_var) args.var_skip = all_objectives(pl.k) & ~pl.var_mask;
  if (sobol) {
    if (ctx->sob_d == 0) return fail(ctx, OMB_ESTATE, "no Sobol state (call omb_set_sobol)");
    if (ctx->sob_d != args.d) return fail(ctx, OMB_EINVAL, "Sobol dimension %d != n_var %d", ctx->sob_d, args.d);
    if (start < 0 || start + N > (int64_t)(1ull << ctx->sob_bits))
      return fail(ctx, OMB_EINVAL, "Sobol indices [%lld, %lld) outside [0, 2^%d)", (long long)start,
                  (long long)(start + N), ctx->sob_bits);
  } else if (N > 0 && !Xc) {
    return fail(ctx, OMB_EINVAL, "null candidate pointer");
  }
  if ((N + 31) / 32 > 0x7fffffffLL) return fail(ctx, OMB_EUNSUP, "N=%lld too large", (long long)N);
  const int k = pl.k;
  const int K = k + pl.n_con;   // rows of the workspace: the objectives, then the constraint models
  const size_t nd = (size_t)N;
  // EHVI-2D with the arg-max's first pass in its launch (launch_ehvi2d_argmax) when only the pair is wanted; its
  // per-workgroup pairs (≤ kArgmaxMaxBlocks) go to ctx->partials
  const bool acq_argmax = result_dev && !vals_out && N > 0 && ctx->fused_chain && pl.kind == PLAN_EHVI2D &&
                          pl.n_con == 0;   // the weight comes between EHVI and the arg-max: the plain path
  // a sampled-front plan holds the (k·S, Nc) path values of one pass over Nc candidates in place of μ | σ² (K, N):
  // both of its kernels are per-candidate functions, so the values do not depend on the chunk
  const int64_t Nc = (paths && ctx->hvi_paths_chunk > 0 && ctx->hvi_paths_chunk < N) ? ctx->hvi_paths_chunk : N;
  const size_t head = paths ? (size_t)(k + pl.path_con) * pl.S * (size_t)Nc : 2 * (size_t)K * nd;
  const size_t doubles = head + nd + (nd + 1) / 2 + (sobol ? nd * args.d : 0);
  if ((rc = grow_dev(ctx, ctx->work, (doubles ? doubles : 1) * sizeof(double), "chain workspace"))) return rc;
  if (paths && N > 0) {
    // the largest any pass asks for (a short last pass may split where the full ones do not): before the marks
    const int64_t wsa = hvi_paths_ws_doubles(Nc, pl.S), wsb = hvi_paths_ws_doubles(N % Nc, pl.S);
    const int64_t wsd = wsa > wsb ? wsa : wsb;
    if (wsd && (rc = grow_dev(ctx, ctx->hws, sizeof(double) * (size_t)wsd, "HVI path workspace"))) return rc;
  }
  // The two-phase arg-max where the plan has a bound, nothing comes between the acquisition and the
  // arg-max, posterior_mean_kernel and a ring kernel exist for the shape, and the batch is large enough for the
  // launches it adds (kPruneMinN; OMB_DEBUG_ARGMAX_PRUNE 2 and 3: any size).  Everything else keeps the dense chain.
  const bool two_phase = result_dev && !vals_out && !acq_raw && !all_var && !ctx->posterior_all_var && !paths &&
                         pl.kind == PLAN_EHVI2D && pl.prune_ok && pl.n_con == 0 && !pl.log && k == 2 &&
                         posterior_gather_fits(args, max_R) && N >= 1 && N <= kPruneMaxN &&
                         (ctx->argmax_prune >= 2 || (ctx->argmax_prune == 1 && N >= kPruneMinN));
  // The seed: each group's best bound — or, under OMB_DEBUG_ARGMAX_PRUNE 2, the strided sample of §29
  const bool seed_by_bound = ctx->argmax_prune != 2;
  const int64_t seed_step = seed_by_bound ? kPruneSeedGroup : kPruneStride;
  // The staged order where the seed by bound runs on the screen: objective 1's screen and its bound for
  // all N, objective 0's screen and the full bound only for those that pass
  const bool staged = two_phase && seed_by_bound && ctx->argmax_screen != 0 && ctx->argmax_staged != 0;
  // ubm1 decreases in μ̃₁ − ε₁, so the staged order's first list is one cut on that number
  const bool cut = staged && ctx->argmax_cut != 0;
  if (two_phase && (rc = grow_dev(ctx, ctx->prws, (size_t)prune_ws_bytes(N), "arg-max pruning workspace"))) return rc;
  if (result_dev) {
    ctx->prune_taken = two_phase ? 1 : 0;
    ctx->prune_seed = two_phase ? (N + seed_step - 1) / seed_step : 0;
    ctx->stage_taken = staged ? 1 : 0;
    ctx->cut_taken = cut ? 1 : 0;
  }
  double* mu = ctx->work.as<double>();
  double* var = mu + (size_t)K * nd;
  double* vals = vals_out ? vals_out : mu + head;
  int32_t* raised = reinterpret_cast<int32_t*>(mu + head + nd);
  double* Xs = mu + head + nd + (nd + 1) / 2;
  // with constraints the caller may want the unweighted acquisition kept (omb_eval_grad): it goes to acq_raw and the
  // weighted value to vals; otherwise the weight is applied in place
  double* acq = (pl.n_con && acq_raw) ? acq_raw : vals;

  hipEvent_t* ev = nullptr;
  if (ctx->timing && ctx->timing_calls++ % ctx->timing_stride == 0) {
    if (ctx->ev_used + 5 > ctx->ev.size() && ctx->ev.size() < 5 * 4096) {
      for (int i = 0; i < 5 * 64; ++i) {
        hipEvent_t e;
        OMB_HIP(ctx, hipEventCreate(&e));
        ctx->ev.push_back(e);
      }
    }
    if (ctx->ev_used + 5 <= ctx->ev.size()) {
      ev = ctx->ev.data() + ctx->ev_used;
      ctx->ev_used += 5;
    }
  }
  // Each event record costs a few µs of GPU time, so level 1 records only around the posterior.
  const int level = ctx->timing;
  auto mark = [&](int i) -> hipError_t {
    if (!ev) return hipSuccess;
    if (level == 1 && i != 1 && i != 2) return hipSuccess;
    return hipEventRecord(ev[i], ctx->stream);
  };
  hipError_t e = mark(0);
  if (e == hipSuccess && sobol && N > 0) e = launch_sobol(ctx->stream, ctx->sob, ctx->sob_d, ctx->sob_bits, start, N, Xs);
  if (sobol) Xc = Xs;
  if (e == hipSuccess) e = mark(1);
  const double* Ld[OMB_MAX_OBJ];
  gather_Ld(ctx, K, Ld);
  if (paths) {
    // per pass: the paths of objectives 0..k-1 at Nc candidates, then their mean improvement into vals.  Mark 2 stands
    // after the last pass's path evaluation: with several passes the "posterior" interval holds the earlier passes'
    // acquisition launches too (the stages alternate on one stream).
    for (int64_t c0 = 0; c0 < N && e == hipSuccess; c0 += Nc) {
      const int64_t nc = (N - c0) < Nc ? (N - c0) : Nc;
      e = launch_paths_eval(ctx->stream, pa, k + pl.path_con, ctx->obj[0].kind, ctx->paths_libcos, Xc + c0 * args.d, nc, nc, mu);
      if (e == hipSuccess && c0 + nc == N) e = mark(2);
      if (e == hipSuccess && (rc = run_hvi_paths(ctx, pl, mu, nc, nc, vals + c0, "fused chain (hvi_paths)"))) return rc;
    }
    if (e == hipSuccess && N == 0) e = mark(2);
  } else if (two_phase) {
    // both means for all N, the full posterior and the acquisition for the seed, the bound of the rest
    // against the seed's best value τ, then the full posterior and the acquisition for the survivors alone; the
    // arg-max over both sets of pairs compares original indices, so the pair is the dense chain's.  All on the stream,
    // the counts stay on the device.
    PruneWs ws;
    prune_ws_carve(ctx->prws.p, N, &ws);
    ws.stats_host = ctx->prune_stats_dev;
    const int64_t ns = (N + seed_step - 1) / seed_step, nv = N - ns;
    const int nbs = prune_list_blocks(ns), nbv = nv > 0 ? prune_list_blocks(nv) : 0;
    double* mu_c = var;                 // the workspace's σ² rows: the gathered launches' compacted μ₀ | σ²₀
    double* var_c = var + nd;
    const double sf2 = args.gp[0].variance;
    // DESIGN §30 (OMB_DEBUG_ARGMAX_SCREEN 1): no dense fp64 mean pass.  The bound reads the screen's μ̃ ± ε; μ₁ of the
    // seed and of the survivors comes from the gathered mean launch, at the candidates' original slots, where the list
    // EHVI reads it.  0: the fp64 means of §29 for all N.
    const bool screen = ctx->argmax_screen != 0;
    const double* bm = screen ? ws.scr_mu : mu;   // the bound's means and, under the screen, their margins
    const double* be0 = screen ? ws.scr_eps : nullptr;
    const double* be1 = screen ? ws.scr_eps + nd : nullptr;
    if (e == hipSuccess && !screen) e = launch_posterior_means(ctx->stream, args, 3u, Xc, N, mu);
    // the means and the bound come first; the seed is each group's best bound, so τ is (nearly) the
    // maximum and the threshold kernel leaves a handful of survivors.  §29's order: the strided seed, then the bound.
    if (e == hipSuccess && seed_by_bound && screen)
      e = launch_posterior_screen(ctx->stream, args, staged ? 2u : 3u, Xc, N, ws.scr_mu, ws.scr_eps);
    // ubm1 from μ̃₁ − ε₁ alone bounds the full bound for every μ₀, so the seed and list A come from it
    // the seed is the smallest μ̃₁ and needs no bound; the bound becomes one cut once τ₀ is known
    if (e == hipSuccess && cut) e = launch_prune_seed1(ctx->stream, ws.scr_mu + nd, N, ws);
    if (e == hipSuccess && staged && !cut)
      e = launch_prune_bound1_seed(ctx->stream, ws.scr_mu + nd, ws.scr_eps + nd, N, pl.geo, pl.P, pl.r[0], pl.s00,
                                   pl.s01, sf2, args.gp[0].alpha, args.gp[0].n, ws);
    if (e == hipSuccess && seed_by_bound && !staged)
      e = launch_prune_bound_seed(ctx->stream, bm, bm + nd, N, pl.geo, pl.P, pl.r[0], pl.s00, pl.s01, sf2, ws, be0,
                                  be1);
    if (e == hipSuccess && !seed_by_bound) e = launch_prune_seed(ctx->stream, N, ws);
    if (e == hipSuccess)
      e = launch_posterior_gather(ctx->stream, args, max_R, Xc, ws.seed_idx, ws.counts, ns, mu_c, var_c);
    if (e == hipSuccess && screen)
      e = launch_posterior_mean_gather(ctx->stream, args, 1, Xc, ws.seed_idx, ws.counts, ns, mu + nd);
    if (e == hipSuccess)
      e = launch_ehvi2d_argmax_list(ctx->stream, mu_c, var_c, mu + nd, ws.seed_idx, ws.counts, ns, pl.geo, pl.P,
                                    pl.r[0], pl.r[1], pl.s00, pl.s01, pl.mode, ws.partials);
    if (e == hipSuccess) e = launch_argmax_reduce(ctx->stream, ws.partials, nbs, 0, ws.tau);
    if (e == hipSuccess && seed_by_bound && !staged) e = launch_prune_threshold(ctx->stream, N, ws);
    if (e == hipSuccess && cut)
      e = launch_prune_cut(ctx->stream, pl.geo, pl.P, pl.r[0], pl.s00, pl.s01, sf2, args.gp[0].alpha, args.gp[0].n, ws);
    const double* cm = cut ? ws.scr_mu + nd : nullptr;   // the threshold by the cut reads μ̃₁ and ε₁
    const double* ce = cut ? ws.scr_eps + nd : nullptr;
    if (staged && nv == 0) {
      // N = 1, nothing but the seed: both lists empty, their counts and stats words written in stream order
      if (e == hipSuccess) e = launch_prune_threshold_a(ctx->stream, N, ws, cm, ce);
      if (e == hipSuccess) e = launch_prune_threshold(ctx->stream, N, ws);
    } else if (staged) {
      // list A by the threshold on ubm1 (or by the cut), objective 0's screen for list A, the full interval bound on
      // list A → list B
      if (e == hipSuccess) e = launch_prune_threshold_a(ctx->stream, N, ws, cm, ce);
      if (e == hipSuccess)
        e = launch_posterior_screen_gather(ctx->stream, args, 0, Xc, ws.list_a, ws.counts + 2, nv, ws.scr_mu,
                                           ws.scr_eps);
      if (e == hipSuccess)
        e = launch_prune_bound_list(ctx->stream, ws.scr_mu, ws.scr_mu + nd, ws.scr_eps, ws.scr_eps + nd, nv, pl.geo,
                                    pl.P, pl.r[0], pl.s00, pl.s01, sf2, ws);
    }
    if (e == hipSuccess && !seed_by_bound && screen)
      e = launch_posterior_screen(ctx->stream, args, 3u, Xc, N, ws.scr_mu, ws.scr_eps);
    if (e == hipSuccess && !seed_by_bound)
      e = launch_prune_bound(ctx->stream, bm, bm + nd, N, pl.geo, pl.P, pl.r[0], pl.s00, pl.s01, sf2, ws, be0, be1);
    if (e == hipSuccess && nv > 0)
      e = launch_posterior_gather(ctx->stream, args, max_R, Xc, ws.surv_idx, ws.counts + 1, nv, mu_c, var_c);
    if (e == hipSuccess && nv > 0 && screen)
      e = launch_posterior_mean_gather(ctx->stream, args, 1, Xc, ws.surv_idx, ws.counts + 1, nv, mu + nd);
    if (e == hipSuccess) e = mark(2);
    if (e == hipSuccess && nv > 0)
      e = launch_ehvi2d_argmax_list(ctx->stream, mu_c, var_c, mu + nd, ws.surv_idx, ws.counts + 1, nv, pl.geo, pl.P,
                                    pl.r[0], pl.r[1], pl.s00, pl.s01, pl.mode, ws.partials + 2 * nbs);
    if (e == hipSuccess) e = mark(3);
    if (e == hipSuccess) e = launch_argmax_reduce(ctx->stream, ws.partials, nbs + nbv, offset, result_dev);
  } else if (e == hipSuccess && N > 0) {
    e = posterior_any(ctx, args, Ld, K, max_R, Xc, N, mu, var);
  }
  if (e == hipSuccess && !paths && !two_phase) e = mark(2);
  if (e == hipSuccess && N > 0 && !paths && !two_phase) {
    if (acq_argmax) {
      unsigned* ticket = ctx->fused_chain == 1 ? reinterpret_cast<unsigned*>(ctx->partials + 2 * kArgmaxMaxBlocks)
                                               : nullptr;
      const ArgmaxOut am{ctx->partials, ticket, result_dev, offset};
      e = launch_ehvi2d_argmax(ctx->stream, mu, var, N, N, pl.geo, pl.P, pl.r[0], pl.r[1], pl.s00, pl.s01, pl.mode, am);
    } else {
      e = launch_acq(ctx, pl, mu, var, N, N, acq, raised);
    }
    if (e == hipSuccess && pl.n_con)
      e = (pl.log ? launch_log_pof : launch_pof_scale)(ctx->stream, pl.n_con, mu + (size_t)k * nd,
                                                       var + (size_t)k * nd, N, N, pl.con_eps, acq, vals);
  }
  if (e == hipSuccess && !two_phase) e = mark(3);
  if (e == hipSuccess && result_dev && !acq_argmax && !two_phase)
    e = launch_argmax(ctx->stream, vals, N, offset, ctx->partials, result_dev, ctx->argmax_one_pass);
  if (e == hipSuccess) e = mark(4);
  if (e != hipSuccess) return hip_fail(ctx, e, "fused chain");
  return OMB_OK;
}

}  // namespace

extern "C" {

int omb_abi_version(void) { return OMB_ABI_VERSION; }

int omb_create(int device, omb_ctx** out) {
  if (!out) return OMB_EINVAL;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return OMB_EINVAL;
  omb_ctx* ctx = new (std::nothrow) omb_ctx();
  if (!ctx) return OMB_ENOMEM;
  ctx->device = device;
  if (hipSetDevice(device) != hipSuccess ||
      hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess ||
      hipMalloc(&ctx->partials, sizeof(double) * (2 * kArgmaxMaxBlocks + 2)) != hipSuccess ||
      hipMemset(ctx->partials, 0, sizeof(double) * (2 * kArgmaxMaxBlocks + 2)) != hipSuccess ||
      hipMalloc(&ctx->result_dev, sizeof(double) * 2) != hipSuccess ||
      hipHostMalloc(&ctx->result_host, sizeof(double) * 2, hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc(&ctx->info_host, sizeof(int) * 4, hipHostMallocDefault) != hipSuccess ||
      hipMalloc(&ctx->sob, sobol_state_bytes(OMB_MAX_DIM, 32)) != hipSuccess ||
      hipHostMalloc(&ctx->fault_host, sizeof(int), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
      hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->fault_dev), ctx->fault_host, 0) != hipSuccess ||
      hipHostMalloc(&ctx->fit_host, sizeof(double) * (OMB_MAX_DIM + 8), hipHostMallocMapped | hipHostMallocCoherent) !=
          hipSuccess ||
      hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->fit_dev), ctx->fit_host, 0) != hipSuccess ||
      hipHostMalloc(&ctx->prune_stats_host, sizeof(int64_t) * 5, hipHostMallocMapped | hipHostMallocCoherent) !=
          hipSuccess ||
      hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->prune_stats_dev), ctx->prune_stats_host, 0) !=
          hipSuccess) {
    omb_destroy(ctx);
    return OMB_ENOMEM;
  }
  *ctx->fault_host = 0;
  for (int i = 0; i < 5; ++i) ctx->prune_stats_host[i] = 0;
  ctx->stream = ctx->own_stream;
  *out = ctx;
  return OMB_OK;
}

int omb_destroy(omb_ctx* ctx) {
  if (!ctx) return OMB_OK;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  for (auto& s : ctx->obj) {
    if (s.buf) (void)hipFree(s.buf);
    if (s.pbuf) (void)hipFree(s.pbuf);
  }
  if (ctx->partials) (void)hipFree(ctx->partials);
  if (ctx->result_dev) (void)hipFree(ctx->result_dev);
  if (ctx->result_host) (void)hipHostFree(ctx->result_host);
  if (ctx->info_host) (void)hipHostFree(ctx->info_host);
  for (DevBuf* b : {&ctx->geo, &ctx->work, &ctx->tws, &ctx->ichol, &ctx->sws, &ctx->ews, &ctx->fws, &ctx->dws, &ctx->gws,
                    &ctx->aws, &ctx->hws, &ctx->pws, &ctx->nws, &ctx->nws2, &ctx->prws, &ctx->vws, &ctx->vws2})
    if (b->p) (void)hipFree(b->p);
  if (ctx->stage) (void)hipHostFree(ctx->stage);
  if (ctx->sob) (void)hipFree(ctx->sob);
  if (ctx->fault_host) (void)hipHostFree(ctx->fault_host);
  if (ctx->fit_host) (void)hipHostFree(ctx->fit_host);
  if (ctx->prune_stats_host) (void)hipHostFree(ctx->prune_stats_host);
  for (hipEvent_t e : ctx->ev) (void)hipEventDestroy(e);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  delete ctx;
  return OMB_OK;
}

int omb_set_stream(omb_ctx* ctx, void* hip_stream) {
  if (!ctx) return OMB_EINVAL;
  ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
  return OMB_OK;
}

int omb_use_own_stream(omb_ctx* ctx) {
  if (!ctx) return OMB_EINVAL;
  ctx->stream = ctx->own_stream;
  return OMB_OK;
}

int omb_synchronize(omb_ctx* ctx) {
  int rc = enter(ctx);
  if (rc) return rc;
  OMB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return check_fault(ctx);
}

// omb_debug_set's plain switches: the value goes into the field when it lies in [lo, hi], else the message (one %lld:
// the value) is the error.  On/off switches have no message: any non-zero value is on.
struct DebugSwitch {
  int code;
  int omb_ctx::*field;
  int64_t lo, hi;
  const char* msg;
};
static const DebugSwitch kDebugSwitches[] = {
    {OMB_DEBUG_SPIN_LIMIT, &omb_ctx::spin_limit, 0, 0x7fffffff, "spin limit %lld outside [0, 2^31)"},
    {OMB_DEBUG_FUSED_CHAIN, &omb_ctx::fused_chain, 0, 2, "fused chain %lld (0, 1 or 2)"},
    {OMB_DEBUG_TIMING_STRIDE, &omb_ctx::timing_stride, 1, 0x7fffffff, "timing stride %lld < 1"},
    {OMB_DEBUG_POSTERIOR_MEAN_KERNEL, &omb_ctx::posterior_mean_kernel, 0, 2,
     "posterior mean kernel %lld (0 off, 1 after the posterior launch, 2 before it)"},
    {OMB_DEBUG_COV_TABLE, &omb_ctx::cov_table, 0, 1, nullptr},
    {OMB_DEBUG_COV_FUSED, &omb_ctx::cov_fused, 0, 1, nullptr},
    {OMB_DEBUG_SYRK_GLDS, &omb_ctx::syrk_glds, 0, 1, nullptr},
    {OMB_DEBUG_SELECT_SEQ, &omb_ctx::select_seq, 0, 1, nullptr},
    {OMB_DEBUG_BOXES_KD, &omb_ctx::boxes_kd_wave, 0, 1, nullptr},
    {OMB_DEBUG_PATHS_LIBCOS, &omb_ctx::paths_libcos, 0, 1, nullptr},
    {OMB_DEBUG_HVI_PATHS_CHUNK, &omb_ctx::hvi_paths_chunk, 0, 0x7fffffff,
     "sampled-front chain chunk %lld outside [0, 2^31) (0: one pass)"},
    {OMB_DEBUG_POSTERIOR_ALL_VAR, &omb_ctx::posterior_all_var, 0, 1, nullptr},
    {OMB_DEBUG_ARGMAX_PRUNE, &omb_ctx::argmax_prune, 0, 3,
     "arg-max pruning %lld (0 dense, 1 two-phase for large batches, 2 strided seed at any size, 3 seed by bound at "
     "any size)"},
    {OMB_DEBUG_ARGMAX_SCREEN, &omb_ctx::argmax_screen, 0, 1, nullptr},
    {OMB_DEBUG_ARGMAX_STAGED, &omb_ctx::argmax_staged, 0, 1, nullptr},
    {OMB_DEBUG_ARGMAX_CUT, &omb_ctx::argmax_cut, 0, 1, nullptr},
};

int omb_debug_set(omb_ctx* ctx, int what, int64_t value) {
  if (!ctx) return OMB_EINVAL;
  for (const DebugSwitch& s : kDebugSwitches) {
    if (s.code != what) continue;
    if (!s.msg) value = value != 0;
    else if (value < s.lo || value > s.hi) return fail(ctx, OMB_EINVAL, s.msg, (long long)value);
    ctx->*s.field = (int)value;
    return OMB_OK;
  }
  if (what == OMB_DEBUG_ARGMAX_PASSES) {
    if (value != 1 && value != 2) return fail(ctx, OMB_EINVAL, "arg-max passes %lld (1 or 2)", (long long)value);
    ctx->argmax_one_pass = value == 1;
    return OMB_OK;
  }
  if (what == OMB_DEBUG_CHOL_MODE) {
    if ((value & 3) == 3 || value < 0 || value > 14)
      return fail(ctx, OMB_EINVAL, "Cholesky mode %lld (0 auto, 1 per-step launches, 2 one persistent launch; + 4: "
                  "release / acquire hand-offs; + 8: the persistent launch's trailing updates one task per step)",
                  (long long)value);
    ctx->chol_mode = (value & 3) == 1 ? kCholSteps : kCholPersistent;   // 0 (auto) and 2 are the same schedule
    ctx->chol_acq_rel = (value & 4) ? 1 : 0;
    ctx->chol_single = (value & 8) ? 1 : 0;
    return OMB_OK;
  }
  return fail(ctx, OMB_EINVAL, "unknown debug setting %d", what);
}

const char* omb_last_error(const omb_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

// Bytes of one objective's buffer at n points, and the packing of a state into it (omb_set_gp, omb_gp_append).
static size_t gp_state_bytes(int n, int d) {
  const int DP = pad_dim(d);
  const int R = (n + 15) / 16;
  const int n_pad = kChunkRows * ((R + 3) / 4);
  const int R_pack = (n <= OMB_MAX_TRAIN) ? R : 0;   // the packed L⁻¹ feeds only the fused kernel
  const size_t doubles = (size_t)n_pad * DP + 2 * (size_t)n_pad + DP + (size_t)packed_L_size(R_pack) + (size_t)n * n +
                         (size_t)packed_X_size(n_pad, DP) + (size_t)n * d;
  return doubles * sizeof(double);
}

// Packs (X, ℓ, α, L⁻¹) of n points into buf (≥ gp_state_bytes(n, d)) on the stream and makes it the state of s;
// s.buf / s.cap are the caller's business.
static hipError_t install_gp(omb_ctx* ctx, ObjState& s, double* buf, int kernel, int n, int d, const double* X_dev,
                             const double* lengthscale_host, double variance, const double* alpha_dev,
                             const double* Linv_dev) {
  const int DP = pad_dim(d);
  const int R = (n + 15) / 16;
  const int Q = (R + 3) / 4;
  const int n_pad = kChunkRows * Q;
  const int R_pack = (n <= OMB_MAX_TRAIN) ? R : 0;
  s.path_S = 0;   // sample paths over the previous state are a silent wrong answer over this one
  double* Xs = buf;
  double* xsq = Xs + (size_t)n_pad * DP;
  double* alpha_p = xsq + n_pad;
  double* ls_p = alpha_p + n_pad;
  double* Lp = ls_p + DP;
  double* Ld = Lp + packed_L_size(R_pack);
  double* Xf = Ld + (size_t)n * n;
  double* Xraw = Xf + (size_t)packed_X_size(n_pad, DP);
  hipError_t e = launch_pack_gp(ctx->stream, n, d, DP, X_dev, lengthscale_host, alpha_dev, Linv_dev, Xs, xsq,
                                alpha_p, Lp, R_pack, n_pad);
  if (e == hipSuccess) e = launch_pack_x(ctx->stream, d, DP, n_pad, Xs, xsq, Xf);
  // the lower triangle only, zeros above: launch_gemm_tn (w = L⁻ᵀV of the gradients and the sample paths) reads all
  // of Ld, and the entries above the diagonal of the caller's L⁻¹ are not part of the contract
  if (e == hipSuccess) e = launch_copy_lower(ctx->stream, n, Linv_dev, Ld);
  if (e == hipSuccess)
    e = hipMemcpyAsync(Xraw, X_dev, sizeof(double) * (size_t)n * d, hipMemcpyDeviceToDevice, ctx->stream);
  if (e != hipSuccess) {
    s.set = false;
    return e;
  }
  s.set = true;
  s.n = n;
  s.d = d;
  s.DP = DP;
  s.R = R;
  s.n_pad = n_pad;
  s.kind = kernel;
  s.variance = variance;
  s.Ld = Ld;
  s.Xraw = Xraw;
  for (int j = 0; j < d; ++j) s.ls[j] = lengthscale_host[j];
  s.dev = GPDev{Xs, xsq, alpha_p, Lp, ls_p, variance, n, R, kernel, 0, Xf};
  return hipSuccess;
}

int omb_set_gp(omb_ctx* ctx, int obj, int kernel, int n, int d, const double* X_dev, const double* lengthscale_host,
               double variance, const double* alpha_dev, const double* Linv_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  if ((rc = check_gp_args(E(ctx), obj, kernel, n, d, X_dev, lengthscale_host, variance, alpha_dev, Linv_dev)))
    return rc;

  ObjState& s = ctx->obj[obj];
  // The previous state may still be read by queued kernels.
  OMB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const size_t bytes = gp_state_bytes(n, d);
  if (bytes > s.cap) {
    if (s.buf) (void)hipFree(s.buf);
    s.buf = nullptr;
    s.cap = 0;
    if (hipMalloc(&s.buf, bytes) != hipSuccess) {
      s.set = false;
      return fail(ctx, OMB_ENOMEM, "hipMalloc(%zu) for objective %d", bytes, obj);
    }
    s.cap = bytes;
  }
  hipError_t e = install_gp(ctx, s, s.buf, kernel, n, d, X_dev, lengthscale_host, variance, alpha_dev, Linv_dev);
  if (e != hipSuccess) return hip_fail(ctx, e, "pack_gp");
  return OMB_OK;
}

int omb_gp_append(omb_ctx* ctx, int obj, int q, const double* Xnew_dev, const double* ynew_dev, double noise,
                  double* mu_out_dev, double* var_out_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  if (obj < 0 || obj >= OMB_MAX_OBJ || !ctx->obj[obj].set) return fail(ctx, OMB_ESTATE, "objective %d not set", obj);
  if (q < 1) return fail(ctx, OMB_EINVAL, "q=%d must be >= 1", q);
  if (!Xnew_dev) return fail(ctx, OMB_EINVAL, "null Xnew_dev");
  if (!(noise >= 0.0) || !(noise <= 1.79769313486231570815e308))
    return fail(ctx, OMB_EINVAL, "noise=%g must be finite and >= 0", noise);
  ObjState& s = ctx->obj[obj];
  const int n = s.n, d = s.d, DP = s.DP;
  if ((int64_t)n + q > OMB_MAX_TRAIN_DENSE)
    return fail(ctx, OMB_EUNSUP, "n_train + q = %lld above %d", (long long)n + q, OMB_MAX_TRAIN_DENSE);
  const int m = n + q;
  if ((rc = grow_dev(ctx, ctx->aws, sizeof(double) * (size_t)append_ws_doubles(m, d, DP), "append workspace")))
    return rc;
  AppendWs ws;
  append_ws_carve(ctx->aws.as<double>(), m, d, DP, &ws);
  hipStream_t st = ctx->stream;
  const auto d2d = hipMemcpyDeviceToDevice;
  // the installed state into the bordered copy; the new rows scaled by the kernel that packs every state's rows
  OMB_HIP(ctx, hipMemsetAsync(ws.info, 0, sizeof(int), st));
  OMB_HIP(ctx, hipMemcpyAsync(ws.alpha, s.dev.alpha, sizeof(double) * n, d2d, st));
  OMB_HIP(ctx, hipMemcpyAsync(ws.Xs, s.dev.Xs, sizeof(double) * (size_t)n * DP, d2d, st));
  OMB_HIP(ctx, hipMemcpyAsync(ws.xsq, s.dev.xsq, sizeof(double) * n, d2d, st));
  OMB_HIP(ctx, hipMemcpyAsync(ws.X, s.Xraw, sizeof(double) * (size_t)n * d, d2d, st));
  OMB_HIP(ctx, hipMemcpyAsync(ws.X + (size_t)n * d, Xnew_dev, sizeof(double) * (size_t)q * d, d2d, st));
  OMB_HIP(ctx, launch_pack_gp(st, q, d, DP, Xnew_dev, s.ls, Xnew_dev, nullptr, ws.Xs + (size_t)n * DP, ws.xsq + n,
                              ws.scratch, nullptr, 0, q));
  OMB_HIP(ctx, launch_append_restride(st, ws, n, s.Ld));
  for (int j = 0; j < q; ++j)
    OMB_HIP(ctx, launch_append_point(st, ws, s.kind, s.variance, n + j, j, ynew_dev, noise, mu_out_dev, var_out_dev));
  OMB_HIP(ctx, hipMemcpyAsync(ctx->info_host, ws.info, sizeof(int), hipMemcpyDeviceToHost, st));
  OMB_HIP(ctx, hipStreamSynchronize(st));
  if (ctx->info_host[0] != 0)
    return fail(ctx, OMB_ENOTPD, "point %d: delta^2 = variance + noise + 1e-8 - v'v is not positive (the state is "
                "unchanged)", ctx->info_host[0]);
  // the grown state through omb_set_gp's packing, into a new buffer where the old one is too small (it is released
  // only once the new one stands, so a failed allocation leaves the installed state as it was)
  double* buf = s.buf;
  double* old = nullptr;
  const size_t need = gp_state_bytes(m, d);
  if (need > s.cap) {
    const int room = m + 64 < OMB_MAX_TRAIN_DENSE ? m + 64 : OMB_MAX_TRAIN_DENSE;   // further appends without a malloc
    size_t cap = gp_state_bytes(room, d);
    if (cap < need) cap = need;
    if (hipMalloc(&buf, cap) != hipSuccess) return fail(ctx, OMB_ENOMEM, "hipMalloc(%zu) for objective %d", cap, obj);
    old = s.buf;
    s.buf = buf;
    s.cap = cap;
  }
  double ls[OMB_MAX_DIM];
  for (int j = 0; j < d; ++j) ls[j] = s.ls[j];
  hipError_t e = install_gp(ctx, s, buf, s.kind, m, d, ws.X, ls, s.variance, ws.alpha, ws.L);
  if (e == hipSuccess) e = hipStreamSynchronize(st);   // the workspace is free again, and so is the old buffer
  if (old) (void)hipFree(old);
  if (e != hipSuccess) return hip_fail(ctx, e, "append install");
  return OMB_OK;
}

int omb_kernel_block(omb_ctx* ctx, int obj, const double* Xc_dev, int64_t N, double* K_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  if (obj < 0 || obj >= OMB_MAX_OBJ || !ctx->obj[obj].set) return fail(ctx, OMB_ESTATE, "objective %d not set", obj);
  if (N < 0 || (N > 0 && (!Xc_dev || !K_dev))) return fail(ctx, OMB_EINVAL, "bad candidate/output arguments");
  if (N == 0) return OMB_OK;
  GPArgs args;
  init_args(ctx, &args);
  args.gp[obj] = ctx->obj[obj].dev;
  args.d = ctx->obj[obj].d;
  args.DP = ctx->obj[obj].DP;
  hipError_t e = launch_kernel_block(ctx->stream, args, obj, Xc_dev, N, K_dev);
  if (e != hipSuccess) return hip_fail(ctx, e, "kernel_block");
  return OMB_OK;
}

int omb_posterior(omb_ctx* ctx, int n_obj, const double* Xc_dev, int64_t N, double* mu_dev, double* var_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  if (N < 0 || (N > 0 && (!Xc_dev || !mu_dev || !var_dev)))
    return fail(ctx, OMB_EINVAL, "bad candidate/output arguments");
  GPArgs args;
  int max_R = 0;
  rc = gather_gp(ctx, n_obj, &args, &max_R);
  if (rc) return rc;
  if (N == 0) return OMB_OK;
  if ((N + 31) / 32 > 0x7fffffffLL) return fail(ctx, OMB_EUNSUP, "N=%lld too large", (long long)N);
  const double* Ld[OMB_MAX_OBJ];
  gather_Ld(ctx, n_obj, Ld);
  hipError_t e = posterior_any(ctx, args, Ld, n_obj, max_R, Xc_dev, N, mu_dev, var_dev);
  if (e != hipSuccess) return hip_fail(ctx, e, "posterior");
  return OMB_OK;
}

int omb_posterior_screen(omb_ctx* ctx, const double* Xc_dev, int64_t N, int n_obj, double* mu_out_dev,
                          double* eps_out_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  if (N < 0 || (N > 0 && (!Xc_dev || !mu_out_dev || !eps_out_dev)))
    return fail(ctx, OMB_EINVAL, "bad candidate/output arguments");
  GPArgs args;
  int max_R = 0;
  if ((rc = gather_gp(ctx, n_obj, &args, &max_R))) return rc;
  if (args.DP > 8) return fail(ctx, OMB_EUNSUP, "the screened mean needs n_var <= 8 (n_var=%d)", args.d);
  if (N == 0) return OMB_OK;
  if ((N + 15) / 16 > 0x7fffffffLL) return fail(ctx, OMB_EUNSUP, "N=%lld too large", (long long)N);
  hipError_t e = launch_posterior_screen(ctx->stream, args, all_objectives(n_obj), Xc_dev, N, mu_out_dev, eps_out_dev);
  if (e != hipSuccess) return hip_fail(ctx, e, "posterior_screen");
  return OMB_OK;
}

int omb_posterior_screen_list(omb_ctx* ctx, const double* Xc_dev, int64_t N, const int32_t* idx_dev,
                               const int32_t* count_dev, int obj, double* mu_dev, double* eps_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  if (N < 0 || (N > 0 && (!Xc_dev || !idx_dev || !count_dev || !mu_dev || !eps_dev)))
    return fail(ctx, OMB_EINVAL, "bad candidate/list/output arguments");
  if (obj < 0 || obj >= OMB_MAX_OBJ) return fail(ctx, OMB_EINVAL, "objective %d", obj);
  GPArgs args;
  int max_R = 0;
  if ((rc = gather_gp(ctx, obj + 1, &args, &max_R))) return rc;
  if (args.DP > 8) return fail(ctx, OMB_EUNSUP, "the screened mean needs n_var <= 8 (n_var=%d)", args.d);
  if (N == 0) return OMB_OK;
  if ((N + 15) / 16 > 0x7fffffffLL) return fail(ctx, OMB_EUNSUP, "N=%lld too large", (long long)N);
  hipError_t e = launch_posterior_screen_gather(ctx->stream, args, obj, Xc_dev, idx_dev, count_dev, N, mu_dev, eps_dev);
  if (e != hipSuccess) return hip_fail(ctx, e, "posterior_screen_list");
  return OMB_OK;
}

int omb_ehvi2d(omb_ctx* ctx, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
               const double* pf_sorted_dev, int P, const double* r_host, double s00, double s01, int mode,
               double* out_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  Plan pl;
  if ((rc = check_moments(E(ctx), mu_dev, var_dev, ld, N, 2, out_dev))) return rc;
  if (!pf_sorted_dev) return fail(ctx, OMB_EINVAL, "null Pareto front");
  if ((rc = describe_ehvi2d(ctx, P, r_host, s00, s01, mode, &pl))) return rc;
  return run_acq(ctx, pl, pf_sorted_dev, nullptr, mu_dev, var_dev, ld, N, out_dev, nullptr, "ehvi2d");
}

int omb_ehvi_mc(omb_ctx* ctx, int k, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
                const double* cache_dev, int M, const double* r_host, double hv_pf, double* out_dev,
                int32_t* raised_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  Plan pl;
  if ((rc = describe_ehvi_mc(ctx, k, M, r_host, hv_pf, &pl))) return rc;
  if ((rc = check_moments(E(ctx), mu_dev, var_dev, ld, N, k, out_dev))) return rc;
  if (!cache_dev) return fail(ctx, OMB_EINVAL, "null cache");
  return run_acq(ctx, pl, cache_dev, nullptr, mu_dev, var_dev, ld, N, out_dev, raised_dev, "ehvi_mc");
}

int omb_ehvi3d_mc(omb_ctx* ctx, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
                  const double* cache_dev, int M, const double* r_host, double hv_pf, double* out_dev,
                  int32_t* raised_dev) {
  return omb_ehvi_mc(ctx, 3, mu_dev, var_dev, ld, N, cache_dev, M, r_host, hv_pf, out_dev, raised_dev);
}

// omb_ehvi_boxes (kd false) and omb_ehvi_boxes_k (kd true, whose kernel reads the box list in 4-byte words)
static int ehvi_boxes_entry(omb_ctx* ctx, bool kd, int k, const double* mu_dev, const double* var_dev, int64_t ld,
                            int64_t N, const double* coords_dev, int C, const uint16_t* boxes_dev, int B,
                            double* out_dev, bool log = false) {
  int rc = enter(ctx);
  if (rc) return rc;
  Plan pl;
  if ((rc = describe_boxes(ctx, kd, k, C, B, &pl))) return rc;
  pl.log = log;
  if ((rc = check_moments(E(ctx), mu_dev, var_dev, ld, N, k, out_dev))) return rc;
  if (!coords_dev || !boxes_dev) return fail(ctx, OMB_EINVAL, "null grid/box list");
  if (kd && (reinterpret_cast<uintptr_t>(boxes_dev) & 3)) return fail(ctx, OMB_EINVAL, "box list not 4-byte aligned");
  return run_acq(ctx, pl, coords_dev, boxes_dev, mu_dev, var_dev, ld, N, out_dev, nullptr,
                 log ? "log_ehvi_boxes" : (kd ? "ehvi_boxes_k" : "ehvi_boxes"));
}

int omb_ehvi_boxes(omb_ctx* ctx, int k, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
                   const double* coords_dev, int C, const uint16_t* boxes_dev, int B, double* out_dev) {
  return ehvi_boxes_entry(ctx, false, k, mu_dev, var_dev, ld, N, coords_dev, C, boxes_dev, B, out_dev);
}

int omb_ehvi_boxes_k(omb_ctx* ctx, int k, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
                     const double* coords_dev, int C, const uint16_t* boxes_dev, int B, double* out_dev) {
  return ehvi_boxes_entry(ctx, true, k, mu_dev, var_dev, ld, N, coords_dev, C, boxes_dev, B, out_dev);
}

int omb_log_ehvi_boxes(omb_ctx* ctx, int k, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
                       const double* coords_dev, int C, const uint16_t* boxes_dev, int B, double* out_dev) {
  return ehvi_boxes_entry(ctx, true, k, mu_dev, var_dev, ld, N, coords_dev, C, boxes_dev, B, out_dev, true);
}

int omb_hvi_boxes(omb_ctx* ctx, int k, const double* y_dev, int64_t ld, int64_t N, const double* coords_dev, int C,
                  const uint16_t* boxes_dev, int B, double* out_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  if ((rc = check_hvi_boxes(E(ctx), k, y_dev, ld, N, coords_dev, C, boxes_dev, B, out_dev))) return rc;
  if (N == 0) return OMB_OK;
  const int64_t wsd = hvi_ws_doubles(N, B);
  if (wsd && (rc = grow_dev(ctx, ctx->hws, sizeof(double) * (size_t)wsd, "HVI slice workspace"))) return rc;
  hipError_t e = launch_hvi_boxes(ctx->stream, k, y_dev, ld, N, coords_dev, C, boxes_dev, B, out_dev,
                                  wsd ? ctx->hws.as<double>() : nullptr);
  if (e != hipSuccess) return hip_fail(ctx, e, "hvi_boxes");
  return OMB_OK;
}

int omb_hvi_paths(omb_ctx* ctx, int k, int S, const double* y_dev, int64_t ld, int64_t N, const double* coords_dev,
                  int C, const int32_t* box_off_host, const uint16_t* boxes_dev, double* out_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  Plan pl;
  if ((rc = describe_hvi_paths(ctx, k, S, y_dev, ld, N, coords_dev, C, box_off_host, boxes_dev, out_dev, &pl)))
    return rc;
  if (N == 0) return OMB_OK;
  pl.geo = coords_dev;
  pl.boxes = boxes_dev;
  return run_hvi_paths(ctx, pl, y_dev, ld, N, out_dev, "hvi_paths");
}

int omb_hvi_paths_con(omb_ctx* ctx, int k, int S, int n_con, const double* y_dev, int64_t ld, int64_t N,
                      const double* coords_dev, int C, const int32_t* box_off_host, const uint16_t* boxes_dev,
                      double eta, unsigned flags, double* out_dev, double* u_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  Plan pl;
  if ((rc = describe_hvi_paths_con(ctx, k, S, n_con, y_dev, ld, N, coords_dev, C, box_off_host, boxes_dev, eta, flags,
                                   out_dev, u_dev, &pl)))
    return rc;
  if (N == 0) return OMB_OK;
  pl.geo = coords_dev;
  pl.boxes = boxes_dev;
  return run_hvi_paths(ctx, pl, y_dev, ld, N, out_dev, "hvi_paths_con", u_dev);
}

// Candidates per pass of omb_hvi_paths_grad: bounds its workspace at S·(k + 1)·chunk doubles (every lane's work
// depends on its candidate alone, so the chunking leaves every bit as it is)
constexpr int64_t kHviPathsGradChunk = 1 << 16;

int omb_hvi_paths_grad(omb_ctx* ctx, int k, int S, int d, const double* y_dev, const double* dy_dev, int64_t ld,
                       int64_t N, const double* coords_dev, int C, const int32_t* box_off_host,
                       const uint16_t* boxes_dev, double* out_dev, double* grad_dev, double* t_dev,
                       double* tgrad_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  if ((rc = check_hvi_paths_grad(E(ctx), k, S, d, y_dev, dy_dev, ld, N, coords_dev, C, box_off_host, boxes_dev, out_dev,
                                 grad_dev, t_dev, tgrad_dev)))
    return rc;
  if (N == 0) return OMB_OK;
  const int64_t chunk = N < kHviPathsGradChunk ? N : kHviPathsGradChunk;
  if ((rc = grow_dev(ctx, ctx->hws, sizeof(double) * (size_t)hvi_paths_grad_ws_doubles(chunk, k, S),
                     "HVI path gradient workspace")))
    return rc;
  for (int64_t c0 = 0; c0 < N; c0 += chunk) {
    const int64_t nc = N - c0 < chunk ? N - c0 : chunk;
    hipError_t e = launch_hvi_paths_grad(ctx->stream, k, S, d, y_dev + c0, dy_dev + c0, ld, nc, coords_dev, C,
                                         boxes_dev, box_off_host, out_dev + c0, grad_dev + c0,
                                         t_dev ? t_dev + c0 : nullptr, tgrad_dev ? tgrad_dev + c0 : nullptr,
                                         ctx->hws.as<double>());
    if (e != hipSuccess) return hip_fail(ctx, e, "hvi_paths_grad");
  }
  return OMB_OK;
}

int omb_nondominated(omb_ctx* ctx, int k, int S, const double* y_dev, int64_t ld, int64_t N, uint8_t* mask_dev,
                     int64_t ldm, int64_t* count_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  if ((rc = check_nondominated(E(ctx), k, S, y_dev, ld, N, mask_dev, ldm, count_dev))) return rc;
  ctx->nd_rounds = 0;
  memset(ctx->nd_survivors, 0, sizeof(ctx->nd_survivors));
  if (N == 0) {
    OMB_HIP(ctx, hipMemsetAsync(count_dev, 0, sizeof(int64_t) * (size_t)S, ctx->stream));
    return OMB_OK;
  }
  // nws: (kNdMaxRounds + 1)·kNdMaxS slot counters | S·nd_final_blocks(N) final-pass counts | list A (S, N)
  constexpr size_t kCnt = (size_t)(kNdMaxRounds + 1) * kNdMaxS;
  const size_t nbc = (size_t)S * (size_t)nd_final_blocks(N);
  if ((rc = grow_dev(ctx, ctx->nws, sizeof(int32_t) * (kCnt + nbc + (size_t)S * (size_t)N), "non-dominated lists")))
    return rc;
  int32_t* cnt = ctx->nws.as<int32_t>();
  int32_t* blockcnt = cnt + kCnt;
  int32_t* listA = blockcnt + nbc;
  OMB_HIP(ctx, hipMemsetAsync(cnt, 0, sizeof(int32_t) * kCnt, ctx->stream));
  // the tile passes: the points themselves into A, then A → B → A → B while a pass still halves the list
  const int32_t* in = nullptr;
  const int32_t* in_cnt = nullptr;
  int64_t in_pitch = 0, before = N;
  int32_t host_cnt[kNdMaxS];
  for (int r = 0;; ++r) {
    int32_t* out = listA;
    int64_t out_pitch = N;
    if (r & 1) {
      if ((rc = grow_dev(ctx, ctx->nws2, sizeof(int32_t) * (size_t)S * (size_t)before, "non-dominated lists")))
        return rc;
      out = ctx->nws2.as<int32_t>();
      out_pitch = before;
    }
    int32_t* out_cnt = cnt + (size_t)r * kNdMaxS;
    hipError_t e = launch_nd_tile(ctx->stream, k, S, y_dev, ld, N, in, in_pitch, in_cnt, before, out, out_pitch,
                                  out_cnt, mask_dev, ldm);
    if (e != hipSuccess) return hip_fail(ctx, e, "nondominated tile pass");
    OMB_HIP(ctx, hipMemcpyAsync(host_cnt, out_cnt, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, ctx->stream));
    OMB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    int64_t now = 0;
    for (int s = 0; s < S; ++s) now = host_cnt[s] > now ? host_cnt[s] : now;
    ctx->nd_rounds = r + 1;
    ctx->nd_survivors[r] = now;
    in = out;
    in_cnt = out_cnt;
    in_pitch = out_pitch;
    const bool more = nd_another_round(r + 1, before, now);
    before = now;
    if (!more) break;
  }
  hipError_t e = launch_nd_final(ctx->stream, k, S, y_dev, ld, in, in_pitch, in_cnt, before, mask_dev, ldm, blockcnt,
                                 count_dev);
  if (e != hipSuccess) return hip_fail(ctx, e, "nondominated final pass");
  return OMB_OK;
}

namespace {

// omb_hypervolume (per_point false: S sets → hv_dev[s]) and omb_hypervolume_contrib (per_point true: one set →
// hv_dev[0] and contrib_dev), after their checks.  vws: header (kHvMaxS, kHvHdr) | totals (kHvPoints + 1) | HvSet × S.
int run_hypervolume(omb_ctx* ctx, int k, int S, const double* y_dev, int64_t ld, int64_t N, const uint8_t* mask_dev,
                    int64_t ldm, const double* r_host, bool per_point, double* hv_dev, double* contrib_dev) {
  int rc;
  if (N == 0) {
    OMB_HIP(ctx, hipMemsetAsync(hv_dev, 0, sizeof(double) * (size_t)S, ctx->stream));
    return OMB_OK;
  }
  constexpr size_t kHdrBytes = sizeof(int32_t) * (size_t)kHvMaxS * kHvHdr;
  constexpr size_t kTotBytes = sizeof(double) * (size_t)(kHvPoints + 1);
  if ((rc = grow_dev(ctx, ctx->vws, kHdrBytes + kTotBytes + sizeof(HvSet) * (size_t)S, "hypervolume sets"))) return rc;
  char* base = ctx->vws.as<char>();
  int32_t* hdr = reinterpret_cast<int32_t*>(base);
  double* tot = reinterpret_cast<double*>(base + kHdrBytes);
  HvSet* sets = reinterpret_cast<HvSet*>(base + kHdrBytes + kTotBytes);
  HvRef ref{};
  for (int j = 0; j < k; ++j) ref.r[j] = r_host[j];
  hipError_t e = launch_hv_prep(ctx->stream, k, S, y_dev, ld, N, mask_dev, ldm, ref, hdr, sets);
  if (e != hipSuccess) return hip_fail(ctx, e, "hypervolume preparation");
  int32_t host_hdr[kHvMaxS * kHvHdr];
  OMB_HIP(ctx, hipMemcpyAsync(host_hdr, hdr, sizeof(int32_t) * (size_t)S * kHvHdr, hipMemcpyDeviceToHost, ctx->stream));
  OMB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  int64_t max_cells = 0;
  if ((rc = check_hv_work(E(ctx), k, S, host_hdr, per_point ? 1 : 0, &max_cells))) return rc;
  const int V = per_point ? host_hdr[0] + 1 : S;
  const int64_t nb = hv_cell_blocks(max_cells), nb2 = hv_reduce_blocks(nb);
  if ((rc = grow_dev(ctx, ctx->vws2, sizeof(double) * (size_t)V * (size_t)(nb + nb2), "hypervolume partial sums")))
    return rc;
  double* partials = ctx->vws2.as<double>();
  e = launch_hv_cells(ctx->stream, k, V, per_point, max_cells, hdr, sets, ref, partials, partials + (size_t)V * nb,
                      per_point ? tot : hv_dev);
  if (e != hipSuccess) return hip_fail(ctx, e, "hypervolume cells");
  if (per_point) {
    OMB_HIP(ctx, hipMemsetAsync(contrib_dev, 0, sizeof(double) * (size_t)N, ctx->stream));
    e = launch_hv_contrib(ctx->stream, tot, hdr, sets, hv_dev, contrib_dev);
    if (e != hipSuccess) return hip_fail(ctx, e, "hypervolume contributions");
  }
  return OMB_OK;
}

}  // namespace

int omb_hypervolume(omb_ctx* ctx, int k, int S, const double* y_dev, int64_t ld, int64_t N, const uint8_t* mask_dev,
                    int64_t ldm, const double* r_host, double* hv_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  if ((rc = check_hypervolume(E(ctx), k, S, y_dev, ld, N, mask_dev, ldm, r_host, hv_dev, 0, nullptr))) return rc;
  return run_hypervolume(ctx, k, S, y_dev, ld, N, mask_dev, ldm, r_host, false, hv_dev, nullptr);
}

int omb_hypervolume_contrib(omb_ctx* ctx, int k, const double* y_dev, int64_t ld, int64_t N, const uint8_t* mask_dev,
                            const double* r_host, double* hv_dev, double* contrib_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  if ((rc = check_hypervolume(E(ctx), k, 1, y_dev, ld, N, mask_dev, N, r_host, hv_dev, 1, contrib_dev))) return rc;
  return run_hypervolume(ctx, k, 1, y_dev, ld, N, mask_dev, N, r_host, true, hv_dev, contrib_dev);
}

int omb_nondominated_stats(omb_ctx* ctx, int64_t* survivors_host, int* rounds_host) {
  if (!ctx) return OMB_EINVAL;
  if (!survivors_host || !rounds_host) return fail(ctx, OMB_EINVAL, "null output");
  for (int r = 0; r <= kNdMaxRounds; ++r) survivors_host[r] = ctx->nd_survivors[r];
  *rounds_host = ctx->nd_rounds;
  return OMB_OK;
}

int omb_argmax_prune_stats(omb_ctx* ctx, int64_t* stats_host) {
  if (!ctx) return OMB_EINVAL;
  if (!stats_host) return fail(ctx, OMB_EINVAL, "null output");
  stats_host[0] = ctx->prune_taken;
  stats_host[1] = ctx->prune_seed;
  stats_host[2] = ctx->prune_taken ? __atomic_load_n(ctx->prune_stats_host, __ATOMIC_ACQUIRE) : 0;
  return OMB_OK;
}

int omb_argmax_stage_stats(omb_ctx* ctx, int64_t* stats_host) {
  if (!ctx) return OMB_EINVAL;
  if (!stats_host) return fail(ctx, OMB_EINVAL, "null output");
  stats_host[0] = ctx->stage_taken;
  stats_host[1] = ctx->stage_taken ? __atomic_load_n(ctx->prune_stats_host + 1, __ATOMIC_ACQUIRE) : 0;
  stats_host[2] = ctx->stage_taken ? __atomic_load_n(ctx->prune_stats_host, __ATOMIC_ACQUIRE) : 0;
  return OMB_OK;
}

int omb_argmax_cut_stats(omb_ctx* ctx, double* stats_host) {
  if (!ctx) return OMB_EINVAL;
  if (!stats_host) return fail(ctx, OMB_EINVAL, "null output");
  stats_host[0] = ctx->cut_taken;
  for (int i = 0; i < 3; ++i) {
    const int64_t bits = __atomic_load_n(ctx->prune_stats_host + 2 + i, __ATOMIC_ACQUIRE);
    double v;
    memcpy(&v, &bits, sizeof(v));
    stats_host[1 + i] = ctx->cut_taken ? v : 0.0;
  }
  return OMB_OK;
}

int omb_hvpoi(omb_ctx* ctx, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
              const double* cells_dev, int C, double* out_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  Plan pl;
  if ((rc = check_moments(E(ctx), mu_dev, var_dev, ld, N, 2, out_dev))) return rc;
  if (!cells_dev) return fail(ctx, OMB_EINVAL, "null cells");
  if ((rc = describe_hvpoi(ctx, C, &pl))) return rc;
  return run_acq(ctx, pl, cells_dev, nullptr, mu_dev, var_dev, ld, N, out_dev, nullptr, "hvpoi");
}

int omb_expdec(omb_ctx* ctx, int k, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
               const double* cache_dev, int M, int scal_id, const double* params_host, const double* weights_host,
               const double* ideal_host, const double* max_host, double agg_min, double* out_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  Plan pl;
  if ((rc = describe_expdec(ctx, k, M, scal_id, params_host, weights_host, ideal_host, max_host, agg_min, &pl)))
    return rc;
  if ((rc = check_moments(E(ctx), mu_dev, var_dev, ld, N, k, out_dev))) return rc;
  if (!cache_dev) return fail(ctx, OMB_EINVAL, "null cache");
  return run_acq(ctx, pl, cache_dev, nullptr, mu_dev, var_dev, ld, N, out_dev, nullptr, "expdec");
}

int omb_ei(omb_ctx* ctx, const double* mu_dev, const double* var_dev, int64_t N, double best, double var_eps,
           double* out_dev) {
  return omb_ei_ext(ctx, OMB_EI_PLAIN, 1, mu_dev, var_dev, N, N, best, var_eps, 0.0, out_dev);
}

int omb_ei_ext(omb_ctx* ctx, int kind, int k, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
               double best, double var_eps, double pof_eps, double* out_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  Plan pl;
  if ((rc = describe_ei(ctx, kind, k, best, var_eps, pof_eps, &pl))) return rc;
  if ((rc = check_moments(E(ctx), mu_dev, var_dev, ld, N, k, out_dev))) return rc;
  return run_acq(ctx, pl, nullptr, nullptr, mu_dev, var_dev, ld, N, out_dev, nullptr, "ei");
}

int omb_feasibility(omb_ctx* ctx, int c, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
                    double pof_eps, const double* acq_dev, double* out_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  if ((rc = check_feasibility(E(ctx), c, mu_dev, var_dev, ld, N, pof_eps, out_dev))) return rc;
  if (N == 0) return OMB_OK;
  hipError_t e = launch_pof_scale(ctx->stream, c, mu_dev, var_dev, ld, N, pof_eps, acq_dev, out_dev);
  if (e != hipSuccess) return hip_fail(ctx, e, "feasibility");
  return OMB_OK;
}

int omb_log_ei(omb_ctx* ctx, int kind, int k, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
               double best, double var_eps, double pof_eps, double* out_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  Plan pl;
  if ((rc = check_log_ei(E(ctx), kind, k, var_eps, pof_eps))) return rc;
  if ((rc = describe_ei(ctx, kind, k, best, var_eps, pof_eps, &pl))) return rc;
  pl.log = true;
  if ((rc = check_moments(E(ctx), mu_dev, var_dev, ld, N, k, out_dev))) return rc;
  return run_acq(ctx, pl, nullptr, nullptr, mu_dev, var_dev, ld, N, out_dev, nullptr, "log_ei");
}

int omb_log_feasibility(omb_ctx* ctx, int c, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
                        double pof_eps, const double* acq_dev, double* out_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  if ((rc = check_feasibility(E(ctx), c, mu_dev, var_dev, ld, N, pof_eps, out_dev))) return rc;
  if (N == 0) return OMB_OK;
  hipError_t e = launch_log_pof(ctx->stream, c, mu_dev, var_dev, ld, N, pof_eps, acq_dev, out_dev);
  if (e != hipSuccess) return hip_fail(ctx, e, "log_feasibility");
  return OMB_OK;
}

int omb_mes(omb_ctx* ctx, int k, const double* mu_dev, const double* var_dev, int64_t ld, int64_t N,
            const double* ystar_dev, int S, double* out_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  Plan pl;
  if ((rc = describe_mes(ctx, k, S, &pl))) return rc;
  if ((rc = check_mes(E(ctx), k, S, mu_dev, var_dev, ld, N, ystar_dev, out_dev))) return rc;
  return run_acq(ctx, pl, ystar_dev, nullptr, mu_dev, var_dev, ld, N, out_dev, nullptr, "mes");
}

int omb_argmax_dev(omb_ctx* ctx, const double* vals_dev, int64_t N, int64_t offset, double* result_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  if (!result_dev || N < 0 || (N > 0 && !vals_dev)) return fail(ctx, OMB_EINVAL, "bad arg-max arguments");
  hipError_t e = launch_argmax(ctx->stream, vals_dev, N, offset, ctx->partials, result_dev, ctx->argmax_one_pass);
  if (e != hipSuccess) return hip_fail(ctx, e, "argmax");
  return OMB_OK;
}

int omb_argmax(omb_ctx* ctx, const double* vals_dev, int64_t N, int64_t offset, double* best_val, int64_t* best_idx) {
  int rc = omb_argmax_dev(ctx, vals_dev, N, offset, ctx ? ctx->result_dev : nullptr);
  if (rc) return rc;
  OMB_HIP(ctx, hipMemcpyAsync(ctx->result_host, ctx->result_dev, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  OMB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (best_val) *best_val = ctx->result_host[0];
  if (best_idx) *best_idx = (int64_t)ctx->result_host[1];
  return OMB_OK;
}

// ---------------------------------------------------------------------------------------
// Fused chain: per-iteration plans, device Sobol' generation, one-call batch evaluation.

int omb_plan_ehvi2d(omb_ctx* ctx, const double* pf_sorted_host, int P, const double* r_host, double s00, double s01,
                    int mode) {
  int rc = plan_enter(ctx);
  if (rc) return rc;
  Plan pl;
  if ((rc = describe_ehvi2d(ctx, P, r_host, s00, s01, mode, &pl))) return rc;
  if (!pf_sorted_host) return fail(ctx, OMB_EINVAL, "null Pareto front");
  // the arg-max chain's bound holds for a = y1[i−1] ≥ b = y1[i] and σB ≥ 0 only
  bool ok = mode == OMB_EHVI_REFERENCE && s00 > 0.0 && s01 > 0.0 && std::isfinite(s00) && std::isfinite(s01) &&
            std::isfinite(r_host[0]);
  double prev = r_host[0];
  for (int i = 0; ok && i < P; ++i) {
    const double f1 = pf_sorted_host[2 * i], f2 = pf_sorted_host[2 * i + 1];
    ok = std::isfinite(f1) && std::isfinite(f2) && f1 <= prev;
    prev = f1;
  }
  pl.prune_ok = ok;
  return install_plan(ctx, pl, pf_sorted_host, sizeof(double) * 2 * (size_t)P);
}

int omb_plan_ehvi_mc(omb_ctx* ctx, int k, const double* cache_host, int M, const double* r_host, double hv_pf) {
  int rc = plan_enter(ctx);
  if (rc) return rc;
  Plan pl;
  if ((rc = describe_ehvi_mc(ctx, k, M, r_host, hv_pf, &pl))) return rc;
  if (!cache_host) return fail(ctx, OMB_EINVAL, "null cache");
  return install_plan(ctx, pl, cache_host, sizeof(double) * (size_t)k * M);
}

int omb_plan_ehvi3d_mc(omb_ctx* ctx, const double* cache_host, int M, const double* r_host, double hv_pf) {
  return omb_plan_ehvi_mc(ctx, 3, cache_host, M, r_host, hv_pf);
}

// omb_plan_ehvi_boxes (kd false) and omb_plan_ehvi_boxes_k (kd true: its kernel trusts the box indices)
static int plan_boxes_entry(omb_ctx* ctx, bool kd, int k, const double* coords_host, int C, const uint16_t* boxes_host,
                            int B) {
  int rc = plan_enter(ctx);
  if (rc) return rc;
  Plan pl;
  if ((rc = describe_boxes(ctx, kd, k, C, B, &pl))) return rc;
  if (!coords_host || !boxes_host) return fail(ctx, OMB_EINVAL, "null grid/box list");
  if (kd && (rc = check_box_list(E(ctx), k, C, boxes_host, B))) return rc;
  // the grid's bytes are a multiple of 8: the box list behind it stays 4-byte aligned
  return install_plan(ctx, pl, coords_host, sizeof(double) * (size_t)k * C, boxes_host,
                      sizeof(uint16_t) * 2 * (size_t)k * B);
}

int omb_plan_ehvi_boxes(omb_ctx* ctx, int k, const double* coords_host, int C, const uint16_t* boxes_host, int B) {
  return plan_boxes_entry(ctx, false, k, coords_host, C, boxes_host, B);
}

int omb_plan_ehvi_boxes_k(omb_ctx* ctx, int k, const double* coords_host, int C, const uint16_t* boxes_host, int B) {
  return plan_boxes_entry(ctx, true, k, coords_host, C, boxes_host, B);
}

int omb_plan_hvpoi(omb_ctx* ctx, const double* cells_host, int C) {
  int rc = plan_enter(ctx);
  if (rc) return rc;
  Plan pl;
  if ((rc = describe_hvpoi(ctx, C, &pl))) return rc;
  if (!cells_host) return fail(ctx, OMB_EINVAL, "null cells");
  return install_plan(ctx, pl, cells_host, sizeof(double) * 4 * (size_t)C);
}

int omb_plan_expdec(omb_ctx* ctx, int k, const double* cache_host, int M, int scal_id, const double* params_host,
                    const double* weights_host, const double* ideal_host, const double* max_host, double agg_min) {
  int rc = plan_enter(ctx);
  if (rc) return rc;
  Plan pl;
  if ((rc = describe_expdec(ctx, k, M, scal_id, params_host, weights_host, ideal_host, max_host, agg_min, &pl)))
    return rc;
  if (!cache_host) return fail(ctx, OMB_EINVAL, "null cache");
  return install_plan(ctx, pl, cache_host, sizeof(double) * (size_t)k * M);
}

int omb_plan_ei(omb_ctx* ctx, double best, double var_eps) {
  return omb_plan_ei_ext(ctx, OMB_EI_PLAIN, 1, best, var_eps, 0.0);
}

int omb_plan_ei_ext(omb_ctx* ctx, int kind, int k, double best, double var_eps, double pof_eps) {
  int rc = plan_enter(ctx);
  if (rc) return rc;
  Plan pl;
  if ((rc = describe_ei(ctx, kind, k, best, var_eps, pof_eps, &pl))) return rc;
  ctx->plan = pl;   // no geometry
  return OMB_OK;
}

int omb_plan_mes(omb_ctx* ctx, int k, int S, const double* ystar_host) {
  int rc = plan_enter(ctx);
  if (rc) return rc;
  Plan pl;
  if ((rc = describe_mes(ctx, k, S, &pl))) return rc;
  if ((rc = check_plan_mes(E(ctx), k, S, ystar_host))) return rc;
  return install_plan(ctx, pl, ystar_host, sizeof(double) * (size_t)k * S);
}

int omb_plan_hvi_paths(omb_ctx* ctx, int k, int S, const double* coords_host, int C, const int32_t* box_off_host,
                       const uint16_t* boxes_host) {
  int rc = plan_enter(ctx);
  if (rc) return rc;
  Plan pl;
  if ((rc = describe_hvi_paths(ctx, k, S, nullptr, 0, 0, coords_host, C, box_off_host, boxes_host, nullptr, &pl)))
    return rc;
  if ((rc = check_box_lists(E(ctx), k, S, C, box_off_host, boxes_host))) return rc;
  // the grids' bytes are a multiple of 8: the box lists behind them stay 4-byte aligned
  return install_plan(ctx, pl, coords_host, sizeof(double) * (size_t)S * k * C, boxes_host,
                      sizeof(uint16_t) * 2 * (size_t)k * (size_t)box_off_host[S]);
}

int omb_plan_hvi_paths_con(omb_ctx* ctx, int k, int S, int n_con, double eta, const double* coords_host, int C,
                           const int32_t* box_off_host, const uint16_t* boxes_host) {
  int rc = plan_enter(ctx);
  if (rc) return rc;
  Plan pl;
  if ((rc = describe_hvi_paths_con(ctx, k, S, n_con, nullptr, 0, 0, coords_host, C, box_off_host, boxes_host, eta, 0u,
                                   nullptr, nullptr, &pl)))
    return rc;
  if ((rc = check_box_lists(E(ctx), k, S, C, box_off_host, boxes_host))) return rc;
  return install_plan(ctx, pl, coords_host, sizeof(double) * (size_t)S * k * C, boxes_host,
                      sizeof(uint16_t) * 2 * (size_t)k * (size_t)box_off_host[S]);
}

int omb_plan_constraints(omb_ctx* ctx, int n_con, double pof_eps) {
  int rc = enter(ctx);
  if (rc) return rc;
  // a failed call leaves the plan and its previous constraints as they were
  if ((rc = check_constraints(E(ctx), ctx->plan.kind == PLAN_NONE ? 0 : ctx->plan.k, n_con, pof_eps))) return rc;
  // the weight needs posterior moments of the constraint slots; the sampled-front chain computes none
  if (ctx->plan.kind == PLAN_HVI_PATHS && n_con > 0)
    return fail(ctx, OMB_EUNSUP, "the sampled-front improvement (noisy EHVI / EI) plan takes no constraints");
  if (ctx->plan.kind == PLAN_HVI_PATHS_CON && n_con > 0)
    return fail(ctx, OMB_EUNSUP, "the constrained sampled-front improvement plan carries its own constraints "
                                 "(omb_plan_hvi_paths_con's n_con)");
  ctx->plan.n_con = n_con;
  ctx->plan.con_eps = n_con ? pof_eps : 0.0;
  return OMB_OK;
}

// The plan kinds without a log form, by name (null: the plan has one).
static const char* log_refused(const Plan& pl) {
  switch (pl.kind) {
    case PLAN_EI: return pl.ei_kind == OMB_EI_PARETO ? "Pareto EI" : nullptr;
    case PLAN_EHVI_BOXES: return nullptr;
    case PLAN_EHVI2D: return "EHVI-2D";
    case PLAN_EHVI_MC: return "Monte-Carlo EHVI";
    case PLAN_HVPOI: return "HV-PoI";
    case PLAN_EXPDEC: return "expected decomposition";
    case PLAN_MES: return "max-value entropy search";
    case PLAN_HVI_PATHS: return "sampled-front improvement (noisy EHVI / EI)";
    case PLAN_HVI_PATHS_CON: return "constrained sampled-front improvement (noisy EHVI / EI)";
    default: return "unknown";
  }
}

int omb_plan_log(omb_ctx* ctx, int on) {
  int rc = enter(ctx);
  if (rc) return rc;
  // a failed call leaves the plan and its flag as they were
  const bool has = ctx->plan.kind != PLAN_NONE;
  if ((rc = check_plan_log(E(ctx), has, on, has ? log_refused(ctx->plan) : nullptr))) return rc;
  ctx->plan.log = on != 0;
  return OMB_OK;
}

int omb_set_sobol(omb_ctx* ctx, int d, int bits, const uint32_t* sv_host, const uint32_t* shift_host,
                  const double* lo_host, const double* hi_host) {
  int rc = enter(ctx);
  if (rc) return rc;
  ctx->sob_d = 0;
  if ((rc = check_sobol_args(E(ctx), d, bits, sv_host, shift_host, lo_host, hi_host))) return rc;
  const size_t bytes = sobol_state_bytes(d, bits);
  void* h = nullptr;
  if ((rc = stage_begin(ctx, bytes, &h))) return rc;
  sobol_pack_state(d, bits, sv_host, shift_host, lo_host, hi_host, h);
  OMB_HIP(ctx, hipMemcpyAsync(ctx->sob, h, bytes, hipMemcpyHostToDevice, ctx->stream));
  ctx->sob_d = d;
  ctx->sob_bits = bits;
  return OMB_OK;
}

int omb_sobol(omb_ctx* ctx, int64_t start, int64_t N, double* X_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  if (ctx->sob_d == 0) return fail(ctx, OMB_ESTATE, "no Sobol state (call omb_set_sobol)");
  if (N < 0 || (N > 0 && !X_dev)) return fail(ctx, OMB_EINVAL, "bad output arguments");
  if (start < 0 || start + N > (int64_t)(1ull << ctx->sob_bits))
    return fail(ctx, OMB_EINVAL, "Sobol indices [%lld, %lld) outside [0, 2^%d)", (long long)start, (long long)(start + N),
                ctx->sob_bits);
  hipError_t e = launch_sobol(ctx->stream, ctx->sob, ctx->sob_d, ctx->sob_bits, start, N, X_dev);
  if (e != hipSuccess) return hip_fail(ctx, e, "sobol");
  return OMB_OK;
}

int omb_eval(omb_ctx* ctx, const double* Xc_dev, int64_t N, double* vals_dev) {
  if (ctx && N > 0 && !vals_dev) return fail(ctx, OMB_EINVAL, "null output");
  return run_chain(ctx, Xc_dev, false, 0, N, 0, vals_dev, nullptr);
}

int omb_eval_argmax(omb_ctx* ctx, const double* Xc_dev, int64_t N, int64_t offset, double* result_dev) {
  if (ctx && !result_dev) return fail(ctx, OMB_EINVAL, "null result");
  return run_chain(ctx, Xc_dev, false, 0, N, offset, nullptr, result_dev);
}

int omb_eval_argmax_sobol(omb_ctx* ctx, int64_t start, int64_t N, double* result_dev) {
  if (ctx && !result_dev) return fail(ctx, OMB_EINVAL, "null result");
  return run_chain(ctx, nullptr, true, start, N, start, nullptr, result_dev);
}

// ---------------------------------------------------------------------------------------
// Gradients with respect to a candidate (omb_grad.hip).  Per pass of up to grad_chunk candidates and per objective:
// K* (omb_kernel_block's launch) → V = L⁻¹K* → w = L⁻ᵀV (two GEMMs with the dense L⁻¹); then one contraction launch
// for all objectives.  aux: doubles in front of the chunk buffers (omb_eval_grad's ∂a/∂μ, ∂a/∂σ²).
static int grad_ws(omb_ctx* ctx, const GPArgs& args, int n_obj, int64_t N, size_t aux, int64_t* Nc, int* n_max) {
  *n_max = 0;
  for (int o = 0; o < n_obj; ++o)
    if (args.gp[o].n > *n_max) *n_max = args.gp[o].n;
  *Nc = grad_chunk(n_obj, *n_max, N);
  const size_t doubles = aux + (size_t)(n_obj + 2) * (size_t)*n_max * (size_t)*Nc;
  return grow_dev(ctx, ctx->gws, doubles * sizeof(double), "gradient workspace");
}

static int grad_chain(omb_ctx* ctx, const GPArgs& args, int n_obj, int n_max, int64_t Nc, size_t aux,
                      const double* Xc, int64_t N, double* dmu, double* dvar, const double* dadm, const double* dadv,
                      const double* vals, double* grad) {
  double* Kst = ctx->gws.as<double>() + aux;
  double* V = Kst + (size_t)n_max * Nc;
  double* W = V + (size_t)n_max * Nc;
  GradArgs ga;
  memset(&ga, 0, sizeof(ga));
  ga.n_obj = n_obj;
  ga.d = args.d;
  ga.DP = args.DP;
  ga.JW = 1;
  while (ga.JW < args.d) ga.JW <<= 1;
  for (int64_t c0 = 0; c0 < N; c0 += Nc) {
    const int64_t nc = (N - c0) < Nc ? (N - c0) : Nc;
    const double* X0 = Xc + c0 * args.d;
    for (int o = 0; o < n_obj; ++o) {
      const GPDev& g = args.gp[o];
      double* Wo = W + (size_t)o * n_max * Nc;
      hipError_t e = launch_kernel_block(ctx->stream, args, o, X0, nc, Kst);
      if (e == hipSuccess) e = launch_gemm_ltri_nn(ctx->stream, g.n, nc, 1.0, ctx->obj[o].Ld, g.n, Kst, nc, 0.0, V, nc);
      if (e == hipSuccess) e = launch_gemm_tn(ctx->stream, g.n, nc, g.n, 1.0, ctx->obj[o].Ld, g.n, V, nc, 0.0, Wo, nc);
      if (e != hipSuccess) return hip_fail(ctx, e, "gradient chain (w = L^-T L^-1 k)");
      ga.o[o] = GradObj{g.Xs, g.alpha, g.ls, Wo, g.variance, g.n, 0};
    }
    hipError_t e = launch_grad_contract(ctx->stream, ga, args.gp[0].kind, X0, nc, c0, N, dmu, dvar, dadm, dadv, vals,
                                        grad);
    if (e != hipSuccess) return hip_fail(ctx, e, "gradient contraction");
  }
  return OMB_OK;
}

int omb_posterior_grad(omb_ctx* ctx, int n_obj, const double* Xc_dev, int64_t N, double* mu_dev, double* var_dev,
                       double* dmu_dev, double* dvar_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  if ((rc = check_posterior_grad(E(ctx), n_obj, Xc_dev, N, mu_dev, var_dev, dmu_dev, dvar_dev))) return rc;
  GPArgs args;
  int max_R = 0;
  if ((rc = gather_gp(ctx, n_obj, &args, &max_R))) return rc;
  if (N == 0) return OMB_OK;
  if ((N + 31) / 32 > 0x7fffffffLL) return fail(ctx, OMB_EUNSUP, "N=%lld too large", (long long)N);
  int64_t Nc = 0;
  int n_max = 0;
  if ((rc = grad_ws(ctx, args, n_obj, N, 0, &Nc, &n_max))) return rc;
  const double* Ld[OMB_MAX_OBJ];
  gather_Ld(ctx, n_obj, Ld);
  hipError_t e = posterior_any(ctx, args, Ld, n_obj, max_R, Xc_dev, N, mu_dev, var_dev);
  if (e != hipSuccess) return hip_fail(ctx, e, "posterior");
  return grad_chain(ctx, args, n_obj, n_max, Nc, 0, Xc_dev, N, dmu_dev, dvar_dev, nullptr, nullptr, nullptr, nullptr);
}

int omb_eval_grad(omb_ctx* ctx, const double* Xc_dev, int64_t N, double* vals_dev, double* grad_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  if ((rc = check_eval_grad(E(ctx), Xc_dev, N, vals_dev, grad_dev))) return rc;
  const Plan pl = ctx->plan;
  if (pl.kind == PLAN_NONE) return fail(ctx, OMB_ESTATE, "no acquisition plan (call an omb_plan_* function)");
  if ((rc = launch_acq_grad(ctx, pl, nullptr, nullptr, 0, nullptr, nullptr))) return rc;   // a plan without a gradient
  GPArgs args;
  int max_R = 0;
  const int k = pl.k, K = pl.k + pl.n_con;   // the constraint models' rows follow the objectives'
  if ((rc = gather_gp(ctx, K, &args, &max_R))) return rc;
  if (N == 0) return OMB_OK;
  if ((N + 31) / 32 > 0x7fffffffLL) return fail(ctx, OMB_EUNSUP, "N=%lld too large", (long long)N);
  // ∂a/∂μ | ∂a/∂σ² (K, N) each, then — with constraints — the unweighted acquisition (N), which a·F does not give back
  const size_t aux = 2 * (size_t)K * (size_t)N + (pl.n_con ? (size_t)N : 0);
  int64_t Nc = 0;
  int n_max = 0;
  if ((rc = grad_ws(ctx, args, K, N, aux, &Nc, &n_max))) return rc;
  double* dadm = ctx->gws.as<double>();
  double* dadv = dadm + (size_t)K * (size_t)N;
  double* acq_raw = pl.n_con ? dadv + (size_t)K * (size_t)N : nullptr;
  // the value: omb_eval's own chain, so vals_dev is bitwise omb_eval's; it leaves μ | σ² (K, N) in ctx->work
  // (every σ²: the gradient kernels below read them all)
  if ((rc = run_chain(ctx, Xc_dev, false, 0, N, 0, vals_dev, nullptr, true, acq_raw))) return rc;
  const double* mu = ctx->work.as<const double>();
  const double* var = mu + (size_t)K * (size_t)N;
  if ((rc = launch_acq_grad(ctx, pl, mu, var, N, dadm, dadv))) return rc;
  if (pl.n_con) {
    // a log plan adds log F: the objectives' rows stay, the constraints' rows get ∂ log F
    hipError_t e = pl.log ? launch_log_pof_grad(ctx->stream, mu + (size_t)k * (size_t)N, var + (size_t)k * (size_t)N,
                                                N, N, k, pl.n_con, pl.con_eps, dadm, dadv)
                          : launch_pof_grad(ctx->stream, acq_raw, mu + (size_t)k * (size_t)N,
                                            var + (size_t)k * (size_t)N, N, N, k, pl.n_con, pl.con_eps, dadm, dadv);
    if (e != hipSuccess) return hip_fail(ctx, e, "acquisition gradient");
  }
  return grad_chain(ctx, args, K, n_max, Nc, aux, Xc_dev, N, nullptr, nullptr, dadm, dadv, vals_dev, grad_dev);
}

int omb_timing(omb_ctx* ctx, int enable) {
  int rc = enter(ctx);
  if (rc) return rc;
  OMB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (enable < 0 || enable > 2) return fail(ctx, OMB_EINVAL, "timing level %d outside [0, 2]", enable);
  ctx->timing = enable;
  ctx->timing_calls = 0;
  ctx->ev_used = 0;
  // create the events of the first 256 chains now, not inside the timed chains
  while (enable && ctx->ev.size() < 5 * 256) {
    hipEvent_t e;
    OMB_HIP(ctx, hipEventCreate(&e));
    ctx->ev.push_back(e);
  }
  return OMB_OK;
}

int omb_timing_read(omb_ctx* ctx, double* stage_ms, int64_t* chains) {
  int rc = enter(ctx);
  if (rc) return rc;
  if (!stage_ms) return fail(ctx, OMB_EINVAL, "null output");
  OMB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int s = 0; s < 4; ++s) stage_ms[s] = 0.0;
  const size_t n = ctx->ev_used / 5;
  for (size_t c = 0; c < n; ++c) {
    for (int s = 0; s < 4; ++s) {
      if (ctx->timing == 1 && s != 1) continue;
      float ms = 0.0f;
      OMB_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev[5 * c + s], ctx->ev[5 * c + s + 1]));
      stage_ms[s] += ms;
    }
  }
  if (chains) *chains = (int64_t)n;
  ctx->ev_used = 0;
  return OMB_OK;
}

// ---------------------------------------------------------------------------------------
// Thompson sampling (TuRBO, turbo.py:75-153): full posterior covariance, Cholesky, joint
// samples and the greedy per-sample arg-min (omb_linalg.hip).

static int check_obj(omb_ctx* ctx, int obj) {
  if (obj < 0 || obj >= OMB_MAX_OBJ || !ctx->obj[obj].set) return fail(ctx, OMB_ESTATE, "objective %d not set", obj);
  return OMB_OK;
}

static int check_cov_n(omb_ctx* ctx, int64_t N) {
  if (N < 0) return fail(ctx, OMB_EINVAL, "N=%lld < 0", (long long)N);
  if (N > kMaxCovN) return fail(ctx, OMB_EUNSUP, "N=%lld candidates exceed the full-covariance limit %lld",
                                (long long)N, (long long)kMaxCovN);
  return OMB_OK;
}

// K* (n, N) by the K block, V = L⁻¹K* (n, N) by GEMM, μ = K*ᵀα and σ² = σ_f² − Σ V² by the column
// reduction over those two (the fused posterior kernel would recompute K* and V; at TuRBO's ≤ 5,000
// candidates it also runs on a few dozen workgroups: 90 µs of a 3 ms step, profiles/r02_v21_c6_kernel_stats.csv).
// scale_ws (omb_posterior_samples): the column reduction also writes launch_cand_scale's rows into it, for the first
// cov_build (prescaled); the fused SYRK path only.
static bool cov_fused_path(const omb_ctx* ctx, const ObjState& s) {
  return !ctx->cov_table && ctx->cov_fused && s.DP <= kMaxFusedDP;
}
static hipError_t cov_prepare(omb_ctx* ctx, const ObjState& s, const double* Xc, int64_t N, double* Kst, double* V,
                              double* mu, double* var, double* scale_ws = nullptr) {
  GPArgs args;
  init_args(ctx, &args);
  args.gp[0] = s.dev;
  args.d = s.d;
  args.DP = s.DP;
  hipError_t e = launch_kernel_block(ctx->stream, args, 0, Xc, N, Kst);
  if (e == hipSuccess) e = launch_gemm_ltri_nn(ctx->stream, s.n, N, 1.0, s.Ld, s.n, Kst, N, 0.0, V, N);
  if (e == hipSuccess)
    e = launch_post_colreduce(ctx->stream, Kst, V, s.n, N, s.dev.alpha, s.dev.variance, mu, var,
                              scale_ws ? &s.dev : nullptr, s.d, s.DP, Xc, scale_ws);
  return e;
}

// lower triangle of Σ = K(X*, X*) − VᵀV (GPy PosteriorExact._raw_predict, full_cov=True); cws:
// cand_cov_ws_doubles(N, DP) doubles.
// zero_ints / n_zero / zero_info: the next Cholesky's sync words and status, zeroed by the fused SYRK's workgroups on
// the side (*zeroed = true when it did: that factorisation then skips its init launch)
static hipError_t cov_build(omb_ctx* ctx, const ObjState& s, const double* Xc, int64_t N, const double* V, double* S,
                            int64_t lds, double* cws, double jitter = 0.0, bool prescaled = false,
                            int* zero_ints = nullptr, int n_zero = 0, int* zero_info = nullptr, bool* zeroed = nullptr) {
  if (zeroed) *zeroed = false;
  if (cov_fused_path(ctx, s)) {
    // K(X*, X*) formed in the SYRK's epilogue (launch_cov_syrk): the two-launch result below to the ulp
    hipError_t e = hipSuccess;
    const int kp = prescaled ? (s.DP + 3) / 4 * 4 : launch_cand_scale(ctx->stream, s.dev, s.d, s.DP, Xc, N, cws, &e);
    if (e == hipSuccess && kp > 0) {
      if (zeroed) *zeroed = zero_ints != nullptr;
      return launch_cov_syrk(ctx->stream, N, s.n, V, N, S, lds, cws, cws + N * kp, kp, s.kind, s.variance, jitter,
                             ctx->syrk_glds, zero_ints, n_zero, zero_info);
    }
    if (e != hipSuccess) return e;
  }
  hipError_t e = launch_cand_cov(ctx->stream, s.dev, s.d, s.DP, Xc, N, S, lds, cws, jitter, ctx->cov_table);
  if (e == hipSuccess) e = launch_gemm_tn_lower(ctx->stream, N, s.n, -1.0, V, N, 1.0, S, lds);
  return e;
}

// In-place lower Cholesky of A + jitter·I; synchronises and returns LAPACK's info in *info.
// The factorisation in two halves, so that a caller can queue work that reads the factor before it waits for the
// status: chol_enqueue queues A += jitter·I, the factor and the status's copy into pinned memory; chol_wait
// synchronises and reads it.
// The factorisation workspace: [info int | pad to 16 B | factor workspace (chol_ws_doubles)]
static int chol_workspace(omb_ctx* ctx, int64_t N, int** dinfo, double** ws) {
  int rc = grow_dev(ctx, ctx->ichol, 16 + sizeof(double) * chol_ws_doubles(N), "Cholesky workspace");
  if (rc) return rc;
  *dinfo = ctx->ichol.as<int>();
  *ws = reinterpret_cast<double*>(ctx->ichol.as<char>() + 16);
  return OMB_OK;
}

// zeroed / n_zeroed: the ints that the covariance SYRK (cov_build) set to 0 together with the status, or none
static int chol_enqueue(omb_ctx* ctx, double* A, int64_t N, int64_t lda, double jitter, const int* zeroed = nullptr,
                        int n_zeroed = 0) {
  int* dinfo = nullptr;
  double* ws = nullptr;
  int rc = chol_workspace(ctx, N, &dinfo, &ws);
  if (rc) return rc;
  OMB_HIP(ctx, launch_add_diag(ctx->stream, A, N, lda, jitter));
  OMB_HIP(ctx, launch_cholesky_mode(ctx->stream, A, N, lda, dinfo, ws, ctx->chol_mode, ctx->spin_limit,
                                    ctx->chol_acq_rel, ctx->chol_single, zeroed, n_zeroed));
  OMB_HIP(ctx, hipMemcpyAsync(ctx->info_host, dinfo, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  return OMB_OK;
}

static int chol_wait(omb_ctx* ctx, int* info) {
  OMB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int h = *ctx->info_host;
  if (h == kCholSpinFault)
    return fail(ctx, OMB_EHIP, "Cholesky: a workgroup's wait for the diagonal block exceeded %d polls; the factor is "
                               "invalid", ctx->spin_limit);
  *info = h;
  return OMB_OK;
}

static int run_cholesky(omb_ctx* ctx, double* A, int64_t N, int64_t lda, double jitter, int* info) {
  int rc = chol_enqueue(ctx, A, N, lda, jitter);
  return rc ? rc : chol_wait(ctx, info);
}

int omb_posterior_cov(omb_ctx* ctx, int obj, const double* Xc_dev, int64_t N, double* mu_dev, double* cov_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  if ((rc = check_obj(ctx, obj)) || (rc = check_cov_n(ctx, N))) return rc;
  if (N > 0 && (!Xc_dev || !mu_dev || !cov_dev)) return fail(ctx, OMB_EINVAL, "null device pointer");
  if (N == 0) return OMB_OK;
  const ObjState& s = ctx->obj[obj];
  const size_t nN = (size_t)s.n * N;
  const size_t cw = (size_t)cand_cov_ws_doubles(N, s.DP);
  if ((rc = grow_dev(ctx, ctx->tws, sizeof(double) * (2 * nN + N + cw), "covariance workspace"))) return rc;
  double* Kst = ctx->tws.as<double>();
  double* V = Kst + nN;
  double* var = V + nN;
  double* cws = var + N;
  hipError_t e = cov_prepare(ctx, s, Xc_dev, N, Kst, V, mu_dev, var, nullptr);
  if (e == hipSuccess) e = cov_build(ctx, s, Xc_dev, N, V, cov_dev, N, cws);
  if (e == hipSuccess) e = launch_mirror_lower(ctx->stream, cov_dev, N, N);
  if (e != hipSuccess) return hip_fail(ctx, e, "posterior_cov");
  return OMB_OK;
}

int omb_cholesky(omb_ctx* ctx, double* A_dev, int64_t N, int64_t lda, double jitter, int* info) {
  int rc = enter(ctx);
  if (rc) return rc;
  if (!info || N < 0 || lda < N || (N > 0 && !A_dev)) return fail(ctx, OMB_EINVAL, "bad Cholesky arguments");
  if (!(jitter >= 0.0)) return fail(ctx, OMB_EINVAL, "jitter=%g must be >= 0", jitter);
  *info = 0;
  if (N == 0) return OMB_OK;
  return run_cholesky(ctx, A_dev, N, lda, jitter, info);
}

// The draws are queued before the factor's status is read (omb_posterior_samples), so a failed call would leave
// draws from an invalid factor in Y: they are overwritten with NaN (all-ones bit patterns) instead.
static void poison_draws(omb_ctx* ctx, double* Y, size_t count) {
  (void)hipMemsetAsync(Y, 0xff, count * sizeof(double), ctx->stream);
  (void)hipStreamSynchronize(ctx->stream);
}

int omb_posterior_samples(omb_ctx* ctx, int obj, const double* Xc_dev, int64_t N, const double* Zt_dev, int B,
                          double jitter_rel, int max_tries, double* Y_dev, double* jitter_used) {
  int rc = enter(ctx);
  if (rc) return rc;
  if ((rc = check_obj(ctx, obj)) || (rc = check_cov_n(ctx, N))) return rc;
  if (N < 1 || B < 1) return fail(ctx, OMB_EINVAL, "need N >= 1 candidates and B >= 1 samples (N=%lld, B=%d)",
                                  (long long)N, B);
  if (!Xc_dev || !Zt_dev || !Y_dev) return fail(ctx, OMB_EINVAL, "null device pointer");
  if (!(jitter_rel >= 0.0) || max_tries < 1 || max_tries > 32)
    return fail(ctx, OMB_EINVAL, "jitter_rel=%g must be >= 0 and max_tries=%d in [1, 32]", jitter_rel, max_tries);
  const ObjState& s = ctx->obj[obj];
  const size_t nN = (size_t)s.n * N;
  const size_t cw = (size_t)cand_cov_ws_doubles(N, s.DP);
  const size_t sw = (size_t)chol_samples_ws_doubles(N, B);
  const size_t doubles = 2 * nN + 2 * (size_t)N + (size_t)N * N + (cw > sw ? cw : sw);
  if ((rc = grow_dev(ctx, ctx->tws, sizeof(double) * doubles, "sampling workspace"))) return rc;
  double* Kst = ctx->tws.as<double>();
  double* V = Kst + nN;
  double* mu = V + nN;
  double* var = mu + N;
  double* S = var + N;
  double* cws = S + (size_t)N * N;
  // the first try's scaled candidates come from the column reduction's launch; later tries rescale (the draws'
  // split-K partials share cws)
  const bool prescale = cov_fused_path(ctx, s);
  hipError_t e = cov_prepare(ctx, s, Xc_dev, N, Kst, V, mu, var, prescale ? cws : nullptr);
  if (e != hipSuccess) return hip_fail(ctx, e, "posterior_samples (posterior)");
  // the factorisation's workspace placed before the covariance build, whose SYRK zeroes its sync words and status
  int* dinfo = nullptr;
  double* cws_chol = nullptr;
  if ((rc = chol_workspace(ctx, N, &dinfo, &cws_chol))) return rc;
  int* sync_ints = nullptr;
  const int n_sync = chol_persist_sync_words(cws_chol, N, &sync_ints);
  double jit = jitter_rel * s.variance;
  int info = -1, t = 0;
  for (; t < max_tries; ++t, jit *= 10.0) {
    bool zeroed = false;
    if ((e = cov_build(ctx, s, Xc_dev, N, V, S, N, cws, jit, prescale && t == 0, sync_ints, n_sync, dinfo, &zeroed)) !=
        hipSuccess)   // Σ + jit·I
      return hip_fail(ctx, e, "posterior_samples (cov)");
    if ((rc = chol_enqueue(ctx, S, N, N, 0.0, zeroed ? sync_ints : nullptr, zeroed ? n_sync : 0))) return rc;
    // the draws are queued before the status is read (no idle GPU between the factor and them); a failed factor's
    // draws are overwritten by the next try's
    if ((e = launch_chol_samples(ctx->stream, S, N, N, mu, Zt_dev, B, Y_dev, cws)) != hipSuccess)
      return hip_fail(ctx, e, "posterior_samples (samples)");
    if ((rc = chol_wait(ctx, &info))) {
      poison_draws(ctx, Y_dev, (size_t)B * N);
      return rc;
    }
    if (info == 0) break;
  }
  if (info != 0) {
    poison_draws(ctx, Y_dev, (size_t)B * N);
    return fail(ctx, OMB_ENOTPD, "posterior covariance + %g I is not positive definite (column %d) after %d tries",
                jit / 10.0, info, max_tries);
  }
  if (jitter_used) *jitter_used = jit;
  return OMB_OK;
}

int omb_thompson_select(omb_ctx* ctx, const double* Y_dev, int B, int64_t N, int64_t* idx_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  if (B < 0 || N < 1) return fail(ctx, OMB_EINVAL, "need B >= 0 samples over N >= 1 candidates");
  if (N > kSelectMaxN) return fail(ctx, OMB_EUNSUP, "N=%lld candidates exceed %lld", (long long)N,
                                   (long long)kSelectMaxN);
  if (B > 0 && (!Y_dev || !idx_dev)) return fail(ctx, OMB_EINVAL, "null device pointer");
  if (B == 0) return OMB_OK;
  const size_t sw = (size_t)select_ws_bytes(B, N);
  if (sw && (rc = grow_dev(ctx, ctx->sws, sw, "selection workspace"))) return rc;
  hipError_t e = launch_select(ctx->stream, Y_dev, B, N, idx_dev, ctx->sws.p, ctx->select_seq);
  if (e != hipSuccess) return hip_fail(ctx, e, "thompson_select");
  return OMB_OK;
}

// ---------------------------------------------------------------------------------------
// GP fit on the device: GPy ExactGaussianInference + jitchol, log marginal
// likelihood and its gradient for the L-BFGS hyperparameter search (optimisers.py:226-231).

struct GPFactor {
  double* Ky;      // (n, n): Ky, then its Cholesky factor (lower)
  double* Linv;    // (n, n): L⁻¹ (upper triangle zero)
  double* Kinv;    // (n, n): Ky⁻¹ (lower triangle)
  double* T;       // (64, n) scratch of the triangular inverse
  double* alpha;   // (n)
  double* v;       // (n)
  double* ls;      // (DP)
  double* part;    // gp_grad_blocks(n)·(DP+1)
  double* out;     // DP + 5
  double* cws;     // cand_cov_ws_doubles(n, DP): X/ℓ and its squared norms for K(X, X)
  double jitter;   // jitter added by jitchol (0 when the first factorisation succeeded)
};

// Ky = K + (noise + 1e-8) I, L = jitchol(Ky) (GPy.util.linalg.jitchol: on failure add
// mean(diag)·1e-6·10^t, t = 0..4), L⁻¹, α = Ky⁻¹ y.  Synchronises (the factorisation status).
static int gp_factor(omb_ctx* ctx, int kernel, int n, int d, const double* X, const double* y, const double* ls_host,
                     double variance, double noise, GPFactor* f) {
  const int DP = pad_dim(d);
  const size_t nn = (size_t)n * n;
  const size_t doubles = 3 * nn + 64 * (size_t)n + 2 * (size_t)n + DP +
                         (size_t)gp_grad_blocks(n) * (DP + 1) + DP + 5 + (size_t)cand_cov_ws_doubles(n, DP);
  int rc = grow_dev(ctx, ctx->fws, sizeof(double) * doubles, "GP fit workspace");
  if (rc) return rc;
  double* p = ctx->fws.as<double>();
  f->Ky = p; p += nn;
  f->Linv = p; p += nn;
  f->Kinv = p; p += nn;
  f->T = p; p += 64 * (size_t)n;
  f->alpha = p; p += n;
  f->v = p; p += n;
  f->ls = p; p += DP;
  f->part = p; p += (size_t)gp_grad_blocks(n) * (DP + 1);
  f->out = p; p += DP + 5;
  f->cws = p;
  void* h = nullptr;
  if ((rc = stage_begin(ctx, sizeof(double) * DP, &h))) return rc;
  for (int j = 0; j < DP; ++j) static_cast<double*>(h)[j] = (j < d) ? ls_host[j] : 1.0;
  OMB_HIP(ctx, hipMemcpyAsync(f->ls, h, sizeof(double) * DP, hipMemcpyHostToDevice, ctx->stream));
  GPDev g{};
  g.ls = f->ls;
  g.variance = variance;
  g.kind = kernel;
  const double base = noise + 1e-8;
  const double mean_diag = variance + base;
  int info = -1;
  f->jitter = 0.0;
  for (int t = -1; t < 5; ++t) {
    const double jit = (t < 0) ? 0.0 : mean_diag * 1e-6 * pow(10.0, (double)t);
    OMB_HIP(ctx, launch_cand_cov(ctx->stream, g, d, DP, X, n, f->Ky, n, f->cws, base + jit, ctx->cov_table));   // Ky = K + (base+jit)·I
    if ((rc = run_cholesky(ctx, f->Ky, n, n, 0.0, &info))) return rc;
    if (info == 0) {
      f->jitter = jit;
      break;
    }
  }
  if (info != 0) return fail(ctx, OMB_ENOTPD, "K + jitter is not positive definite, even with jitter (column %d)", info);
  OMB_HIP(ctx, hipMemsetAsync(f->Linv, 0, sizeof(double) * nn, ctx->stream));
  OMB_HIP(ctx, launch_trinv(ctx->stream, f->Ky, n, n, f->Linv, n, f->T));
  // α = L⁻ᵀ (L⁻¹ y)
  OMB_HIP(ctx, launch_gemm_nn(ctx->stream, n, 1, n, 1.0, f->Linv, n, y, 1, 0.0, f->v, 1));
  OMB_HIP(ctx, launch_gemm_tn(ctx->stream, n, 1, n, 1.0, f->Linv, n, f->v, 1, 0.0, f->alpha, 1));
  return OMB_OK;
}

// ∂ lml / ∂ log σ_n² = ½ tr((ααᵀ − Ky⁻¹) ∂Ky/∂log σ_n²) = ½ σ_n² (αᵀα − tr Ky⁻¹); exactly 0 at σ_n² = 0
static double noise_entry(double noise, double aa, double tr_kinv) {
  return noise == 0.0 ? 0.0 : 0.5 * noise * (aa - tr_kinv);
}

// omb_gp_lml_grad (noise_grad false: grad has d + 1 entries) and omb_gp_lml_grad_noise (d + 2): the same
// launches and the same first d + 1 entries; the kernels always leave αᵀα and tr Ky⁻¹ beside the other sums.
static int gp_lml_grad_impl(omb_ctx* ctx, int kernel, int n, int d, const double* X_dev, const double* y_dev,
                            const double* lengthscale_host, double variance, double noise, double* lml, double* grad,
                            double* jitter_used, bool noise_grad) {
  int rc = enter(ctx);
  if (rc) return rc;
  if (kernel != OMB_KERNEL_MATERN52 && kernel != OMB_KERNEL_RBF) return fail(ctx, OMB_EINVAL, "unknown kernel %d", kernel);
  if (n < 1 || n > 16384) return fail(ctx, OMB_EUNSUP, "n_train=%d outside [1, 16384]", n);
  if (d < 1 || d > OMB_MAX_DIM) return fail(ctx, OMB_EUNSUP, "n_var=%d outside [1, %d]", d, OMB_MAX_DIM);
  if (!X_dev || !y_dev || !lengthscale_host || !lml || !grad) return fail(ctx, OMB_EINVAL, "null pointer");
  for (int j = 0; j < d; ++j)
    if (!(lengthscale_host[j] > 0.0)) return fail(ctx, OMB_EINVAL, "lengthscale[%d]=%g must be > 0", j, lengthscale_host[j]);
  if (!(variance > 0.0) || !(noise >= 0.0)) return fail(ctx, OMB_EINVAL, "variance must be > 0 and noise >= 0");
  const int DP = pad_dim(d);
  if (gp_lml_small_fits(n, DP)) {
    // one workgroup, one launch, one synchronisation (launch_gp_lml_small); the kernel stores its
    // DP + 7 results straight into the pinned, host-mapped fit_host (no D2H copy per evaluation)
    OMB_HIP(ctx, launch_gp_lml_small(ctx->stream, kernel, DP, X_dev, d, n, lengthscale_host, variance, noise + 1e-8,
                                     y_dev, ctx->fit_dev));
    OMB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const volatile double* h = ctx->fit_host;
    if (h[DP + 4] != 0.0)
      return fail(ctx, OMB_ENOTPD, "K + jitter is not positive definite, even with jitter (column %d)", (int)h[DP + 4]);
    *lml = -0.5 * h[DP + 2] - h[DP + 1] - 0.5 * n * log(2.0 * M_PI);
    for (int q = 0; q <= d; ++q) grad[q] = h[q];
    if (noise_grad) grad[d + 1] = noise_entry(noise, h[DP + 5], -h[DP + 6]);   // slot DP+6 holds −tr Ky⁻¹
    if (jitter_used) *jitter_used = h[DP + 3];
    return OMB_OK;
  }
  GPFactor f;
  if ((rc = gp_factor(ctx, kernel, n, d, X_dev, y_dev, lengthscale_host, variance, noise, &f))) return rc;
  // Ky⁻¹ = L⁻ᵀ L⁻¹ (lower triangle), then the gradient sums, log det and yᵀα
  OMB_HIP(ctx, launch_gemm_tn_lower(ctx->stream, n, n, 1.0, f.Linv, n, 0.0, f.Kinv, n));
  OMB_HIP(ctx, launch_gp_grad(ctx->stream, kernel, DP, X_dev, d, n, f.ls, variance, f.alpha, f.Kinv, n, f.part,
                              f.Ky, n, y_dev, f.out));
  OMB_HIP(ctx, hipMemcpyAsync(ctx->fit_host, f.out, sizeof(double) * (DP + 5), hipMemcpyDeviceToHost, ctx->stream));
  OMB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const volatile double* h = ctx->fit_host;
  // GPy: log p(y) = −½ yᵀα − Σ log L_ii − ½ n log 2π
  *lml = -0.5 * h[DP + 2] - h[DP + 1] - 0.5 * n * log(2.0 * M_PI);
  for (int q = 0; q <= d; ++q) grad[q] = h[q];
  if (noise_grad) grad[d + 1] = noise_entry(noise, h[DP + 3], h[DP + 4]);
  if (jitter_used) *jitter_used = f.jitter;
  return OMB_OK;
}

int omb_gp_lml_grad(omb_ctx* ctx, int kernel, int n, int d, const double* X_dev, const double* y_dev,
                    const double* lengthscale_host, double variance, double noise, double* lml, double* grad,
                    double* jitter_used) {
  return gp_lml_grad_impl(ctx, kernel, n, d, X_dev, y_dev, lengthscale_host, variance, noise, lml, grad, jitter_used,
                          false);
}

int omb_gp_lml_grad_noise(omb_ctx* ctx, int kernel, int n, int d, const double* X_dev, const double* y_dev,
                          const double* lengthscale_host, double variance, double noise, double* lml, double* grad,
                          double* jitter_used) {
  return gp_lml_grad_impl(ctx, kernel, n, d, X_dev, y_dev, lengthscale_host, variance, noise, lml, grad, jitter_used,
                          true);
}

// omb_gp_lml_grad_batch (one noise for all, d + 1 entries per problem) and omb_gp_lml_grad_noise_batch (a noise
// per problem, d + 2 entries): noise_host has k values in both.
static int gp_lml_grad_batch_impl(omb_ctx* ctx, int kernel, int k, int n, int d, const double* X_dev,
                                  const double* const* y_dev, const double* lengthscale_host,
                                  const double* variance_host, const double* noise_host, double* lml,
                                  double* grad_host, double* jitter_used, int* status, bool noise_grad) {
  int rc = enter(ctx);
  if (rc) return rc;
  if (k < 1 || k > kFitBatchMax) return fail(ctx, OMB_EUNSUP, "k=%d outside [1, %d]", k, kFitBatchMax);
  if (kernel != OMB_KERNEL_MATERN52 && kernel != OMB_KERNEL_RBF) return fail(ctx, OMB_EINVAL, "unknown kernel %d", kernel);
  if (n < 1 || n > 16384) return fail(ctx, OMB_EUNSUP, "n_train=%d outside [1, 16384]", n);
  if (d < 1 || d > OMB_MAX_DIM) return fail(ctx, OMB_EUNSUP, "n_var=%d outside [1, %d]", d, OMB_MAX_DIM);
  if (!X_dev || !y_dev || !lengthscale_host || !variance_host || !noise_host || !lml || !grad_host || !status)
    return fail(ctx, OMB_EINVAL, "null pointer");
  const int G = noise_grad ? d + 2 : d + 1;   // gradient entries per problem
  for (int p = 0; p < k; ++p) {
    if (!y_dev[p]) return fail(ctx, OMB_EINVAL, "null y_dev[%d]", p);
    for (int j = 0; j < d; ++j)
      if (!(lengthscale_host[p * d + j] > 0.0))
        return fail(ctx, OMB_EINVAL, "lengthscale[%d][%d]=%g must be > 0", p, j, lengthscale_host[p * d + j]);
    if (!(variance_host[p] > 0.0)) return fail(ctx, OMB_EINVAL, "variance[%d] must be > 0", p);
    if (!(noise_host[p] >= 0.0)) return fail(ctx, OMB_EINVAL, "noise must be >= 0");
  }
  const int DP = pad_dim(d);
  // gp_lml_small_fits (n ≤ 128, n_var ≤ 8): one launch, a workgroup per problem.  The batch routes exactly as
  // omb_gp_lml_grad does, so every problem gives bitwise what its own omb_gp_lml_grad gives (the concurrent and the
  // sequential fits then walk the same L-BFGS-B path).  The one-workgroup and the blocked route do differ in the
  // last digits; both are within what a LAPACK evaluation in fp64 achieves on ill-conditioned K.
  if (!gp_lml_small_fits(n, DP)) {
    // blocked path: the problems one after another, each exactly omb_gp_lml_grad
    for (int p = 0; p < k; ++p) {
      rc = gp_lml_grad_impl(ctx, kernel, n, d, X_dev, y_dev[p], lengthscale_host + p * d, variance_host[p],
                            noise_host[p], lml + p, grad_host + p * G, jitter_used ? jitter_used + p : nullptr,
                            noise_grad);
      if (rc != OMB_OK && rc != OMB_ENOTPD) return rc;
      status[p] = rc;
    }
    return OMB_OK;
  }
  // fit_host holds OMB_MAX_DIM + 8 doubles: problem p's DP + 7 results at p·(DP + 7) (DP ≤ 8: k·15 ≤ 60 ≤ 264)
  double* outs[kFitBatchMax];
  double base[kFitBatchMax];
  for (int p = 0; p < k; ++p) {
    outs[p] = ctx->fit_dev + p * (DP + 7);
    base[p] = noise_host[p] + 1e-8;
  }
  OMB_HIP(ctx, launch_gp_lml_small_batch(ctx->stream, kernel, DP, X_dev, d, n, k, y_dev, lengthscale_host,
                                         variance_host, base, outs));
  OMB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int p = 0; p < k; ++p) {
    const volatile double* h = ctx->fit_host + p * (DP + 7);
    status[p] = h[DP + 4] != 0.0 ? OMB_ENOTPD : OMB_OK;
    lml[p] = -0.5 * h[DP + 2] - h[DP + 1] - 0.5 * n * log(2.0 * M_PI);
    for (int q = 0; q <= d; ++q) grad_host[p * G + q] = h[q];
    if (noise_grad) grad_host[p * G + d + 1] = noise_entry(noise_host[p], h[DP + 5], -h[DP + 6]);
    if (jitter_used) jitter_used[p] = h[DP + 3];
  }
  return OMB_OK;
}

int omb_gp_lml_grad_batch(omb_ctx* ctx, int kernel, int k, int n, int d, const double* X_dev,
                          const double* const* y_dev, const double* lengthscale_host, const double* variance_host,
                          double noise, double* lml, double* grad_host, double* jitter_used, int* status) {
  double noises[kFitBatchMax];
  for (int p = 0; p < kFitBatchMax; ++p) noises[p] = noise;
  return gp_lml_grad_batch_impl(ctx, kernel, k, n, d, X_dev, y_dev, lengthscale_host, variance_host, noises, lml,
                                grad_host, jitter_used, status, false);
}

int omb_gp_lml_grad_noise_batch(omb_ctx* ctx, int kernel, int k, int n, int d, const double* X_dev,
                                const double* const* y_dev, const double* lengthscale_host,
                                const double* variance_host, const double* noise_host, double* lml, double* grad_host,
                                double* jitter_used, int* status) {
  return gp_lml_grad_batch_impl(ctx, kernel, k, n, d, X_dev, y_dev, lengthscale_host, variance_host, noise_host, lml,
                                grad_host, jitter_used, status, true);
}

int omb_gp_fit_state(omb_ctx* ctx, int obj, int kernel, int n, int d, const double* X_dev, const double* y_dev,
                     const double* lengthscale_host, double variance, double noise, double* jitter_used) {
  int rc = enter(ctx);
  if (rc) return rc;
  if (obj < 0 || obj >= OMB_MAX_OBJ) return fail(ctx, OMB_EINVAL, "obj=%d outside [0, %d)", obj, OMB_MAX_OBJ);
  if (kernel != OMB_KERNEL_MATERN52 && kernel != OMB_KERNEL_RBF) return fail(ctx, OMB_EINVAL, "unknown kernel %d", kernel);
  if (n < 1 || n > OMB_MAX_TRAIN_DENSE)
    return fail(ctx, OMB_EUNSUP, "n_train=%d outside [1, %d]", n, OMB_MAX_TRAIN_DENSE);
  if (d < 1 || d > OMB_MAX_DIM) return fail(ctx, OMB_EUNSUP, "n_var=%d outside [1, %d]", d, OMB_MAX_DIM);
  if (!X_dev || !y_dev || !lengthscale_host) return fail(ctx, OMB_EINVAL, "null pointer");
  for (int j = 0; j < d; ++j)
    if (!(lengthscale_host[j] > 0.0)) return fail(ctx, OMB_EINVAL, "lengthscale[%d]=%g must be > 0", j, lengthscale_host[j]);
  if (!(variance > 0.0) || !(noise >= 0.0)) return fail(ctx, OMB_EINVAL, "variance must be > 0 and noise >= 0");
  GPFactor f;
  if ((rc = gp_factor(ctx, kernel, n, d, X_dev, y_dev, lengthscale_host, variance, noise, &f))) return rc;
  if (jitter_used) *jitter_used = f.jitter;
  return omb_set_gp(ctx, obj, kernel, n, d, X_dev, lengthscale_host, variance, f.alpha, f.Linv);
}

// ---------------------------------------------------------------------------------------
// Posterior sample paths (omb_paths.hip): pathwise conditioning over the installed state.
static PathsObjInfo paths_info(const ObjState& s) { return PathsObjInfo{s.set ? 1 : 0, s.d, s.n, s.path_S}; }

int omb_paths_set(omb_ctx* ctx, int obj, int S, int m, const double* omega_host, const double* phase_host,
                  const double* w_host, const double* z_host, double noise) {
  int rc = enter(ctx);
  if (rc) return rc;
  PathsObjInfo info{};
  if (obj >= 0 && obj < OMB_MAX_OBJ) {
    ctx->obj[obj].path_S = 0;   // a failed call leaves the objective without paths
    info = paths_info(ctx->obj[obj]);
  }
  if ((rc = check_paths_set(E(ctx), obj, S, m, omega_host, phase_host, w_host, noise, &info))) return rc;
  ObjState& s = ctx->obj[obj];
  const int n = s.n, d = s.d, DP = s.DP;
  const size_t nOf = (size_t)paths_of_doubles(m, DP), nWf = (size_t)paths_wf_doubles(m);
  const size_t nVf = (size_t)paths_vf_doubles(s.R), nS = (size_t)n * kPathsMaxS;
  const size_t bytes = sizeof(double) * (nOf + nWf + nVf + 5 * nS);
  void* host = nullptr;
  // synchronises the stream: queued evaluations may still read the previous paths
  if ((rc = stage_begin(ctx, sizeof(double) * (nOf + nWf + (size_t)n * S), &host))) return rc;
  if (bytes > s.pcap) {
    if (s.pbuf) (void)hipFree(s.pbuf);
    s.pbuf = nullptr;
    s.pcap = 0;
    if (hipMalloc(&s.pbuf, bytes) != hipSuccess)
      return fail(ctx, OMB_ENOMEM, "hipMalloc(%zu) for the paths of objective %d", bytes, obj);
    s.pcap = bytes;
  }
  double* Of = s.pbuf;
  double* Wf = Of + nOf;
  double* Vf = Wf + nWf;
  double* zd = Vf + nVf;
  double* F = zd + nS;
  double* U = F + nS;
  double* T = U + nS;
  double* G = T + nS;
  double* hs = static_cast<double*>(host);
  paths_pack(m, d, DP, S, omega_host, phase_host, w_host, sqrt(2.0 * s.variance / m), hs, hs + nOf);
  if (z_host) memcpy(hs + nOf + nWf, z_host, sizeof(double) * (size_t)n * S);
  hipStream_t st = ctx->stream;
  OMB_HIP(ctx, hipMemcpyAsync(Of, hs, sizeof(double) * (nOf + nWf), hipMemcpyHostToDevice, st));
  if (z_host)
    OMB_HIP(ctx, hipMemcpyAsync(zd, hs + nOf + nWf, sizeof(double) * (size_t)n * S, hipMemcpyHostToDevice, st));
  // the prior paths at the training inputs (the evaluation kernel without its update term), then
  // U = Φ(X)·w·sqrt(2σ_f²/m) + sqrt(noise + 1e-8)·z and V = α − L⁻ᵀ(L⁻¹U)
  PathArgs pa{};
  pa.o[0] = PathObj{s.dev, Of, Wf, Vf, (m + 15) / 16, 0, S, 0};
  pa.d = d;
  pa.DP = DP;
  OMB_HIP(ctx, launch_paths_eval(st, pa, 1, s.kind, ctx->paths_libcos, s.Xraw, n, n, F));
  OMB_HIP(ctx, launch_paths_u(st, F, z_host ? zd : nullptr, sqrt(noise + 1e-8), n, S, U));
  OMB_HIP(ctx, launch_gemm_ltri_nn(st, n, S, 1.0, s.Ld, n, U, S, 0.0, T, S));
  OMB_HIP(ctx, launch_gemm_tn(st, n, S, n, 1.0, s.Ld, n, T, S, 0.0, G, S));
  OMB_HIP(ctx, launch_paths_pack_v(st, s.dev.alpha, G, n, S, s.R, Vf));
  s.path_S = S;
  s.path_MT = (m + 15) / 16;
  s.path_Of = Of;
  s.path_Wf = Wf;
  s.path_Vf = Vf;
  return OMB_OK;
}

int omb_paths_eval(omb_ctx* ctx, int n_obj, const double* Xc_dev, int64_t N, int64_t ld, double* out_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  PathsObjInfo info[OMB_MAX_OBJ];
  for (int o = 0; o < OMB_MAX_OBJ; ++o) info[o] = paths_info(ctx->obj[o]);
  if ((rc = check_paths_eval(E(ctx), n_obj, Xc_dev, N, ld, out_dev, info))) return rc;
  PathArgs pa{};
  for (int o = 0; o < n_obj; ++o) {
    const ObjState& s = ctx->obj[o];
    if (s.d != ctx->obj[0].d) return fail(ctx, OMB_EINVAL, "objectives disagree on n_var (%d vs %d)", s.d, ctx->obj[0].d);
    if (s.kind != ctx->obj[0].kind) return fail(ctx, OMB_EINVAL, "objectives disagree on kernel kind");
    pa.o[o] = PathObj{s.dev, s.path_Of, s.path_Wf, s.path_Vf, s.path_MT, s.R, s.path_S, 0};
  }
  pa.d = ctx->obj[0].d;
  pa.DP = ctx->obj[0].DP;
  if (N == 0) return OMB_OK;
  if ((N + 63) / 64 > 0x7fffffffLL) return fail(ctx, OMB_EUNSUP, "N=%lld too large", (long long)N);
  hipError_t e = launch_paths_eval(ctx->stream, pa, n_obj, ctx->obj[0].kind, ctx->paths_libcos, Xc_dev, N, ld, out_dev);
  if (e != hipSuccess) return hip_fail(ctx, e, "paths_eval");
  return OMB_OK;
}

int omb_paths_grad(omb_ctx* ctx, int n_obj, const double* Xc_dev, int64_t N, int64_t ld, double* out_dev,
                   double* grad_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  PathsObjInfo info[OMB_MAX_OBJ];
  for (int o = 0; o < OMB_MAX_OBJ; ++o) info[o] = paths_info(ctx->obj[o]);
  if ((rc = check_paths_grad(E(ctx), n_obj, Xc_dev, N, ld, out_dev, grad_dev, info))) return rc;
  PathArgs pa{};
  for (int o = 0; o < n_obj; ++o) {
    const ObjState& s = ctx->obj[o];
    if (s.d != ctx->obj[0].d) return fail(ctx, OMB_EINVAL, "objectives disagree on n_var (%d vs %d)", s.d, ctx->obj[0].d);
    if (s.kind != ctx->obj[0].kind) return fail(ctx, OMB_EINVAL, "objectives disagree on kernel kind");
    pa.o[o] = PathObj{s.dev, s.path_Of, s.path_Wf, s.path_Vf, s.path_MT, s.R, s.path_S, 0};
  }
  pa.d = ctx->obj[0].d;
  pa.DP = ctx->obj[0].DP;
  if (N == 0) return OMB_OK;
  if ((N + 63) / 64 > 0x7fffffffLL) return fail(ctx, OMB_EUNSUP, "N=%lld too large", (long long)N);
  hipError_t e = launch_paths_grad(ctx->stream, pa, n_obj, ctx->obj[0].kind, ctx->paths_libcos, Xc_dev, N, ld, out_dev,
                                   grad_dev);
  if (e != hipSuccess) return hip_fail(ctx, e, "paths_grad");
  return OMB_OK;
}

int omb_paths_min(omb_ctx* ctx, int n_obj, const double* Xc_dev, int64_t N, int64_t offset, double* res_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  PathsObjInfo info[OMB_MAX_OBJ];
  for (int o = 0; o < OMB_MAX_OBJ; ++o) info[o] = paths_info(ctx->obj[o]);
  if ((rc = check_paths_min(E(ctx), n_obj, Xc_dev, N, res_dev, info))) return rc;
  PathArgs pa{};
  for (int o = 0; o < n_obj; ++o) {
    const ObjState& s = ctx->obj[o];
    if (s.d != ctx->obj[0].d) return fail(ctx, OMB_EINVAL, "objectives disagree on n_var (%d vs %d)", s.d, ctx->obj[0].d);
    if (s.kind != ctx->obj[0].kind) return fail(ctx, OMB_EINVAL, "objectives disagree on kernel kind");
    pa.o[o] = PathObj{s.dev, s.path_Of, s.path_Wf, s.path_Vf, s.path_MT, s.R, s.path_S, 0};
  }
  pa.d = ctx->obj[0].d;
  pa.DP = ctx->obj[0].DP;
  if ((N + 63) / 64 > 0x7fffffffLL) return fail(ctx, OMB_EUNSUP, "N=%lld too large", (long long)N);
  const size_t pairs = (size_t)paths_min_blocks(N) * (size_t)n_obj * kPathsMaxS;
  if ((rc = grow_dev(ctx, ctx->pws, sizeof(double) * 2 * (pairs ? pairs : 1), "paths_min partials"))) return rc;
  hipError_t e = launch_paths_min(ctx->stream, pa, n_obj, ctx->obj[0].kind, ctx->paths_libcos, Xc_dev, N, offset,
                                  ctx->pws.as<double>(), res_dev);
  if (e != hipSuccess) return hip_fail(ctx, e, "paths_min");
  return OMB_OK;
}

// ---------------------------------------------------------------------------------------
// ParEGO / KEEP evolutionary acquisition search: parego.py:223-271, keep.py:240-292.
int omb_ea_search(omb_ctx* ctx, int mode, double best, double var_eps, const double* pop_dev, int P, int iters,
                  const int32_t* sel_dev, const int8_t* cross_dev, const double* beta_dev, const int8_t* mut_dev,
                  const double* lower_dev, const double* upper_dev, double* out_dev) {
  int rc = enter(ctx);
  if (rc) return rc;
  if (mode != OMB_EA_EI && mode != OMB_EA_PARETO_EI) return fail(ctx, OMB_EINVAL, "unknown search mode %d", mode);
  if ((rc = check_obj(ctx, 0))) return rc;
  if (mode == OMB_EA_PARETO_EI && (rc = check_obj(ctx, 1))) return rc;
  const ObjState& s0 = ctx->obj[0];
  if (mode == OMB_EA_PARETO_EI && ctx->obj[1].d != s0.d)
    return fail(ctx, OMB_EINVAL, "objectives 0 and 1 disagree on n_var (%d vs %d)", s0.d, ctx->obj[1].d);
  if (P < 3 || P > kEAMaxPop) return fail(ctx, OMB_EINVAL, "population size %d outside [3, %d]", P, kEAMaxPop);
  if (iters < 0) return fail(ctx, OMB_EINVAL, "iters=%d must be >= 0", iters);
  if (s0.n > kEAMaxTrain || (mode == OMB_EA_PARETO_EI && ctx->obj[1].n > kEAMaxTrain))
    return fail(ctx, OMB_EUNSUP, "n_train above %d", kEAMaxTrain);
  if (!(var_eps >= 0.0)) return fail(ctx, OMB_EINVAL, "var_eps=%g must be >= 0", var_eps);
  if (!pop_dev || !lower_dev || !upper_dev || !out_dev || (iters > 0 && (!sel_dev || !cross_dev || !beta_dev || !mut_dev)))
    return fail(ctx, OMB_EINVAL, "null device pointer");
  if ((rc = grow_dev(ctx, ctx->ews, sizeof(double) * (size_t)s0.n * s0.n, "search workspace"))) return rc;
  EASearch es{};
  es.g0 = s0.dev;
  es.g1 = (mode == OMB_EA_PARETO_EI) ? ctx->obj[1].dev : s0.dev;
  es.Ld0 = s0.Ld;
  es.mode = mode;
  es.d = s0.d;
  es.DP = s0.DP;
  es.P = P;
  es.iters = iters;
  es.best = best;
  es.var_eps = var_eps;
  es.pop = pop_dev;
  es.sel = sel_dev;
  es.cross = cross_dev;
  es.beta = beta_dev;
  es.mut = mut_dev;
  es.lower = lower_dev;
  es.upper = upper_dev;
  es.out = out_dev;
  hipError_t e = launch_ea_search(ctx->stream, es, ctx->ews.as<double>());
  if (e != hipSuccess) return hip_fail(ctx, e, "ea_search");
  return OMB_OK;
}

}  // extern "C"
