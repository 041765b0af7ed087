// Internal declarations shared by the HIP translation units of liboptimobo_hip.so.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/optimobo_hip.h"
#include "omb_host.h"
#include "omb_math.h"

namespace omb {

// Rows of the training set handled per streamed K* chunk (4 row tiles of 16).
constexpr int kChunkRows = 64;
constexpr int kBlockThreads = 512;
// Training rows per workgroup of the standalone K-block kernel.
constexpr int kKBlockRows = 256;

// Device-side state of one fitted GP (objective), built by omb_set_gp.
struct GPDev {
  const double* Xs;     // (n_pad, DP) training inputs / ℓ, zero padded
  const double* xsq;    // (n_pad) Σ_j Xs[k][j]²
  const double* alpha;  // (n_pad) woodbury vector, zero padded
  const double* Lp;     // packed lower-triangular L^-1 in MFMA fragment order (see pack kernel)
  const double* ls;     // (DP) lengthscales, padded with 1
  double variance;      // σ_f²
  int n;                // n_train
  int R;                // row tiles = ceil(n / 16)
  int kind;             // OMB_KERNEL_*
  int pad_;
  const double* Xf;     // Xs in A-fragment order for the MFMA cross term (see pack_X_kernel)
};

struct GPArgs {
  GPDev gp[OMB_MAX_OBJ];
  int d;    // true n_var (≤ DP)
  int DP;   // padded dim used by the packed Xs
  ExpCoef ec;      // exp_nonpos coefficients as kernel arguments (set by launch_posterior)
  int* fault;      // context fault word (pinned host memory): bit 0 = an LDS-counter wait ran out
  int spin_limit;  // polls per LDS-counter wait before the fault word is marked
  // bit o set: nothing reads σ² of objective o, so its workgroups take the fused kernels' mean-only path (K*
  // generation and μ as always, no V = L⁻¹K*, var_out untouched).  The complement of the plan's var_mask, so that
  // zeroed arguments compute everything.
  unsigned var_skip;
  // non-zero: the launch covers the objectives whose bits are set and blockIdx.y counts them in ascending order (set
  // by launch_posterior where it gives the masked objectives' μ a launch of its own); 0: objective blockIdx.y
  unsigned obj_sel;
  // non-null (launch_posterior_gather only): the launch covers candidates idx[0 .. *count − 1] of Xc and writes μ, σ²
  // compacted (slot p of the list at p, pitch N = the list's capacity); workgroups past *count exit at once.  null: the
  // identity, candidates 0..N-1 (every other launch)
  const int32_t* idx;
  const int32_t* count;
};

// launch_posterior's mean_kernel argument (OMB_DEBUG_POSTERIOR_MEAN_KERNEL): μ of the objectives in var_skip by
// posterior_mean_kernel after (default) or before the launch that computes the others' μ and σ², or — off — inside
// that launch, by its kernels' mean-only path
enum { kMeanKernelOff = 0, kMeanKernelAfter = 1, kMeanKernelBefore = 2 };

constexpr int kFaultSpin = 1;          // fault word bit: posterior counter-ring wait exhausted
constexpr int kDefaultSpinLimit = 1 << 22;

// ---------------------------------------------------------------------------------------
// Launchers (host functions; each launches on `stream` and returns hipGetLastError()).
hipError_t launch_pack_gp(hipStream_t stream, int n, int d, int DP, const double* X, const double* ls_dev,
                          const double* alpha, const double* Linv, double* Xs, double* xsq, double* alpha_p,
                          double* Lp, int R, int n_pad);
// Xf = Xs in the A-fragment order of the posterior kernel's MFMA cross term (after launch_pack_gp)
hipError_t launch_pack_x(hipStream_t stream, int d, int DP, int n_pad, const double* Xs, const double* xsq,
                         double* Xf);

hipError_t launch_kernel_block(hipStream_t stream, const GPArgs& args, int obj, const double* Xc, int64_t N,
                               double* K);

hipError_t launch_posterior(hipStream_t stream, const GPArgs& args, int n_obj, int max_R, const double* Xc,
                            int64_t N, double* mu, double* var, int mean_kernel = kMeanKernelAfter);

// The arg-max chain's two-phase path (run_chain).
//   launch_posterior_means   μ of the objectives in `objs` (bits) for all N candidates by posterior_mean_kernel
//                            (n_var ≤ 8, n_train > 128: posterior_gather_fits), rows o·N of mu; the ring kernels' bits
//   launch_posterior_gather  μ, σ² of objective 0 alone for the candidates idx[0 .. *count − 1] (device list and count,
//                            count ≤ cap) by the ring instantiation max_R picks for a dense launch, written compacted
//                            to mu_c / var_c (cap each)
bool posterior_gather_fits(const GPArgs& args, int max_R);
hipError_t launch_posterior_means(hipStream_t stream, const GPArgs& args, unsigned objs, const double* Xc, int64_t N,
                                  double* mu);
hipError_t launch_posterior_gather(hipStream_t stream, const GPArgs& args, int max_R, const double* Xc,
                                   const int32_t* idx, const int32_t* count, int64_t cap, double* mu_c, double* var_c);
// The screened path, n_var ≤ 8.
//   launch_posterior_mean_gather  μ of objective `obj` for the listed candidates by posterior_mean_kernel's gathered
//                                 instantiation, to mu_row[idx[p]] (the objective's own row: original slots), the
//                                 dense launch's bits
//   launch_posterior_screen       μ̃ (fp32 transform of the fp64 r², fp64 sum) and a margin ε ≥ |μ̃ − μ| of the
//                                 objectives in `objs` for all N candidates, rows o·N of mu and eps
hipError_t launch_posterior_mean_gather(hipStream_t stream, const GPArgs& args, int obj, const double* Xc,
                                        const int32_t* idx, const int32_t* count, int64_t cap, double* mu_row);
hipError_t launch_posterior_screen(hipStream_t stream, const GPArgs& args, unsigned objs, const double* Xc, int64_t N,
                                   double* mu, double* eps);
//   launch_posterior_screen_gather  μ̃ and ε of objective `obj` for the listed candidates by posterior_screen_kernel's
//                                   gathered instantiation, to mu_row[idx[p]], eps_row[idx[p]]: the dense
//                                   launch's bits
hipError_t launch_posterior_screen_gather(hipStream_t stream, const GPArgs& args, int obj, const double* Xc,
                                          const int32_t* idx, const int32_t* count, int64_t cap, double* mu_row,
                                          double* eps_row);

// Pruning of the EHVI-2D arg-max in OMB_EHVI_REFERENCE (omb_acquisition.hip).  A list is int32 indices into the batch
// with a device-side count; "seed" is the strided sample 0, kPruneStride, 2·kPruneStride, … or,
// seeded by the bound, the candidate with the largest margined bound of each run of kPruneSeedGroup
// consecutive candidates.
constexpr int kPruneStride = 16;
constexpr int kPruneBlock = 256;   // candidates per workgroup of the bound / threshold / compaction kernels
constexpr int kPruneSeedGroup = 256;   // a multiple of kPruneBlock, at most 1024
static_assert(kPruneSeedGroup % kPruneBlock == 0 && kPruneSeedGroup >= kPruneStride && kPruneSeedGroup <= 1024,
              "seed groups are whole workgroups of the threshold kernel and seed_idx holds ⌈N/kPruneStride⌉ entries");
struct PruneWs {
  int32_t* seed_idx;     // ⌈N/kPruneStride⌉ (the seed by bound uses the first ⌈N/kPruneSeedGroup⌉)
  int32_t* surv_idx;     // N
  int32_t* counts;       // [0] seed count, [1] survivor count, [2] the staged order's list A count
  int32_t* block_cnt;    // ⌈N/kPruneBlock⌉ survivors per workgroup, then (in place) their exclusive prefix sums
  uint8_t* keep;         // N flags (the staged order's second compaction: over list A positions)
  double* ubm;           // N margined bounds ub·(1 + 1e-9) + tiny (the seed by bound; staged: ubm1)
  double* scr_mu;        // (2, N) the screen's μ̃
  double* scr_eps;       // (2, N) its margins ε
  double* partials;      // 2 × kArgmaxMaxBlocks (value, index) pairs: the seed's, then the survivors'
  double* tau;           // {τ, its index}: the seed sample's arg-max
  int32_t* list_a;       // N: the staged order's list A, the candidates objective 1's bound leaves
  int32_t* block_cnt_b;  // ⌈N/kPruneBlock⌉: the full bound's kept count per workgroup of list A positions, then offsets
  double* cut;           // {m*, τ₀, ubm1(m*), unused}: objective 1's bound as a cut on μ̃₁ − ε₁
  int64_t* stats_host;   // pinned, device-mapped: [0] the survivor count of the last call (a system-scope store),
                         // [1] the staged order's list A count, [2..4] the bits of the cut's three doubles
};
// ≈ 49.3·N bytes: 45.3·N of the two lists' first (seed_idx N/4, surv_idx 4N), block_cnt N/64, keep N, ubm 8N and the
// screen's rows 32N, and the staged order's list_a 4N and block_cnt_b N/64.  The staged order stores ubm1 in the ubm row
// (under the cut of §34 nothing does) and reuses keep for its second compaction's flags.
int64_t prune_ws_bytes(int64_t N);
void prune_ws_carve(void* base, int64_t N, PruneWs* ws);
// seed_idx and counts[0]
hipError_t launch_prune_seed(hipStream_t stream, int64_t N, const PruneWs& ws);
// EHVI-2D (ehvi2d_point: the dense kernels' bits) of the candidates idx[0 .. *count − 1] — μ₀ and σ²₀ compacted (slot
// p), μ₁ at mu1[idx[p]] — and their arg-max by original index into `partials` (prune_list_blocks(cap) pairs, all
// written)
int prune_list_blocks(int64_t cap);
hipError_t launch_ehvi2d_argmax_list(hipStream_t stream, const double* mu0_c, const double* var0_c, const double* mu1,
                                     const int32_t* idx, const int32_t* count, int64_t cap, const double* pf, int P,
                                     double r0, double r1, double s00, double s01, int mode, double* partials);
// keep flags of the non-seed candidates from the upper bound of the acquisition over σ²₀ ∈ [0, sf2] against *tau, the
// ordered compaction of the kept indices into surv_idx, counts[1] and *stats_host
// eps0 / eps1 non-null: the interval form — mu0, mu1 are known to ±eps0, ±eps1 and every factor of the
// bound is taken at the end of its interval that makes it largest
hipError_t launch_prune_bound(hipStream_t stream, const double* mu0, const double* mu1, int64_t N, const double* pf,
                              int P, double r0, double s00, double s01, double sf2, const PruneWs& ws,
                              const double* eps0 = nullptr, const double* eps1 = nullptr);
// The seed by bound, in two steps around the seed's evaluation.
//   launch_prune_bound_seed  the same bound with the same margin for every candidate, with no τ: ws.ubm, the index of
//                            each group's largest comparable ubm (lowest index on ties; the group's first candidate
//                            where none compares) to ws.seed_idx — ascending — and counts[0] = ⌈N/kPruneSeedGroup⌉
//   launch_prune_threshold   keep = not its group's seed and not (τ > 0 and ubm < τ) against *ws.tau, then the scan
//                            and the compaction of launch_prune_bound: surv_idx, counts[1], *stats_host
hipError_t launch_prune_bound_seed(hipStream_t stream, const double* mu0, const double* mu1, int64_t N,
                                   const double* pf, int P, double r0, double s00, double s01, double sf2,
                                   const PruneWs& ws, const double* eps0 = nullptr, const double* eps1 = nullptr);
hipError_t launch_prune_threshold(hipStream_t stream, int64_t N, const PruneWs& ws);
// The staged order: objective 1's screen alone decides who gets objective 0's.
//   launch_prune_bound1_seed  ubm1 = ub1·(1 + 1e-9) + tiny1 from μ̃₁ − ε₁ alone (ub1 = Σ_i C_i·ψ(y2_i, y2_i, ·, σ_f²·s01),
//                             C_i the supremum over μ₀ of the bound's second factor; alpha0, n0: objective 0's α row
//                             for M₀ ≥ |μ₀|) to ws.ubm, and the seed of launch_prune_bound_seed by it
//   launch_prune_threshold_a  launch_prune_threshold into ws.list_a, its count to counts[2] and stats_host[1]
//   launch_prune_bound_list   the interval bound of launch_prune_bound (mu0, eps0 at original slots) for list A's
//                             candidates alone against *ws.tau; the kept ones, ascending, to surv_idx, counts[1],
//                             stats_host[0].  cap: list A's capacity
hipError_t launch_prune_bound1_seed(hipStream_t stream, const double* mu1, const double* eps1, int64_t N,
                                    const double* pf, int P, double r0, double s00, double s01, double sf2,
                                    const double* alpha0, int n0, const PruneWs& ws);
hipError_t launch_prune_threshold_a(hipStream_t stream, int64_t N, const PruneWs& ws, const double* mu1 = nullptr,
                                    const double* eps1 = nullptr);
// Objective 1's bound as one cut: ubm1 decreases in its one argument, so "ubm1 < τ₀" is "μ̃₁ − ε₁ ≥ m*".
//   launch_prune_seed1        launch_prune_bound1_seed's seeds (the smallest μ̃₁ of each group, the same rule) and
//                             counts[0] with no bound evaluated and ws.ubm left alone
//   launch_prune_cut          one workgroup, after *ws.tau is written: m* with the computed ubm1(m*) < τ₀ and
//                             ubm1(m*) ≥ τ₀·(1 − 1e-7) (or m*'s predecessor not below τ₀), +∞ where nothing may be
//                             dropped; {m*, τ₀, ubm1(m*)} to ws.cut and stats_host[2..4]
//   launch_prune_threshold_a  with mu1, eps1: keep = not the seed and not (m* < ∞ and μ̃₁ − ε₁ ≥ m*) against ws.cut
hipError_t launch_prune_seed1(hipStream_t stream, const double* mu1, int64_t N, const PruneWs& ws);
hipError_t launch_prune_cut(hipStream_t stream, const double* pf, int P, double r0, double s00, double s01, double sf2,
                            const double* alpha0, int n0, const PruneWs& ws);
hipError_t launch_prune_bound_list(hipStream_t stream, const double* mu0, const double* mu1, const double* eps0,
                                   const double* eps1, int64_t cap, const double* pf, int P, double r0, double s00,
                                   double s01, double sf2, const PruneWs& ws);

// EHVI-2D and the arg-max in one launch (omb_acquisition.hip): each workgroup's (value, index) pair goes to
// `partials` (2 doubles per workgroup, ehvi2d_argmax_blocks(N) ≤ kArgmaxMaxBlocks); the last workgroup to finish (an
// agent-scope ticket, 0 between launches) reduces them and writes result = {value, index + offset} — or, with
// ticket == nullptr, a second launch (argmax_pass2) does.
struct ArgmaxOut {
  double* partials;
  unsigned* ticket;
  double* result;
  int64_t offset;
};
int64_t ehvi2d_argmax_blocks(int64_t N);
hipError_t launch_ehvi2d_argmax(hipStream_t stream, const double* mu, const double* var, int64_t ld, int64_t N,
                                const double* pf, int P, double r0, double r1, double s00, double s01, int mode,
                                const ArgmaxOut& am);

hipError_t launch_ehvi2d(hipStream_t stream, const double* mu, const double* var, int64_t ld, int64_t N,
                         const double* pf, int P, double r0, double r1, double s00, double s01, int mode,
                         double* out);

hipError_t launch_ehvi_mc(hipStream_t stream, int k, const double* mu, const double* var, int64_t ld, int64_t N,
                          const double* cache, int M, const double* r, double hv_pf, double* out, int32_t* raised);

hipError_t launch_ehvi_boxes(hipStream_t stream, int k, const double* mu, const double* var, int64_t ld, int64_t N,
                             const double* coords, int C, const uint16_t* boxes, int B, double* out);

// Exact EHVI for 2 ≤ k ≤ OMB_MAX_OBJ (omb_ehvi_boxes_k): the candidate-blocked kernel (boxes 4-byte aligned;
// check_boxes_k holds C to its LDS budget), and the one-wavefront-per-candidate kernel of launch_ehvi_boxes
// instantiated for every k (9·k·C ≤ kMaxLdsDoubles), the baseline it is measured against.
hipError_t launch_ehvi_boxes_kd(hipStream_t stream, int k, const double* mu, const double* var, int64_t ld, int64_t N,
                                const double* coords, int C, const uint16_t* boxes, int B, double* out);
hipError_t launch_ehvi_boxes_wave(hipStream_t stream, int k, const double* mu, const double* var, int64_t ld,
                                  int64_t N, const double* coords, int C, const uint16_t* boxes, int B, double* out);

// Hypervolume improvement of N points over the same box lists (omb_hvi.hip, omb_hvi_boxes): one lane per point, the
// grid alone in LDS (k·C ≤ kMaxLdsDoubles), boxes 4-byte aligned.  ws: hvi_ws_doubles(N, B) device doubles — the
// slices' sums where a small batch is split over the box list's slices, 0 otherwise; null runs unsplit.  Bitwise
// the same values either way.
int64_t hvi_ws_doubles(int64_t N, int B);
hipError_t launch_hvi_boxes(hipStream_t stream, int k, const double* y, int64_t ld, int64_t N, const double* coords,
                            int C, const uint16_t* boxes, int B, double* out, double* ws);

// The mean of that improvement over S sampled fronts (omb_hvi.hip, omb_hvi_paths / omb_plan_hvi_paths): y holds
// omb_paths_eval's rows (path s of objective j at row j·S + s, pitch ld), list s is rows box_off[s]..box_off[s+1] of
// boxes (S + 1 host offsets from 0) over the grid coords + s·k·C; 1 ≤ k ≤ OMB_MAX_OBJ, 1 ≤ S ≤ kPathsMaxS, N > 0.
// ws: hvi_paths_ws_doubles(N, S) device doubles — the per-path values where a small batch gives every path a
// workgroup row, 0 otherwise; null runs unsplit.  Bitwise the same values either way.
int64_t hvi_paths_ws_doubles(int64_t N, int S);
hipError_t launch_hvi_paths(hipStream_t stream, int k, int S, const double* y, int64_t ld, int64_t N,
                            const double* coords, int C, const uint16_t* boxes, const int32_t* box_off, double* out,
                            double* ws);
// launch_hvi_paths with n_con constraint slots behind the k objectives (rows (k + j)·S + s of y; omb_hvi_paths_con,
// DESIGN §26): u_s = t_s·w_s with the per-path feasibility weight w_s (eta = 0: the indicator; eta > 0: the sigmoid),
// violation != 0 (eta = 0): u_s = −(total violation) where w_s = 0.  out (N) the mean, u (S, ld) the u_s; either may be
// null, not both.  ws as launch_hvi_paths'.  At n_con = 0 out is bitwise launch_hvi_paths'.
hipError_t launch_hvi_paths_con(hipStream_t stream, int k, int S, int n_con, const double* y, int64_t ld, int64_t N,
                                const double* coords, int C, const uint16_t* boxes, const int32_t* box_off, double eta,
                                int violation, double* out, double* u, double* ws);
// launch_hvi_paths' out (bitwise) with grad[j·ld + i] = ∂out_i/∂x_j through dy, omb_paths_grad's gradient of the
// rows of y at the same pitch ((k·S, d, ld)); t_out (S, ld) / tgrad (S, d, ld): the per-path t_s and ∂t_s/∂x, both
// null or both set.  ws: hvi_paths_grad_ws_doubles(N, k, S) device doubles (the per-path t_s and ∂t_s/∂y).
int64_t hvi_paths_grad_ws_doubles(int64_t N, int k, int S);
hipError_t launch_hvi_paths_grad(hipStream_t stream, int k, int S, int d, const double* y, const double* dy,
                                 int64_t ld, int64_t N, const double* coords, int C, const uint16_t* boxes,
                                 const int32_t* box_off, double* out, double* grad, double* t_out, double* tgrad,
                                 double* ws);

hipError_t launch_hvpoi(hipStream_t stream, const double* mu, const double* var, int64_t ld, int64_t N,
                        const double* cells, int C, double* out);


hipError_t launch_expdec(hipStream_t stream, const ScalParams& sp, const double* mu, const double* var,
                         int64_t ld, int64_t N, const double* cache, int M, double* out);

hipError_t launch_ei(hipStream_t stream, int kind, int k, const double* mu, const double* var, int64_t ld, int64_t N,
                     double best, double var_eps, double pof_eps, double* out);

// out = acq·F (acq null: F), F the probability of feasibility over c rows of constraint moments (mu, var at row 0 of
// the constraints, pitch ld); out may be acq (omb_feasibility, omb_plan_constraints)
hipError_t launch_pof_scale(hipStream_t stream, int c, const double* mu, const double* var, int64_t ld, int64_t N,
                            double pof_eps, const double* acq, double* out);

// Log-space acquisitions (omb_logacq.hip; Plan::log, omb_log_ei / omb_log_ehvi_boxes / omb_log_feasibility):
//   launch_log_ei          log EI for OMB_EI_PLAIN / OMB_EI_CONSTRAINED over launch_ei's arguments
//   launch_log_pof         out = acq + log F (acq null: log F) over launch_pof_scale's arguments; out may be acq
//   launch_log_ehvi_boxes  log of the exact EHVI, 2 ≤ k ≤ OMB_MAX_OBJ, within check_boxes_k's limits (boxes 4-byte
//                          aligned): the one kernel behind both box plans
//   launch_log_ei_grad     ∂ log EI / ∂μ, ∂σ² into rows 0..k-1 of dadm / dadv (pitch N)
//   launch_log_pof_grad    rows k..k+c-1 of dadm / dadv: ∂ log F / ∂μ_j, ∂σ²_j (the objectives' rows stay: the weight
//                          is a sum in log space)
hipError_t launch_log_ei(hipStream_t stream, int kind, int k, const double* mu, const double* var, int64_t ld,
                         int64_t N, double best, double var_eps, double pof_eps, double* out);
hipError_t launch_log_pof(hipStream_t stream, int c, const double* mu, const double* var, int64_t ld, int64_t N,
                          double pof_eps, const double* acq, double* out);
hipError_t launch_log_ehvi_boxes(hipStream_t stream, int k, const double* mu, const double* var, int64_t ld, int64_t N,
                                 const double* coords, int C, const uint16_t* boxes, int B, double* out);
hipError_t launch_log_ei_grad(hipStream_t stream, int kind, int k, const double* mu, const double* var, int64_t ld,
                              int64_t N, double best, double var_eps, double pof_eps, double* dadm, double* dadv);
hipError_t launch_log_pof_grad(hipStream_t stream, const double* mu, const double* var, int64_t ld, int64_t N, int k,
                               int c, double pof_eps, double* dadm, double* dadv);

// Max-value entropy search (omb_mes.hip; omb_mes / omb_plan_mes): α over the moments (k, N) at pitch ld and the
// sampled minima ystar (k, S) on the device, 1 ≤ S ≤ kMesMaxS; the partials into rows 0..k-1 of dadm / dadv (pitch N)
hipError_t launch_mes(hipStream_t stream, int k, const double* mu, const double* var, int64_t ld, int64_t N,
                      const double* ystar, int S, double* out);
hipError_t launch_mes_grad(hipStream_t stream, int k, const double* mu, const double* var, int64_t ld, int64_t N,
                           const double* ystar, int S, double* dadm, double* dadv);

// Non-dominated filter (omb_pareto.hip; omb_nondominated) over S point sets y[(j·S + s)·ld + i], 1 ≤ k ≤ OMB_MAX_OBJ.
//   launch_nd_tile   one tile pass: in == nullptr runs over the points 0..N-1 themselves (Mmax = N), clears mask
//                    bytes 0..N-1 of every row and drops the NaN rows; else over the in_cnt[s] ≤ Mmax indices of
//                    in + s·in_pitch.  Survivors are appended to out + s·out_pitch (out_pitch ≥ Mmax) at slots taken
//                    from out_cnt[s], which the caller zeroed.
//   launch_nd_final  the cnt[s] ≤ Mmax survivors of list + s·pitch against one another: sets the mask bytes of those
//                    nothing dominates, then count[s]; blockcnt holds S·nd_final_blocks(Mmax) ints.
hipError_t launch_nd_tile(hipStream_t stream, int k, int S, const double* y, int64_t ld, int64_t N, const int32_t* in,
                          int64_t in_pitch, const int32_t* in_cnt, int64_t Mmax, int32_t* out, int64_t out_pitch,
                          int32_t* out_cnt, uint8_t* mask, int64_t ldm);
hipError_t launch_nd_final(hipStream_t stream, int k, int S, const double* y, int64_t ld, const int32_t* list,
                           int64_t pitch, const int32_t* cnt, int64_t Mmax, uint8_t* mask, int64_t ldm,
                           int32_t* blockcnt, int64_t* count);

// Exact hypervolume (omb_hypervolume.hip; omb_hypervolume / omb_hypervolume_contrib), sets in omb_nondominated's layout.
struct HvRef {
  double r[OMB_MAX_OBJ];
};
// What launch_hv_prep leaves of one set for launch_hv_cells: the kept points sorted by (y_{k-2}, y_{k-1}, row) — k = 1:
// (0, y_0) —, their grid ranks as 16-bit fields (objectives 0..3 in rlo, 4..5 in rhi), their rows, and per grid
// objective j its n_j distinct values followed by r_j.  n and the n_j are in the header: hdr[s·kHvHdr + 0 | 1 + j].
struct HvSet {
  double xs[kHvPoints], ys[kHvPoints];
  uint64_t rlo[kHvPoints];
  uint32_t rhi[kHvPoints];
  int32_t orig[kHvPoints];
  double grid[kHvGrid][kHvPoints + 1];
};
//   launch_hv_prep     filters, sorts and ranks the S sets (1 ≤ N ≤ kHvMaxN; mask may be null); a set with more than
//                      kHvPoints kept rows leaves a count above kHvPoints and nothing else
//   launch_hv_cells    out[v] = Σ_c w(c)·A(c) for v < V: the sets 0..V-1, or (per_point) set 0 whole and without its
//                      sorted point v − 1.  max_cells: the largest set's cell count (check_hv_work).  partials holds
//                      V·hv_cell_blocks(max_cells) doubles, scratch V·hv_reduce_blocks(that)
//   launch_hv_contrib  hv[0] = tot[0], contrib[orig[v]] = tot[0] − tot[v + 1] for the set's n kept points
hipError_t launch_hv_prep(hipStream_t stream, int k, int S, const double* y, int64_t ld, int64_t N,
                          const uint8_t* mask, int64_t ldm, const HvRef& ref, int32_t* hdr, HvSet* sets);
hipError_t launch_hv_cells(hipStream_t stream, int k, int V, bool per_point, int64_t max_cells, const int32_t* hdr,
                           const HvSet* sets, const HvRef& ref, double* partials, double* scratch, double* out);
hipError_t launch_hv_contrib(hipStream_t stream, const double* tot, const int32_t* hdr, const HvSet* set, double* hv,
                             double* contrib);

// Deterministic arg-max; `partials` must hold kArgmaxMaxBlocks (val, idx) pairs followed by one zeroed ticket word
// (one_pass: both passes in one launch, the last workgroup to arrive reducing; it leaves the word zeroed again).
constexpr int kArgmaxMaxBlocks = 1024;
hipError_t launch_argmax(hipStream_t stream, const double* vals, int64_t N, int64_t offset, double* partials,
                         double* result, bool one_pass = false);
// argmax_pass2 alone: nb (value, index) pairs → result {value, index + offset}
hipError_t launch_argmax_reduce(hipStream_t stream, const double* partials, int nb, int64_t offset, double* result);

// Scrambled Sobol' generation (omb_sobol.hip).  The packed state holds the direction
// numbers, shift and box of one engine; sobol_pack_state (omb_host.cpp) fills a host buffer of
// sobol_state_bytes(d, bits) that is then copied to the device.
hipError_t launch_sobol(hipStream_t stream, const void* state_dev, int d, int bits, int64_t start, int64_t N,
                        double* X);

// Dense fp64 linear algebra for Thompson sampling (omb_linalg.hip).  Row-major throughout.
constexpr int64_t kSelectMaxN = 1 << 18;    // candidates per selection (LDS exclusion bitmap)
constexpr int64_t kMaxCovN = 32768;         // candidates of one full posterior covariance
// GEMM tile geometry (omb_gemm.hip; the Cholesky trailing update and K(X*, X*) reuse it)
constexpr int kGT = 64;         // C tile edge
constexpr int kGK = 16;         // k slab
constexpr int kGP = kGT + 2;    // LDS row pitch in doubles (rows 528 B apart: conflict-free stores)
// C (M, Nc) = β·C + α·L·B with L (M, M) lower-triangular: its upper triangle is never read, and slabs past
// each row tile are skipped (half the work of launch_gemm_nn)
hipError_t launch_gemm_ltri_nn(hipStream_t s, int64_t M, int64_t Nc, double alpha, const double* L, int64_t ldl,
                               const double* B, int64_t ldb, double beta, double* C, int64_t ldc);
// C (M, Nc) = β C + α A B, A (M, K), B (K, Nc).
hipError_t launch_gemm_nn(hipStream_t s, int64_t M, int64_t Nc, int64_t K, double alpha, const double* A, int64_t lda,
                          const double* B, int64_t ldb, double beta, double* C, int64_t ldc);
// lower triangle of C (N, N) = β C + α AᵀA, A (K, N).
hipError_t launch_gemm_tn_lower(hipStream_t s, int64_t N, int64_t K, double alpha, const double* A, int64_t lda,
                                double beta, double* C, int64_t ldc);
// lower triangle of K(X*, X*) of one GP's kernel (ℓ, σ_f² from g) at Xc (N, d), diag_add added to the
// diagonal as it is stored (the jitter, without an add_diag launch); ws: cand_cov_ws_doubles device doubles
// (X*/ℓ and its squared norms).
int64_t cand_cov_ws_doubles(int64_t N, int DP);
hipError_t launch_cand_cov(hipStream_t stream, const GPDev& g, int d, int DP, const double* Xc, int64_t N, double* S,
                           int64_t lds, double* ws, double diag_add = 0.0, bool table = false);
// X*/ℓ rows (kp = ⌈DP/4⌉·4 doubles, written to ws) and their squared norms (ws + N·kp), as launch_cand_cov stages
// them; returns kp (0 for DP > kMaxFusedDP: the wide path has its own staging)
int launch_cand_scale(hipStream_t stream, const GPDev& g, int d, int DP, const double* Xc, int64_t N, double* ws,
                      hipError_t* err);
// lower triangle of S = K(X*, X*) + diag_add·I − VᵀV, V (K, N): the covariance SYRK with K(X*, X*) formed in its
// epilogue from launch_cand_scale's rows (omb_gemm.hip gemm_kernel<…, KSS>; glds: syrk_glds_kernel, the three-stage
// direct-to-LDS operand pipeline, where K % 16 = 0 and N, ldv even — bitwise the same C)
// zero_ints (n_zero ints) and zero_info: words the launch's workgroups set to 0 on the side (the next persistent
// Cholesky's sync words and status), so that factorisation needs no init launch
hipError_t launch_cov_syrk(hipStream_t s, int64_t N, int64_t K, const double* V, int64_t ldv, double* S, int64_t lds,
                           const double* xs, const double* xsq, int kp, int kind, double variance, double diag_add,
                           bool glds = true, int* zero_ints = nullptr, int n_zero = 0, int* zero_info = nullptr);
hipError_t launch_mirror_lower(hipStream_t stream, double* S, int64_t N, int64_t lds);
hipError_t launch_add_diag(hipStream_t stream, double* S, int64_t N, int64_t lds, double v);
// in-place lower Cholesky; info (device int, zeroed by the first kernel) = first bad column (1-based);
// ws: chol_ws_doubles(N) device doubles of workspace (the inverses of the diagonal blocks, as MFMA fragments for the
// panel product, then the schedule's flags).  info = kCholSpinFault: a workgroup's
// wait for the diagonal block ran out after spin_limit polls (the factor is invalid; reported as OMB_EHIP).
constexpr int kCholWsDoubles = 64 * 64;
constexpr int kCholSpinFault = -2147483647;
// Two schedules.  kCholPersistent, the default: the whole factorisation in one persistent launch (chol_persist_kernel:
// one workgroup walks the diagonal, the others draw panel and update tasks from a table), or kCholSteps where A is too
// large for that launch's 32-bit buffer offsets.  kCholSteps: one launch per 64-column step (chol_update_kernel, with
// the next diagonal block and panel inside).
enum { kCholPersistent = 0, kCholSteps = 1 };
int64_t chol_ws_doubles(int64_t N);
// acq_rel = 1: every cross-workgroup hand-off of the schedule as an agent-scope release / acquire pair (the HIP memory
// model's form; the default relaxed / sc1 form is measured valid on gfx950 and checked bitwise against this one).
// single_steps = 1: the persistent launch's workers take every trailing update as its own task (the default batches
// far tiles' updates, bitwise the same factor — checked against this one)
// zeroed / n_zeroed: ints that an earlier launch on the stream has set to 0 together with info (the covariance SYRK of
// the Thompson chain).  Where they are exactly the persistent launch's sync words (chol_persist_sync_words), it goes
// without its init kernel; any other range, and the per-step schedule, ignore them.
hipError_t launch_cholesky_mode(hipStream_t stream, double* A, int64_t N, int64_t lda, int* info, double* ws, int mode,
                                int spin_limit = kDefaultSpinLimit, int acq_rel = 0, int single_steps = 0,
                                const int* zeroed = nullptr, int n_zeroed = 0);
int chol_persist_sync_words(double* ws, int64_t N, int** ints);
// Y (B, N) = μ + Zt Lᵀ (L lower, N×N): row b of Y is the sample μ + L z_b.
// ws: chol_samples_ws_doubles(N, B) device doubles (split-K partial products; 0 when unsplit).
int64_t chol_samples_ws_doubles(int64_t N, int B);
hipError_t launch_chol_samples(hipStream_t stream, const double* L, int64_t N, int64_t ldl, const double* mu,
                               const double* Zt, int B, double* Y, double* ws);
// greedy per-sample arg-min (TuRBO select_candidates); ws: select_ws_bytes(B, N) bytes of device memory
// (the sorted heads of every sample when N ≤ kSelectSortN; 0 otherwise).
constexpr int64_t kSelectSortN = 8192;
int64_t select_ws_bytes(int B, int64_t N);
hipError_t launch_select(hipStream_t stream, const double* Y, int B, int64_t N, int64_t* idx, void* ws, bool seq = false);
// C (M, Nc) = β C + α AᵀB, A (K, M), B (K, Nc).
hipError_t launch_gemm_tn(hipStream_t s, int64_t M, int64_t Nc, int64_t K, double alpha, const double* A, int64_t lda,
                          const double* B, int64_t ldb, double beta, double* C, int64_t ldc);
// X (n, n) = L⁻¹ for lower-triangular L; X zeroed by the caller; T: workspace of 64·n doubles.
hipError_t launch_trinv(hipStream_t stream, const double* L, int64_t n, int64_t lda, double* X, int64_t ldx,
                        double* T);
// GP log-marginal-likelihood pieces: out[0..DP] = ½ Σ W ∂K/∂θ (θ = log σ_f², log ℓ_j; entries past
// d are 0), out[DP+1] = Σ log L_ii, out[DP+2] = yᵀα, and the noise entry's sums out[DP+3] = αᵀα,
// out[DP+4] = tr Ky⁻¹ (out: DP+5 doubles).  partials: gp_grad_blocks(n)·(DP+1) doubles.
int64_t gp_grad_blocks(int64_t n);
// n ≤ 128 and n_var ≤ 8 (gp_lml_small_fits): the whole evaluation in one workgroup (sweep-operator
// inverse in LDS, jitter retries in-kernel); out (DP+7 doubles): launch_gp_grad's first DP+3 slots, then
// out[DP+3] = jitter, out[DP+4] = info, out[DP+5] = αᵀα, out[DP+6] = −tr Ky⁻¹ (at that jitter).
bool gp_lml_small_fits(int n, int DP);
hipError_t launch_gp_lml_small(hipStream_t stream, int kind, int DP, const double* X, int d, int n,
                               const double* ls_host, double variance, double base, const double* y, double* out);
// k ≤ kFitBatchMax problems on the same X (y[p], ls_host[p·d..], variance[p], base[p] = σ_n² + 1e-8 of
// problem p → out[p]), one workgroup each
constexpr int kFitBatchMax = 4;
hipError_t launch_gp_lml_small_batch(hipStream_t stream, int kind, int DP, const double* X, int d, int n, int k,
                                     const double* const* y, const double* ls_host, const double* variance,
                                     const double* base, double* const* out);
// dense posterior path: μ, σ² of a candidate chunk from K* (n, Nc) and V = L⁻¹K* (n, Nc).
hipError_t launch_post_colreduce(hipStream_t stream, const double* Kst, const double* V, int64_t n, int64_t Nc,
                                 const double* alpha, double variance, double* mu, double* var,
                                 const GPDev* scale_g = nullptr, int d = 0, int DP = 0, const double* Xc = nullptr,
                                 double* ws = nullptr);   // scale_g: also launch_cand_scale's rows into ws
hipError_t launch_gp_grad(hipStream_t stream, int kind, int DP, const double* X, int d, int64_t n, const double* ls,
                          double variance, const double* alpha, const double* Kinv, int64_t ldk, double* partials,
                          const double* L, int64_t lda, const double* y, double* out);

// ParEGO / KEEP evolutionary acquisition search (omb_ea.hip): one workgroup runs the whole search from a
// host-replayed tape of the reference's random draws.  ldt_ws: n0·n0 doubles (L0⁻¹ transposed).
constexpr int kEAMaxPop = 32;
constexpr int kEAMaxTrain = 2048;
constexpr int kEALdsN = 128;      // L0⁻¹ kept in LDS (packed lower) up to this n_train
struct EASearch {
  GPDev g0, g1;          // g0: the EI model; g1: KEEP's Pareto-membership model (mode 1)
  const double* Ld0;     // dense row-major L0⁻¹ (n0, n0)
  int mode, d, DP, P, iters;
  double best, var_eps;
  const double* pop;
  const int* sel;
  const int8_t* cross;
  const double* beta;
  const int8_t* mut;
  const double* lower;
  const double* upper;
  double* out;
};
hipError_t launch_ea_search(hipStream_t stream, const EASearch& s, double* ldt_ws);

// ---------------------------------------------------------------------------------------
// Wide inputs (omb_wide.hip): n_var 65 .. OMB_MAX_DIM, DP = 128 or 256.  The fused posterior kernel and the
// register-fragment K-block / covariance / gradient kernels hold a candidate's coordinates in registers, which
// is only affordable up to kMaxFusedDP; above it the cross terms run as GEMM tiles with the k loop over slabs of
// kWideSlab dimensions staged in LDS, and the posterior takes the dense path (K block → V = L⁻¹K* → column
// reduction, posterior_any).  Every entry point keeps its meaning and its parity bar.
constexpr int kMaxFusedDP = 64;
constexpr int kWideSlab = 16;
// K (M, N) row-major, pitch ldk: K[i][c] = k(X_i, X*_c) for the training rows of g (pre-scaled g.Xs, g.xsq, pitch
// DP) against the raw candidates Xc (N, d), divided by ℓ as they are staged.
hipError_t launch_kernel_block_wide(hipStream_t stream, const GPDev& g, int d, int DP, const double* Xc, int64_t N,
                                    double* K, int64_t ldk);
// launch_cand_cov for DP > kMaxFusedDP (same arguments and workspace, cand_cov_ws_doubles(N, DP))
hipError_t launch_cand_cov_wide(hipStream_t stream, const GPDev& g, int d, int DP, const double* Xc, int64_t N,
                                double* S, int64_t lds, double* ws, double diag_add);
// gp_grad_kernel's partial sums for DP > kMaxFusedDP (the same layout: gp_grad_blocks(n) blocks × (DP + 1))
hipError_t launch_gp_grad_partials_wide(hipStream_t stream, int kind, int DP, const double* X, int d, int64_t n,
                                        const double* ls, double variance, const double* alpha, const double* Kinv,
                                        int64_t ldk, double* partials);

// ---------------------------------------------------------------------------------------
// Gradients with respect to a candidate (omb_grad.hip): omb_posterior_grad, omb_eval_grad.
struct GradObj {
  const double* Xs;     // GPDev::Xs (n_pad, DP)
  const double* alpha;  // GPDev::alpha
  const double* ls;     // GPDev::ls
  const double* W;      // (n, nc) row-major: w = L⁻ᵀ(L⁻¹k) of the chunk's candidates
  double variance;
  int n;
  int pad_;
};
struct GradArgs {
  GradObj o[OMB_MAX_OBJ];
  int n_obj, d, DP;
  int JW;   // the power of two ≥ d (≤ 256): threads per training row in the contraction
};
// ∂μ_o/∂x, ∂σ²_o/∂x of the nc candidates Xc (nc, d) — candidates c0 .. c0 + nc − 1 of a batch of N — into dmu / dvar
// (n_obj, N, d) when dmu is non-null, and, when grad is non-null, grad (N, d) = Σ_o dadm[o]·∂μ_o/∂x + dadv[o]·∂σ²_o/∂x
// (dadm, dadv (n_obj, N); an all-NaN row where vals[c] is NaN).  One workgroup per candidate.
hipError_t launch_grad_contract(hipStream_t stream, const GradArgs& ga, int kind, const double* Xc, int64_t nc,
                                int64_t c0, int64_t N, double* dmu, double* dvar, const double* dadm,
                                const double* dadv, const double* vals, double* grad);
// ∂a/∂μ_o, ∂a/∂σ²_o of the acquisitions (rows o of dadm / dadv, pitch N), arguments as the value launchers'
hipError_t launch_ei_grad(hipStream_t stream, int kind, int k, const double* mu, const double* var, int64_t ld,
                          int64_t N, double best, double var_eps, double pof_eps, double* dadm, double* dadv);
// the product rule of a·F over dadm / dadv (k + c rows, pitch N): rows 0..k-1, the plan's partials, scaled by F; rows
// k.. filled with the constraints' (a: the unweighted acquisition; mu / var: constraint row 0, pitch ld)
hipError_t launch_pof_grad(hipStream_t stream, const double* a, const double* mu, const double* var, int64_t ld,
                           int64_t N, int k, int c, double pof_eps, double* dadm, double* dadv);
hipError_t launch_ehvi2d_grad(hipStream_t stream, const double* mu, const double* var, int64_t ld, int64_t N,
                              const double* pf, int P, double r0, double r1, double s00, double s01, int mode,
                              double* dadm, double* dadv);
hipError_t launch_ehvi_boxes_grad(hipStream_t stream, int k, const double* mu, const double* var, int64_t ld,
                                  int64_t N, const double* coords, int C, const uint16_t* boxes, int B, double* dadm,
                                  double* dadv);

// ---------------------------------------------------------------------------------------
// Conditioning an installed state on more observations (omb_append.hip): omb_gp_append.
// The bordered state of m = n + q points as the kernels grow it, carved from one workspace.
struct AppendWs {
  double* L;        // (m, m) row-major L⁻¹, zeros above the diagonal
  double* alpha;    // (m)
  double* Xs;       // (m, DP) inputs / ℓ as pack_rows_kernel writes them
  double* xsq;      // (m)
  double* X;        // (m, d) unscaled inputs
  double* kvec;     // (m) k = K(X, x) of the point being appended
  double* v;        // (m) v = L⁻¹k
  double* wpart;    // (⌈m/256⌉, m) partial sums of w = L⁻ᵀv
  double* mupart;   // (⌈m/256⌉) partial sums of μ = k·α
  double* scal;     // {δ, ζ/δ}
  int* info;        // 0, or the 1-based index of the first point whose δ² is not positive and finite
  double* scratch;  // (m + DP) pack_rows_kernel's α / ℓ outputs for the new rows (not used)
  int m, d, DP;
};
int64_t append_ws_doubles(int m, int d, int DP);
void append_ws_carve(double* base, int m, int d, int DP, AppendWs* ws);
// ws.L ← the lower triangle of Ld (n, n), re-strided to pitch m, zeros elsewhere
hipError_t launch_append_restride(hipStream_t stream, const AppendWs& ws, int n, const double* Ld);
// Ld (n, n) ← the lower triangle of Linv (n, n), zeros above the diagonal (the same kernel at m = n): the installed
// dense L⁻¹, so that the transposed products (w = L⁻ᵀV) never see what a caller left above the diagonal
hipError_t launch_copy_lower(hipStream_t stream, int n, const double* Linv, double* Ld);
// point j of the call (row c = n + j of ws.Xs / ws.xsq, already scaled) joins the c points of ws: row c of ws.L,
// ws.alpha updated; ynew null = the Kriging believer (y = μ); mu_out[j] = μ, var_out[j] = δ² (either may be null)
hipError_t launch_append_point(hipStream_t stream, const AppendWs& ws, int kind, double variance, int c, int j,
                               const double* ynew, double noise, double* mu_out, double* var_out);

// ---------------------------------------------------------------------------------------
// Posterior sample paths (omb_paths.hip): omb_paths_set, omb_paths_eval.
struct PathObj {
  GPDev g;
  const double* Of;   // [ω̃, b] of the features, A-fragment order (omb_host.h paths_pack)
  const double* Wf;   // sqrt(2σ_f²/m)·w, A-fragment order, zero padded to 16 paths
  const double* Vf;   // v = α − L⁻ᵀL⁻¹U, A-fragment order, zero padded (launch_paths_pack_v)
  int MT;             // feature tiles ⌈m/16⌉
  int R;              // training-row tiles of the update term (0: the prior paths alone)
  int S;              // paths
  int pad_;
};
struct PathArgs {
  PathObj o[OMB_MAX_OBJ];
  int d, DP;
};
// out[(o·S + s)·ld + i] = path s of objective o at Xc_i (N > 0, DP ≤ kMaxFusedDP); libcos: the library cosine
// in place of the kernel's own (OMB_DEBUG_PATHS_LIBCOS, the baseline it is measured against)
hipError_t launch_paths_eval(hipStream_t stream, const PathArgs& pa, int n_obj, int kind, bool libcos,
                             const double* Xc, int64_t N, int64_t ld, double* out);
// launch_paths_eval's out (bitwise) and grad[((o·S + s)·d + j)·ld + i] = ∂(path s of objective o)/∂x_j at Xc_i
hipError_t launch_paths_grad(hipStream_t stream, const PathArgs& pa, int n_obj, int kind, bool libcos,
                             const double* Xc, int64_t N, int64_t ld, double* out, double* grad);
// res[(o·S + s)·2 + {0, 1}] = {min_i of path s of objective o over Xc (N ≥ 0), the lowest such i + offset}; {+inf, −1}
// where no value is comparable.  partials: paths_min_blocks(N)·n_obj·16·2 doubles (the workgroups' pairs of the first
// launch; a second launch reduces them in a fixed order).
int paths_min_blocks(int64_t N);
hipError_t launch_paths_min(hipStream_t stream, const PathArgs& pa, int n_obj, int kind, bool libcos, const double* Xc,
                            int64_t N, int64_t offset, double* partials, double* res);
// U (n, S) = Fᵀ + sd·z, F (S rows of pitch n), z (n, S) or null
hipError_t launch_paths_u(hipStream_t stream, const double* F, const double* z, double sd, int n, int S, double* U);
// Vf (paths_vf_doubles(R)) from α (n) and G = L⁻ᵀL⁻¹U (n, S)
hipError_t launch_paths_pack_v(hipStream_t stream, const double* alpha, const double* G, int n, int S, int R,
                               double* Vf);

// Packed-L^-1 size in doubles for R row tiles: Σ_{r<R} 4(r+1)·64 = 128·R·(R+1).
inline int64_t packed_L_size(int R) { return 128ll * R * (R + 1); }
// k-step pairs of the training-row A fragments [x/ℓ, ‖x/ℓ‖², 1]: ⌈⌈(DP+2)/4⌉/2⌉
inline int packed_X_pairs(int DP) { return ((DP + 5) / 4 + 1) / 2; }
inline int64_t packed_X_size(int n_pad, int DP) { return (int64_t)(n_pad / 16) * packed_X_pairs(DP) * 128; }

}  // namespace omb
