// Host-only argument validation and upload packing of liboptimobo_hip.so's C-ABI (no HIP runtime, no device code).
//
// omb_api.hip calls these before it touches the device, so every entry point's argument checks, the
// expected-decomposition parameter block and the Sobol' state packing are plain C++ that builds with a host
// compiler alone: `make -C optimobo_amd/csrc asan` compiles this file under ASan + UBSan into the fuzz driver
// tests/asan/omb_host_fuzz.cpp (and into an ASan build of the library that tests/test_lib_cpu.py loads).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/optimobo_hip.h"

namespace omb {

// Acquisition kernels stage their per-iteration geometry in ≤ 64 KiB of dynamic LDS.
constexpr int kMaxLdsDoubles = 8192;
constexpr int kMaxStripes = (kMaxLdsDoubles - 1) / 2;

// Parameters of one expected_decomposition scalarisation (omb_acquisition.hip's expdec_kernel).
struct ScalParams {
  int id;
  int k;
  double w[OMB_MAX_OBJ];
  double ideal[OMB_MAX_OBJ];
  double range[OMB_MAX_OBJ];   // max − ideal
  double p[4];
  double wnorm;                // ‖w‖ (PBI family)
  double d_star;               // QPBI
  double agg_min;
};

// Formats the message into *err (when err is non-null) and returns code.
int errf(std::string* err, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));

// n_var padded to the posterior kernels' DP ∈ {2, 4, 6, 8, 16, 32, 64, 128, 256}; −1 above OMB_MAX_DIM.
int pad_dim(int d);

int check_moments(std::string* err, const void* mu, const void* var, int64_t ld, int64_t N, int k, const void* out);
int check_ehvi2d(std::string* err, int P, const double* r, int mode);
int check_ehvi_mc(std::string* err, int k, int M, const double* r);
int check_boxes(std::string* err, int k, int C, int B);
// omb_ehvi_boxes_k / omb_plan_ehvi_boxes_k: 2 ≤ k ≤ OMB_MAX_OBJ, 3·k·C + 2·k + 4 ≤ kMaxLdsDoubles, 1 ≤ B ≤ kMaxBoxesK.
constexpr int kMaxBoxesK = 1 << 24;
int check_boxes_k(std::string* err, int k, int C, int64_t B);
// omb_hvi_boxes, in this order: OMB_EINVAL for k outside [2, OMB_MAX_OBJ], N < 0, B < 1, a null grid / box list (and,
// with N > 0, a null y / out), a pointer off its alignment (8 bytes; the box list 4) or ld < N; OMB_EUNSUP for C < 2,
// k·C > kMaxLdsDoubles or B > kMaxBoxesK.
int check_hvi_boxes(std::string* err, int k, const void* y, int64_t ld, int64_t N, const void* coords, int C,
                    const void* boxes, int64_t B, const void* out);
// Every box of a host box list (B, 2k): lo index < hi index < C (an index past the grid would be read from LDS).
int check_box_list(std::string* err, int k, int C, const uint16_t* boxes, int64_t B);
int check_ei(std::string* err, int kind, int k, double var_eps, double pof_eps);
int check_hvpoi(std::string* err, int C);
// omb_plan_constraints on a plan over plan_k objectives (0: none set): OMB_ESTATE with no plan, OMB_EINVAL for
// n_con < 0 or a negative / non-finite pof_eps, OMB_EUNSUP for plan_k + n_con > OMB_MAX_OBJ — in that order.
int check_constraints(std::string* err, int plan_k, int n_con, double pof_eps);
// omb_plan_log, in this order: OMB_ESTATE with no plan (has_plan 0), OMB_EINVAL for `on` outside {0, 1}, OMB_EUNSUP
// naming the plan when it has no log form (refused: its name; null for a plan that has one).
int check_plan_log(std::string* err, int has_plan, int on, const char* refused);
// omb_log_ei: check_ei, then OMB_EUNSUP for OMB_EI_PARETO (μ₁·EI has no logarithm where μ₁ ≤ 0).
int check_log_ei(std::string* err, int kind, int k, double var_eps, double pof_eps);
// omb_feasibility: 1 ≤ c ≤ OMB_MAX_OBJ, pof_eps finite and ≥ 0, then check_moments over the c rows.
int check_feasibility(std::string* err, int c, const void* mu, const void* var, int64_t ld, int64_t N, double pof_eps,
                      const void* out);
// omb_posterior_grad: 1 ≤ n_obj ≤ OMB_MAX_OBJ, N ≥ 0, and with N > 0 no null candidate / output pointer.
int check_posterior_grad(std::string* err, int n_obj, const void* Xc, int64_t N, const void* mu, const void* var,
                         const void* dmu, const void* dvar);
// omb_eval_grad: N ≥ 0, and with N > 0 no null candidate / output pointer.
int check_eval_grad(std::string* err, const void* Xc, int64_t N, const void* vals, const void* grad);
// Candidates per pass of the gradient chain: its workspace holds (n_obj + 2)·n_train doubles per candidate (K*, V
// and one w per objective) and is kept to 512 MiB; at least 64, at most 2^20 and N (0 for an empty or out-of-range request).
int64_t grad_chunk(int n_obj, int n_train, int64_t N);
// Posterior sample paths (omb_paths_set / omb_paths_eval, omb_paths.hip).
constexpr int kPathsMaxS = 16;            // paths per objective: one MFMA accumulator tile
constexpr int kPathsMaxFeatures = 65536;  // random Fourier features per objective
constexpr int kPathsMaxDim = 64;          // n_var: the candidates' fragments stay in registers
// State of one objective as the checks see it: whether a GP is installed, its shape, and the S of its paths (0: none).
struct PathsObjInfo {
  int set, n_var, n_train, S;
};
// omb_paths_set, in this order: OMB_EINVAL for obj outside [0, OMB_MAX_OBJ), S outside [1, kPathsMaxS], m outside
// [1, kPathsMaxFeatures], a null omega / phase / w or a negative or non-finite noise; OMB_ESTATE for an objective
// without a GP; OMB_EUNSUP for n_var > kPathsMaxDim or n_train > OMB_MAX_TRAIN_DENSE.
int check_paths_set(std::string* err, int obj, int S, int m, const void* omega, const void* phase, const void* w,
                    double noise, const PathsObjInfo* info);
// omb_paths_eval over info[0..n_obj-1] (info: OMB_MAX_OBJ entries), in this order: OMB_EINVAL for n_obj outside
// [1, OMB_MAX_OBJ], N < 0, ld < N or (N > 0) a null Xc / out; OMB_ESTATE for an objective without a GP or without
// paths, or with another S than objective 0; OMB_EUNSUP for n_var > kPathsMaxDim or n_train > OMB_MAX_TRAIN_DENSE.
int check_paths_eval(std::string* err, int n_obj, const void* Xc, int64_t N, int64_t ld, const void* out,
                     const PathsObjInfo* info);
// omb_paths_grad: check_paths_eval's refusals in its order, a null grad (N > 0) refused where a null out is.
int check_paths_grad(std::string* err, int n_obj, const void* Xc, int64_t N, int64_t ld, const void* out,
                     const void* grad, const PathsObjInfo* info);
// omb_paths_min: check_paths_eval's refusals in its order, without a pitch and with res in out's place — and res may
// not be null even at N = 0 (the empty batch still writes {+inf, −1} for every path): OMB_EINVAL for n_obj outside
// [1, OMB_MAX_OBJ], N < 0, a null res or (N > 0) a null Xc; then OMB_ESTATE and OMB_EUNSUP as there.
int check_paths_min(std::string* err, int n_obj, const void* Xc, int64_t N, const void* res, const PathsObjInfo* info);
// Workgroups per objective of omb_paths_min's first launch (each leaves one (value, index) pair per path).
constexpr int kPathsMinMaxBlocks = 1024;
// Max-value entropy search (omb_mes / omb_plan_mes, omb_mes.hip): sampled minima per objective.
constexpr int kMesMaxS = 64;
// omb_mes, in this order: OMB_EINVAL for k outside [1, OMB_MAX_OBJ], S outside [1, kMesMaxS], N < 0, (N > 0) a null
// mu / var / ystar / out, or ld < N with k > 1.
int check_mes(std::string* err, int k, int S, const void* mu, const void* var, int64_t ld, int64_t N,
              const void* ystar, const void* out);
// omb_plan_mes, in this order: OMB_EINVAL for k outside [1, OMB_MAX_OBJ], S outside [1, kMesMaxS], a null ystar, or a
// non-finite entry among its k·S (a plan built on it would be NaN everywhere).
int check_plan_mes(std::string* err, int k, int S, const double* ystar);
// omb_hvi_paths (and, with y = out = null and N = 0, omb_plan_hvi_paths over its host arrays), in this order:
// OMB_EINVAL for k outside [1, OMB_MAX_OBJ], S outside [1, kPathsMaxS], N < 0, a null grid / box list / offsets,
// offsets that do not start at 0 or decrease or leave a list empty, (N > 0) a null y / out, a pointer off its alignment
// (8 bytes; the box list 4) or ld < N; OMB_EUNSUP for C < 2, k·C > kMaxLdsDoubles or box_off[S] > kMaxBoxesK.
int check_hvi_paths(std::string* err, int k, int S, const void* y, int64_t ld, int64_t N, const void* coords, int C,
                    const int32_t* box_off, const void* boxes, const void* out);
// omb_hvi_paths_grad: check_hvi_paths' OMB_EINVAL refusals in its order; then OMB_EINVAL for d outside
// [1, kPathsMaxDim], (N > 0) a null dy / grad, exactly one of t / tgrad null, or one of the four off its 8-byte
// alignment; then check_hvi_paths' OMB_EUNSUP refusals.
int check_hvi_paths_grad(std::string* err, int k, int S, int d, const void* y, const void* dy, int64_t ld, int64_t N,
                         const void* coords, int C, const int32_t* box_off, const void* boxes, const void* out,
                         const void* grad, const void* t, const void* tgrad);
// omb_hvi_paths_con (and, with y = out = u = null, N = 0 and flags = 0, omb_plan_hvi_paths_con): check_hvi_paths'
// refusals in its order, a null out allowed; then OMB_EINVAL for n_con < 0, eta negative or not finite, flag bits
// other than OMB_CON_VIOLATION, that flag with eta > 0, (N > 0) out and u both null, or u off its 8-byte alignment;
// then OMB_EUNSUP for k + n_con > OMB_MAX_OBJ.
int check_hvi_paths_con(std::string* err, int k, int S, int n_con, const void* y, int64_t ld, int64_t N,
                        const void* coords, int C, const int32_t* box_off, const void* boxes, double eta,
                        unsigned flags, const void* out, const void* u);
// Non-dominated filter (omb_nondominated, omb_pareto.hip).
constexpr int kNdMaxS = OMB_NONDOM_SETS;        // point sets of one call (omb_paths_eval's S)
constexpr int64_t kNdMaxN = OMB_NONDOM_POINTS;  // points per set
constexpr int kNdTile = 1024;                   // points of one LDS tile = lanes of its workgroup (64 KiB at k = 8)
constexpr int kNdMaxRounds = 4;                 // tile passes before the final pass
// omb_nondominated, in this order: OMB_EINVAL for k outside [1, OMB_MAX_OBJ], S outside [1, kNdMaxS], N < 0, ld < N or
// ldm < N, a null count, (N > 0) a null y / mask, or y / count off 8-byte alignment; OMB_EUNSUP for N > kNdMaxN.
int check_nondominated(std::string* err, int k, int S, const void* y, int64_t ld, int64_t N, const void* mask,
                       int64_t ldm, const void* count);
// Whether another tile pass follows one that left `now` survivors (the largest set's) of `before`: while the list is
// longer than one tile, the last pass at least halved it and fewer than kNdMaxRounds passes have run.
inline bool nd_another_round(int rounds_done, int64_t before, int64_t now) {
  return rounds_done < kNdMaxRounds && now > kNdTile && 2 * now <= before;
}
// Workgroups per set of the final pass over at most M survivors (at least one: an empty set still writes its count).
inline int64_t nd_final_blocks(int64_t M) { return M < 1 ? 1 : (M + kNdTile - 1) / kNdTile; }
// Exact hypervolume (omb_hypervolume / omb_hypervolume_contrib, omb_hypervolume.hip).
constexpr int kHvMaxS = OMB_NONDOM_SETS;        // point sets of one call
constexpr int64_t kHvMaxN = OMB_NONDOM_POINTS;  // rows per set
constexpr int kHvPoints = OMB_HV_POINTS;        // kept rows per set = lanes of the preparation workgroup
constexpr int kHvGrid = OMB_MAX_OBJ - 2;        // grid objectives at most
constexpr int kHvHdr = 8;                       // ints per set of the header: n, n_0..n_5, one spare
constexpr int kHvCellLanes = 512;               // lanes of a cell workgroup
constexpr int kHvCellsPerLane = 4;
constexpr int64_t kHvBlockCells = (int64_t)kHvCellLanes * kHvCellsPerLane;
constexpr int kHvReduceLanes = 256;             // a reduction workgroup adds 2·kHvReduceLanes partial sums
// omb_hypervolume (contrib: 0) and omb_hypervolume_contrib (contrib: 1, called with S = 1 and ldm = N), in this order:
// OMB_EINVAL for k outside [1, OMB_MAX_OBJ], S outside [1, kHvMaxS], N < 0, ld < N or ldm < N, a null r or a non-finite
// r_j, a null hv (contrib: or a null out), (N > 0) a null y, or y / hv / out off 8-byte alignment; OMB_EUNSUP for
// N > kHvMaxN.  The mask is bytes and may be null.
int check_hypervolume(std::string* err, int k, int S, const void* y, int64_t ld, int64_t N, const void* mask,
                      int64_t ldm, const double* r, const void* hv, int contrib, const void* out);
// Π of the g grid sizes nj[0..g-1] (1 for g = 0), saturating at INT64_MAX; 0 when one of them is < 1.
int64_t hv_cells(int g, const int32_t* nj);
// What the preparation kernel left for S sets of k objectives (hdr: S rows of kHvHdr ints), before the cell launch is
// sized from it: OMB_EUNSUP for a set with more than kHvPoints kept rows, OMB_EHIP for a header no preparation can
// leave (n < 0, a grid size outside [1, n]), then OMB_EUNSUP for Σ_s cells_s·n_s·variants above OMB_HV_MAX_WORK
// (variants: n_s + 1 with per_point, else 1; every product and the sum saturate).  *max_cells: the largest set's cells.
int check_hv_work(std::string* err, int k, int S, const int32_t* hdr, int per_point, int64_t* max_cells);
// Workgroups per set (variant) of the cell launch, at least one; partial sums after one reduction pass over m.
inline int64_t hv_cell_blocks(int64_t cells) { return cells < 1 ? 1 : (cells - 1) / kHvBlockCells + 1; }
inline int64_t hv_reduce_blocks(int64_t m) { return m < 1 ? 1 : (m - 1) / (2 * kHvReduceLanes) + 1; }
// check_box_list over every list of a host (box_off[S], 2k) list whose offsets passed check_hvi_paths.
int check_box_lists(std::string* err, int k, int S, int C, const int32_t* box_off, const uint16_t* boxes);
// Candidates per pass of the fused chain under an omb_plan_hvi_paths plan (the default of OMB_DEBUG_HVI_PATHS_CHUNK):
// the chain holds the (k·S, chunk) path values, not (k·S, N).
constexpr int64_t kHviPathsChunk = OMB_HVI_PATHS_CHUNK;
// The paths' operands in the A-fragment order of v_mfma_f64_16x16x4_f64 (lane l holds A[l & 15][l >> 4]), zero
// padded to whole tiles of 16 features and to 16 paths:
//   Of[(T·ksf + s)·64 + l] = [ω̃_i, b_i, 0 …][4s + (l >> 4)] of feature i = 16T + (l & 15)   (ksf = paths_ksf(DP))
//   Wf[(4T + e)·64 + l]    = scale · w[16T + 4e + (l >> 4)][l & 15]
inline int paths_ksf(int DP) { return (DP + 4) / 4; }
inline int64_t paths_of_doubles(int m, int DP) { return (int64_t)((m + 15) / 16) * paths_ksf(DP) * 64; }
inline int64_t paths_wf_doubles(int m) { return (int64_t)((m + 15) / 16) * 256; }
inline int64_t paths_vf_doubles(int R) { return (int64_t)R * 256; }
void paths_pack(int m, int d, int DP, int S, const double* omega, const double* phase, const double* w, double scale,
                double* Of, double* Wf);
// Validates an expected_decomposition request and fills its ScalParams.
int build_scal(std::string* err, int k, int M, int scal_id, const double* params_host, const double* weights_host,
               const double* ideal_host, const double* max_host, double agg_min, ScalParams* out);
// omb_set_gp's host-side checks (before any device work).
int check_gp_args(std::string* err, int obj, int kernel, int n, int d, const void* X_dev, const double* lengthscale_host,
                  double variance, const void* alpha_dev, const void* Linv_dev);
// omb_set_sobol's host-side checks.
int check_sobol_args(std::string* err, int d, int bits, const void* sv_host, const void* shift_host,
                     const double* lo_host, const double* hi_host);

// The packed Sobol' state (sobol_kernel's layout): sv (d·bits uint32) | shift (d uint32) | [pad] | lo (d f64) |
// width (d f64).
size_t sobol_state_bytes(int d, int bits);
void sobol_pack_state(int d, int bits, const uint32_t* sv, const uint32_t* shift, const double* lo, const double* hi,
                      void* dst);

}  // namespace omb
