// Host-only validation and packing of the C-ABI's arguments (see omb_host.h).  Every size product is formed in
// 64 bits: the entry points take int / int64_t counts straight from the caller, so a hostile M or C must fail the
// check, not overflow it (UBSan in `make asan` holds this file to that).
#include "omb_host.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

namespace omb {

int errf(std::string* err, int code, const char* fmt, ...) {
  if (err) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    *err = buf;
  }
  return code;
}

int pad_dim(int d) {
  const int opts[] = {2, 4, 6, 8, 16, 32, 64, 128, 256};   // > 64: the wide path (omb_wide.hip)
  for (int o : opts)
    if (d <= o) return o;
  return -1;
}

int check_moments(std::string* err, const void* mu, const void* var, int64_t ld, int64_t N, int k, const void* out) {
  if (N < 0) return errf(err, OMB_EINVAL, "N=%lld < 0", (long long)N);
  if (N > 0 && (!mu || !var || !out)) return errf(err, OMB_EINVAL, "null device pointer");
  if (k > 1 && ld < N) return errf(err, OMB_EINVAL, "ld=%lld < N=%lld", (long long)ld, (long long)N);
  return OMB_OK;
}

int check_ehvi2d(std::string* err, int P, const double* r, int mode) {
  // stripes y1[0..P], y2[1..P] are staged in ≤ 64 KiB of LDS
  if (P < 1 || P > kMaxStripes) return errf(err, OMB_EUNSUP, "Pareto front size P=%d outside [1, %d]", P, kMaxStripes);
  if (!r) return errf(err, OMB_EINVAL, "null reference point");
  if (mode != OMB_EHVI_REFERENCE && mode != OMB_EHVI_TEXTBOOK && mode != OMB_EHVI_SIGMA)
    return errf(err, OMB_EINVAL, "unknown EHVI mode %d", mode);
  return OMB_OK;
}

int check_ehvi_mc(std::string* err, int k, int M, const double* r) {
  if (k < 2 || k > OMB_MAX_OBJ)
    return errf(err, OMB_EINVAL, "Monte-Carlo EHVI needs 2 <= k <= %d objectives (k=%d)", OMB_MAX_OBJ, k);
  // the (M, k) cache is staged in <= 64 KiB of dynamic LDS
  if (M < 1 || (int64_t)k * M > kMaxLdsDoubles)
    return errf(err, OMB_EUNSUP, "cache size M=%d outside [1, %d] for k=%d", M, kMaxLdsDoubles / k, k);
  if (!r) return errf(err, OMB_EINVAL, "null reference point");
  return OMB_OK;
}

int check_boxes(std::string* err, int k, int C, int B) {
  if (k != 2 && k != 3) return errf(err, OMB_EUNSUP, "exact EHVI needs k = 2 or 3 objectives (k=%d)", k);
  // grid + 4 per-wave Φ/φ tables must fit the 64 KiB of dynamic LDS
  if (C < 2 || (int64_t)k * C * 9 > kMaxLdsDoubles)
    return errf(err, OMB_EUNSUP, "grid size C=%d outside [2, %d] for k=%d", C, kMaxLdsDoubles / (9 * k), k);
  if (B < 1) return errf(err, OMB_EINVAL, "empty box list");
  return OMB_OK;
}

int check_boxes_k(std::string* err, int k, int C, int64_t B) {
  if (k < 2 || k > OMB_MAX_OBJ)
    return errf(err, OMB_EINVAL, "exact EHVI needs 2 <= k <= %d objectives (k=%d)", OMB_MAX_OBJ, k);
  // one candidate's (Φ, φ) tables, its (μ, σ), the grid and the reduction words must fit the 64 KiB of dynamic LDS
  const int64_t c_max = (kMaxLdsDoubles - 2 * k - 4) / (3 * (int64_t)k);
  if (C < 2 || 3 * (int64_t)k * C + 2 * k + 4 > kMaxLdsDoubles)
    return errf(err, OMB_EUNSUP, "grid size C=%d outside [2, %lld] for k=%d", C, (long long)c_max, k);
  if (B < 1) return errf(err, OMB_EINVAL, "empty box list");
  if (B > kMaxBoxesK) return errf(err, OMB_EUNSUP, "box count B=%lld above %d", (long long)B, kMaxBoxesK);
  return OMB_OK;
}

int check_hvi_boxes(std::string* err, int k, const void* y, int64_t ld, int64_t N, const void* coords, int C,
                    const void* boxes, int64_t B, const void* out) {
  if (k < 2 || k > OMB_MAX_OBJ)
    return errf(err, OMB_EINVAL, "hypervolume improvement needs 2 <= k <= %d objectives (k=%d)", OMB_MAX_OBJ, k);
  if (N < 0) return errf(err, OMB_EINVAL, "N=%lld < 0", (long long)N);
  if (B < 1) return errf(err, OMB_EINVAL, "empty box list");
  if (!coords || !boxes) return errf(err, OMB_EINVAL, "null grid/box list");
  if (N > 0 && (!y || !out)) return errf(err, OMB_EINVAL, "null device pointer");
  if (((uintptr_t)y | (uintptr_t)coords | (uintptr_t)out) & 7)
    return errf(err, OMB_EINVAL, "points, grid or output not 8-byte aligned");
  if ((uintptr_t)boxes & 3) return errf(err, OMB_EINVAL, "box list not 4-byte aligned");
  if (ld < N) return errf(err, OMB_EINVAL, "ld=%lld < N=%lld", (long long)ld, (long long)N);
  // the grid alone is staged in the 64 KiB of dynamic LDS; the box list is streamed
  if (C < 2 || (int64_t)k * C > kMaxLdsDoubles)
    return errf(err, OMB_EUNSUP, "grid size C=%d outside [2, %d] for k=%d (k*C <= %d)", C, kMaxLdsDoubles / k, k,
                kMaxLdsDoubles);
  if (B > kMaxBoxesK) return errf(err, OMB_EUNSUP, "box count B=%lld above %d", (long long)B, kMaxBoxesK);
  return OMB_OK;
}

int check_box_list(std::string* err, int k, int C, const uint16_t* boxes, int64_t B) {
  for (int64_t b = 0; b < B; ++b)
    for (int j = 0; j < k; ++j) {
      const int lo = boxes[2 * k * b + 2 * j], hi = boxes[2 * k * b + 2 * j + 1];
      if (hi >= C || lo >= hi)
        return errf(err, OMB_EINVAL, "box %lld, objective %d: grid indices [%d, %d) not increasing inside [0, %d)",
                    (long long)b, j, lo, hi, C);
    }
  return OMB_OK;
}

int check_ei(std::string* err, int kind, int k, double var_eps, double pof_eps) {
  const bool ok = (kind == OMB_EI_PLAIN && k == 1) || (kind == OMB_EI_PARETO && k == 2) ||
                  (kind == OMB_EI_CONSTRAINED && k >= 2 && k <= OMB_MAX_OBJ);
  if (!ok) return errf(err, OMB_EINVAL, "EI kind %d does not take k=%d posterior rows", kind, k);
  if (!(var_eps >= 0.0) || !(pof_eps >= 0.0)) return errf(err, OMB_EINVAL, "var_eps/pof_eps must be >= 0");
  return OMB_OK;
}

static bool finite_nonneg(double v) { return v >= 0.0 && v <= 1.79769313486231570815e308; }

static int check_paths_shape(std::string* err, int o, const PathsObjInfo& s) {
  if (s.n_var > kPathsMaxDim)
    return errf(err, OMB_EUNSUP, "objective %d: sample paths need n_var <= %d (n_var=%d)", o, kPathsMaxDim, s.n_var);
  if (s.n_train > OMB_MAX_TRAIN_DENSE)
    return errf(err, OMB_EUNSUP, "objective %d: n_train=%d above %d", o, s.n_train, OMB_MAX_TRAIN_DENSE);
  return OMB_OK;
}

int check_paths_set(std::string* err, int obj, int S, int m, const void* omega, const void* phase, const void* w,
                    double noise, const PathsObjInfo* info) {
  if (obj < 0 || obj >= OMB_MAX_OBJ) return errf(err, OMB_EINVAL, "obj=%d outside [0, %d)", obj, OMB_MAX_OBJ);
  if (S < 1 || S > kPathsMaxS) return errf(err, OMB_EINVAL, "S=%d paths outside [1, %d]", S, kPathsMaxS);
  if (m < 1 || m > kPathsMaxFeatures)
    return errf(err, OMB_EINVAL, "m=%d features outside [1, %d]", m, kPathsMaxFeatures);
  if (!omega || !phase || !w || !info) return errf(err, OMB_EINVAL, "null frequencies, phases or weights");
  if (!finite_nonneg(noise)) return errf(err, OMB_EINVAL, "noise=%g must be finite and >= 0", noise);
  if (!info->set) return errf(err, OMB_ESTATE, "objective %d has no GP state (call omb_set_gp)", obj);
  return check_paths_shape(err, obj, *info);
}

int check_paths_eval(std::string* err, int n_obj, const void* Xc, int64_t N, int64_t ld, const void* out,
                     const PathsObjInfo* info) {
  if (n_obj < 1 || n_obj > OMB_MAX_OBJ) return errf(err, OMB_EINVAL, "n_obj=%d outside [1, %d]", n_obj, OMB_MAX_OBJ);
  if (N < 0) return errf(err, OMB_EINVAL, "N=%lld < 0", (long long)N);
  if (ld < N) return errf(err, OMB_EINVAL, "ld=%lld < N=%lld", (long long)ld, (long long)N);
  if (!info || (N > 0 && (!Xc || !out))) return errf(err, OMB_EINVAL, "null candidate/output pointer");
  for (int o = 0; o < n_obj; ++o) {
    if (!info[o].set) return errf(err, OMB_ESTATE, "objective %d has no GP state (call omb_set_gp)", o);
    if (info[o].S < 1) return errf(err, OMB_ESTATE, "objective %d has no sample paths (call omb_paths_set)", o);
    if (info[o].S != info[0].S)
      return errf(err, OMB_ESTATE, "objectives 0 and %d hold %d and %d paths", o, info[0].S, info[o].S);
  }
  for (int o = 0; o < n_obj; ++o) {
    const int rc = check_paths_shape(err, o, info[o]);
    if (rc) return rc;
  }
  return OMB_OK;
}

int check_paths_grad(std::string* err, int n_obj, const void* Xc, int64_t N, int64_t ld, const void* out,
                     const void* grad, const PathsObjInfo* info) {
  // a null grad is refused where a null out is: the remaining refusals are check_paths_eval's own, in its order
  return check_paths_eval(err, n_obj, Xc, N, ld, (N > 0 && !grad) ? nullptr : out, info);
}

int check_paths_min(std::string* err, int n_obj, const void* Xc, int64_t N, const void* res, const PathsObjInfo* info) {
  if (n_obj < 1 || n_obj > OMB_MAX_OBJ) return errf(err, OMB_EINVAL, "n_obj=%d outside [1, %d]", n_obj, OMB_MAX_OBJ);
  if (N < 0) return errf(err, OMB_EINVAL, "N=%lld < 0", (long long)N);
  if (!res) return errf(err, OMB_EINVAL, "null result pointer");
  // N as the pitch: the remaining refusals are check_paths_eval's own, in its order
  return check_paths_eval(err, n_obj, Xc, N, N, res, info);
}

static int check_mes_shape(std::string* err, int k, int S) {
  if (k < 1 || k > OMB_MAX_OBJ) return errf(err, OMB_EINVAL, "k=%d outside [1, %d]", k, OMB_MAX_OBJ);
  if (S < 1 || S > kMesMaxS) return errf(err, OMB_EINVAL, "S=%d sampled minima outside [1, %d]", S, kMesMaxS);
  return OMB_OK;
}

int check_mes(std::string* err, int k, int S, const void* mu, const void* var, int64_t ld, int64_t N,
              const void* ystar, const void* out) {
  int rc = check_mes_shape(err, k, S);
  if (rc) return rc;
  if (N < 0) return errf(err, OMB_EINVAL, "N=%lld < 0", (long long)N);
  if (N > 0 && !ystar) return errf(err, OMB_EINVAL, "null device pointer");
  return check_moments(err, mu, var, ld, N, k, out);
}

int check_plan_mes(std::string* err, int k, int S, const double* ystar) {
  int rc = check_mes_shape(err, k, S);
  if (rc) return rc;
  if (!ystar) return errf(err, OMB_EINVAL, "null sampled minima");
  for (int i = 0; i < k * S; ++i)
    if (!(ystar[i] >= -1.79769313486231570815e308 && ystar[i] <= 1.79769313486231570815e308))
      return errf(err, OMB_EINVAL, "ystar[%d][%d]=%g is not finite", i / S, i % S, ystar[i]);
  return OMB_OK;
}

// check_hvi_paths' OMB_EINVAL refusals, then its OMB_EUNSUP ones (check_hvi_paths_grad puts its own between them)
static int check_hvi_paths_args(std::string* err, int k, int S, const void* y, int64_t ld, int64_t N,
                                const void* coords, const int32_t* box_off, const void* boxes, const void* out,
                                bool out_optional = false) {
  if (k < 1 || k > OMB_MAX_OBJ)
    return errf(err, OMB_EINVAL, "the sampled-front improvement needs 1 <= k <= %d objectives (k=%d)", OMB_MAX_OBJ, k);
  if (S < 1 || S > kPathsMaxS) return errf(err, OMB_EINVAL, "S=%d paths outside [1, %d]", S, kPathsMaxS);
  if (N < 0) return errf(err, OMB_EINVAL, "N=%lld < 0", (long long)N);
  if (!coords || !boxes || !box_off) return errf(err, OMB_EINVAL, "null grids, box lists or offsets");
  if (box_off[0] != 0) return errf(err, OMB_EINVAL, "box_off[0]=%d, not 0", box_off[0]);
  for (int s = 0; s < S; ++s)
    if (box_off[s + 1] <= box_off[s])
      return errf(err, OMB_EINVAL, "box_off[%d]=%d, box_off[%d]=%d: list %d is empty or the offsets decrease", s,
                  box_off[s], s + 1, box_off[s + 1], s);
  if (N > 0 && (!y || (!out && !out_optional))) return errf(err, OMB_EINVAL, "null device pointer");
  if (((uintptr_t)y | (uintptr_t)coords | (uintptr_t)out) & 7)
    return errf(err, OMB_EINVAL, "path values, grids or output not 8-byte aligned");
  if ((uintptr_t)boxes & 3) return errf(err, OMB_EINVAL, "box lists not 4-byte aligned");
  if (ld < N) return errf(err, OMB_EINVAL, "ld=%lld < N=%lld", (long long)ld, (long long)N);
  return OMB_OK;
}

static int check_hvi_paths_limits(std::string* err, int k, int S, int C, const int32_t* box_off) {
  // one path's grid is staged in the 64 KiB of dynamic LDS; the box lists are streamed
  if (C < 2 || (int64_t)k * C > kMaxLdsDoubles)
    return errf(err, OMB_EUNSUP, "grid size C=%d outside [2, %d] for k=%d (k*C <= %d)", C, kMaxLdsDoubles / k, k,
                kMaxLdsDoubles);
  if (box_off[S] > kMaxBoxesK)
    return errf(err, OMB_EUNSUP, "box count box_off[%d]=%d above %d", S, box_off[S], kMaxBoxesK);
  return OMB_OK;
}

int check_hvi_paths(std::string* err, int k, int S, const void* y, int64_t ld, int64_t N, const void* coords, int C,
                    const int32_t* box_off, const void* boxes, const void* out) {
  const int rc = check_hvi_paths_args(err, k, S, y, ld, N, coords, box_off, boxes, out);
  return rc ? rc : check_hvi_paths_limits(err, k, S, C, box_off);
}

int check_hvi_paths_grad(std::string* err, int k, int S, int d, const void* y, const void* dy, int64_t ld, int64_t N,
                         const void* coords, int C, const int32_t* box_off, const void* boxes, const void* out,
                         const void* grad, const void* t, const void* tgrad) {
  const int rc = check_hvi_paths_args(err, k, S, y, ld, N, coords, box_off, boxes, out);
  if (rc) return rc;
  if (d < 1 || d > kPathsMaxDim) return errf(err, OMB_EINVAL, "d=%d outside [1, %d]", d, kPathsMaxDim);
  if (N > 0 && (!dy || !grad)) return errf(err, OMB_EINVAL, "null path gradients or gradient output");
  if ((t == nullptr) != (tgrad == nullptr))
    return errf(err, OMB_EINVAL, "the per-path outputs t and tgrad come together or not at all");
  if (((uintptr_t)dy | (uintptr_t)grad | (uintptr_t)t | (uintptr_t)tgrad) & 7)
    return errf(err, OMB_EINVAL, "path gradients or gradient outputs not 8-byte aligned");
  return check_hvi_paths_limits(err, k, S, C, box_off);
}

int check_hvi_paths_con(std::string* err, int k, int S, int n_con, const void* y, int64_t ld, int64_t N,
                        const void* coords, int C, const int32_t* box_off, const void* boxes, double eta,
                        unsigned flags, const void* out, const void* u) {
  int rc = check_hvi_paths_args(err, k, S, y, ld, N, coords, box_off, boxes, out, true);
  if (!rc) rc = check_hvi_paths_limits(err, k, S, C, box_off);
  if (rc) return rc;
  if (n_con < 0) return errf(err, OMB_EINVAL, "n_con=%d < 0", n_con);
  if (!(eta >= 0.0 && eta <= 1.79769313486231570815e308))
    return errf(err, OMB_EINVAL, "eta=%g is negative or not finite", eta);
  if (flags & ~(unsigned)OMB_CON_VIOLATION) return errf(err, OMB_EINVAL, "unknown flag bits 0x%x", flags);
  if ((flags & OMB_CON_VIOLATION) && eta > 0.0)
    return errf(err, OMB_EINVAL, "OMB_CON_VIOLATION needs eta = 0 (eta=%g)", eta);
  if (N > 0 && !out && !u) return errf(err, OMB_EINVAL, "null outputs: neither the mean nor the per-path values");
  if ((uintptr_t)u & 7) return errf(err, OMB_EINVAL, "per-path output not 8-byte aligned");
  if ((int64_t)k + n_con > OMB_MAX_OBJ)   // n_con up to INT_MAX: the sum in 64 bits
    return errf(err, OMB_EUNSUP, "k=%d objectives and n_con=%d constraints need %lld slots, above %d", k, n_con,
                (long long)k + n_con, OMB_MAX_OBJ);
  return OMB_OK;
}

int check_nondominated(std::string* err, int k, int S, const void* y, int64_t ld, int64_t N, const void* mask,
                       int64_t ldm, const void* count) {
  if (k < 1 || k > OMB_MAX_OBJ) return errf(err, OMB_EINVAL, "k=%d outside [1, %d]", k, OMB_MAX_OBJ);
  if (S < 1 || S > kNdMaxS) return errf(err, OMB_EINVAL, "S=%d outside [1, %d]", S, kNdMaxS);
  if (N < 0) return errf(err, OMB_EINVAL, "N=%lld < 0", (long long)N);
  if (ld < N || ldm < N)
    return errf(err, OMB_EINVAL, "ld=%lld or ldm=%lld < N=%lld", (long long)ld, (long long)ldm, (long long)N);
  if (!count) return errf(err, OMB_EINVAL, "null count pointer");
  if (N > 0 && (!y || !mask)) return errf(err, OMB_EINVAL, "null point or mask pointer");
  if (((uintptr_t)y & 7) || ((uintptr_t)count & 7)) return errf(err, OMB_EINVAL, "y or count not 8-byte aligned");
  if (N > kNdMaxN)
    return errf(err, OMB_EUNSUP, "N=%lld above %lld points per set", (long long)N, (long long)kNdMaxN);
  return OMB_OK;
}

int check_hypervolume(std::string* err, int k, int S, const void* y, int64_t ld, int64_t N, const void* mask,
                      int64_t ldm, const double* r, const void* hv, int contrib, const void* out) {
  (void)mask;   // bytes at any address, or null for every row
  if (k < 1 || k > OMB_MAX_OBJ) return errf(err, OMB_EINVAL, "k=%d outside [1, %d]", k, OMB_MAX_OBJ);
  if (S < 1 || S > kHvMaxS) return errf(err, OMB_EINVAL, "S=%d outside [1, %d]", S, kHvMaxS);
  if (N < 0) return errf(err, OMB_EINVAL, "N=%lld < 0", (long long)N);
  if (ld < N || ldm < N)
    return errf(err, OMB_EINVAL, "ld=%lld or ldm=%lld < N=%lld", (long long)ld, (long long)ldm, (long long)N);
  if (!r) return errf(err, OMB_EINVAL, "null reference point");
  for (int j = 0; j < k; ++j)
    if (!(r[j] >= -1.79769313486231570815e308 && r[j] <= 1.79769313486231570815e308)) return errf(err, OMB_EINVAL, "reference point coordinate %d is not finite", j);
  if (!hv || (contrib && !out)) return errf(err, OMB_EINVAL, "null output pointer");
  if (N > 0 && !y) return errf(err, OMB_EINVAL, "null point pointer");
  if (((uintptr_t)y & 7) || ((uintptr_t)hv & 7) || (contrib && ((uintptr_t)out & 7)))
    return errf(err, OMB_EINVAL, "y or an output not 8-byte aligned");
  if (N > kHvMaxN) return errf(err, OMB_EUNSUP, "N=%lld above %lld rows per set", (long long)N, (long long)kHvMaxN);
  return OMB_OK;
}

namespace {
int64_t sat_mul(int64_t a, int64_t b) {   // a, b ≥ 0
  int64_t p;
  return __builtin_mul_overflow(a, b, &p) ? INT64_MAX : p;
}
}  // namespace

int64_t hv_cells(int g, const int32_t* nj) {
  int64_t cells = 1;
  for (int j = 0; j < g; ++j) {
    if (nj[j] < 1) return 0;
    cells = sat_mul(cells, nj[j]);
  }
  return cells;
}

int check_hv_work(std::string* err, int k, int S, const int32_t* hdr, int per_point, int64_t* max_cells) {
  const int g = k > 2 ? k - 2 : 0;
  int64_t work = 0;
  *max_cells = 0;
  for (int s = 0; s < S; ++s) {
    const int32_t* h = hdr + (size_t)s * kHvHdr;
    const int64_t n = h[0];
    if (n > kHvPoints)
      return errf(err, OMB_EUNSUP, "set %d keeps more than %d rows below the reference point", s, kHvPoints);
    if (n < 0) return errf(err, OMB_EHIP, "set %d: kept count %lld", s, (long long)n);
    if (n == 0) continue;
    for (int j = 0; j < g; ++j)
      if (h[1 + j] < 1 || h[1 + j] > n)
        return errf(err, OMB_EHIP, "set %d: grid %d has %d values for %lld rows", s, j, h[1 + j], (long long)n);
    const int64_t cells = hv_cells(g, h + 1);
    const int64_t w = sat_mul(sat_mul(cells, n), per_point ? n + 1 : 1);
    work = w > INT64_MAX - work ? INT64_MAX : work + w;
    if (cells > *max_cells) *max_cells = cells;
  }
  if (work > OMB_HV_MAX_WORK)
    return errf(err, OMB_EUNSUP, "%lld point tests above %lld (cells x kept rows x variants)", (long long)work,
                (long long)OMB_HV_MAX_WORK);
  return OMB_OK;
}

int check_box_lists(std::string* err, int k, int S, int C, const int32_t* box_off, const uint16_t* boxes) {
  for (int s = 0; s < S; ++s) {
    std::string one;
    const int rc = check_box_list(err ? &one : nullptr, k, C, boxes + 2 * (size_t)k * (size_t)box_off[s],
                                  (int64_t)box_off[s + 1] - box_off[s]);
    if (rc) return errf(err, rc, "list %d, %s", s, one.c_str());
  }
  return OMB_OK;
}

void paths_pack(int m, int d, int DP, int S, const double* omega, const double* phase, const double* w, double scale,
                double* Of, double* Wf) {
  const int ksf = paths_ksf(DP);
  const int64_t MT = (m + 15) / 16;
  for (int64_t T = 0; T < MT; ++T) {
    for (int s = 0; s < ksf; ++s)
      for (int l = 0; l < 64; ++l) {
        const int64_t i = 16 * T + (l & 15);
        const int j = 4 * s + (l >> 4);
        double v = 0.0;
        if (i < m) v = j < d ? omega[i * d + j] : (j == d ? phase[i] : 0.0);
        Of[(T * ksf + s) * 64 + l] = v;
      }
    for (int e = 0; e < 4; ++e)
      for (int l = 0; l < 64; ++l) {
        const int64_t i = 16 * T + 4 * e + (l >> 4);
        const int p = l & 15;
        Wf[(4 * T + e) * 64 + l] = (i < m && p < S) ? scale * w[i * S + p] : 0.0;
      }
  }
}

int check_constraints(std::string* err, int plan_k, int n_con, double pof_eps) {
  if (plan_k < 1) return errf(err, OMB_ESTATE, "no acquisition plan to constrain (call an omb_plan_* function first)");
  if (n_con < 0) return errf(err, OMB_EINVAL, "n_con=%d < 0", n_con);
  if (!finite_nonneg(pof_eps)) return errf(err, OMB_EINVAL, "pof_eps=%g must be finite and >= 0", pof_eps);
  if ((int64_t)plan_k + n_con > OMB_MAX_OBJ)
    return errf(err, OMB_EUNSUP, "%d objectives + %d constraints above the context's %d models", plan_k, n_con,
                OMB_MAX_OBJ);
  return OMB_OK;
}

int check_plan_log(std::string* err, int has_plan, int on, const char* refused) {
  if (!has_plan) return errf(err, OMB_ESTATE, "no acquisition plan to take the log of (call an omb_plan_* function first)");
  if (on != 0 && on != 1) return errf(err, OMB_EINVAL, "on=%d outside {0, 1}", on);
  if (refused) return errf(err, OMB_EUNSUP, "the %s plan has no log form", refused);
  return OMB_OK;
}

int check_log_ei(std::string* err, int kind, int k, double var_eps, double pof_eps) {
  int rc = check_ei(err, kind, k, var_eps, pof_eps);
  if (rc) return rc;
  if (kind == OMB_EI_PARETO) return errf(err, OMB_EUNSUP, "Pareto EI (mu_1 * EI) has no log form");
  return OMB_OK;
}

int check_feasibility(std::string* err, int c, const void* mu, const void* var, int64_t ld, int64_t N, double pof_eps,
                      const void* out) {
  if (c < 1 || c > OMB_MAX_OBJ) return errf(err, OMB_EINVAL, "c=%d outside [1, %d]", c, OMB_MAX_OBJ);
  if (!finite_nonneg(pof_eps)) return errf(err, OMB_EINVAL, "pof_eps=%g must be finite and >= 0", pof_eps);
  return check_moments(err, mu, var, ld, N, c, out);
}

int check_hvpoi(std::string* err, int C) {
  if (C < 1 || 4 * (int64_t)C > kMaxLdsDoubles)
    return errf(err, OMB_EUNSUP, "cell count C=%d outside [1, %d]", C, kMaxLdsDoubles / 4);
  return OMB_OK;
}

int check_posterior_grad(std::string* err, int n_obj, const void* Xc, int64_t N, const void* mu, const void* var,
                         const void* dmu, const void* dvar) {
  if (n_obj < 1 || n_obj > OMB_MAX_OBJ) return errf(err, OMB_EINVAL, "n_obj=%d outside [1, %d]", n_obj, OMB_MAX_OBJ);
  if (N < 0) return errf(err, OMB_EINVAL, "N=%lld < 0", (long long)N);
  if (N > 0 && !Xc) return errf(err, OMB_EINVAL, "null candidate pointer");
  if (N > 0 && (!mu || !var)) return errf(err, OMB_EINVAL, "null moment output (mu_dev / var_dev may not be NULL)");
  if (N > 0 && (!dmu || !dvar)) return errf(err, OMB_EINVAL, "null gradient output");
  return OMB_OK;
}

int check_eval_grad(std::string* err, const void* Xc, int64_t N, const void* vals, const void* grad) {
  if (N < 0) return errf(err, OMB_EINVAL, "N=%lld < 0", (long long)N);
  if (N > 0 && !Xc) return errf(err, OMB_EINVAL, "null candidate pointer");
  if (N > 0 && (!vals || !grad)) return errf(err, OMB_EINVAL, "null output");
  return OMB_OK;
}

int64_t grad_chunk(int n_obj, int n_train, int64_t N) {
  if (N <= 0 || n_obj < 1 || n_obj > OMB_MAX_OBJ || n_train < 1 || n_train > OMB_MAX_TRAIN_DENSE) return 0;
  const int64_t per = (int64_t)(n_obj + 2) * n_train * (int64_t)sizeof(double);
  int64_t nc = ((int64_t)512 << 20) / per;
  nc = nc < 64 ? 64 : (nc > (1 << 20) ? (1 << 20) : nc);
  return nc < N ? nc : N;
}

int build_scal(std::string* err, int k, int M, int scal_id, const double* params_host, const double* weights_host,
               const double* ideal_host, const double* max_host, double agg_min, ScalParams* out) {
  if (k < 1 || k > OMB_MAX_OBJ) return errf(err, OMB_EINVAL, "k=%d outside [1, %d]", k, OMB_MAX_OBJ);
  if (M < 1 || (int64_t)k * M > kMaxLdsDoubles)
    return errf(err, OMB_EUNSUP, "cache size M=%d x k=%d exceeds %d doubles of LDS", M, k, kMaxLdsDoubles);
  if (scal_id < OMB_SCAL_WS || scal_id > OMB_SCAL_APD) return errf(err, OMB_EINVAL, "unknown scalarisation %d", scal_id);
  if (!weights_host || !ideal_host || !max_host) return errf(err, OMB_EINVAL, "null weights/ideal/max");
  ScalParams& sp = *out;
  memset(&sp, 0, sizeof(sp));
  sp.id = scal_id;
  sp.k = k;
  sp.agg_min = agg_min;
  double wq = 0.0, rsum = 0.0;
  for (int i = 0; i < k; ++i) {
    sp.w[i] = weights_host[i];
    sp.ideal[i] = ideal_host[i];
    sp.range[i] = max_host[i] - ideal_host[i];
    wq += sp.w[i] * sp.w[i];
    rsum += sp.range[i];
  }
  sp.wnorm = sqrt(wq);
  const int np = (scal_id == OMB_SCAL_QPBI || scal_id == OMB_SCAL_APD) ? 3
                 : (scal_id == OMB_SCAL_WS || scal_id == OMB_SCAL_TCH || scal_id == OMB_SCAL_WPR) ? 0 : 1;
  if (np > 0 && !params_host) return errf(err, OMB_EINVAL, "scalarisation %d needs %d parameter(s)", scal_id, np);
  for (int i = 0; i < np; ++i) sp.p[i] = params_host[i];
  if (scal_id == OMB_SCAL_APD && sp.wnorm == 0.0) {
    // scalarisations.py:392-393 substitutes 1e-5 weights (the reference then fails for k > 1).
    for (int i = 0; i < k; ++i) sp.w[i] = 1e-5;
    sp.wnorm = sqrt(k * 1e-10);
  }
  if (scal_id == OMB_SCAL_QPBI) {
    // scalarisations.py:347: alpha * (1/H * 1/k * Σ(max − ideal))
    sp.d_star = sp.p[1] * ((1.0 / sp.p[2]) * (1.0 / (double)k) * rsum);
  }
  return OMB_OK;
}

int check_gp_args(std::string* err, int obj, int kernel, int n, int d, const void* X_dev, const double* lengthscale_host,
                  double variance, const void* alpha_dev, const void* Linv_dev) {
  if (obj < 0 || obj >= OMB_MAX_OBJ) return errf(err, OMB_EINVAL, "obj=%d outside [0, %d)", obj, OMB_MAX_OBJ);
  if (kernel != OMB_KERNEL_MATERN52 && kernel != OMB_KERNEL_RBF) return errf(err, OMB_EINVAL, "unknown kernel %d", kernel);
  if (n < 1 || n > OMB_MAX_TRAIN_DENSE)
    return errf(err, OMB_EUNSUP, "n_train=%d outside [1, %d]", n, OMB_MAX_TRAIN_DENSE);
  if (d < 1 || d > OMB_MAX_DIM) return errf(err, OMB_EUNSUP, "n_var=%d outside [1, %d]", d, OMB_MAX_DIM);
  if (!X_dev || !lengthscale_host || !alpha_dev || !Linv_dev) return errf(err, OMB_EINVAL, "null pointer");
  for (int j = 0; j < d; ++j)
    if (!(lengthscale_host[j] > 0.0))
      return errf(err, OMB_EINVAL, "lengthscale[%d]=%g must be > 0", j, lengthscale_host[j]);
  if (!(variance >= 0.0)) return errf(err, OMB_EINVAL, "variance=%g must be >= 0", variance);
  return OMB_OK;
}

int check_sobol_args(std::string* err, int d, int bits, const void* sv_host, const void* shift_host,
                     const double* lo_host, const double* hi_host) {
  if (d < 1 || d > OMB_MAX_DIM) return errf(err, OMB_EUNSUP, "Sobol dimension %d outside [1, %d]", d, OMB_MAX_DIM);
  if (bits < 1 || bits > 32) return errf(err, OMB_EUNSUP, "Sobol bits=%d outside [1, 32]", bits);
  if (!sv_host || !shift_host || !lo_host || !hi_host) return errf(err, OMB_EINVAL, "null Sobol state");
  for (int j = 0; j < d; ++j)
    if (!(hi_host[j] >= lo_host[j]))
      return errf(err, OMB_EINVAL, "box [%g, %g] of dimension %d is empty", lo_host[j], hi_host[j], j);
  return OMB_OK;
}

size_t sobol_state_bytes(int d, int bits) {
  const int words = d * bits + d;
  return (size_t)((words + 1) & ~1) * 4 + (size_t)2 * d * sizeof(double);
}

void sobol_pack_state(int d, int bits, const uint32_t* sv, const uint32_t* shift, const double* lo, const double* hi,
                      void* dst) {
  uint32_t* w = static_cast<uint32_t*>(dst);
  const int words = d * bits + d;
  for (int t = 0; t < d * bits; ++t) w[t] = sv[t];
  for (int t = 0; t < d; ++t) w[d * bits + t] = shift[t];
  if (words & 1) w[words] = 0;
  double* f = reinterpret_cast<double*>(w + ((words + 1) & ~1));
  for (int t = 0; t < d; ++t) {
    f[t] = lo[t];
    f[d + t] = hi[t] - lo[t];   // numpy's (hi - lo), rounded once
  }
}

}  // namespace omb
