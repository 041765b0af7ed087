// Log-space acquisitions on gfx950: log EI, log probability of feasibility, log of the exact EHVI
// over boxes, and the analytic partials of the first two.
//
// The linear kernels of omb_acquisition.hip return exactly 0.0 where the improvement lies more than ~38 σ away
// (Φ and φ underflow), which is most of a late-run search box: the arg-max then has nothing to compare and the
// gradients are 0.  The logarithms are finite there and keep their slope (Ament et al. 2023, "Unexpected
// improvements to expected improvement").  Everything below is written on omb_math.h's log_h / log_ndtr / log1mexp,
// unfused, so a value does not depend on which kernel or chain computed it.
//
// Edge rules:
//   * a NaN moment gives NaN for that candidate only;
//   * log EI at σ = 0 is −inf, the log of the linear kernel's 0; σ² + var_eps < 0 is NaN, as there;
//   * the box kernel gives NaN for σ²_j ≤ 0 (the linear kernel: NaN below 0; at exactly 0 the log form would be
//     −inf + inf — callers take the log of omb_hvi_boxes, the σ → 0 limit);
//   * −inf and NaN never win the arg-max (omb_argmax.hip's rule, unchanged).
#include <math.h>

#include "omb_internal.h"
#include "omb_math.h"

namespace omb {

constexpr int kLogThreads = 256;

static unsigned log_grid(int64_t N) {
  int64_t b = (N + kLogThreads - 1) / kLogThreads;
  if (b > 65536) b = 65536;
  return (unsigned)(b < 1 ? 1 : b);
}

// ------------------------------------------------------------------------------ log EI
// σ and γ exactly as ei_kernel forms them (σ = sqrt(σ² + var_eps), γ = (best − μ)/(σ + 1e-10));
//   MODE 0  log σ + log h(γ)
//   MODE 2  … + ((0 + log Φ(z_1)) + log Φ(z_2)) + …,  z_c = (0 − μ_c)/sqrt(σ²_c + pof_eps): ei_kernel<2>'s z, and the
//           sum log_pof_kernel forms, so the constrained kind is bitwise log_pof_kernel over MODE 0.
// (μ₁·EI of OMB_EI_PARETO has no logarithm where μ₁ ≤ 0: refused at the API.)  One thread per candidate.
template <int MODE>
__global__ __launch_bounds__(kLogThreads) void log_ei_kernel(const double* __restrict__ mu,
                                                             const double* __restrict__ var, int64_t ld, int64_t N,
                                                             int k, double best, double var_eps, double pof_eps,
                                                             double* __restrict__ out) {
#pragma clang fp contract(off)
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < N; c += (int64_t)gridDim.x * blockDim.x) {
    const double sigma = sqrt(var[c] + var_eps);
    const double gamma = (best - mu[c]) / (sigma + 1e-10);
    double v = log(sigma) + log_h(gamma);
    if (MODE == 2) {
      double lf = 0.0;
      for (int j = 1; j < k; ++j) lf += log_ndtr((0.0 - mu[j * ld + c]) / sqrt(var[j * ld + c] + pof_eps));
      v = v + lf;
    }
    out[c] = v;
  }
}

hipError_t launch_log_ei(hipStream_t stream, int kind, int k, const double* mu, const double* var, int64_t ld,
                         int64_t N, double best, double var_eps, double pof_eps, double* out) {
  const dim3 grid(log_grid(N)), block(kLogThreads);
  if (kind == OMB_EI_CONSTRAINED)
    hipLaunchKernelGGL(log_ei_kernel<2>, grid, block, 0, stream, mu, var, ld, N, k, best, var_eps, pof_eps, out);
  else if (kind == OMB_EI_PLAIN)
    hipLaunchKernelGGL(log_ei_kernel<0>, grid, block, 0, stream, mu, var, ld, N, k, best, var_eps, pof_eps, out);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

// ------------------------------------------------------------------------------ log probability of feasibility
// out = (acq ? acq[i] : 0) + log F,  log F = ((0 + log Φ(z_0)) + log Φ(z_1)) + …, z_j and the order over j those of
// pof_scale_kernel.  out may be acq (neither is __restrict__).
__global__ __launch_bounds__(kLogThreads) void log_pof_kernel(const double* __restrict__ mu,
                                                              const double* __restrict__ var, int64_t ld, int64_t N,
                                                              int c, double pof_eps, const double* acq, double* out) {
#pragma clang fp contract(off)
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    double lf = 0.0;
    for (int j = 0; j < c; ++j) lf += log_ndtr((0.0 - mu[j * ld + i]) / sqrt(var[j * ld + i] + pof_eps));
    out[i] = (acq ? acq[i] : 0.0) + lf;
  }
}

hipError_t launch_log_pof(hipStream_t stream, int c, const double* mu, const double* var, int64_t ld, int64_t N,
                          double pof_eps, const double* acq, double* out) {
  hipLaunchKernelGGL(log_pof_kernel, dim3(log_grid(N)), dim3(kLogThreads), 0, stream, mu, var, ld, N, c, pof_eps, acq,
                     out);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------ log exact EHVI over boxes
// EHVI = Σ_b Π_j σ_j (h(β_bj) − h(α_bj)), α, β = (lo, hi − μ_j)/σ_j (ehvi_boxes_kd_kernel's product, rewritten on
// h(t) = tΦ(t) + φ(t): G(l, u) = σ(h(β) − h(α))).  In log space, with lh = log h at a grid coordinate,
//   L_b = Σ_j [lh_hi + log1mexp(lh_lo − lh_hi)],   out = Σ_j log σ_j + logsumexp_b L_b
// (log σ_j is the same in every box and is added once, after the sum).  A lower index at the −∞ column has
// lh_lo = −inf: log1mexp(−inf) = 0 and the objective contributes lh_hi alone.
//
// The candidate-blocked shape of ehvi_boxes_kd_kernel: one workgroup owns CT candidates;
//   1. all threads tabulate lh at the K·C grid coordinates for each of the CT candidates — one double per entry in
//      place of that kernel's (Φ, φ) pair;
//   2. thread t takes boxes t, t + 256, …: the box's K index words once from global memory, then for each of the CT
//      candidates two table reads, one exp and one log per objective; each candidate's boxes enter an online pair
//      (m, s), Σ e^L = s·e^m (LogSum);
//   3. the pairs meet in a fixed order: xor shuffles in the wave, then the four waves' pairs from LDS in wave order.
//      `combine` is symmetric in its arguments — max(a.m, b.m), then a.s·e^(a.m−M) + b.s·e^(b.m−M), unfused, and an
//      addition commutes — so both sides of a shuffle hold the same bits.  No atomics.
// A candidate's value depends on (K, C, B, the box list) alone: not on N, its column, CT or the launch grid.  This one
// kernel serves omb_plan_ehvi_boxes and omb_plan_ehvi_boxes_k (and omb_log_ehvi_boxes): the k-D bound
// 3·K·C + 2·K + 4 ≤ 8192 admits every grid the k ≤ 3 entry admits, and with it CT = 1 always fits.
// LDS doubles: CT·K·C (tables) + K·C (grid) + 2·CT·K (μ, σ) + 8·CT (reduction) + CT (Σ log σ).
// The work per box and candidate is 2K transcendental calls against the linear kernel's 5K flops (timings: DESIGN
// §22); K·CT bodies of it are unrolled, so CT shrinks as K grows (log_boxes_max_ct).
struct LogSum {
  double m, s;
};

__device__ __forceinline__ LogSum logsum_add(LogSum a, double L) {
#pragma clang fp contract(off)
  // one exp either way: e = e^−|L − m|.  L = −inf adds nothing (and −inf − −inf never forms); a NaN L makes s NaN.
  const double e = (L == -HUGE_VAL) ? 0.0 : exp(-fabs(L - a.m));
  if (L > a.m) {
    a.s = a.s * e + 1.0;
    a.m = L;
  } else {
    a.s = a.s + e;
  }
  return a;
}

__device__ __forceinline__ LogSum logsum_combine(LogSum a, LogSum b) {
#pragma clang fp contract(off)
  const double M = a.m > b.m ? a.m : b.m;
  const double ea = a.m == M ? 1.0 : exp(a.m - M);   // the equal case first: M may be −inf (no finite box yet)
  const double eb = b.m == M ? 1.0 : exp(b.m - M);
  return LogSum{M, a.s * ea + b.s * eb};
}

constexpr int kLogBoxThreads = 256;

template <int K, int CT>
__global__ __launch_bounds__(kLogBoxThreads, 2) void log_ehvi_boxes_kernel(const double* __restrict__ mu,
                                                                         const double* __restrict__ var, int64_t ld,
                                                                         int64_t N, const double* __restrict__ coords,
                                                                         int C, const uint32_t* __restrict__ boxes,
                                                                         int B, double* __restrict__ out) {
#pragma clang fp contract(off)
  extern __shared__ double lsm[];
  const int KC = K * C;
  double* tab = lsm;                  // CT × K·C: log h at every grid coordinate
  double* grid = tab + CT * KC;       // K·C coordinates (−inf stays −inf: t = −inf, lh = −inf)
  double* ms = grid + KC;             // CT × K × (μ, σ)
  double* red = ms + 2 * CT * K;      // waves × CT × (m, s)
  double* slog = red + 2 * (kLogBoxThreads / 64) * CT;   // CT: Σ_j log σ_j
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < KC; i += kLogBoxThreads) grid[i] = coords[i];
  for (int64_t base = (int64_t)blockIdx.x * CT; base < N; base += (int64_t)gridDim.x * CT) {
    __syncthreads();                  // grid staged; the previous block's reads done
    if (tid < CT * K) {
      const int c = tid / K, j = tid - c * K;
      const int64_t cc = base + c < N ? base + c : N - 1;   // the tail block computes its last candidate again
      const double v = var[j * ld + cc];
      ms[2 * tid] = mu[j * ld + cc];
      ms[2 * tid + 1] = v > 0.0 ? sqrt(v) : __builtin_nan("");
    }
    __syncthreads();
    if (tid < CT) {
      double a = 0.0;
      for (int j = 0; j < K; ++j) a += log(ms[2 * (tid * K + j) + 1]);
      slog[tid] = a;
    }
    for (int i = tid; i < CT * KC; i += kLogBoxThreads) {
      const int c = i / KC, r = i - c * KC;
      const double* m = ms + 2 * (c * K + r / C);
      tab[i] = log_h((grid[r] - m[0]) / m[1]);
    }
    __syncthreads();
    LogSum acc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[c] = LogSum{-HUGE_VAL, 0.0};
    for (int b = tid; b < B; b += kLogBoxThreads) {
      int il[K], ih[K];
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const uint32_t w = boxes[(size_t)b * K + j];         // lo | hi << 16
        il[j] = j * C + (int)(w & 0xffffu);
        ih[j] = j * C + (int)(w >> 16);
      }
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        const double* t = tab + c * KC;
        double L = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j) {
          const double hi = t[ih[j]];
          double d = t[il[j]] - hi;
          d = d > 0.0 ? 0.0 : d;      // lh rises with the coordinate; a rounding inversion is an empty cell (NaN stays)
          L += hi + log1mexp(d);
        }
        acc[c] = logsum_add(acc[c], L);
      }
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      LogSum v = acc[c];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v = logsum_combine(v, LogSum{__shfl_xor(v.m, off), __shfl_xor(v.s, off)});
      if (lane == 0) {
        red[2 * (wave * CT + c)] = v.m;
        red[2 * (wave * CT + c) + 1] = v.s;
      }
    }
    __syncthreads();
    if (tid < CT && base + tid < N) {
      LogSum v{red[2 * tid], red[2 * tid + 1]};
      for (int w = 1; w < kLogBoxThreads / 64; ++w)
        v = logsum_combine(v, LogSum{red[2 * (w * CT + tid)], red[2 * (w * CT + tid) + 1]});
      out[base + tid] = slog[tid] + (v.m + log(v.s));
    }
  }
}

static size_t log_boxes_lds(int k, int C, int ct) {
  return sizeof(double) * ((size_t)(ct + 1) * k * C + (size_t)2 * ct * k + (size_t)(2 * (kLogBoxThreads / 64) + 1) * ct);
}

// candidates per workgroup: K·CT unrolled bodies of (exp, log) stay at 16, and the tables within 64 KiB
constexpr int log_boxes_max_ct(int k) { return k <= 2 ? 8 : (k <= 4 ? 4 : 2); }

static int log_boxes_ct(int k, int C) {
  for (int ct = log_boxes_max_ct(k); ct >= 1; ct >>= 1)
    if (log_boxes_lds(k, C, ct) <= 64 * 1024) return ct;
  return 0;
}

template <int K>
static void launch_log_boxes_k(int ct, dim3 g, size_t shm, hipStream_t stream, const double* mu, const double* var,
                               int64_t ld, int64_t N, const double* coords, int C, const uint32_t* boxes, int B,
                               double* out) {
  const dim3 b(kLogBoxThreads);
  if constexpr (log_boxes_max_ct(K) >= 8)
    if (ct == 8) {
      hipLaunchKernelGGL((log_ehvi_boxes_kernel<K, 8>), g, b, shm, stream, mu, var, ld, N, coords, C, boxes, B, out);
      return;
    }
  if constexpr (log_boxes_max_ct(K) >= 4)
    if (ct == 4) {
      hipLaunchKernelGGL((log_ehvi_boxes_kernel<K, 4>), g, b, shm, stream, mu, var, ld, N, coords, C, boxes, B, out);
      return;
    }
  if (ct == 2) {
    hipLaunchKernelGGL((log_ehvi_boxes_kernel<K, 2>), g, b, shm, stream, mu, var, ld, N, coords, C, boxes, B, out);
    return;
  }
  hipLaunchKernelGGL((log_ehvi_boxes_kernel<K, 1>), g, b, shm, stream, mu, var, ld, N, coords, C, boxes, B, out);
}

hipError_t launch_log_ehvi_boxes(hipStream_t stream, int k, const double* mu, const double* var, int64_t ld, int64_t N,
                                 const double* coords, int C, const uint16_t* boxes, int B, double* out) {
  const int ct = log_boxes_ct(k, C);
  if (ct == 0 || (reinterpret_cast<uintptr_t>(boxes) & 3)) return hipErrorInvalidValue;
  const size_t shm = log_boxes_lds(k, C, ct);
  const int64_t nb = (N + ct - 1) / ct;
  const dim3 g((unsigned)(nb > 65536 ? 65536 : (nb < 1 ? 1 : nb)));
  const uint32_t* bw = reinterpret_cast<const uint32_t*>(boxes);
  switch (k) {
#define OMB_LB(KV) \
  case KV: launch_log_boxes_k<KV>(ct, g, shm, stream, mu, var, ld, N, coords, C, bw, B, out); break;
    OMB_LB(2) OMB_LB(3) OMB_LB(4) OMB_LB(5) OMB_LB(6) OMB_LB(7) OMB_LB(8)
#undef OMB_LB
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// ------------------------------------------------------------------------------ gradients of log EI and log F
// log EI = log σ + log h(γ), h' = Φ, σ = sqrt(σ² + ε), γ = (best − μ)/(σ + 1e-10).  With ρ = Φ(γ)/h(γ):
//   ∂/∂μ = −ρ/(σ + 1e-10),   ∂/∂σ² = (1/σ − ρ·γ/(σ + 1e-10))/(2σ).
// ρ = R/T (tail_ratios) for γ < 0 and the direct quotient for γ ≥ 0 — never exp(log Φ − log h), whose error grows
// with γ².  A constraint row adds log Φ(z), z = −μ/s, s = sqrt(σ² + pof_eps):
//   ∂/∂μ = q·(−1/s),  ∂/∂σ² = q·μ/(2s³),  q = φ(z)/Φ(z) = 1/R(z) for z < 0
// (pof_grad_kernel's ∂z/∂μ and ∂z/∂σ²).  Finite where the linear gradients are 0 (γ < −38).
__device__ __forceinline__ double phi_over_h(double g) {
#pragma clang fp contract(off)
  if (g < 0.0) {
    const TailRatios r = tail_ratios(g);
    return r.R / r.T;
  }
  const double P = ndtr(g);
  return P / (g * P + npdf(g));
}

__device__ __forceinline__ double pdf_over_cdf(double z) {
#pragma clang fp contract(off)
  if (z < 0.0) return 1.0 / tail_ratios(z).R;
  return npdf(z) / ndtr(z);
}

// rows j0..j1-1 of (mu, var) (pitch ld) are constraint rows: their partials of log Φ(z_j) go to rows row0 + (j − j0)
__device__ __forceinline__ void log_pof_partials(const double* __restrict__ mu, const double* __restrict__ var,
                                                 int64_t ld, int64_t N, int64_t i, int j0, int j1, int row0,
                                                 double pof_eps, double* __restrict__ dadm,
                                                 double* __restrict__ dadv) {
#pragma clang fp contract(off)
  for (int j = j0; j < j1; ++j) {
    const double mj = mu[j * ld + i], sj = sqrt(var[j * ld + i] + pof_eps);
    const double q = pdf_over_cdf((0.0 - mj) / sj);
    dadm[(row0 + j - j0) * N + i] = q * (-1.0 / sj);
    dadv[(row0 + j - j0) * N + i] = q * (mj / (2.0 * sj * sj * sj));
  }
}

template <int MODE>
__global__ __launch_bounds__(kLogThreads) void log_ei_grad_kernel(const double* __restrict__ mu,
                                                                  const double* __restrict__ var, int64_t ld,
                                                                  int64_t N, int k, double best, double var_eps,
                                                                  double pof_eps, double* __restrict__ dadm,
                                                                  double* __restrict__ dadv) {
#pragma clang fp contract(off)
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < N; c += (int64_t)gridDim.x * blockDim.x) {
    const double sigma = sqrt(var[c] + var_eps);
    const double s1 = sigma + 1e-10;
    const double gamma = (best - mu[c]) / s1;
    const double rho = phi_over_h(gamma);
    dadm[c] = -rho / s1;
    dadv[c] = (1.0 / sigma - rho * gamma / s1) / (2.0 * sigma);
    if (MODE == 2) log_pof_partials(mu, var, ld, N, c, 1, k, 1, pof_eps, dadm, dadv);
  }
}

hipError_t launch_log_ei_grad(hipStream_t stream, int kind, int k, const double* mu, const double* var, int64_t ld,
                              int64_t N, double best, double var_eps, double pof_eps, double* dadm, double* dadv) {
  const dim3 grid(log_grid(N)), block(kLogThreads);
  if (kind == OMB_EI_CONSTRAINED)
    hipLaunchKernelGGL(log_ei_grad_kernel<2>, grid, block, 0, stream, mu, var, ld, N, k, best, var_eps, pof_eps, dadm,
                       dadv);
  else if (kind == OMB_EI_PLAIN)
    hipLaunchKernelGGL(log_ei_grad_kernel<0>, grid, block, 0, stream, mu, var, ld, N, k, best, var_eps, pof_eps, dadm,
                       dadv);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

// omb_plan_constraints on a log plan: rows k..k+c-1 of dadm / dadv (mu / var point at constraint row 0)
__global__ __launch_bounds__(kLogThreads) void log_pof_grad_kernel(const double* __restrict__ mu,
                                                                   const double* __restrict__ var, int64_t ld,
                                                                   int64_t N, int k, int c, double pof_eps,
                                                                   double* __restrict__ dadm,
                                                                   double* __restrict__ dadv) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x)
    log_pof_partials(mu, var, ld, N, i, 0, c, k, pof_eps, dadm, dadv);
}

hipError_t launch_log_pof_grad(hipStream_t stream, const double* mu, const double* var, int64_t ld, int64_t N, int k,
                               int c, double pof_eps, double* dadm, double* dadv) {
  hipLaunchKernelGGL(log_pof_grad_kernel, dim3(log_grid(N)), dim3(kLogThreads), 0, stream, mu, var, ld, N, k, c,
                     pof_eps, dadm, dadv);
  return hipGetLastError();
}

}  // namespace omb
