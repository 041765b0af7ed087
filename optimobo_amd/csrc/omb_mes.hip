// Max-value entropy search on gfx950: omb_mes / omb_plan_mes.
//
// MES (Wang & Jegelka 2017) and its multi-objective form MESMO (Belakaria et al. 2019) score a candidate by the
// information it gives about the minimum of each objective.  With y*_js the minimum of objective j under posterior
// sample path s (omb_paths_min), σ_j = sqrt(σ²_j) and γ_js = (μ_j − y*_js)/σ_j (everything is minimised):
//   α(x) = Σ_j [ (Σ_s a(γ_js)) / S ],   a(γ) = γφ(γ)/(2Φ(γ)) − log Φ(γ)   (≥ 0, decreasing in γ)
//   ∂α/∂μ_j = (1/S) Σ_s a'(γ_js)/σ_j,   ∂α/∂σ²_j = (1/S) Σ_s a'(γ_js)·(−γ_js)/(2σ²_j).
// a and a' come from omb_math.h's mes_term (tail ratios below 0: finite and accurate where Φ underflows), unfused,
// and both sums run in index order, so a value does not depend on which kernel or chain computed it, on N or on the
// candidate's column.
//
// Edge rules: σ²_j ≤ 0 or a NaN moment gives NaN for that candidate only; a NaN y* gives NaN; NaN never wins the
// arg-max (omb_argmax.hip's rule, unchanged).
#include <math.h>

#include "omb_internal.h"
#include "omb_math.h"

namespace omb {

constexpr int kMesThreads = 256;

static unsigned mes_grid(int64_t N) {
  int64_t b = (N + kMesThreads - 1) / kMesThreads;
  if (b > 65536) b = 65536;
  return (unsigned)(b < 1 ? 1 : b);
}

// One lane per candidate; y* (k·S ≤ kMesMaxObjSamples doubles) staged in LDS, objectives and samples in index order.
__global__ __launch_bounds__(kMesThreads) void mes_kernel(const double* __restrict__ mu, const double* __restrict__ var,
                                                          int64_t ld, int64_t N, int k, int S,
                                                          const double* __restrict__ ystar, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double ys[OMB_MAX_OBJ * kMesMaxS];
  for (int i = threadIdx.x; i < k * S; i += kMesThreads) ys[i] = ystar[i];
  __syncthreads();
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < N; c += (int64_t)gridDim.x * blockDim.x) {
    double alpha = 0.0;
    for (int j = 0; j < k; ++j) {
      const double m = mu[j * ld + c], v = var[j * ld + c];
      const double sd = v > 0.0 ? sqrt(v) : __builtin_nan("");
      double sj = 0.0;
      for (int s = 0; s < S; ++s) sj = sj + mes_term((m - ys[j * S + s]) / sd).a;
      alpha = alpha + sj / (double)S;
    }
    out[c] = alpha;
  }
}

hipError_t launch_mes(hipStream_t stream, int k, const double* mu, const double* var, int64_t ld, int64_t N,
                      const double* ystar, int S, double* out) {
  if (k < 1 || k > OMB_MAX_OBJ || S < 1 || S > kMesMaxS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mes_kernel, dim3(mes_grid(N)), dim3(kMesThreads), 0, stream, mu, var, ld, N, k, S, ystar, out);
  return hipGetLastError();
}

// ∂α/∂μ_j, ∂α/∂σ²_j into rows j of dadm / dadv (pitch N): the layout of launch_acq_grad's other kernels.
__global__ __launch_bounds__(kMesThreads) void mes_grad_kernel(const double* __restrict__ mu,
                                                               const double* __restrict__ var, int64_t ld, int64_t N,
                                                               int k, int S, const double* __restrict__ ystar,
                                                               double* __restrict__ dadm, double* __restrict__ dadv) {
#pragma clang fp contract(off)
  __shared__ double ys[OMB_MAX_OBJ * kMesMaxS];
  for (int i = threadIdx.x; i < k * S; i += kMesThreads) ys[i] = ystar[i];
  __syncthreads();
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < N; c += (int64_t)gridDim.x * blockDim.x) {
    for (int j = 0; j < k; ++j) {
      const double m = mu[j * ld + c], v = var[j * ld + c];
      const double sd = v > 0.0 ? sqrt(v) : __builtin_nan("");
      double sm = 0.0, sv = 0.0;
      for (int s = 0; s < S; ++s) {
        const double g = (m - ys[j * S + s]) / sd;
        const double da = mes_term(g).da;
        sm = sm + da;
        sv = sv + da * (-g);
      }
      dadm[j * N + c] = (sm / (double)S) / sd;
      dadv[j * N + c] = (sv / (double)S) / (2.0 * (sd * sd));
    }
  }
}

hipError_t launch_mes_grad(hipStream_t stream, int k, const double* mu, const double* var, int64_t ld, int64_t N,
                           const double* ystar, int S, double* dadm, double* dadv) {
  if (k < 1 || k > OMB_MAX_OBJ || S < 1 || S > kMesMaxS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mes_grad_kernel, dim3(mes_grid(N)), dim3(kMesThreads), 0, stream, mu, var, ld, N, k, S, ystar,
                     dadm, dadv);
  return hipGetLastError();
}

}  // namespace omb
