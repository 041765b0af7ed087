// Conditioning an installed GP state on one more observation without a refit (omb_gp_append): the bordered
// update of the dense L⁻¹ and of α.  With k = K(X, x), μ = kᵀα, v = L⁻¹k, δ² = σ_f² + σ_n² + 1e-8 − vᵀv,
// w = L⁻ᵀv and ζ = (y − μ)/δ, the state of n + 1 points is
//     L⁻¹' = [[L⁻¹, 0], [−wᵀ/δ, 1/δ]],   α' = [α − w·ζ/δ ; ζ/δ],   X' = [X ; x].
// Two dependent mat-vecs over the lower triangle of L⁻¹ per point, O(n²) against the O(n³) of a refit.
//
// The kernels work on a bordered copy in the workspace (AppendWs: L of pitch m = n + q, zeros above the diagonal);
// omb_gp_append installs it through omb_set_gp's packing once every point is in.  Per point c (the current size):
//   append_k_kernel      k_i and the per-256-row partial sums of k·α            (one thread per row)
//   append_v_kernel      v_i = Σ_{j ≤ i} L⁻¹_ij k_j                              (one wave per row, lanes on columns)
//   append_scal_kernel   μ, vᵀv, δ², ζ/δ; the status word                        (one workgroup)
//   append_w_kernel      partial sums of w_j = Σ_{i ≥ j} L⁻¹_ij v_i per 256 rows (lanes on consecutive columns:
//                        every row segment is one coalesced read)
//   append_finish_kernel w from its partials; row c of L⁻¹, α' and α'_c
// Every sum has one order fixed by c alone (strided per-lane sums, xor butterflies, LDS trees, ascending partials;
// no atomics), so the update is bitwise repeatable and q points in one call equal q calls of one point.
// No loop below stores to global memory, so no load waits behind a store (DESIGN §4's vmcnt note).
#include "omb_internal.h"
#include "omb_math.h"

namespace omb {

namespace {

constexpr int kAppThreads = 256;
constexpr int kAppChunk = 256;   // rows per partial sum (k·α and w)

// Sum over the workgroup's 256 values in a fixed tree; every thread returns the total.
__device__ __forceinline__ double block_sum256(double x, double* red) {
  red[threadIdx.x] = x;
  __syncthreads();
#pragma unroll
  for (int off = kAppThreads / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  const double s = red[0];
  __syncthreads();
  return s;
}

// Lnew (m, m) = the lower triangle of Ld (n, n) in the top-left corner, zeros elsewhere.
__global__ __launch_bounds__(kAppThreads) void append_restride_kernel(int n, int m, const double* __restrict__ Ld,
                                                                      double* __restrict__ Lnew) {
  const int i = blockIdx.y;
  const int j = blockIdx.x * kAppThreads + threadIdx.x;
  if (j >= m) return;
  Lnew[(int64_t)i * m + j] = (i < n && j <= i) ? Ld[(int64_t)i * n + j] : 0.0;
}

// k_i = k(X_i, x) for i < c, x = row c of Xs: GPy's scaled distance r² = ‖a‖² + ‖b‖² − 2a·b on the ℓ-scaled rows
// (clipped at 0) and kernel_of_r2, the transform of the library's K(X, X) builder.  mupart[b] = Σ k_i α_i over the
// workgroup's rows.
template <int KIND>
__global__ __launch_bounds__(kAppThreads) void append_k_kernel(int c, int d, int DP, const double* __restrict__ Xs,
                                                               const double* __restrict__ xsq,
                                                               const double* __restrict__ alpha, double variance,
                                                               double* __restrict__ kvec, double* __restrict__ mupart,
                                                               const int* __restrict__ info) {
  __shared__ double xn[OMB_MAX_DIM];
  __shared__ double red[kAppThreads];
  if (*info != 0) return;
  for (int j = threadIdx.x; j < d; j += kAppThreads) xn[j] = Xs[(int64_t)c * DP + j];
  __syncthreads();
  const int i = blockIdx.x * kAppThreads + threadIdx.x;
  double p = 0.0;
  if (i < c) {
    const double* xi = Xs + (int64_t)i * DP;
    double dot = 0.0;
    for (int j = 0; j < d; ++j) dot = fma(xi[j], xn[j], dot);
    const double r2 = fma(-2.0, dot, xsq[i] + xsq[c]);
    const double kv = kernel_of_r2<KIND>(r2, variance);
    kvec[i] = kv;
    p = kv * alpha[i];
  }
  const double s = block_sum256(p, red);
  if (threadIdx.x == 0) mupart[blockIdx.x] = s;
}

// v_i = Σ_{j ≤ i} L_ij k_j: one wave per row, lane l takes columns l, l + 64, ... (two running sums), then a
// xor butterfly.  Only columns ≤ row are read.
__global__ __launch_bounds__(kAppThreads) void append_v_kernel(int c, int ldl, const double* __restrict__ L,
                                                               const double* __restrict__ kvec, double* __restrict__ v,
                                                               const int* __restrict__ info) {
  if (*info != 0) return;
  const int row = blockIdx.x * (kAppThreads / 64) + (threadIdx.x >> 6);
  if (row >= c) return;
  const int lane = threadIdx.x & 63;
  const double* Lr = L + (int64_t)row * ldl;
  double a0 = 0.0, a1 = 0.0;
  int col = lane;
  for (; col + 64 <= row; col += 128) {
    a0 = fma(Lr[col], kvec[col], a0);
    a1 = fma(Lr[col + 64], kvec[col + 64], a1);
  }
  if (col <= row) a0 = fma(Lr[col], kvec[col], a0);
  double a = a0 + a1;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);
  if (lane == 0) v[row] = a;
}

// scal = {δ, ζ/δ}; mu_out[j] = μ, var_out[j] = δ².  A δ² that is not positive and finite marks info with the
// 1-based index of the point (the kernels of this and every later point then return at once).
__global__ __launch_bounds__(kAppThreads) void append_scal_kernel(int c, int j, int nparts,
                                                                  const double* __restrict__ mupart,
                                                                  const double* __restrict__ v, double variance,
                                                                  double noise, const double* __restrict__ ynew,
                                                                  double* __restrict__ scal, double* __restrict__ mu_out,
                                                                  double* __restrict__ var_out, int* __restrict__ info) {
  __shared__ double red[kAppThreads];
  if (*info != 0) return;
  double s = 0.0;
  for (int i = threadIdx.x; i < c; i += kAppThreads) s = fma(v[i], v[i], s);
  const double vv = block_sum256(s, red);
  if (threadIdx.x != 0) return;
  double mu = 0.0;
  for (int b = 0; b < nparts; ++b) mu += mupart[b];
  const double d2 = ((variance + noise) + 1e-8) - vv;
  if (mu_out) mu_out[j] = mu;
  if (var_out) var_out[j] = d2;
  if (!(d2 > 0.0) || !isfinite(d2) || !isfinite(mu)) {
    *info = j + 1;
    return;
  }
  const double delta = sqrt(d2);
  const double y = ynew ? ynew[j] : mu;
  scal[0] = delta;
  scal[1] = ((y - mu) / delta) / delta;
}

// wpart[by][col] = Σ L_i,col v_i over the rows i ≥ col of chunk by (256 rows; wave w its rows 64w .. 64w + 63 in
// ascending order, then the four waves in order).  Workgroup (bx, by): columns 64bx .. 64bx + 63; chunks that lie
// wholly above the diagonal (by < bx/4) hold nothing and are never read.
__global__ __launch_bounds__(kAppThreads) void append_w_kernel(int c, int ldl, const double* __restrict__ L,
                                                               const double* __restrict__ v, double* __restrict__ wpart,
                                                               int ldw, const int* __restrict__ info) {
  __shared__ double red[kAppThreads];
  if (*info != 0) return;
  const int bx = blockIdx.x, by = blockIdx.y;
  if (by < bx / 4) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = 64 * bx + lane;
  const int r0 = kAppChunk * by + 64 * wave;
  const int r1 = min(r0 + 64, c);
  double acc = 0.0;
  if (col < c) {
#pragma unroll 8
    for (int i = r0; i < r1; ++i) {
      const double l = (i >= col) ? L[(int64_t)i * ldl + col] : 0.0;   // above the diagonal: not read
      acc = fma(l, v[i], acc);
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (wave == 0 && col < c)
    wpart[(int64_t)by * ldw + col] = ((red[lane] + red[64 + lane]) + red[128 + lane]) + red[192 + lane];
}

// w_j from its partials (ascending chunks); row c of L = [−w/δ, 1/δ], α_j −= w_j·ζ/δ, α_c = ζ/δ.  With the
// believer's ζ = 0 the old α entries keep their bits and the new one is exactly 0.
__global__ __launch_bounds__(kAppThreads) void append_finish_kernel(int c, int ldl, int nchunks,
                                                                    const double* __restrict__ wpart, int ldw,
                                                                    const double* __restrict__ scal,
                                                                    double* __restrict__ L, double* __restrict__ alpha,
                                                                    const int* __restrict__ info) {
  if (*info != 0) return;
  const int j = blockIdx.x * kAppThreads + threadIdx.x;
  if (j > c) return;
  const double delta = scal[0], zd = scal[1];
  double* Lc = L + (int64_t)c * ldl;
  if (j == c) {
    Lc[c] = 1.0 / delta;
    alpha[c] = zd;
    return;
  }
  double w = 0.0;
  for (int by = j / kAppChunk; by < nchunks; ++by) w += wpart[(int64_t)by * ldw + j];
  Lc[j] = -w / delta;
  alpha[j] = fma(-w, zd, alpha[j]);
}

}  // namespace

int64_t append_ws_doubles(int m, int d, int DP) {
  const int64_t chunks = (m + kAppChunk - 1) / kAppChunk;
  // L | α | Xs | xsq | X | k | v | w partials | μ partials | scal (2) + info | pack scratch (m + DP)
  return (int64_t)m * m + m + (int64_t)m * DP + m + (int64_t)m * d + 2 * (int64_t)m + chunks * m + chunks + 4 +
         m + DP;
}

void append_ws_carve(double* base, int m, int d, int DP, AppendWs* ws) {
  const int64_t chunks = (m + kAppChunk - 1) / kAppChunk;
  double* p = base;
  ws->L = p; p += (int64_t)m * m;
  ws->alpha = p; p += m;
  ws->Xs = p; p += (int64_t)m * DP;
  ws->xsq = p; p += m;
  ws->X = p; p += (int64_t)m * d;
  ws->kvec = p; p += m;
  ws->v = p; p += m;
  ws->wpart = p; p += chunks * m;
  ws->mupart = p; p += chunks;
  ws->scal = p; p += 2;
  ws->info = reinterpret_cast<int*>(p); p += 2;
  ws->scratch = p;
  ws->m = m;
  ws->d = d;
  ws->DP = DP;
}

// Both launches below put one matrix row on gridDim.y, which ends at 65535.
static_assert(OMB_MAX_TRAIN_DENSE <= 65535, "append_restride_kernel: one grid row per matrix row");

hipError_t launch_append_restride(hipStream_t stream, const AppendWs& ws, int n, const double* Ld) {
  const int m = ws.m;
  hipLaunchKernelGGL(append_restride_kernel, dim3((m + kAppThreads - 1) / kAppThreads, m), dim3(kAppThreads), 0,
                     stream, n, m, Ld, ws.L);
  return hipGetLastError();
}

hipError_t launch_copy_lower(hipStream_t stream, int n, const double* Linv, double* Ld) {
  hipLaunchKernelGGL(append_restride_kernel, dim3((n + kAppThreads - 1) / kAppThreads, n), dim3(kAppThreads), 0,
                     stream, n, n, Linv, Ld);
  return hipGetLastError();
}

hipError_t launch_append_point(hipStream_t stream, const AppendWs& ws, int kind, double variance, int c, int j,
                               const double* ynew, double noise, double* mu_out, double* var_out) {
  const int m = ws.m;
  const int parts = (c + kAppThreads - 1) / kAppThreads;
  if (kind == OMB_KERNEL_RBF)
    hipLaunchKernelGGL(append_k_kernel<OMB_KERNEL_RBF>, dim3(parts), dim3(kAppThreads), 0, stream, c, ws.d, ws.DP,
                       ws.Xs, ws.xsq, ws.alpha, variance, ws.kvec, ws.mupart, ws.info);
  else
    hipLaunchKernelGGL(append_k_kernel<OMB_KERNEL_MATERN52>, dim3(parts), dim3(kAppThreads), 0, stream, c, ws.d,
                       ws.DP, ws.Xs, ws.xsq, ws.alpha, variance, ws.kvec, ws.mupart, ws.info);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(append_v_kernel, dim3((c + 3) / 4), dim3(kAppThreads), 0, stream, c, m, ws.L, ws.kvec, ws.v,
                     ws.info);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(append_scal_kernel, dim3(1), dim3(kAppThreads), 0, stream, c, j, parts, ws.mupart, ws.v,
                     variance, noise, ynew, ws.scal, mu_out, var_out, ws.info);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const int chunks = (c + kAppChunk - 1) / kAppChunk;
  hipLaunchKernelGGL(append_w_kernel, dim3((c + 63) / 64, chunks), dim3(kAppThreads), 0, stream, c, m, ws.L, ws.v,
                     ws.wpart, m, ws.info);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(append_finish_kernel, dim3((c + 1 + kAppThreads - 1) / kAppThreads), dim3(kAppThreads), 0,
                     stream, c, m, chunks, ws.wpart, m, ws.scal, ws.L, ws.alpha, ws.info);
  return hipGetLastError();
}

}  // namespace omb
