// Hypervolume improvement of points over a box decomposition (omb_hvi_boxes): the σ → 0 limit of the exact EHVI,
//   HVI(y) = Σ_b Π_j (hi_bj − max(y_j, lo_bj))⁺,
// over the boxes omb_ehvi_boxes_k takes (grid (k, C) with a leading −∞ column, uint16 index pairs).  No Φ, no φ and
// no division: a box costs a point 4 VALU operations per objective, so nothing is tabulated per point.
//
//   * One lane per point; its K coordinates stay in registers (K a template parameter).
//   * LDS holds the K·C grid doubles alone, staged once per workgroup.  The box index is wave-uniform: the box's K
//     32-bit index words come through the scalar cache, and the 2K grid reads go to addresses every lane shares, which
//     the LDS broadcasts (one pass per 32-lane half, no conflicts).  Grid indices are clamped to the grid, so a bad
//     list reads a wrong coordinate, never past the staged doubles.
//   * Every lane walks the boxes in list order, in slices of kHviSlice boxes: a slice's terms are summed from 0 in
//     list order, and the slices' sums are added in slice order.  The slice boundaries depend on B alone.  A large
//     batch walks all slices in one launch; a small one (too few workgroups to fill the chip) gives every slice a
//     workgroup row of its own (blockIdx.y), which stores the slice's sum to a workspace, and hvi_finish_kernel adds
//     them in slice order.  Both forms perform the same additions in the same order: a point's value depends on its
//     coordinates, the grid and the box list, not on N, its column, the launch shape or which form ran.  No atomics.
//   * A NaN coordinate makes the point's value NaN (fmax would drop it); y_j ≥ r_j zeroes every box's factor j, as
//     every hi_bj ≤ r_j, so the value is exactly 0.
#include "omb_internal.h"

namespace omb {

constexpr int kHviThreads = 256;
constexpr int kHviSlice = 1024;           // boxes per slice
constexpr int64_t kHviSplitBlocks = 512;  // fewer point workgroups than this (2 per CU): one workgroup row per slice
constexpr int64_t kHviSplitWs = 1 << 23;  // workspace doubles the split form may ask for (64 MiB)

// one slice's sum for the point y: boxes [b0, b1) in list order
template <int K>
__device__ __forceinline__ double hvi_slice(const double (&y)[K], const double* grid, int C,
                                            const uint32_t* __restrict__ boxes, int b0, int b1) {
#pragma clang fp contract(off)   // the one fused operation is the explicit fma below, in both forms of the kernel
  double p = 0.0;
  for (int b = b0; b < b1; ++b) {
    double t[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const uint32_t w = boxes[(size_t)b * K + j];   // lo | hi << 16, wave-uniform
      const int il = min((int)(w & 0xffffu), C - 1), ih = min((int)(w >> 16), C - 1);
      const double lo = grid[j * C + il], hi = grid[j * C + ih];
      t[j] = fmax(hi - fmax(y[j], lo), 0.0);
    }
    double prod = t[0];
#pragma unroll
    for (int j = 1; j < K - 1; ++j) prod *= t[j];
    p = fma(prod, t[K - 1], p);
  }
  return p;
}

// SPLIT: blockIdx.y is the slice, out is the workspace (slices, N).  Otherwise out (N) takes the values.
template <int K, bool SPLIT>
__global__ __launch_bounds__(kHviThreads) void hvi_boxes_kernel(const double* __restrict__ y, int64_t ld, int64_t N,
                                                                const double* __restrict__ coords, int C,
                                                                const uint32_t* __restrict__ boxes, int B,
                                                                double* __restrict__ out) {
  extern __shared__ double hvi_grid[];
  for (int i = threadIdx.x; i < K * C; i += kHviThreads) hvi_grid[i] = coords[i];
  __syncthreads();
  const int S = (B + kHviSlice - 1) / kHviSlice;
  for (int64_t i = (int64_t)blockIdx.x * kHviThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kHviThreads) {
    double yv[K];
    bool nan = false;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      yv[j] = y[j * ld + i];
      nan |= yv[j] != yv[j];
    }
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    if constexpr (SPLIT) {
      const int s = blockIdx.y;
      const double p = hvi_slice<K>(yv, hvi_grid, C, boxes, s * kHviSlice, min(B, (s + 1) * kHviSlice));
      out[(int64_t)s * N + i] = nan ? qnan : p;
    } else {
      double total = 0.0;
      for (int s = 0; s < S; ++s) {
        const double p = hvi_slice<K>(yv, hvi_grid, C, boxes, s * kHviSlice, min(B, (s + 1) * kHviSlice));
        total += nan ? qnan : p;
      }
      out[i] = total;
    }
  }
}

// out[i] = Σ_s part[s][i] in slice order, from 0: the additions of the unsplit kernel
__global__ __launch_bounds__(kHviThreads) void hvi_finish_kernel(const double* __restrict__ part, int S, int64_t N,
                                                                 double* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * kHviThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kHviThreads) {
    double total = 0.0;
    for (int s = 0; s < S; ++s) total += part[(int64_t)s * N + i];
    out[i] = total;
  }
}

int64_t hvi_ws_doubles(int64_t N, int B) {
  const int64_t S = ((int64_t)B + kHviSlice - 1) / kHviSlice;
  const int64_t nb = (N + kHviThreads - 1) / kHviThreads;
  if (S < 2 || N < 1 || nb >= kHviSplitBlocks || S * N > kHviSplitWs) return 0;
  return S * N;
}

hipError_t launch_hvi_boxes(hipStream_t stream, int k, const double* y, int64_t ld, int64_t N, const double* coords,
                            int C, const uint16_t* boxes, int B, double* out, double* ws) {
  if (N < 1 || B < 1 || (int64_t)k * C > kMaxLdsDoubles || (reinterpret_cast<uintptr_t>(boxes) & 3))
    return hipErrorInvalidValue;
  const bool split = ws != nullptr && hvi_ws_doubles(N, B) > 0;
  const int S = (B + kHviSlice - 1) / kHviSlice;
  const size_t shm = sizeof(double) * (size_t)k * C;
  const int64_t nb = (N + kHviThreads - 1) / kHviThreads;
  const dim3 g((unsigned)(nb > (1 << 20) ? (1 << 20) : nb), split ? (unsigned)S : 1u), b(kHviThreads);
  const uint32_t* bw = reinterpret_cast<const uint32_t*>(boxes);
  switch (k) {
#define OMB_HVI(KV)                                                                                               \
  case KV:                                                                                                        \
    if (split) hipLaunchKernelGGL((hvi_boxes_kernel<KV, true>), g, b, shm, stream, y, ld, N, coords, C, bw, B, ws); \
    else hipLaunchKernelGGL((hvi_boxes_kernel<KV, false>), g, b, shm, stream, y, ld, N, coords, C, bw, B, out);    \
    break;
    OMB_HVI(2) OMB_HVI(3) OMB_HVI(4) OMB_HVI(5) OMB_HVI(6) OMB_HVI(7) OMB_HVI(8)
#undef OMB_HVI
    default: return hipErrorInvalidValue;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !split) return e;
  hipLaunchKernelGGL(hvi_finish_kernel, dim3(g.x), b, 0, stream, ws, S, N, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// The mean hypervolume improvement over S sampled fronts (omb_hvi_paths): candidate i holds one value per posterior
// sample path and objective (row j·S + s of y, omb_paths_eval's layout), path s has a box list and a grid of its own,
//   out[i] = ((…((0 + t_0) + t_1) + …) + t_{S−1}) / S,   t_s = hvi_boxes_kernel's value of list s on rows {j·S + s}.
//   * One lane per candidate, as above.  LDS holds the current path's K·C grid doubles, re-staged per path between two
//     barriers (a grid is a few hundred doubles; the S grids together would cost occupancy for nothing, and every
//     workgroup reads each grid once).  The lists' offsets are a kernel argument: list s is rows off[s]..off[s+1] of
//     the concatenated list, its index words wave-uniform as above.
//   * t_s is hvi_slice's sum over slices of kHviSlice boxes counted from the list's own start, added in slice order
//     from 0 — the additions of hvi_boxes_kernel, so t_s is bitwise omb_hvi_boxes' value.  K = 1 (noisy EI: list s is
//     the box (−∞, b_s]) has a single factor per box, which hvi_slice's product would square: hvi_slice1 adds it.
//   * A small batch (too few workgroups to fill the chip) gives every path a workgroup row of its own (blockIdx.y),
//     which stores t_s to a workspace, and hvi_paths_finish_kernel adds them in path order and divides.  Both forms
//     perform the same operations in the same order.  No atomics.
//   * A NaN coordinate of any path makes the candidate's value NaN.
struct HviPathOff {
  int32_t off[kPathsMaxS + 1];
};

// hvi_slice for one objective: the box's single factor, added in list order
__device__ __forceinline__ double hvi_slice1(double y, const double* grid, int C, const uint32_t* __restrict__ boxes,
                                             int b0, int b1) {
#pragma clang fp contract(off)
  double p = 0.0;
  for (int b = b0; b < b1; ++b) {
    const uint32_t w = boxes[b];   // lo | hi << 16, wave-uniform
    const int il = min((int)(w & 0xffffu), C - 1), ih = min((int)(w >> 16), C - 1);
    p = p + fmax(grid[ih] - fmax(y, grid[il]), 0.0);
  }
  return p;
}

// SPLIT: blockIdx.y is the path, out is the workspace (S, N) of the t_s.  Otherwise out (N) takes the means.
template <int K, bool SPLIT>
__global__ __launch_bounds__(kHviThreads) void hvi_paths_kernel(const double* __restrict__ y, int64_t ld, int64_t N,
                                                                int S, const double* __restrict__ coords, int C,
                                                                const uint32_t* __restrict__ boxes, HviPathOff po,
                                                                double* __restrict__ out) {
#pragma clang fp contract(off)
  extern __shared__ double hvi_paths_grid[];
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const int s0 = SPLIT ? (int)blockIdx.y : 0, s1 = SPLIT ? s0 + 1 : S;
  // the tile loop is uniform over the workgroup: every lane reaches the barriers
  for (int64_t base = (int64_t)blockIdx.x * kHviThreads; base < N; base += (int64_t)gridDim.x * kHviThreads) {
    const int64_t i = base + threadIdx.x;
    double total = 0.0;
    for (int s = s0; s < s1; ++s) {
      __syncthreads();   // the previous path's grid is read to the end
      const double* g = coords + (size_t)s * K * C;
      for (int t = threadIdx.x; t < K * C; t += kHviThreads) hvi_paths_grid[t] = g[t];
      __syncthreads();
      if (i < N) {
        double yv[K];
        bool nan = false;
#pragma unroll
        for (int j = 0; j < K; ++j) {
          yv[j] = y[((int64_t)j * S + s) * ld + i];
          nan |= yv[j] != yv[j];
        }
        const int B = po.off[s + 1] - po.off[s];
        const uint32_t* bl = boxes + (size_t)po.off[s] * K;
        const int slices = (B + kHviSlice - 1) / kHviSlice;
        double ts = 0.0;
        for (int c = 0; c < slices; ++c) {
          double p;
          if constexpr (K == 1) p = hvi_slice1(yv[0], hvi_paths_grid, C, bl, c * kHviSlice, min(B, (c + 1) * kHviSlice));
          else p = hvi_slice<K>(yv, hvi_paths_grid, C, bl, c * kHviSlice, min(B, (c + 1) * kHviSlice));
          ts += nan ? qnan : p;
        }
        if constexpr (SPLIT) out[(int64_t)s * N + i] = ts;
        else total += ts;
      }
    }
    if constexpr (!SPLIT)
      if (i < N) out[i] = total / (double)S;
  }
}

// out[i] = (Σ_s part[s][i] in path order, from 0) / S: the operations of the unsplit kernel
__global__ __launch_bounds__(kHviThreads) void hvi_paths_finish_kernel(const double* __restrict__ part, int S,
                                                                       int64_t N, double* __restrict__ out) {
#pragma clang fp contract(off)
  for (int64_t i = (int64_t)blockIdx.x * kHviThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kHviThreads) {
    double total = 0.0;
    for (int s = 0; s < S; ++s) total += part[(int64_t)s * N + i];
    out[i] = total / (double)S;
  }
}

int64_t hvi_paths_ws_doubles(int64_t N, int S) {
  const int64_t nb = (N + kHviThreads - 1) / kHviThreads;
  if (S < 2 || N < 1 || nb >= kHviSplitBlocks) return 0;
  return (int64_t)S * N;
}

hipError_t launch_hvi_paths(hipStream_t stream, int k, int S, const double* y, int64_t ld, int64_t N,
                            const double* coords, int C, const uint16_t* boxes, const int32_t* box_off, double* out,
                            double* ws) {
  if (N < 1 || S < 1 || S > kPathsMaxS || C < 2 || (int64_t)k * C > kMaxLdsDoubles ||
      (reinterpret_cast<uintptr_t>(boxes) & 3))
    return hipErrorInvalidValue;
  HviPathOff po;
  for (int s = 0; s <= kPathsMaxS; ++s) po.off[s] = box_off[s < S ? s : S];
  const bool split = ws != nullptr && hvi_paths_ws_doubles(N, S) > 0;
  const size_t shm = sizeof(double) * (size_t)k * C;
  const int64_t nb = (N + kHviThreads - 1) / kHviThreads;
  const dim3 g((unsigned)(nb > (1 << 20) ? (1 << 20) : nb), split ? (unsigned)S : 1u), b(kHviThreads);
  const uint32_t* bw = reinterpret_cast<const uint32_t*>(boxes);
  switch (k) {
#define OMB_HVIP(KV)                                                                                          \
  case KV:                                                                                                    \
    if (split)                                                                                                \
      hipLaunchKernelGGL((hvi_paths_kernel<KV, true>), g, b, shm, stream, y, ld, N, S, coords, C, bw, po, ws); \
    else                                                                                                      \
      hipLaunchKernelGGL((hvi_paths_kernel<KV, false>), g, b, shm, stream, y, ld, N, S, coords, C, bw, po, out); \
    break;
    OMB_HVIP(1) OMB_HVIP(2) OMB_HVIP(3) OMB_HVIP(4) OMB_HVIP(5) OMB_HVIP(6) OMB_HVIP(7) OMB_HVIP(8)
#undef OMB_HVIP
    default: return hipErrorInvalidValue;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !split) return e;
  hipLaunchKernelGGL(hvi_paths_finish_kernel, dim3(g.x), b, 0, stream, ws, S, N, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// omb_hvi_paths_con: omb_hvi_paths with constraints through sample paths.  Rows (K + j)·S + s of y hold
// path s of constraint j (g ≤ 0 feasible), n_con of them behind the K objectives:
//   ω(g)   = 1[g ≤ 0] (eta = 0), or the sigmoid 1/(1 + e^{g/η}) written without overflow on either side (eta > 0)
//   w_s    = ((1·ω(g_0s))·ω(g_1s))·…,  u_s = t_s·w_s, exactly 0.0 where w_s == 0.0,  out = ((0 + u_0) + … + u_{S−1}) / S
// and with OMB_CON_VIOLATION (eta = 0) u_s = −((0 + max(g_0s, 0)) + max(g_1s, 0) + …) where w_s == 0.
//   * hvi_paths_kernel's lane, staging, barriers and two launch forms; t_s is its t_s (hvi_slice / hvi_slice1 over the
//     same slices), so at n_con = 0 every bit is omb_hvi_paths'.
//   * The lane forms w_s before the box loop (a running product and a running sum: no per-constraint registers, so
//     n_con stays a runtime value).  A wavefront none of whose lanes needs t_s (w_s == 0, a NaN, or past N) skips
//     the box loop on a ballot; the skipped u_s is the defined value, so the skip changes no bit.  The barriers stand
//     outside the skipped region.
//   * A NaN among the K + n_con values of path s makes u_s, and so out, NaN.
//   * u (S, ld), when given, takes every u_s; out may then be null.
//   * SOFT is eta > 0: the indicator's instantiations carry no exponential and keep hvi_paths_kernel's occupancy.
template <int K, bool SPLIT, bool SOFT>
__global__ __launch_bounds__(kHviThreads) void hvi_paths_con_kernel(const double* __restrict__ y, int64_t ld, int64_t N,
                                                                    int S, int n_con, const double* __restrict__ coords,
                                                                    int C, const uint32_t* __restrict__ boxes,
                                                                    HviPathOff po, double eta, int violation,
                                                                    double* __restrict__ out, double* __restrict__ u) {
#pragma clang fp contract(off)
  extern __shared__ double hvi_paths_grid[];
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const int s0 = SPLIT ? (int)blockIdx.y : 0, s1 = SPLIT ? s0 + 1 : S;
  // the tile loop is uniform over the workgroup: every lane reaches the barriers
  for (int64_t base = (int64_t)blockIdx.x * kHviThreads; base < N; base += (int64_t)gridDim.x * kHviThreads) {
    const int64_t i = base + threadIdx.x;
    double total = 0.0;
    for (int s = s0; s < s1; ++s) {
      __syncthreads();   // the previous path's grid is read to the end
      const double* g = coords + (size_t)s * K * C;
      for (int t = threadIdx.x; t < K * C; t += kHviThreads) hvi_paths_grid[t] = g[t];
      __syncthreads();
      double w = 1.0, viol = 0.0;
      bool nan = false;
      if (i < N) {
        for (int j = 0; j < n_con; ++j) {
          const double gv = y[((int64_t)(K + j) * S + s) * ld + i];
          nan |= gv != gv;
          double om;
          if constexpr (SOFT) {
            if (gv <= 0.0) om = 1.0 / (1.0 + exp(gv / eta));
            else {
              const double e = exp(-gv / eta);
              om = e / (1.0 + e);
            }
          } else {
            om = gv <= 0.0 ? 1.0 : 0.0;
          }
          w = w * om;
          viol = viol + fmax(gv, 0.0);
        }
      }
      double yv[K];
      if (i < N) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
          yv[j] = y[((int64_t)j * S + s) * ld + i];
          nan |= yv[j] != yv[j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < K; ++j) yv[j] = 0.0;
      }
      const bool need = i < N && !nan && w != 0.0;
      double ts = 0.0;
      if (__ballot(need) != 0ull) {   // wave-uniform: a wavefront of infeasible candidates walks no box
        if (need) {
          const int B = po.off[s + 1] - po.off[s];
          const uint32_t* bl = boxes + (size_t)po.off[s] * K;
          const int slices = (B + kHviSlice - 1) / kHviSlice;
          for (int c = 0; c < slices; ++c) {
            double p;
            if constexpr (K == 1) p = hvi_slice1(yv[0], hvi_paths_grid, C, bl, c * kHviSlice, min(B, (c + 1) * kHviSlice));
            else p = hvi_slice<K>(yv, hvi_paths_grid, C, bl, c * kHviSlice, min(B, (c + 1) * kHviSlice));
            ts += p;
          }
        }
      }
      if (i < N) {
        double us;
        if (nan) us = 0.0 + qnan;
        else if (w == 0.0) us = violation ? -viol : 0.0;
        else us = ts * w;
        if (u) u[(int64_t)s * ld + i] = us;
        if constexpr (SPLIT) {
          if (out) out[(int64_t)s * N + i] = us;
        } else {
          total += us;
        }
      }
    }
    if constexpr (!SPLIT)
      if (i < N && out) out[i] = total / (double)S;
  }
}

hipError_t launch_hvi_paths_con(hipStream_t stream, int k, int S, int n_con, const double* y, int64_t ld, int64_t N,
                                const double* coords, int C, const uint16_t* boxes, const int32_t* box_off, double eta,
                                int violation, double* out, double* u, double* ws) {
  if (N < 1 || S < 1 || S > kPathsMaxS || C < 2 || (int64_t)k * C > kMaxLdsDoubles || n_con < 0 ||
      k + n_con > OMB_MAX_OBJ || (!out && !u) || ld < N || (reinterpret_cast<uintptr_t>(boxes) & 3))
    return hipErrorInvalidValue;
  HviPathOff po;
  for (int s = 0; s <= kPathsMaxS; ++s) po.off[s] = box_off[s < S ? s : S];
  const bool split = ws != nullptr && hvi_paths_ws_doubles(N, S) > 0;
  const size_t shm = sizeof(double) * (size_t)k * C;
  const int64_t nb = (N + kHviThreads - 1) / kHviThreads;
  const dim3 g((unsigned)(nb > (1 << 20) ? (1 << 20) : nb), split ? (unsigned)S : 1u), b(kHviThreads);
  const uint32_t* bw = reinterpret_cast<const uint32_t*>(boxes);
  double* part = out ? ws : nullptr;   // the split form's u_s for the finish launch: not wanted without out
  const bool soft = eta > 0.0;
  switch (k) {
#define OMB_HVIPC(KV)                                                                                              \
  case KV:                                                                                                         \
    if (split && soft)                                                                                             \
      hipLaunchKernelGGL((hvi_paths_con_kernel<KV, true, true>), g, b, shm, stream, y, ld, N, S, n_con, coords, C, \
                         bw, po, eta, violation, part, u);                                                         \
    else if (split)                                                                                                \
      hipLaunchKernelGGL((hvi_paths_con_kernel<KV, true, false>), g, b, shm, stream, y, ld, N, S, n_con, coords, C, \
                         bw, po, eta, violation, part, u);                                                         \
    else if (soft)                                                                                                 \
      hipLaunchKernelGGL((hvi_paths_con_kernel<KV, false, true>), g, b, shm, stream, y, ld, N, S, n_con, coords, C, \
                         bw, po, eta, violation, out, u);                                                          \
    else                                                                                                           \
      hipLaunchKernelGGL((hvi_paths_con_kernel<KV, false, false>), g, b, shm, stream, y, ld, N, S, n_con, coords,  \
                         C, bw, po, eta, violation, out, u);                                                       \
    break;
    OMB_HVIPC(1) OMB_HVIPC(2) OMB_HVIPC(3) OMB_HVIPC(4) OMB_HVIPC(5) OMB_HVIPC(6) OMB_HVIPC(7) OMB_HVIPC(8)
#undef OMB_HVIPC
    default: return hipErrorInvalidValue;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !split || !out) return e;
  hipLaunchKernelGGL(hvi_paths_finish_kernel, dim3(g.x), b, 0, stream, ws, S, N, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// omb_hvi_paths_grad: omb_hvi_paths' value and its gradient through the paths.  Two launches, no atomics:
//   1. hvi_paths_dy_kernel, one workgroup row per path (blockIdx.y) and one lane per candidate, walks list s as
//      hvi_paths_kernel does and leaves t_s (its operations, so bitwise its value) and
//          ∂t_s/∂y_j = −Σ_b 1[lo_bj < y_j < hi_bj] Π_{l≠j} (hi_bl − max(y_l, lo_bl))⁺
//      in a workspace, (S, K + 1, N): the slices of kHviSlice boxes from the list's own start are summed from 0 in list
//      order and added in slice order, as the value's are.  The inequalities are strict: a value on a grid coordinate
//      takes derivative 0 for that factor (the kink convention), and y_j ≥ r_j, above every hi_bj, zeroes everything.
//   2. hvi_paths_chain_kernel, one lane per (candidate, dimension): ∂t_s/∂x = Σ_j ∂t_s/∂y_j·dy[(j·S + s)·d + ·], j
//      ascending, added over the paths in path order from 0 and divided by S; the lanes of dimension 0 add the t_s the
//      same way into out.  A NaN t_s makes its own ∂t_s/∂x NaN, a NaN value every entry of the candidate's gradient.
// Every lane's work depends on its candidate alone: bitwise independent of N, the column and the launch shape.
template <int K>
__device__ __forceinline__ void hvi_slice_grad(const double (&y)[K], const double* grid, int C,
                                               const uint32_t* __restrict__ boxes, int b0, int b1, double& p_out,
                                               double (&dp)[K]) {
#pragma clang fp contract(off)
  double p = 0.0;
#pragma unroll
  for (int j = 0; j < K; ++j) dp[j] = 0.0;
  for (int b = b0; b < b1; ++b) {
    double t[K];
    bool in[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const uint32_t w = boxes[(size_t)b * K + j];   // lo | hi << 16, wave-uniform
      const int il = min((int)(w & 0xffffu), C - 1), ih = min((int)(w >> 16), C - 1);
      const double lo = grid[j * C + il], hi = grid[j * C + ih];
      t[j] = fmax(hi - fmax(y[j], lo), 0.0);
      in[j] = lo < y[j] && y[j] < hi;
    }
    if constexpr (K == 1) {
      p = p + t[0];
      dp[0] = dp[0] - (in[0] ? 1.0 : 0.0);
    } else {
      double prod = t[0];
#pragma unroll
      for (int j = 1; j < K - 1; ++j) prod *= t[j];
      p = fma(prod, t[K - 1], p);
      // Π_{l≠j} t_l = (t_0 ⋯ t_{j−1})·(t_{j+1} ⋯ t_{K−1}), both in ascending order
      double suf[K];
      suf[K - 1] = 1.0;
#pragma unroll
      for (int j = K - 2; j >= 0; --j) suf[j] = t[j + 1] * suf[j + 1];
      double pre = 1.0;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        dp[j] = dp[j] - (in[j] ? pre * suf[j] : 0.0);
        pre *= t[j];
      }
    }
  }
  p_out = p;
}

// ws[(s·(K + 1) + 0)·N + i] = t_s, ws[(s·(K + 1) + 1 + j)·N + i] = ∂t_s/∂y_j; grid (candidate blocks, S)
template <int K>
__global__ __launch_bounds__(kHviThreads) void hvi_paths_dy_kernel(const double* __restrict__ y, int64_t ld, int64_t N,
                                                                   int S, const double* __restrict__ coords, int C,
                                                                   const uint32_t* __restrict__ boxes, HviPathOff po,
                                                                   double* __restrict__ ws) {
#pragma clang fp contract(off)
  extern __shared__ double hvi_paths_grid[];
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const int s = blockIdx.y;
  const double* g = coords + (size_t)s * K * C;
  for (int t = threadIdx.x; t < K * C; t += kHviThreads) hvi_paths_grid[t] = g[t];
  __syncthreads();
  const int B = po.off[s + 1] - po.off[s];
  const uint32_t* bl = boxes + (size_t)po.off[s] * K;
  const int slices = (B + kHviSlice - 1) / kHviSlice;
  for (int64_t i = (int64_t)blockIdx.x * kHviThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kHviThreads) {
    double yv[K];
    bool nan = false;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      yv[j] = y[((int64_t)j * S + s) * ld + i];
      nan |= yv[j] != yv[j];
    }
    double ts = 0.0, dts[K];
#pragma unroll
    for (int j = 0; j < K; ++j) dts[j] = 0.0;
    for (int c = 0; c < slices; ++c) {
      double p, dp[K];
      hvi_slice_grad<K>(yv, hvi_paths_grid, C, bl, c * kHviSlice, min(B, (c + 1) * kHviSlice), p, dp);
      ts += nan ? qnan : p;
#pragma unroll
      for (int j = 0; j < K; ++j) dts[j] += dp[j];
    }
    double* w = ws + (int64_t)s * (K + 1) * N + i;
    w[0] = ts;
#pragma unroll
    for (int j = 0; j < K; ++j) w[(int64_t)(1 + j) * N] = dts[j];
  }
}

// grid (candidate blocks, d): lane (i, jx) chains and averages; t / tgrad (S, ld) / (S, d, ld) or both null
__global__ __launch_bounds__(kHviThreads) void hvi_paths_chain_kernel(const double* __restrict__ ws, int K, int S,
                                                                      int d, const double* __restrict__ dy,
                                                                      int64_t ld, int64_t N, double* __restrict__ out,
                                                                      double* __restrict__ grad,
                                                                      double* __restrict__ t_out,
                                                                      double* __restrict__ tgrad) {
#pragma clang fp contract(off)
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const int jx = blockIdx.y;
  for (int64_t i = (int64_t)blockIdx.x * kHviThreads + threadIdx.x; i < N; i += (int64_t)gridDim.x * kHviThreads) {
    double total = 0.0, gtotal = 0.0;
    for (int s = 0; s < S; ++s) {
      const double* w = ws + (int64_t)s * (K + 1) * N + i;
      const double ts = w[0];
      double tg = 0.0;
      for (int j = 0; j < K; ++j) tg += w[(int64_t)(1 + j) * N] * dy[(((int64_t)j * S + s) * d + jx) * ld + i];
      if (ts != ts) tg = qnan;
      total += ts;
      gtotal += tg;
      if (t_out) {
        if (jx == 0) t_out[(int64_t)s * ld + i] = ts;
        tgrad[((int64_t)s * d + jx) * ld + i] = tg;
      }
    }
    const double v = total / (double)S;
    if (jx == 0) out[i] = v;
    grad[(int64_t)jx * ld + i] = (v != v) ? qnan : gtotal / (double)S;
  }
}

int64_t hvi_paths_grad_ws_doubles(int64_t N, int k, int S) { return N < 1 ? 0 : (int64_t)S * (k + 1) * N; }

hipError_t launch_hvi_paths_grad(hipStream_t stream, int k, int S, int d, const double* y, const double* dy,
                                 int64_t ld, int64_t N, const double* coords, int C, const uint16_t* boxes,
                                 const int32_t* box_off, double* out, double* grad, double* t_out, double* tgrad,
                                 double* ws) {
  if (N < 1 || S < 1 || S > kPathsMaxS || d < 1 || d > kPathsMaxDim || C < 2 || (int64_t)k * C > kMaxLdsDoubles ||
      (reinterpret_cast<uintptr_t>(boxes) & 3) || !ws || (t_out == nullptr) != (tgrad == nullptr))
    return hipErrorInvalidValue;
  HviPathOff po;
  for (int s = 0; s <= kPathsMaxS; ++s) po.off[s] = box_off[s < S ? s : S];
  const size_t shm = sizeof(double) * (size_t)k * C;
  const int64_t nb = (N + kHviThreads - 1) / kHviThreads;
  const unsigned gx = (unsigned)(nb > (1 << 20) ? (1 << 20) : nb);
  const dim3 b(kHviThreads);
  const uint32_t* bw = reinterpret_cast<const uint32_t*>(boxes);
  switch (k) {
#define OMB_HVIP(KV)                                                                                              \
  case KV:                                                                                                        \
    hipLaunchKernelGGL((hvi_paths_dy_kernel<KV>), dim3(gx, (unsigned)S), b, shm, stream, y, ld, N, S, coords, C, bw, \
                       po, ws);                                                                                   \
    break;
    OMB_HVIP(1) OMB_HVIP(2) OMB_HVIP(3) OMB_HVIP(4) OMB_HVIP(5) OMB_HVIP(6) OMB_HVIP(7) OMB_HVIP(8)
#undef OMB_HVIP
    default: return hipErrorInvalidValue;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(hvi_paths_chain_kernel, dim3(gx, (unsigned)d), b, 0, stream, ws, k, S, d, dy, ld, N, out, grad,
                     t_out, tgrad);
  return hipGetLastError();
}

}  // namespace omb
