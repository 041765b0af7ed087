// Posterior sample paths on gfx950 (omb_paths_set / omb_paths_eval / omb_paths_min): pathwise conditioning with random Fourier
// features (Wilson et al. 2020, "Efficiently sampling functions from Gaussian process posteriors"),
//     f_s(x) = Σ_i w_is·sqrt(2σ_f²/m)·cos(ω̃_i·(x/ℓ) + b_i)  +  Σ_j k(x, X_j)·v_js.
// A draw is a function: evaluating S ≤ 16 of them at N points is O(N·(m + n)·S), nothing is N × N, nothing is
// factorised, and the same paths can be evaluated again anywhere.
//
// paths_eval_kernel: a wave owns 16 candidates (a workgroup 4 waves, no LDS traffic between them, no barriers after
// the table staging, no atomics) and one 16 paths × 16 candidates accumulator of v_mfma_f64_16x16x4_f64 (4 VGPR
// pairs per lane).
//   * Features, 16 at a time: the arguments ω̃ᵀ(x/ℓ) + b of a 16 × 16 tile are ⌈(d+1)/4⌉ MFMA k-steps of the
//     augmented dot product [ω̃_i, b_i]·[x/ℓ, 1] (A fragments packed by the host, omb_host.cpp paths_pack).  The
//     accumulator's register e holds rows 4e + (lane>>4) — exactly the B fragment of k-step e — so after the cosine
//     the four values feed acc += Wᵀ-fragment · cos-tile straight from registers.
//   * Update term, 16 training rows at a time: r² from the training rows' fragments as in kernel_block_mfma_kernel,
//     the same table-driven Matern / RBF transform, then acc += Vᵀ-fragment · K*-tile.
// W and V are stored in A-fragment order, zero padded to 16 paths and whole tiles: padded features and rows meet
// zeros.  A column of the B operand only ever meets its own column of the accumulator and the tile order is fixed
// (features, then training rows), so a path's value at a point is bitwise the same whatever N, the point's column
// and the grid.
#include "omb_internal.h"
#include "omb_math.h"

namespace omb {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

// cos(t) for |t| ≤ 2^20 (kPathsMaxArg): Cody–Waite reduction by π/2 in three constants, then fdlibm's minimax
// polynomials of sin and cos on [−π/4, π/4].  The first constant keeps 33 bits, so n·P1 is exact for the
// n < 2^20 of the range and the first fma is exact; the other two fmas round once each (≤ 2^-54 absolute each).
// The absolute error is below 2 ulp of 1.  Outside the range the reduction's n·P1 is no longer exact and the
// error grows with |t|/2^20 ulp; NaN and ±inf give NaN.
__device__ __forceinline__ double cos_cw(double t) {
  const double n = rint(t * 0.6366197723675814);
  double r = fma(-n, 0x1.921fb54400000p+0, t);
  r = fma(-n, 0x1.0b4611a626331p-34, r);
  r = fma(-n, 0x1.1701b839a2520p-88, r);
  const int q = (int)n;
  const double z = r * r;
  double ps = fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
  double pc = fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
  ps = fma(ps, z, 2.75573137070700676789e-06);
  pc = fma(pc, z, -2.75573143513906633035e-07);
  ps = fma(ps, z, -1.98412698298579493134e-04);
  pc = fma(pc, z, 2.48015872894767294178e-05);
  ps = fma(ps, z, 8.33333333332248946124e-03);
  pc = fma(pc, z, -1.38888888888741095749e-03);
  ps = fma(ps, z, -1.66666666666666324348e-01);
  pc = fma(pc, z, 4.16666666666666019037e-02);
  const double sn = fma(r * z, ps, r);
  const double hz = 0.5 * z, w = 1.0 - hz;
  const double cs = w + (((1.0 - w) - hz) + (z * z) * pc);
  // quadrant 0: cos r, 1: −sin r, 2: −cos r, 3: sin r
  const double v = (q & 1) ? sn : cs;
  return (((q + 1) & 2) != 0) ? -v : v;
}

template <bool LIBCOS>
__device__ __forceinline__ double path_cos(double t) {
  if constexpr (LIBCOS)
    return cos(t);
  else
    return cos_cw(t);
}

// The k-step counts of one instantiation (n_var padded to DP).
template <int DP>
struct PathsDims {
  static constexpr bool kAug = DP <= 8;
  static constexpr int KSD = kAug ? (DP + 5) / 4 : (DP + 3) / 4;
  static constexpr int KSDP = ((DP + 5) / 4 + 1) / 2;   // = packed_X_pairs(DP)
  static constexpr int KSF = (DP + 4) / 4;              // = paths_ksf(DP): k-steps of [x/ℓ, 1]
};

// exp2 table of the Matern / RBF transform into LDS (256 threads; the caller's barrier follows)
template <int KIND>
__device__ __forceinline__ void paths_stage_table(double* etab, int tid) {
  if constexpr (KIND == OMB_KERNEL_MATERN52)
    etab[tid] = kExp2Tab256[tid];
  else if (tid < 64)
    etab[tid] = kExp2Tab64[tid];
}

// A lane's B fragments of candidate ci: the r² operand [−2·x/ℓ, 1, ‖x/ℓ‖²] (n_var ≤ 8) or x/ℓ, and the feature
// operand [x/ℓ, 1]
template <int DP>
__device__ __forceinline__ void paths_operands(const GPDev& g, int d, const double* __restrict__ Xc, int64_t ci,
                                               int lane, double& csq, double (&bfr)[PathsDims<DP>::KSD],
                                               double (&bff)[PathsDims<DP>::KSF]) {
  constexpr bool kAug = PathsDims<DP>::kAug;
  constexpr int KSD = PathsDims<DP>::KSD, KSF = PathsDims<DP>::KSF;
  csq = 0.0;
#pragma unroll
  for (int j = 0; j < DP; ++j) {
    const double c = (j < d) ? Xc[ci * d + j] / g.ls[j] : 0.0;
    csq = fma(c, c, csq);
  }
#pragma unroll
  for (int s = 0; s < KSD; ++s) {
    const int j = 4 * s + (lane >> 4);
    const double c = (j < d) ? Xc[ci * d + j] / g.ls[j] : 0.0;
    if constexpr (kAug)
      bfr[s] = (j < d) ? -2.0 * c : (j == d ? 1.0 : (j == d + 1 ? csq : 0.0));
    else
      bfr[s] = c;
  }
#pragma unroll
  for (int s = 0; s < KSF; ++s) {
    const int j = 4 * s + (lane >> 4);
    const double c = (j < d) ? Xc[ci * d + j] / g.ls[j] : 0.0;
    bff[s] = (j < d) ? c : (j == d ? 1.0 : 0.0);
  }
}

// The 16 paths × 16 candidates tile of a wave: features, then training rows (register e of the result: path
// 4e + (lane >> 4) at the wave's candidate lane & 15)
template <int DP, int KIND, bool LIBCOS>
__device__ __forceinline__ d4 paths_tile(const PathObj& po, int lane, double csq,
                                         const double (&bfr)[PathsDims<DP>::KSD],
                                         const double (&bff)[PathsDims<DP>::KSF], const double* etab,
                                         const ExpCoef& ec) {
  constexpr bool kAug = PathsDims<DP>::kAug;
  constexpr int KSD = PathsDims<DP>::KSD, KSDP = PathsDims<DP>::KSDP, KSF = PathsDims<DP>::KSF;
  constexpr bool kTab256 = KIND == OMB_KERNEL_MATERN52;
  const GPDev& g = po.g;
  const double pm[3] = {g.variance, kSqrt5 * g.variance, kFiveThirds * g.variance};
  d4 acc = d4{0.0, 0.0, 0.0, 0.0};
  // features
  for (int T = 0; T < po.MT; ++T) {
    const double* fa = po.Of + (int64_t)T * (KSF * 64) + lane;
    double a[KSF];
#pragma unroll
    for (int s = 0; s < KSF; ++s) a[s] = fa[64 * s];
    const double* wa = po.Wf + (int64_t)T * 256 + lane;
    double wv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) wv[e] = wa[64 * e];
    d4 cr = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < KSF; ++s) cr = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], bff[s], cr, 0, 0, 0);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wv[e], path_cos<LIBCOS>(cr[e]), acc, 0, 0, 0);
  }
  // update term
  for (int T = 0; T < po.R; ++T) {
    const d2* xa = reinterpret_cast<const d2*>(g.Xf + (int64_t)T * (KSDP * 128) + 2 * lane);
    d2 a[(KSD + 1) / 2];
#pragma unroll
    for (int p = 0; p < (KSD + 1) / 2; ++p) a[p] = xa[64 * p];
    const double* va = po.Vf + (int64_t)T * 256 + lane;
    double vv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) vv[e] = va[64 * e];
    d4 cr = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < KSD; ++s)
      cr = __builtin_amdgcn_mfma_f64_16x16x4f64((s & 1) ? a[s >> 1].y : a[s >> 1].x, bfr[s], cr, 0, 0, 0);
#pragma unroll
    for (int e = 0; e < 4; e += 2) {
      const int k0 = 16 * T + 4 * e + (lane >> 4), k1 = k0 + 4;
      const double r2a = kAug ? cr[e] : fma(-2.0, cr[e], g.xsq[k0] + csq);
      const double r2b = kAug ? cr[e + 1] : fma(-2.0, cr[e + 1], g.xsq[k1] + csq);
      double v0, v1;
      if constexpr (kTab256)
        matern_r2_tab256_x2(r2a, r2b, pm, ec, etab, v0, v1);
      else
        kernel_of_r2_tab_x2<KIND>(r2a, r2b, pm, ec, etab, v0, v1);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(vv[e], v0, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(vv[e + 1], v1, acc, 0, 0, 0);
    }
  }
  return acc;
}

template <int DP, int KIND, bool LIBCOS>
__global__ __launch_bounds__(256) void paths_eval_kernel(PathArgs pa, const double* __restrict__ Xc, int64_t N,
                                                         int64_t ld, double* __restrict__ out, ExpCoef ec) {
  __shared__ double etab[KIND == OMB_KERNEL_MATERN52 ? 256 : 64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  paths_stage_table<KIND>(etab, tid);
  const int o = blockIdx.y;
  const PathObj& po = pa.o[o];
  const int64_t col = (int64_t)blockIdx.x * 64 + 16 * wave + (lane & 15);
  const int64_t ci = col < N ? col : N - 1;
  double csq, bfr[PathsDims<DP>::KSD], bff[PathsDims<DP>::KSF];
  paths_operands<DP>(po.g, pa.d, Xc, ci, lane, csq, bfr, bff);
  __syncthreads();
  const d4 acc = paths_tile<DP, KIND, LIBCOS>(po, lane, csq, bfr, bff, etab, ec);
  if (col < N) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int s = 4 * e + (lane >> 4);
      if (s < po.S) out[((int64_t)o * po.S + s) * ld + col] = acc[e];
    }
  }
}

// ---------------------------------------------------------------------------------------
// omb_paths_min: the same tiles, the minimum of every path in the epilogue.  A (value, index) pair is better when
// its value is smaller, else — at equal values — when its index is lower; index < 0 = none yet (NaN never enters).
// The order is total, so the result does not depend on how the candidates are spread over lanes, waves and
// workgroups.  Four stages, no atomics:
//   1. a lane keeps the best pair of its column in every 64-column block its workgroup visits (grid-stride);
//   2. the 16 candidate lanes of a path meet by xor shuffles, the workgroup's four waves through LDS in wave order;
//   3. thread s < S writes the workgroup's pair of path s to partials[((o·16 + s)·nb + block)·2];
//   4. paths_min_reduce_kernel, one workgroup per (objective, path), reduces the nb pairs and adds the offset.
__device__ __forceinline__ bool min_better(double av, long long ai, double bv, long long bi) {
  if (ai < 0) return false;
  if (bi < 0) return true;
  return (av < bv) || (av == bv && ai < bi);
}

template <int DP, int KIND, bool LIBCOS>
__global__ __launch_bounds__(256) void paths_min_kernel(PathArgs pa, const double* __restrict__ Xc, int64_t N,
                                                        double* __restrict__ partials, ExpCoef ec) {
  __shared__ double etab[KIND == OMB_KERNEL_MATERN52 ? 256 : 64];
  __shared__ double red_v[4 * 16];
  __shared__ long long red_i[4 * 16];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  paths_stage_table<KIND>(etab, tid);
  __syncthreads();
  const int o = blockIdx.y;
  const PathObj& po = pa.o[o];
  double bv[4];
  long long bi[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    bv[e] = HUGE_VAL;
    bi[e] = -1;
  }
  const int64_t nblk = (N + 63) / 64;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t col = blk * 64 + 16 * wave + (lane & 15);
    const int64_t ci = col < N ? col : N - 1;
    double csq, bfr[PathsDims<DP>::KSD], bff[PathsDims<DP>::KSF];
    paths_operands<DP>(po.g, pa.d, Xc, ci, lane, csq, bfr, bff);
    const d4 acc = paths_tile<DP, KIND, LIBCOS>(po, lane, csq, bfr, bff, etab, ec);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double v = acc[e];
      const long long i = (col < N && v == v) ? (long long)col : -1;
      if (min_better(v, i, bv[e], bi[e])) {
        bv[e] = v;
        bi[e] = i;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
      const double ov = __shfl_xor(bv[e], off);
      const long long oi = __shfl_xor(bi[e], off);
      if (min_better(ov, oi, bv[e], bi[e])) {
        bv[e] = ov;
        bi[e] = oi;
      }
    }
    if ((lane & 15) == 0) {
      red_v[16 * wave + 4 * e + (lane >> 4)] = bv[e];
      red_i[16 * wave + 4 * e + (lane >> 4)] = bi[e];
    }
  }
  __syncthreads();
  if (tid < po.S) {
    double v = red_v[tid];
    long long i = red_i[tid];
    for (int w = 1; w < 4; ++w)
      if (min_better(red_v[16 * w + tid], red_i[16 * w + tid], v, i)) {
        v = red_v[16 * w + tid];
        i = red_i[16 * w + tid];
      }
    double* p = partials + (((int64_t)o * 16 + tid) * gridDim.x + blockIdx.x) * 2;
    p[0] = i < 0 ? HUGE_VAL : v;
    p[1] = (double)i;
  }
}

// grid (S, n_obj): the nb pairs of one path → res[(o·S + s)·2 + {0, 1}] = {value, index + offset} or {+inf, −1}
__global__ __launch_bounds__(256) void paths_min_reduce_kernel(const double* __restrict__ partials, int nb, int S,
                                                               int64_t offset, double* __restrict__ res) {
  __shared__ double red_v[4];
  __shared__ long long red_i[4];
  const int s = blockIdx.x, o = blockIdx.y, tid = threadIdx.x;
  const double* p = partials + ((int64_t)o * 16 + s) * nb * 2;
  double v = HUGE_VAL;
  long long i = -1;
  for (int b = tid; b < nb; b += 256) {
    const double pv = p[2 * b];
    const long long pi = (long long)p[2 * b + 1];
    if (min_better(pv, pi, v, i)) {
      v = pv;
      i = pi;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_xor(v, off);
    const long long oi = __shfl_xor(i, off);
    if (min_better(ov, oi, v, i)) {
      v = ov;
      i = oi;
    }
  }
  if ((tid & 63) == 0) {
    red_v[tid >> 6] = v;
    red_i[tid >> 6] = i;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w)
      if (min_better(red_v[w], red_i[w], v, i)) {
        v = red_v[w];
        i = red_i[w];
      }
    double* r = res + ((int64_t)o * S + s) * 2;
    r[0] = i < 0 ? HUGE_VAL : v;
    r[1] = i < 0 ? -1.0 : (double)(i + offset);
  }
}

int paths_min_blocks(int64_t N) {
  const int64_t nblk = (N + 63) / 64;
  return (int)(nblk < kPathsMinMaxBlocks ? nblk : kPathsMinMaxBlocks);
}

template <int KIND, bool LIBCOS>
static hipError_t launch_paths_min_kind(hipStream_t stream, const PathArgs& pa, int n_obj, const double* Xc, int64_t N,
                                        double* partials) {
  const dim3 grid((unsigned)paths_min_blocks(N), (unsigned)n_obj);
  switch (pa.DP) {
#define OMB_PATHS(DPV)                                                                                          \
  case DPV:                                                                                                     \
    hipLaunchKernelGGL((paths_min_kernel<DPV, KIND, LIBCOS>), grid, dim3(256), 0, stream, pa, Xc, N, partials,  \
                       exp_coef());                                                                             \
    break;
    OMB_PATHS(2) OMB_PATHS(4) OMB_PATHS(6) OMB_PATHS(8) OMB_PATHS(16) OMB_PATHS(32) OMB_PATHS(64)
#undef OMB_PATHS
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_paths_min(hipStream_t stream, const PathArgs& pa, int n_obj, int kind, bool libcos, const double* Xc,
                            int64_t N, int64_t offset, double* partials, double* res) {
  const int nb = paths_min_blocks(N);
  if (nb > 0) {
    hipError_t e;
    if (kind == OMB_KERNEL_RBF)
      e = libcos ? launch_paths_min_kind<OMB_KERNEL_RBF, true>(stream, pa, n_obj, Xc, N, partials)
                 : launch_paths_min_kind<OMB_KERNEL_RBF, false>(stream, pa, n_obj, Xc, N, partials);
    else
      e = libcos ? launch_paths_min_kind<OMB_KERNEL_MATERN52, true>(stream, pa, n_obj, Xc, N, partials)
                 : launch_paths_min_kind<OMB_KERNEL_MATERN52, false>(stream, pa, n_obj, Xc, N, partials);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(paths_min_reduce_kernel, dim3((unsigned)pa.o[0].S, (unsigned)n_obj), dim3(256), 0, stream,
                     partials, nb, pa.o[0].S, offset, res);
  return hipGetLastError();
}

template <int KIND, bool LIBCOS>
static hipError_t launch_paths_kind(hipStream_t stream, const PathArgs& pa, int n_obj, const double* Xc, int64_t N,
                                    int64_t ld, double* out) {
  const dim3 grid((unsigned)((N + 63) / 64), (unsigned)n_obj);
  switch (pa.DP) {
#define OMB_PATHS(DPV)                                                                                          \
  case DPV:                                                                                                     \
    hipLaunchKernelGGL((paths_eval_kernel<DPV, KIND, LIBCOS>), grid, dim3(256), 0, stream, pa, Xc, N, ld, out,  \
                       exp_coef());                                                                             \
    break;
    OMB_PATHS(2) OMB_PATHS(4) OMB_PATHS(6) OMB_PATHS(8) OMB_PATHS(16) OMB_PATHS(32) OMB_PATHS(64)
#undef OMB_PATHS
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_paths_eval(hipStream_t stream, const PathArgs& pa, int n_obj, int kind, bool libcos,
                             const double* Xc, int64_t N, int64_t ld, double* out) {
  if (kind == OMB_KERNEL_RBF)
    return libcos ? launch_paths_kind<OMB_KERNEL_RBF, true>(stream, pa, n_obj, Xc, N, ld, out)
                  : launch_paths_kind<OMB_KERNEL_RBF, false>(stream, pa, n_obj, Xc, N, ld, out);
  return libcos ? launch_paths_kind<OMB_KERNEL_MATERN52, true>(stream, pa, n_obj, Xc, N, ld, out)
                : launch_paths_kind<OMB_KERNEL_MATERN52, false>(stream, pa, n_obj, Xc, N, ld, out);
}

// ---------------------------------------------------------------------------------------
// omb_paths_grad: the paths' values and their gradients with respect to the candidate,
//     ∂f_s/∂x_j = (1/ℓ_j)·[ −Σ_i w_is·sqrt(2σ_f²/m)·ω̃_ij·sin(ω̃_i·(x/ℓ) + b_i)  +  Σ_r v_rs·g_r·(x_j/ℓ_j − X_rj/ℓ_j) ],
// g_r = −(5/3)σ_f²(1 + √5 r)e^{−√5 r} (Matern-5/2, finite at r = 0) or −k_r (RBF).
// The wave of paths_eval_kernel with one more 16 paths × 16 candidates accumulator per input dimension: the feature
// tile's B operand of dimension j is −sin-tile[e]·ω̃[16T + 4e + (lane>>4), j] against the value's W fragment, the
// update tile's is g_r·(x_j/ℓ_j − X_rj/ℓ_j) against the value's V fragment (the difference is formed first, so a
// candidate on a training row meets an exact 0), and the epilogue divides by ℓ_j once.  The dimensions go in groups
// of kPathsGradGroup = 8 (8 accumulators = 64 registers per lane beside the value's 8): one pass over the tiles per
// group, the sine and g recomputed per pass, the value accumulated in the first pass alone by paths_tile's own
// sequence of operations — bitwise omb_paths_eval's.  An accumulator column only ever meets its own candidate, the
// tile order is fixed (features, then training rows) and nothing is atomic: a gradient entry is bitwise the same
// whatever N, the column and the grid.
constexpr int kPathsGradGroup = 8;

// cos_cw's reduction and polynomials with the sine it computes beside the cosine (cs is cos_cw's value bit for bit)
__device__ __forceinline__ void sincos_cw(double t, double& sn_out, double& cs_out) {
  const double n = rint(t * 0.6366197723675814);
  double r = fma(-n, 0x1.921fb54400000p+0, t);
  r = fma(-n, 0x1.0b4611a626331p-34, r);
  r = fma(-n, 0x1.1701b839a2520p-88, r);
  const int q = (int)n;
  const double z = r * r;
  double ps = fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
  double pc = fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
  ps = fma(ps, z, 2.75573137070700676789e-06);
  pc = fma(pc, z, -2.75573143513906633035e-07);
  ps = fma(ps, z, -1.98412698298579493134e-04);
  pc = fma(pc, z, 2.48015872894767294178e-05);
  ps = fma(ps, z, 8.33333333332248946124e-03);
  pc = fma(pc, z, -1.38888888888741095749e-03);
  ps = fma(ps, z, -1.66666666666666324348e-01);
  pc = fma(pc, z, 4.16666666666666019037e-02);
  const double sn = fma(r * z, ps, r);
  const double hz = 0.5 * z, w = 1.0 - hz;
  const double cs = w + (((1.0 - w) - hz) + (z * z) * pc);
  // quadrant 0: (sin r, cos r), 1: (cos r, −sin r), 2: (−sin r, −cos r), 3: (−cos r, sin r)
  const double vc = (q & 1) ? sn : cs;
  const double vs = (q & 1) ? cs : sn;
  cs_out = (((q + 1) & 2) != 0) ? -vc : vc;
  sn_out = ((q & 2) != 0) ? -vs : vs;
}

template <bool LIBCOS>
__device__ __forceinline__ void path_sincos(double t, double& sn, double& cs) {
  if constexpr (LIBCOS) {
    cs = cos(t);
    sn = sin(t);
  } else {
    sincos_cw(t, sn, cs);
  }
}

// paths_tile's kernel transform with g beside k (k0, k1 are its values bit for bit): Matern-5/2 is
// matern_r2_tab256_x2's sequence with g = −(5/3)σ_f²(1 + √5 r)·e^{−√5 r} from the same r and exponential
template <int KIND>
__device__ __forceinline__ void paths_kg_x2(double r2a, double r2b, const double (&pm)[3], const ExpCoef& ec,
                                            const double* tab, double& k0, double& k1, double& g0, double& g1) {
  if constexpr (KIND == OMB_KERNEL_MATERN52) {
    r2a = r2_clamp(r2a, ec.t[7]);
    r2b = r2_clamp(r2b, ec.t[7]);
    const double ya = __builtin_amdgcn_rsq(r2a), yb = __builtin_amdgcn_rsq(r2b);
    double ga = r2a * ya, gb = r2b * yb, ha = 0.5 * ya, hb = 0.5 * yb;
    const double qa = fma(-ga, ha, 0.5), qb = fma(-gb, hb, 0.5);
    ga = fma(ga, qa, ga);
    gb = fma(gb, qb, gb);
    ha = fma(ha, qa, ha);
    hb = fma(hb, qb, hb);
    ga = fma(fma(-ga, ga, r2a), ha, ga);
    gb = fma(fma(-gb, gb, r2b), hb, gb);
    const double pa_ = fma(pm[2], r2a, fma(pm[1], ga, pm[0]));
    const double pb_ = fma(pm[2], r2b, fma(pm[1], gb, pm[0]));
    const RoundedK rka = round_shift(fma(ga, ec.u[0], 6755399441055744.0));
    const RoundedK rkb = round_shift(fma(gb, ec.u[0], 6755399441055744.0));
    double fa = fma(rka.k, ec.u[1], ga), fb = fma(rkb.k, ec.u[1], gb);
    fa = fma(rka.k, ec.u[2], fa);
    fb = fma(rkb.k, ec.u[2], fb);
    double sa = fma(fa, ec.u[3], ec.u[4]), sb = fma(fb, ec.u[3], ec.u[4]);
    sa = fma_vvs(sa, fa, ec.u[5]);
    sb = fma_vvs(sb, fb, ec.u[5]);
    sa = fma_vvs(sa, fa, ec.u[6]);
    sb = fma_vvs(sb, fb, ec.u[6]);
    const int ia = rka.ki, ib = rkb.ki;
    const double Ta = tab[ia & 255], Tb = tab[ib & 255];
    const double ea = ldexp(fma(Ta, sa * fa, Ta), ia >> 8), eb = ldexp(fma(Tb, sb * fb, Tb), ib >> 8);
    k0 = pa_ * ea;
    k1 = pb_ * eb;
    g0 = -(pm[2] * fma(kSqrt5, ga, 1.0)) * ea;
    g1 = -(pm[2] * fma(kSqrt5, gb, 1.0)) * eb;
  } else {
    kernel_of_r2_tab_x2<KIND>(r2a, r2b, pm, ec, tab, k0, k1);
    g0 = -k0;
    g1 = -k1;
  }
}

template <int DP, int KIND, bool LIBCOS>
__global__ __launch_bounds__(256) void paths_grad_kernel(PathArgs pa, const double* __restrict__ Xc, int64_t N,
                                                         int64_t ld, double* __restrict__ out,
                                                         double* __restrict__ grad, ExpCoef ec) {
  constexpr bool kAug = PathsDims<DP>::kAug;
  constexpr int KSD = PathsDims<DP>::KSD, KSDP = PathsDims<DP>::KSDP, KSF = PathsDims<DP>::KSF;
  constexpr int DG = DP < kPathsGradGroup ? DP : kPathsGradGroup;
  __shared__ double etab[KIND == OMB_KERNEL_MATERN52 ? 256 : 64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  paths_stage_table<KIND>(etab, tid);
  const int o = blockIdx.y;
  const PathObj& po = pa.o[o];
  const GPDev& g = po.g;
  const int d = pa.d;
  const int64_t col = (int64_t)blockIdx.x * 64 + 16 * wave + (lane & 15);
  const int64_t ci = col < N ? col : N - 1;
  double csq, bfr[KSD], bff[KSF];
  paths_operands<DP>(g, d, Xc, ci, lane, csq, bfr, bff);
  __syncthreads();
  const double pm[3] = {g.variance, kSqrt5 * g.variance, kFiveThirds * g.variance};
  const int rq = lane >> 4;   // the B operand's row within a k-step
  for (int j0 = 0; j0 < d; j0 += DG) {
    const bool first = j0 == 0;   // wave-uniform: the value rides the first pass
    double xl[DG];
#pragma unroll
    for (int jj = 0; jj < DG; ++jj) xl[jj] = (j0 + jj < d) ? Xc[ci * d + j0 + jj] / g.ls[j0 + jj] : 0.0;
    d4 acc = d4{0.0, 0.0, 0.0, 0.0};
    d4 ga[DG];
#pragma unroll
    for (int jj = 0; jj < DG; ++jj) ga[jj] = d4{0.0, 0.0, 0.0, 0.0};
    // features
    for (int T = 0; T < po.MT; ++T) {
      const double* fa = po.Of + (int64_t)T * (KSF * 64) + lane;
      double a[KSF];
#pragma unroll
      for (int s = 0; s < KSF; ++s) a[s] = fa[64 * s];
      const double* wa = po.Wf + (int64_t)T * 256 + lane;
      double wv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) wv[e] = wa[64 * e];
      d4 cr = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < KSF; ++s) cr = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], bff[s], cr, 0, 0, 0);
      double sn[4], cs[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) path_sincos<LIBCOS>(cr[e], sn[e], cs[e]);
      if (first) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wv[e], cs[e], acc, 0, 0, 0);
      }
      // ω̃[16T + 4e + rq, j] out of the A-fragment order: component j of feature (4e + rq) of the tile
      const double* om = po.Of + (int64_t)T * (KSF * 64) + rq;
#pragma unroll
      for (int jj = 0; jj < DG; ++jj) {
        const int j = j0 + jj;
        if (j < d) {
          const double* oj = om + (j >> 2) * 64 + ((j & 3) << 4);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            ga[jj] = __builtin_amdgcn_mfma_f64_16x16x4f64(wv[e], -(sn[e] * oj[4 * e]), ga[jj], 0, 0, 0);
        }
      }
    }
    // update term
    for (int T = 0; T < po.R; ++T) {
      const d2* xa = reinterpret_cast<const d2*>(g.Xf + (int64_t)T * (KSDP * 128) + 2 * lane);
      d2 a[(KSD + 1) / 2];
#pragma unroll
      for (int p = 0; p < (KSD + 1) / 2; ++p) a[p] = xa[64 * p];
      const double* va = po.Vf + (int64_t)T * 256 + lane;
      double vv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) vv[e] = va[64 * e];
      d4 cr = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < KSD; ++s)
        cr = __builtin_amdgcn_mfma_f64_16x16x4f64((s & 1) ? a[s >> 1].y : a[s >> 1].x, bfr[s], cr, 0, 0, 0);
      double kv[4], gv[4];
#pragma unroll
      for (int e = 0; e < 4; e += 2) {
        const int k0 = 16 * T + 4 * e + rq, k1 = k0 + 4;
        const double r2a = kAug ? cr[e] : fma(-2.0, cr[e], g.xsq[k0] + csq);
        const double r2b = kAug ? cr[e + 1] : fma(-2.0, cr[e + 1], g.xsq[k1] + csq);
        paths_kg_x2<KIND>(r2a, r2b, pm, ec, etab, kv[e], kv[e + 1], gv[e], gv[e + 1]);
      }
      if (first) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(vv[e], kv[e], acc, 0, 0, 0);
      }
      // training row 16T + 4e + rq of Xs = X/ℓ (n_pad ≥ 16R rows of pitch DP, zero padded)
      const double* xr = g.Xs + ((int64_t)16 * T + rq) * DP;
#pragma unroll
      for (int jj = 0; jj < DG; ++jj) {
        const int j = j0 + jj;
        if (j < d) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const double df = xl[jj] - xr[(4 * e) * DP + j];
            ga[jj] = __builtin_amdgcn_mfma_f64_16x16x4f64(vv[e], gv[e] * df, ga[jj], 0, 0, 0);
          }
        }
      }
    }
    if (col < N) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int s = 4 * e + rq;
        if (s < po.S) {
          if (first) out[((int64_t)o * po.S + s) * ld + col] = acc[e];
#pragma unroll
          for (int jj = 0; jj < DG; ++jj)
            if (j0 + jj < d) grad[(((int64_t)o * po.S + s) * d + j0 + jj) * ld + col] = ga[jj][e] / g.ls[j0 + jj];
        }
      }
    }
  }
}

template <int KIND, bool LIBCOS>
static hipError_t launch_paths_grad_kind(hipStream_t stream, const PathArgs& pa, int n_obj, const double* Xc,
                                         int64_t N, int64_t ld, double* out, double* grad) {
  const dim3 grid((unsigned)((N + 63) / 64), (unsigned)n_obj);
  switch (pa.DP) {
#define OMB_PATHS(DPV)                                                                                          \
  case DPV:                                                                                                     \
    hipLaunchKernelGGL((paths_grad_kernel<DPV, KIND, LIBCOS>), grid, dim3(256), 0, stream, pa, Xc, N, ld, out,  \
                       grad, exp_coef());                                                                       \
    break;
    OMB_PATHS(2) OMB_PATHS(4) OMB_PATHS(6) OMB_PATHS(8) OMB_PATHS(16) OMB_PATHS(32) OMB_PATHS(64)
#undef OMB_PATHS
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_paths_grad(hipStream_t stream, const PathArgs& pa, int n_obj, int kind, bool libcos,
                             const double* Xc, int64_t N, int64_t ld, double* out, double* grad) {
  if (kind == OMB_KERNEL_RBF)
    return libcos ? launch_paths_grad_kind<OMB_KERNEL_RBF, true>(stream, pa, n_obj, Xc, N, ld, out, grad)
                  : launch_paths_grad_kind<OMB_KERNEL_RBF, false>(stream, pa, n_obj, Xc, N, ld, out, grad);
  return libcos ? launch_paths_grad_kind<OMB_KERNEL_MATERN52, true>(stream, pa, n_obj, Xc, N, ld, out, grad)
                : launch_paths_grad_kind<OMB_KERNEL_MATERN52, false>(stream, pa, n_obj, Xc, N, ld, out, grad);
}

// U (n, S) row-major = F (S rows of pitch n: the prior paths at the training inputs) transposed + sd·z
__global__ void paths_u_kernel(const double* __restrict__ F, const double* __restrict__ z, double sd, int n, int S,
                               double* __restrict__ U) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)n * S) return;
  const int i = (int)(t / S), s = (int)(t % S);
  const double f = F[(int64_t)s * n + i];
  U[t] = z ? fma(sd, z[t], f) : f;
}

hipError_t launch_paths_u(hipStream_t stream, const double* F, const double* z, double sd, int n, int S, double* U) {
  const int64_t total = (int64_t)n * S;
  hipLaunchKernelGGL(paths_u_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, F, z, sd, n, S, U);
  return hipGetLastError();
}

// Vf: v = α − G (G (n, S) = L⁻ᵀL⁻¹U) as the A operand of the update term, row tile T, k-step e:
//     Vf[(4T + e)·64 + lane] = v[16T + 4e + (lane>>4)][lane&15], 0 past n rows or S paths
__global__ void paths_pack_v_kernel(const double* __restrict__ alpha, const double* __restrict__ G, int n, int S,
                                    int64_t total, double* __restrict__ Vf) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int lane = (int)(t & 63);
  const int64_t row = 4 * (t >> 6) + (lane >> 4);
  const int s = lane & 15;
  Vf[t] = (row < n && s < S) ? alpha[row] - G[row * S + s] : 0.0;
}

hipError_t launch_paths_pack_v(hipStream_t stream, const double* alpha, const double* G, int n, int S, int R,
                               double* Vf) {
  const int64_t total = paths_vf_doubles(R);
  hipLaunchKernelGGL(paths_pack_v_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, alpha, G, n,
                     S, total, Vf);
  return hipGetLastError();
}

}  // namespace omb
