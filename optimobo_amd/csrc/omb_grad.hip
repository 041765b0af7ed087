// Analytic gradients with respect to a candidate on gfx950 (omb_posterior_grad, omb_eval_grad).
//
//   ∂k_i/∂x_j = g_i·s_ij,  s_ij = (x_j − X_ij)/ℓ_j²,  g_i = −(5/3)σ_f²(1 + √5 r_i)e^{−√5 r_i} (Matern-5/2; finite at
//   r = 0, nothing is divided by r) or −k_i (RBF);  ∂μ/∂x_j = Σ_i α_i g_i s_ij;  ∂σ²/∂x_j = −2 Σ_i w_i g_i s_ij with
//   w = L⁻ᵀ(L⁻¹k) — the two triangular products with the dense L⁻¹ run as the library's FP64-MFMA GEMMs (omb_api.hip),
//   their result W (n, Nc) is the only per-training-row tensor that exists: g_i and s_ij are formed here, inside the
//   contraction, from the packed Xs = X/ℓ and ℓ.
//
// The acquisition kernels below give ∂a/∂μ_o and ∂a/∂σ²_o per candidate (rows o of dadm / dadv, pitch N); the
// contraction kernel applies the chain rule as it finishes each objective, so no (n_obj, N, d) tensor is stored on
// the omb_eval_grad path.  Every sum has one fixed order that depends on (n, d, P, B) alone: a candidate's gradient
// does not depend on N or on its place in the batch.  No floating-point atomics.
#include <math.h>

#include "omb_internal.h"
#include "omb_math.h"

namespace omb {

constexpr int kGradThreads = 256;

template <int KIND>
__device__ __forceinline__ double kernel_g(double r2, double variance) {
  if constexpr (KIND == OMB_KERNEL_MATERN52) {
    const double r = sqrt(r2);
    return -(kFiveThirds * variance) * (1.0 + kSqrt5 * r) * exp(-(kSqrt5 * r));
  } else {
    return -(variance * exp(-0.5 * r2));
  }
}

// ------------------------------------------------------------------------------ contraction (+ chain rule)
// One workgroup per candidate.  Per objective: the candidate is scaled by that objective's ℓ into LDS; the training
// rows go by in tiles of 256 — thread t forms r², g and the two coefficients α_i g_i, w_i g_i of row i0 + t (LDS),
// then the threads regroup as (dimension jj, row group ip): thread (jj, ip) adds coefficient·(x_jj − X_i,jj)/ℓ over
// the rows ip, ip + G, … of the tile (consecutive threads read consecutive dimensions of a row).  The G row groups'
// sums meet in group order.  The difference is accumulated directly, never as x_j Σa − Σ a X_ij.
template <int KIND>
__global__ __launch_bounds__(kGradThreads) void grad_contract_kernel(GradArgs ga, const double* __restrict__ Xc,
                                                                    int64_t nc, int64_t c0, int64_t N,
                                                                    double* __restrict__ dmu,
                                                                    double* __restrict__ dvar,
                                                                    const double* __restrict__ dadm,
                                                                    const double* __restrict__ dadv,
                                                                    const double* __restrict__ vals,
                                                                    double* __restrict__ grad) {
  __shared__ double xs[OMB_MAX_DIM];
  __shared__ double ca[kGradThreads], cb[kGradThreads];
  __shared__ double rm[kGradThreads], rv[kGradThreads];
  const int t = threadIdx.x;
  const int64_t cl = blockIdx.x, c = c0 + cl;
  const int d = ga.d, DP = ga.DP, JW = ga.JW, G = kGradThreads / JW;
  const int jj = t & (JW - 1), ip = t / JW;
  double gacc = 0.0;
  for (int o = 0; o < ga.n_obj; ++o) {
    const GradObj& g = ga.o[o];
    for (int j = t; j < d; j += kGradThreads) xs[j] = Xc[cl * d + j] / g.ls[j];
    __syncthreads();
    double am = 0.0, av = 0.0;
    for (int i0 = 0; i0 < g.n; i0 += kGradThreads) {
      const int i = i0 + t;
      double a = 0.0, b = 0.0;
      if (i < g.n) {
        const double* row = g.Xs + (size_t)i * DP;
        double r2 = 0.0;
        for (int j = 0; j < d; ++j) {
          const double df = xs[j] - row[j];
          r2 = fma(df, df, r2);
        }
        const double gi = kernel_g<KIND>(r2, g.variance);
        a = g.alpha[i] * gi;
        b = g.W[(size_t)i * nc + cl] * gi;
      }
      ca[t] = a;
      cb[t] = b;
      __syncthreads();
      const int rows = (g.n - i0) < kGradThreads ? (g.n - i0) : kGradThreads;
      if (jj < d) {
        const double xj = xs[jj];
        const double* col = g.Xs + (size_t)i0 * DP + jj;
        for (int q = ip; q < rows; q += G) {
          const double df = xj - col[(size_t)q * DP];
          am = fma(ca[q], df, am);
          av = fma(cb[q], df, av);
        }
      }
      __syncthreads();
    }
    rm[t] = am;
    rv[t] = av;
    __syncthreads();
    if (t < JW && t < d) {
      double sm = 0.0, sv = 0.0;
      for (int q = 0; q < G; ++q) {
        sm += rm[q * JW + t];
        sv += rv[q * JW + t];
      }
      const double l = g.ls[t];
      const double dm = sm / l, dv = -2.0 * (sv / l);
      if (dmu) {
        dmu[((size_t)o * N + c) * d + t] = dm;
        dvar[((size_t)o * N + c) * d + t] = dv;
      }
      if (grad) gacc += dadm[(size_t)o * N + c] * dm + dadv[(size_t)o * N + c] * dv;
    }
    __syncthreads();
  }
  if (grad && t < JW && t < d) {
    const double v = vals[c];
    grad[(size_t)c * d + t] = (v != v) ? __builtin_nan("") : gacc;   // a NaN value: an all-NaN row
  }
}

hipError_t launch_grad_contract(hipStream_t stream, const GradArgs& ga, int kind, const double* Xc, int64_t nc,
                                int64_t c0, int64_t N, double* dmu, double* dvar, const double* dadm,
                                const double* dadv, const double* vals, double* grad) {
  if (nc <= 0) return hipSuccess;
  const dim3 g((unsigned)nc), b(kGradThreads);
  if (kind == OMB_KERNEL_RBF)
    hipLaunchKernelGGL(grad_contract_kernel<OMB_KERNEL_RBF>, g, b, 0, stream, ga, Xc, nc, c0, N, dmu, dvar, dadm, dadv,
                       vals, grad);
  else
    hipLaunchKernelGGL(grad_contract_kernel<OMB_KERNEL_MATERN52>, g, b, 0, stream, ga, Xc, nc, c0, N, dmu, dvar, dadm,
                       dadv, vals, grad);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------ EI family
// EI = σ h(γ), h = γΦ(γ) + φ(γ), h' = Φ, σ = sqrt(σ² + ε), γ = (best − μ)/(σ + 1e-10):
//   ∂EI/∂μ = −σΦ/(σ + 1e-10),  ∂EI/∂σ² = (h − σΦγ/(σ + 1e-10))/(2σ).
// MODE 1 multiplies by μ1 (∂/∂μ1 = EI), MODE 2 by Π_c Φ(z_c), z_c = −μ_c/s_c, s_c = sqrt(σ²_c + pof_eps):
//   ∂/∂μ_c = EI Π_{q≠c}Φ(z_q) φ(z_c)(−1/s_c),  ∂/∂σ²_c = EI Π_{q≠c}Φ(z_q) φ(z_c) μ_c/(2 s_c³).
template <int MODE>
__global__ __launch_bounds__(kGradThreads) void ei_grad_kernel(const double* __restrict__ mu,
                                                               const double* __restrict__ var, int64_t ld, int64_t N,
                                                               int k, double best, double var_eps, double pof_eps,
                                                               double* __restrict__ dadm, double* __restrict__ dadv) {
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < N; c += (int64_t)gridDim.x * blockDim.x) {
    const double sigma = sqrt(var[c] + var_eps);
    const double s1 = sigma + 1e-10;
    const double gamma = (best - mu[c]) / s1;
    const double Pg = ndtr(gamma), pg = npdf(gamma);
    const double h = gamma * Pg + pg;
    const double ei = sigma * h;
    const double dm0 = -(sigma * Pg) / s1;
    const double dv0 = (h - sigma * Pg * gamma / s1) / (2.0 * sigma);
    if (MODE == 0) {
      dadm[c] = dm0;
      dadv[c] = dv0;
    } else if (MODE == 1) {
      const double m1 = mu[ld + c];
      dadm[c] = m1 * dm0;
      dadv[c] = m1 * dv0;
      dadm[N + c] = ei;
      dadv[N + c] = 0.0;
    } else {
      double pof = 1.0;
      for (int j = 1; j < k; ++j) pof *= ndtr((0.0 - mu[j * ld + c]) / sqrt(var[j * ld + c] + pof_eps));
      dadm[c] = dm0 * pof;
      dadv[c] = dv0 * pof;
      for (int j = 1; j < k; ++j) {
        double others = ei;
        for (int q = 1; q < k; ++q)
          if (q != j) others *= ndtr((0.0 - mu[q * ld + c]) / sqrt(var[q * ld + c] + pof_eps));
        const double mj = mu[j * ld + c], sj = sqrt(var[j * ld + c] + pof_eps);
        const double pz = npdf((0.0 - mj) / sj);
        dadm[j * N + c] = others * pz * (-1.0 / sj);
        dadv[j * N + c] = others * pz * (mj / (2.0 * sj * sj * sj));
      }
    }
  }
}

hipError_t launch_ei_grad(hipStream_t stream, int kind, int k, const double* mu, const double* var, int64_t ld,
                          int64_t N, double best, double var_eps, double pof_eps, double* dadm, double* dadv) {
  int64_t nb = (N + kGradThreads - 1) / kGradThreads;
  const dim3 grid((unsigned)(nb > 65536 ? 65536 : (nb < 1 ? 1 : nb))), block(kGradThreads);
  if (kind == OMB_EI_PARETO)
    hipLaunchKernelGGL(ei_grad_kernel<1>, grid, block, 0, stream, mu, var, ld, N, k, best, var_eps, pof_eps, dadm, dadv);
  else if (kind == OMB_EI_CONSTRAINED)
    hipLaunchKernelGGL(ei_grad_kernel<2>, grid, block, 0, stream, mu, var, ld, N, k, best, var_eps, pof_eps, dadm, dadv);
  else
    hipLaunchKernelGGL(ei_grad_kernel<0>, grid, block, 0, stream, mu, var, ld, N, k, best, var_eps, pof_eps, dadm, dadv);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------ probability of feasibility
// Product rule of a·F, F = Π_j Φ(z_j) over the c constraint rows (omb_plan_constraints; pof_scale_kernel's z): a is
// the unweighted acquisition, rows 0..k−1 of dadm / dadv hold its partials and are scaled by F, rows k..k+c−1 get
//   ∂(aF)/∂μ_j = a Π_{q≠j}Φ(z_q) φ(z_j)(−1/s_j),  ∂(aF)/∂σ²_j = a Π_{q≠j}Φ(z_q) φ(z_j) μ_j/(2 s_j³),  s_j = sqrt(σ²_j + pof_eps).
// The products leave factor j out instead of dividing F by Φ(z_j): finite where F underflows to 0.  mu / var point at
// constraint row 0 (pitch ld).  The loops have the constant bound kMaxCon and unroll, so Φ and φ stay in registers.
constexpr int kMaxCon = OMB_MAX_OBJ - 1;
__global__ __launch_bounds__(kGradThreads) void pof_grad_kernel(const double* __restrict__ a,
                                                                const double* __restrict__ mu,
                                                                const double* __restrict__ var, int64_t ld, int64_t N,
                                                                int k, int c, double pof_eps,
                                                                double* __restrict__ dadm, double* __restrict__ dadv) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    double P[kMaxCon], cm[kMaxCon], cv[kMaxCon];
    double F = 1.0;
#pragma unroll
    for (int j = 0; j < kMaxCon; ++j) {
      P[j] = 1.0;
      cm[j] = 0.0;
      cv[j] = 0.0;
      if (j < c) {
        const double mj = mu[j * ld + i], sj = sqrt(var[j * ld + i] + pof_eps);
        const double z = (0.0 - mj) / sj, pz = npdf(z);
        P[j] = ndtr(z);
        cm[j] = pz * (-1.0 / sj);
        cv[j] = pz * (mj / (2.0 * sj * sj * sj));
        F *= P[j];
      }
    }
    for (int o = 0; o < k; ++o) {
      dadm[o * N + i] *= F;
      dadv[o * N + i] *= F;
    }
    const double ai = a[i];
#pragma unroll
    for (int j = 0; j < kMaxCon; ++j) {
      if (j < c) {
        double others = ai;
#pragma unroll
        for (int q = 0; q < kMaxCon; ++q)
          if (q != j) others *= P[q];   // P[q] = 1 past c
        dadm[(k + j) * N + i] = others * cm[j];
        dadv[(k + j) * N + i] = others * cv[j];
      }
    }
  }
}

hipError_t launch_pof_grad(hipStream_t stream, const double* a, const double* mu, const double* var, int64_t ld,
                           int64_t N, int k, int c, double pof_eps, double* dadm, double* dadv) {
  int64_t nb = (N + kGradThreads - 1) / kGradThreads;
  const dim3 grid((unsigned)(nb > 65536 ? 65536 : (nb < 1 ? 1 : nb))), block(kGradThreads);
  hipLaunchKernelGGL(pof_grad_kernel, grid, block, 0, stream, a, mu, var, ld, N, k, c, pof_eps, dadm, dadv);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------ EHVI 2-D
// With E(a; m, s) = sφ(t) + (a − m)Φ(t), t = (a − m)/s (∂E/∂m = −Φ(t), ∂E/∂s = φ(t), any s ≠ 0), stripe i of
// ehvi2d_point is A_i·E(y2_i; μ1, σB),  A_i = (y1_{i−1} − y1_i)Φ(t_i) + ψ(y1_{i−1}, y1_{i−1}) − ψ(y1_{i−1}, y1_i), and
//   ∂A_i/∂μ0 = Φ(t_i) − Φ(t_{i−1}),   ∂A_i/∂σA = φ(t_{i−1}) − φ(t_i)
// (the (y1_{i−1} − y1_i) terms cancel).  TEXTBOOK adds the stripe E(y1_P; μ0, σA)·E(r1; μ1, σB) and has σA = sqrt(σ²0),
// σB = sqrt(σ²1); REFERENCE has σA = σ²0·s00, σB = σ²0·s01 and no last stripe — differentiated as they are.
// One wavefront per candidate: lane l takes stripes 1 + l, 65 + l, …; the four sums meet by xor shuffles.
__global__ __launch_bounds__(kGradThreads) void ehvi2d_grad_kernel(const double* __restrict__ mu,
                                                                   const double* __restrict__ var, int64_t ld,
                                                                   int64_t N, const double* __restrict__ pf, int P,
                                                                   double r0, double r1, double s00, double s01,
                                                                   int mode, double* __restrict__ dadm,
                                                                   double* __restrict__ dadv) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int WPB = kGradThreads / 64;
  for (int64_t c = (int64_t)blockIdx.x * WPB + wave; c < N; c += (int64_t)gridDim.x * WPB) {
    const double m0 = mu[c], m1 = mu[ld + c], v0 = var[c], v1 = var[ld + c];
    double sA, sB;
    if (mode == OMB_EHVI_REFERENCE) {
      sA = v0 * s00;
      sB = v0 * s01;
    } else {
      sA = sqrt(v0);
      sB = sqrt(v1);
    }
    double gm0 = 0.0, gsA = 0.0, gm1 = 0.0, gsB = 0.0;
    for (int i = 1 + lane; i <= P; i += 64) {
      const double y1p = (i == 1) ? r0 : pf[2 * (i - 2)], y1i = pf[2 * (i - 1)], y2i = pf[2 * (i - 1) + 1];
      const double tp = (y1p - m0) / sA, t = (y1i - m0) / sA, u = (y2i - m1) / sB;
      const double Pt = ndtr(t), Ptp = ndtr(tp), pt = npdf(t), ptp = npdf(tp), Pu = ndtr(u), pu = npdf(u);
      const double p2 = sB * pu + (y2i - m1) * Pu;
      const double A = (y1p - y1i) * Pt + (sA * ptp + (y1p - m0) * Ptp) - (sA * pt + (y1p - m0) * Pt);
      gm0 += (Pt - Ptp) * p2;
      gsA += (ptp - pt) * p2;
      gm1 -= A * Pu;
      gsB += A * pu;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      gm0 += __shfl_xor(gm0, off);
      gsA += __shfl_xor(gsA, off);
      gm1 += __shfl_xor(gm1, off);
      gsB += __shfl_xor(gsB, off);
    }
    if (lane == 0) {
      double dv0, dv1;
      if (mode == OMB_EHVI_TEXTBOOK) {
        const double y1P = pf[2 * (P - 1)];
        const double tP = (y1P - m0) / sA, u = (r1 - m1) / sB;
        const double PtP = ndtr(tP), ptP = npdf(tP), Pu = ndtr(u), pu = npdf(u);
        const double EA = sA * ptP + (y1P - m0) * PtP, EB = sB * pu + (r1 - m1) * Pu;
        gm0 -= PtP * EB;
        gsA += ptP * EB;
        gm1 -= EA * Pu;
        gsB += EA * pu;
        dv0 = gsA / (2.0 * sA);
        dv1 = gsB / (2.0 * sB);
      } else {
        dv0 = gsA * s00 + gsB * s01;
        dv1 = 0.0;
      }
      dadm[c] = gm0;
      dadm[N + c] = gm1;
      dadv[c] = dv0;
      dadv[N + c] = dv1;
    }
  }
}

hipError_t launch_ehvi2d_grad(hipStream_t stream, const double* mu, const double* var, int64_t ld, int64_t N,
                              const double* pf, int P, double r0, double r1, double s00, double s01, int mode,
                              double* dadm, double* dadv) {
  constexpr int WPB = kGradThreads / 64;
  int64_t nb = (N + WPB - 1) / WPB;
  const dim3 grid((unsigned)(nb > 65536 ? 65536 : (nb < 1 ? 1 : nb))), block(kGradThreads);
  hipLaunchKernelGGL(ehvi2d_grad_kernel, grid, block, 0, stream, mu, var, ld, N, pf, P, r0, r1, s00, s01, mode, dadm,
                     dadv);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------ exact EHVI over boxes
// EHVI = Σ_b Π_j T_j,  T_j = G(l_bj, u_bj) = E(u; μ_j, σ_j) − E(l; μ_j, σ_j) (ehvi_boxes_kernel's expression), so
//   ∂T_j/∂μ_j = −(Φ(β) − Φ(α)),  ∂T_j/∂σ_j = φ(β) − φ(α),  ∂EHVI/∂μ_j = Σ_b (Π_{i≠j} T_i) ∂T_j/∂μ_j, likewise σ_j,
// and ∂/∂σ²_j = ∂/∂σ_j / (2σ_j).  One workgroup per candidate: Φ and φ at the K·C grid coordinates go to LDS, thread t
// takes boxes t, t + 256, … (prefix / suffix products give Π_{i≠j}), and the 2K sums are reduced in the value kernels'
// fixed order: xor shuffles in the wave, then the four waves in wave order.  LDS doubles: 2·K·C + 8·K, within 64 KiB
// for every grid check_boxes / check_boxes_k admit.  Grid indices are clamped to the grid (omb_plan_ehvi_boxes does
// not check its list), so nothing is read past the coordinates.
template <int K>
__global__ __launch_bounds__(kGradThreads) void ehvi_boxes_grad_kernel(const double* __restrict__ mu,
                                                                       const double* __restrict__ var, int64_t ld,
                                                                       int64_t N, const double* __restrict__ coords,
                                                                       int C, const uint16_t* __restrict__ boxes, int B,
                                                                       double* __restrict__ dadm,
                                                                       double* __restrict__ dadv) {
  extern __shared__ double gsm[];
  const int KC = K * C;
  double* tabP = gsm;
  double* tabp = gsm + KC;
  double* red = gsm + 2 * KC;   // waves × 2K
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int64_t c = blockIdx.x; c < N; c += gridDim.x) {
    __syncthreads();   // the previous candidate's table and reduction reads are done
    double m[K], s[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      m[j] = mu[j * ld + c];
      s[j] = sqrt(var[j * ld + c]);
    }
    for (int i = tid; i < KC; i += kGradThreads) {
      const int j = i / C;
      double mj = m[0], sj = s[0];
#pragma unroll
      for (int q = 1; q < K; ++q)
        if (j == q) {
          mj = m[q];
          sj = s[q];
        }
      const double t = (fmax(coords[i], -1e300) - mj) / sj;
      tabP[i] = ndtr(t);
      tabp[i] = npdf(t);
    }
    __syncthreads();
    double dm[K], ds[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      dm[j] = 0.0;
      ds[j] = 0.0;
    }
    for (int b = tid; b < B; b += kGradThreads) {
      double T[K], Tm[K], Ts[K], left[K];
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const int lo = boxes[(size_t)2 * K * b + 2 * j], hi = boxes[(size_t)2 * K * b + 2 * j + 1];
        const int il = j * C + (lo < C ? lo : C - 1), ih = j * C + (hi < C ? hi : C - 1);
        const double l = fmax(coords[il], -1e300), u = fmax(coords[ih], -1e300);
        const double Pl = tabP[il], Pu = tabP[ih], pl = tabp[il], pu = tabp[ih];
        T[j] = (u - l) * Pl + (u - m[j]) * (Pu - Pl) + s[j] * (pu - pl);
        Tm[j] = -(Pu - Pl);
        Ts[j] = pu - pl;
      }
      double pre = 1.0;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        left[j] = pre;
        pre *= T[j];
      }
      double suf = 1.0;
#pragma unroll
      for (int j = K - 1; j >= 0; --j) {
        const double others = left[j] * suf;
        dm[j] += others * Tm[j];
        ds[j] += others * Ts[j];
        suf *= T[j];
      }
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
      double a = dm[j], b2 = ds[j];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off);
        b2 += __shfl_xor(b2, off);
      }
      if (lane == 0) {
        red[wave * 2 * K + j] = a;
        red[wave * 2 * K + K + j] = b2;
      }
    }
    __syncthreads();
    if (tid < 2 * K) {
      const double v = ((red[tid] + red[2 * K + tid]) + red[4 * K + tid]) + red[6 * K + tid];
      if (tid < K)
        dadm[(size_t)tid * N + c] = v;
      else
        dadv[(size_t)(tid - K) * N + c] = v / (2.0 * sqrt(var[(tid - K) * ld + c]));
    }
  }
}

hipError_t launch_ehvi_boxes_grad(hipStream_t stream, int k, const double* mu, const double* var, int64_t ld,
                                  int64_t N, const double* coords, int C, const uint16_t* boxes, int B, double* dadm,
                                  double* dadv) {
  const size_t shm = sizeof(double) * ((size_t)2 * k * C + 8 * (size_t)k);
  if (shm > 64 * 1024 || C < 1) return hipErrorInvalidValue;
  const dim3 g((unsigned)(N > 65535 ? 65535 : (N < 1 ? 1 : N))), b(kGradThreads);
  switch (k) {
#define OMB_BG(KV) \
  case KV: hipLaunchKernelGGL(ehvi_boxes_grad_kernel<KV>, g, b, shm, stream, mu, var, ld, N, coords, C, boxes, B, dadm, dadv); break;
    OMB_BG(2) OMB_BG(3) OMB_BG(4) OMB_BG(5) OMB_BG(6) OMB_BG(7) OMB_BG(8)
#undef OMB_BG
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace omb
