// Timing of the blocked Cholesky (launch_cholesky_mode: chol_diag_blk / chol_panel / chol_update kernels, and the
// persistent launch) on an SPD matrix (tools only; not part of the library).  Correctness is tests/test_gpu_turbo.py.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/ablate/ablate_chol tools/ablate/ablate_chol.hip \
//          -lrocsolver -lrocblas
// Run on the GPU box: ./tools/ablate/ablate_chol [N ...]
// The per-step launches (kCholSteps), the same with release / acquire hand-offs, and the persistent launch
// (kCholPersistent), interleaved, with the per-wave phase trace of the blocked diagonal factor; rocsolver_dpotrf on
// the same matrices as a stated reference rate (not a dependency).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

__device__ unsigned long long g_btrace[4][16];
__device__ int64_t g_btrace_r0 = 0;        // chol64_blocked calls traced: the block at this r0
#define OMB_CHOL_BTRACE(w, id, cond)                                                                   \
  do {                                                                                                 \
    if ((cond) && r0 == g_btrace_r0) g_btrace[w][id] = __builtin_readcyclecounter();                  \
  } while (0)
// step-level stamps (100 MHz constant clock) of steps g_strace_step and g_strace_step + 1:
// 0 WG0 start, 1 WG0 factor done, 2 W published, 3 WG1 start, 4 WG(1,0) waits, 5 flag seen, 6 panel done
__device__ int g_strace_step = -1;
__device__ unsigned long long g_strace[2][8];
#define OMB_CHOL_STRACE(step, id, cond)                                                                \
  do {                                                                                                 \
    if ((cond) && (step == g_strace_step || step == g_strace_step + 1))                               \
      g_strace[step - g_strace_step][id] = __builtin_amdgcn_s_memrealtime();                            \
  } while (0)

#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#define OMB_TOOLS_KNOBS
#include "../../optimobo_amd/csrc/omb_linalg.hip"
#include "../../optimobo_amd/csrc/omb_wide.hip"
#include "../../optimobo_amd/csrc/omb_gemm.hip"

using namespace omb;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1);} } while (0)

static void* g_strace_ptr() {
  void* p = nullptr;
  CK(hipGetSymbolAddress(&p, HIP_SYMBOL(g_strace)));
  return p;
}

// per-wave phases of the blocked diagonal factor (chol_diag_blk_kernel, alone on the GPU)
static void trace_diag_blocked() {
  const int N = 64;
  std::vector<double> h(N * N);
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) h[i * N + j] = (i == j) ? N : 1.0 / (1.0 + std::abs((double)(i - j)));
  double *A, *ws;
  int* info;
  CK(hipMalloc(&A, N * N * 8));
  CK(hipMalloc(&ws, chol_ws_doubles(N) * 8));
  CK(hipMalloc(&info, 64));
  unsigned long long t0[4][16];
  for (int rep = 0; rep < 3; ++rep) {
    CK(hipMemcpy(A, h.data(), N * N * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(chol_diag_blk_kernel, dim3(1), dim3(256), 0, 0, A, (int64_t)N, (int64_t)N, ws, info,
                       reinterpret_cast<int*>(ws + kCholWsDoubles), 0);
    CK(hipDeviceSynchronize());
    CK(hipMemcpyFromSymbol(t0, HIP_SYMBOL(g_btrace), sizeof(t0)));
  }
  unsigned long long base = t0[0][0];
  for (int w = 0; w < 4; ++w) base = std::min(base, t0[w][0]);
  const char* names[14] = {"start", "D tiles", "P0 wait", "P0/U0", "P1 wait", "P1/U1", "P2 wait", "P2/U2",
                           "F begin", "F end", "W_ww post", "W_1w", "W_2w", "W_3w"};
  printf("chol_diag_blk_kernel per-wave phases (cycles from the first wave's start)\n");
  for (int w = 0; w < 4; ++w) {
    printf("  wave %d:", w);
    for (int id = 0; id < 14; ++id) {
      const bool used = (id < 2) || (id >= 2 && id < 8 && (id - 2) / 2 < w) || (id >= 8 && id <= 10) ||
                        (id >= 11 && id - 10 > w);
      if (used) printf(" %s %lld |", names[id], (long long)(t0[w][id] - base));
    }
    printf("\n");
  }
  std::vector<double> L(N * N);
  CK(hipMemcpy(L.data(), A, N * N * 8, hipMemcpyDeviceToHost));
  double worst = 0.0;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = 0.0;
      for (int k = 0; k <= j; ++k) s += L[i * N + k] * L[j * N + k];
      worst = std::max(worst, std::abs(s - h[i * N + j]) / std::abs(h[i * N + i]));
    }
  printf("  blocked 64x64: max |LLt - A|/A_ii %.2e\n", worst);
  CK(hipFree(A)); CK(hipFree(ws)); CK(hipFree(info));
}

static void time_rocsolver(const std::vector<int64_t>& sizes) {
  rocblas_handle handle;
  if (rocblas_create_handle(&handle) != rocblas_status_success) {
    printf("rocblas_create_handle failed\n");
    return;
  }
  for (int64_t N : sizes) {
    std::vector<double> h(N * N);
    for (int64_t i = 0; i < N; ++i)
      for (int64_t j = 0; j < N; ++j) h[i * N + j] = (i == j) ? N : 1.0 / (1.0 + std::abs((double)(i - j)));
    double *A0, *A;
    int* info;
    CK(hipMalloc(&A0, N * N * 8));
    CK(hipMalloc(&A, N * N * 8));
    CK(hipMalloc(&info, 64));
    CK(hipMemcpy(A0, h.data(), N * N * 8, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    float sum = 0.f, best = 1e30f;
    const int reps = 10;
    for (int r = 0; r < reps + 2; ++r) {
      CK(hipMemcpy(A, A0, N * N * 8, hipMemcpyDeviceToDevice));
      CK(hipDeviceSynchronize());
      CK(hipEventRecord(e0));
      // row-major lower = column-major upper
      rocblas_status st = rocsolver_dpotrf(handle, rocblas_fill_upper, (rocblas_int)N, A, (rocblas_int)N, info);
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      if (st != rocblas_status_success) printf("rocsolver_dpotrf status %d\n", (int)st);
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (r >= 2) {
        sum += ms;
        best = std::min(best, ms);
      }
    }
    int hinfo = -1;
    CK(hipMemcpy(&hinfo, info, 4, hipMemcpyDeviceToHost));
    printf("N=%lld  rocsolver_dpotrf %.3f ms (best %.3f)  info %d\n", (long long)N, sum / reps, best, hinfo);
    CK(hipFree(A0)); CK(hipFree(A)); CK(hipFree(info));
  }
  rocblas_destroy_handle(handle);
}

// one blocked factorisation at N with the step-level stamps and the diagonal phases of step `st`
static void trace_steps(int64_t N, int st) {
  std::vector<double> h(N * N);
  for (int64_t i = 0; i < N; ++i)
    for (int64_t j = 0; j < N; ++j) h[i * N + j] = (i == j) ? N : 1.0 / (1.0 + std::abs((double)(i - j)));
  double *A, *ws;
  int* info;
  CK(hipMalloc(&A, N * N * 8));
  CK(hipMalloc(&ws, chol_ws_doubles(N) * 8));
  CK(hipMalloc(&info, 64));
  const int64_t r0 = (int64_t)(st + 1) * 64;
  CK(hipMemcpyToSymbol(HIP_SYMBOL(g_strace_step), &st, sizeof(int)));
  CK(hipMemcpyToSymbol(HIP_SYMBOL(g_btrace_r0), &r0, sizeof(int64_t)));
  unsigned long long t[2][8], b[4][16];
  for (int rep = 0; rep < 3; ++rep) {
    CK(hipMemcpy(A, h.data(), N * N * 8, hipMemcpyHostToDevice));
    CK(hipMemset(g_strace_ptr(), 0, sizeof(t)));
    CK(launch_cholesky_mode(0, A, N, N, info, ws, kCholSteps));
    CK(hipDeviceSynchronize());
  }
  CK(hipMemcpyFromSymbol(t, HIP_SYMBOL(g_strace), sizeof(t)));
  CK(hipMemcpyFromSymbol(b, HIP_SYMBOL(g_btrace), sizeof(b)));
  const char* nm[7] = {"WG0 start", "WG0 factored", "W published", "WG1 start", "WG(1,0) waits", "flag seen",
                       "panel done"};
  printf("N=%lld step %d (blocked): stamps in us from WG0's start (100 MHz clock)\n", (long long)N, st);
  for (int k = 0; k < 2; ++k) {
    printf("  step %d:", st + k);
    for (int id = 0; id < 7; ++id)
      if (t[k][id]) printf(" %s %.2f |", nm[id], ((long long)t[k][id] - (long long)t[0][0]) / 100.0);
    printf("\n");
  }
  unsigned long long base = b[0][0];
  for (int w = 0; w < 4; ++w) base = std::min(base, b[w][0]);
  printf("  its diagonal block (cycles from the first wave's start):\n");
  for (int w = 0; w < 4; ++w) {
    printf("    wave %d: tiles %lld | F %lld-%lld | post %lld\n", w, (long long)(b[w][1] - base),
           (long long)(b[w][8] - base), (long long)(b[w][9] - base), (long long)(b[w][10] - base));
  }
  CK(hipFree(A)); CK(hipFree(ws)); CK(hipFree(info));
  const int64_t none = -1;
  CK(hipMemcpyToSymbol(HIP_SYMBOL(g_btrace_r0), &none, sizeof(int64_t)));
  const int nostep = -1;
  CK(hipMemcpyToSymbol(HIP_SYMBOL(g_strace_step), &nostep, sizeof(int)));
}

int main(int argc, char** argv) {
  setvbuf(stdout, nullptr, _IOLBF, 0);
  trace_diag_blocked();
  trace_steps(3000, 20);
  trace_steps(3000, 2);
  std::vector<int64_t> sizes;
  for (int i = 1; i < argc; ++i) sizes.push_back(atoll(argv[i]));
  if (sizes.empty()) sizes = {512, 1024, 3000};
  for (int64_t N : sizes) {
    std::vector<double> h(N * N);
    for (int64_t i = 0; i < N; ++i)
      for (int64_t j = 0; j < N; ++j) h[i * N + j] = (i == j) ? N : 1.0 / (1.0 + std::abs((double)(i - j)));
    double *A0, *A, *ws;
    int* info;
    CK(hipMalloc(&A0, N * N * 8));
    CK(hipMalloc(&A, N * N * 8));
    CK(hipMalloc(&ws, chol_ws_doubles(N) * 8));
    CK(hipMalloc(&info, 64));
    CK(hipMemcpy(A0, h.data(), N * N * 8, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    // the launch schedules interleaved: the per-step launches, the same with the agent-scope release / acquire flag,
    // the persistent launch
    const int modes[3] = {kCholSteps, kCholSteps, kCholPersistent};
    const int acq_rel[3] = {0, 1, 0};
    float msum[3] = {0, 0, 0}, mbest[3] = {1e30f, 1e30f, 1e30f};
    const int reps = 10;
    std::vector<double> Lref(N * N), Lm(N * N);
    double mdiff[3] = {0, 0, 0};
    int minfo[3] = {0, 0, 0};
    for (int r = 0; r < reps + 1; ++r) {
      for (int m = 0; m < 3; ++m) {
        CK(hipMemcpy(A, A0, N * N * 8, hipMemcpyDeviceToDevice));
        CK(hipMemset(info, 0, 4));
        CK(hipEventRecord(e0));
        CK(launch_cholesky_mode(0, A, N, N, info, ws, modes[m], kDefaultSpinLimit, acq_rel[m]));
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (r > 0) {
          msum[m] += ms;
          mbest[m] = std::min(mbest[m], ms);
        } else {
          CK(hipMemcpy(m == 0 ? Lref.data() : Lm.data(), A, N * N * 8, hipMemcpyDeviceToHost));
          CK(hipMemcpy(&minfo[m], info, 4, hipMemcpyDeviceToHost));
          if (m > 0)
            for (int64_t i = 0; i < N; ++i)
              for (int64_t j = 0; j <= i; ++j)
                mdiff[m] = std::max(mdiff[m], std::abs(Lm[i * N + j] - Lref[i * N + j]) / std::sqrt(h[i * N + i]));
        }
      }
    }
    printf("N=%lld  per-step %.3f (best %.3f) | per-step acq/rel %.3f (%.3f) | persistent %.3f (%.3f) ms; info %d %d %d; "
           "max |L - L_steps|/sqrt(A_ii) %.1e %.1e\n",
           (long long)N, msum[0] / reps, mbest[0], msum[1] / reps, mbest[1], msum[2] / reps, mbest[2], minfo[0],
           minfo[1], minfo[2], mdiff[1], mdiff[2]);
    {
      // the non-diagonal workgroups of each per-step launch start after delay × ≈ 0.85 µs
      const int delays[5] = {0, 1, 2, 4, 6};
      float sx[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
      for (int r = 0; r < reps + 1; ++r)
        for (int v = 0; v < 5; ++v) {
          set_chol_update_delay(delays[v]);
          CK(hipMemcpy(A, A0, N * N * 8, hipMemcpyDeviceToDevice));
          CK(hipEventRecord(e0));
          CK(launch_cholesky_mode(0, A, N, N, info, ws, kCholSteps));
          CK(hipEventRecord(e1));
          CK(hipEventSynchronize(e1));
          float ms;
          CK(hipEventElapsedTime(&ms, e0, e1));
          if (r > 0) sx[v] += ms;
        }
      set_chol_update_delay(0);
      printf("N=%lld  blocked, other workgroups delayed by 0 / 0.85 / 1.7 / 3.4 / 5.1 us: %.3f / %.3f / %.3f / %.3f / %.3f ms\n",
             (long long)N, sx[0] / reps, sx[1] / reps, sx[2] / reps, sx[3] / reps, sx[4] / reps);
    }
    // the same launch sequence captured once into a hipGraph and replayed (launch-gap ablation)
    float gbest = 1e30f, gsum = 0.f;
    {
      hipStream_t s;
      CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      hipGraph_t graph;
      hipGraphExec_t exec;
      CK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      CK(launch_cholesky_mode(s, A, N, N, info, ws, kCholPersistent));
      CK(hipStreamEndCapture(s, &graph));
      CK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
      for (int r = 0; r < reps + 1; ++r) {
        CK(hipMemcpyAsync(A, A0, N * N * 8, hipMemcpyDeviceToDevice, s));
        CK(hipMemsetAsync(info, 0, 4, s));
        CK(hipEventRecord(e0, s));
        CK(hipGraphLaunch(exec, s));
        CK(hipEventRecord(e1, s));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (r > 0) {
          gbest = ms < gbest ? ms : gbest;
          gsum += ms;
        }
      }
      CK(hipStreamSynchronize(s));
      CK(hipGraphExecDestroy(exec));
      CK(hipGraphDestroy(graph));
      CK(hipStreamDestroy(s));
    }
    printf("N=%lld  hipGraph replay %.3f ms (best %.3f)\n", (long long)N, gsum / reps, gbest);
    int hinfo = -1;
    CK(hipMemcpy(&hinfo, info, 4, hipMemcpyDeviceToHost));
    // residual spot check on a few entries: (L Lᵀ)[i][j] vs A[i][j]
    std::vector<double> L(N * N);
    CK(hipMemcpy(L.data(), A, N * N * 8, hipMemcpyDeviceToHost));
    double worst = 0.0;
    for (int t = 0; t < 200; ++t) {
      const int64_t i = (t * 7919) % N, j = (t * 104729) % (i + 1);
      double s = 0.0;
      for (int64_t k = 0; k <= j; ++k) s += L[i * N + k] * L[j * N + k];
      worst = std::max(worst, std::abs(s - h[i * N + j]) / std::abs(h[i * N + i]));
    }
    // the library's default schedule after the loops above: the residual of the persistent launch's factor
    printf("N=%lld  Cholesky (persistent) %.3f ms (best %.3f, %d steps = %.1f us/step)  info %d  max |LLt - A|/A_ii %.2e\n",
           (long long)N, msum[2] / reps, mbest[2], (int)((N + 63) / 64), mbest[2] * 1e3 / ((N + 63) / 64), hinfo, worst);
    CK(hipFree(A0)); CK(hipFree(A)); CK(hipFree(ws)); CK(hipFree(info));
  }
  time_rocsolver(sizes);
  return 0;
}
