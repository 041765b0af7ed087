// Stand-alone driver (ASan + UBSan, CPU only) of the gradient entry points' argument checks in omb_host.cpp:
// check_posterior_grad and check_eval_grad with hostile sizes and null pointers (return codes against the header's
// contract: n_obj out of range, N < 0 and null pointers are OMB_EINVAL; N = 0 passes with any pointers), and
// grad_chunk's workspace arithmetic at the largest sizes (a 32-bit product or a zero divisor is a sanitizer report).
// Built by `make -C optimobo_amd/csrc asan` as build/asan/omb_grad_check.
#include <limits.h>
#include <stdio.h>

#include <string>

#include "../../optimobo_amd/csrc/omb_host.h"

using namespace omb;

static long calls = 0, bad = 0;

static void expect(long long got, long long want, const char* what) {
  ++calls;
  if (got != want) {
    ++bad;
    fprintf(stderr, "MISMATCH %s: got %lld want %lld\n", what, got, want);
  }
}

int main() {
  std::string err;
  double x = 0.0;
  const void* ptrs[] = {nullptr, &x};
  const int objs[] = {INT_MIN, -1, 0, 1, 2, OMB_MAX_OBJ, OMB_MAX_OBJ + 1, INT_MAX};
  const int64_t Ns[] = {INT64_MIN, -1, 0, 1, 33, INT_MAX, INT64_MAX};
  for (int n_obj : objs)
    for (int64_t N : Ns)
      for (int mask = 0; mask < 32; ++mask) {
        const void* Xc = ptrs[mask & 1];
        const void* mu = ptrs[(mask >> 1) & 1];
        const void* var = ptrs[(mask >> 2) & 1];
        const void* dmu = ptrs[(mask >> 3) & 1];
        const void* dvar = ptrs[(mask >> 4) & 1];
        int want = OMB_OK;
        if (n_obj < 1 || n_obj > OMB_MAX_OBJ || N < 0) want = OMB_EINVAL;
        else if (N > 0 && mask != 31) want = OMB_EINVAL;
        expect(check_posterior_grad(&err, n_obj, Xc, N, mu, var, dmu, dvar), want, "check_posterior_grad");
        expect(check_posterior_grad(nullptr, n_obj, Xc, N, mu, var, dmu, dvar), want, "check_posterior_grad (no message)");
        if (want != OMB_OK && err.empty()) {
          ++bad;
          fprintf(stderr, "MISMATCH check_posterior_grad: failure without a message\n");
        }
      }
  for (int64_t N : Ns)
    for (int mask = 0; mask < 8; ++mask) {
      const void* Xc = ptrs[mask & 1];
      const void* vals = ptrs[(mask >> 1) & 1];
      const void* grad = ptrs[(mask >> 2) & 1];
      const int want = (N < 0 || (N > 0 && mask != 7)) ? OMB_EINVAL : OMB_OK;
      expect(check_eval_grad(&err, Xc, N, vals, grad), want, "check_eval_grad");
      expect(check_eval_grad(nullptr, Xc, N, vals, grad), want, "check_eval_grad (no message)");
    }
  // chunks: within [1, N], at most 2^20, at least min(N, 64), and the workspace they imply within 512 MiB unless the
  // floor of 64 candidates applies
  const int trains[] = {INT_MIN, 0, 1, 17, 1024, 1040, OMB_MAX_TRAIN_DENSE, INT_MAX};
  for (int n_obj : objs)
    for (int n : trains)
      for (int64_t N : Ns) {
        const int64_t nc = grad_chunk(n_obj, n, N);
        if (N <= 0 || n_obj < 1 || n_obj > OMB_MAX_OBJ || n < 1 || n > OMB_MAX_TRAIN_DENSE) {
          expect(nc, 0, "grad_chunk of an empty or out-of-range request");
          continue;
        }
        ++calls;
        const bool ok = nc >= 1 && nc <= N && nc <= (1 << 20) && (nc == N || nc >= 64) &&
                        (nc <= 64 || (__int128)nc * (n_obj + 2) * n * 8 <= ((__int128)512 << 20));
        if (!ok) {
          ++bad;
          fprintf(stderr, "MISMATCH grad_chunk(%d, %d, %lld) = %lld\n", n_obj, n, (long long)N, (long long)nc);
        }
      }
  printf("omb_grad_check: %ld calls, %ld mismatches\n", calls, bad);
  return bad ? 1 : 0;
}
