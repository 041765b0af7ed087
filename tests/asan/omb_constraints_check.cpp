// Stand-alone driver (ASan + UBSan, CPU only) of the constraint entry points' argument checks in omb_host.cpp:
// check_constraints (omb_plan_constraints) and check_feasibility (omb_feasibility) swept over their boundary values,
// return codes against the header's contract — check_constraints: OMB_ESTATE with no plan, then OMB_EINVAL for
// n_con < 0 or a negative / non-finite pof_eps, then OMB_EUNSUP for plan_k + n_con > OMB_MAX_OBJ (the sum in 64 bits:
// INT_MAX + INT_MAX in int would be a sanitizer report); check_feasibility: OMB_EINVAL for c outside
// [1, OMB_MAX_OBJ], a bad pof_eps, N < 0, a null pointer with N > 0, or ld < N with c > 1.
// Built by `make -C optimobo_amd/csrc asan` as build/asan/omb_constraints_check.
#include <limits.h>
#include <math.h>
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
  const double epss[] = {-INFINITY, -1.0, -1e-300, -0.0, 0.0, 4.9e-324, 1e-5, 1.0, 1.7976931348623157e308, INFINITY, NAN};
  const int ks[] = {INT_MIN, -1, 0, 1, 2, OMB_MAX_OBJ - 1, OMB_MAX_OBJ, OMB_MAX_OBJ + 1, INT_MAX};
  const int cons[] = {INT_MIN, -1, 0, 1, 2, OMB_MAX_OBJ - 2, OMB_MAX_OBJ - 1, OMB_MAX_OBJ, OMB_MAX_OBJ + 1, INT_MAX};
  for (int k : ks)
    for (int n_con : cons)
      for (double eps : epss) {
        const bool eps_ok = eps >= 0.0 && eps <= 1.7976931348623157e308;   // false for NaN
        int want = OMB_OK;
        if (k < 1) want = OMB_ESTATE;
        else if (n_con < 0 || !eps_ok) want = OMB_EINVAL;
        else if ((long long)k + n_con > OMB_MAX_OBJ) want = OMB_EUNSUP;
        err.clear();
        expect(check_constraints(&err, k, n_con, eps), want, "check_constraints");
        expect(check_constraints(nullptr, k, n_con, eps), want, "check_constraints (no message)");
        if (want != OMB_OK && err.empty()) {
          ++bad;
          fprintf(stderr, "MISMATCH check_constraints: failure without a message\n");
        }
      }
  double x = 0.0;
  const void* ptrs[] = {nullptr, &x};
  const int64_t Ns[] = {INT64_MIN, -1, 0, 1, 33, INT_MAX, INT64_MAX};
  const int64_t lds[] = {INT64_MIN, -1, 0, 1, 32, 33, INT64_MAX};
  for (int c : cons)
    for (double eps : epss)
      for (int64_t N : Ns)
        for (int64_t ld : lds)
          for (int mask = 0; mask < 8; ++mask) {
            const void* mu = ptrs[mask & 1];
            const void* var = ptrs[(mask >> 1) & 1];
            const void* out = ptrs[(mask >> 2) & 1];
            const bool eps_ok = eps >= 0.0 && eps <= 1.7976931348623157e308;
            int want = OMB_OK;
            if (c < 1 || c > OMB_MAX_OBJ || !eps_ok || N < 0) want = OMB_EINVAL;
            else if (N > 0 && mask != 7) want = OMB_EINVAL;
            else if (c > 1 && ld < N) want = OMB_EINVAL;
            expect(check_feasibility(&err, c, mu, var, ld, N, eps, out), want, "check_feasibility");
            expect(check_feasibility(nullptr, c, mu, var, ld, N, eps, out), want, "check_feasibility (no message)");
          }
  printf("omb_constraints_check: %ld calls, %ld mismatches\n", calls, bad);
  return bad ? 1 : 0;
}
