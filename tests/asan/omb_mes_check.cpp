// Stand-alone driver (ASan + UBSan, CPU only) of the max-value-entropy-search and path-minimum entry points' argument
// checks in omb_host.cpp: check_mes (omb_mes), check_plan_mes (omb_plan_mes) and check_paths_min (omb_paths_min) swept
// over their boundary values, return codes against the header's contract —
//   check_mes:       OMB_EINVAL for k outside [1, OMB_MAX_OBJ], then S outside [1, kMesMaxS], then N < 0, then (N > 0) a
//                    null mu / var / ystar / out, then ld < N with k > 1; N = 0 accepts null pointers;
//   check_plan_mes:  the same k and S ranges, then a null ystar, then a non-finite entry (read over exactly k·S
//                    doubles of a heap array: an index past it is ASan's to report);
//   check_paths_min: check_paths_eval's refusals in its order, without a pitch, res in out's place and never null.
// Built by `make -C optimobo_amd/csrc asan` as build/asan/omb_mes_check.
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

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
  const int ks[] = {INT_MIN, -1, 0, 1, 2, OMB_MAX_OBJ, OMB_MAX_OBJ + 1, INT_MAX};
  const int Ss[] = {INT_MIN, -1, 0, 1, 16, kMesMaxS, kMesMaxS + 1, INT_MAX};
  const int64_t Ns[] = {INT64_MIN, -1, 0, 1, 9, INT64_MAX};
  double dummy = 0.0;
  const void* P = &dummy;   // never dereferenced by the checks
  // ---- check_mes
  for (int k : ks)
    for (int S : Ss)
      for (int64_t N : Ns)
        for (int64_t ld : {(int64_t)INT64_MIN, (int64_t)-1, (int64_t)0, N > INT64_MIN ? N - 1 : N, N,
                           N < INT64_MAX - 3 ? N + 3 : N, (int64_t)INT64_MAX})
          for (int nulls = 0; nulls < 16; ++nulls) {
            const void* mu = (nulls & 1) ? nullptr : P;
            const void* var = (nulls & 2) ? nullptr : P;
            const void* ys = (nulls & 4) ? nullptr : P;
            const void* out = (nulls & 8) ? nullptr : P;
            int want = OMB_OK;
            if (k < 1 || k > OMB_MAX_OBJ) want = OMB_EINVAL;
            else if (S < 1 || S > kMesMaxS) want = OMB_EINVAL;
            else if (N < 0) want = OMB_EINVAL;
            else if (N > 0 && nulls) want = OMB_EINVAL;
            else if (k > 1 && ld < N) want = OMB_EINVAL;
            err.clear();
            expect(check_mes(&err, k, S, mu, var, ld, N, ys, out), want, "check_mes");
            expect(check_mes(nullptr, k, S, mu, var, ld, N, ys, out), want, "check_mes (no message)");
            if (want != OMB_OK && err.empty()) {
              ++bad;
              fprintf(stderr, "MISMATCH check_mes: failure without a message\n");
            }
          }
  // the order: k before S before N (each message names what failed first)
  check_mes(&err, 0, 0, nullptr, nullptr, 0, -1, nullptr, nullptr);
  expect(err.find("k=") != std::string::npos, 1, "check_mes names k first");
  check_mes(&err, 1, 0, nullptr, nullptr, 0, -1, nullptr, nullptr);
  expect(err.find("S=") != std::string::npos, 1, "check_mes names S second");
  check_mes(&err, 1, 1, nullptr, nullptr, 0, -1, nullptr, nullptr);
  expect(err.find("N=") != std::string::npos, 1, "check_mes names N third");
  // ---- check_plan_mes over exactly-sized heap arrays
  const double bads[] = {NAN, INFINITY, -INFINITY};
  for (int k : ks)
    for (int S : Ss) {
      const bool shape = k >= 1 && k <= OMB_MAX_OBJ && S >= 1 && S <= kMesMaxS;
      expect(check_plan_mes(&err, k, S, nullptr), OMB_EINVAL, "check_plan_mes (null)");
      if (!shape) {
        expect(check_plan_mes(&err, k, S, &dummy), OMB_EINVAL, "check_plan_mes (shape)");   // refused before it reads
        continue;
      }
      std::vector<double> y((size_t)k * S);
      for (size_t i = 0; i < y.size(); ++i) y[i] = (i % 3 == 0 ? -1.0 : 1.0) * 1.79769313486231570815e308 / (double)(i + 1);
      expect(check_plan_mes(&err, k, S, y.data()), OMB_OK, "check_plan_mes (finite, to the largest double)");
      expect(check_plan_mes(nullptr, k, S, y.data()), OMB_OK, "check_plan_mes (no message)");
      for (double b : bads)
        for (size_t at : {(size_t)0, y.size() / 2, y.size() - 1}) {
          const double keep = y[at];
          y[at] = b;
          err.clear();
          expect(check_plan_mes(&err, k, S, y.data()), OMB_EINVAL, "check_plan_mes (non-finite)");
          if (err.find("not finite") == std::string::npos) {
            ++bad;
            fprintf(stderr, "MISMATCH check_plan_mes: the message does not say what was wrong\n");
          }
          y[at] = keep;
        }
    }
  // ---- check_paths_min
  PathsObjInfo info[OMB_MAX_OBJ];
  const int nobjs[] = {INT_MIN, -1, 0, 1, 2, OMB_MAX_OBJ, OMB_MAX_OBJ + 1, INT_MAX};
  for (int state = 0; state < 6; ++state) {
    for (int o = 0; o < OMB_MAX_OBJ; ++o) info[o] = PathsObjInfo{1, 3, 17, 5};
    if (state == 1) info[1].set = 0;                          // objective 1 has no GP
    if (state == 2) info[1].S = 0;                            // … no paths
    if (state == 3) info[1].S = 3;                            // … another S
    if (state == 4) info[0].n_var = kPathsMaxDim + 1;         // too wide
    if (state == 5) info[1].n_train = OMB_MAX_TRAIN_DENSE + 1;
    for (int n_obj : nobjs)
      for (int64_t N : Ns)
        for (int nulls = 0; nulls < 8; ++nulls) {
          const void* Xc = (nulls & 1) ? nullptr : P;
          const void* res = (nulls & 2) ? nullptr : P;
          const PathsObjInfo* inf = (nulls & 4) ? nullptr : info;
          int want = OMB_OK;
          if (n_obj < 1 || n_obj > OMB_MAX_OBJ) want = OMB_EINVAL;
          else if (N < 0) want = OMB_EINVAL;
          else if (!res) want = OMB_EINVAL;
          else if (!inf || (N > 0 && !Xc)) want = OMB_EINVAL;
          else if (n_obj >= 2 && state >= 1 && state <= 3) want = OMB_ESTATE;
          else if (state == 4 || (state == 5 && n_obj >= 2)) want = OMB_EUNSUP;
          expect(check_paths_min(&err, n_obj, Xc, N, res, inf), want, "check_paths_min");
          expect(check_paths_min(nullptr, n_obj, Xc, N, res, inf), want, "check_paths_min (no message)");
          // with the same arguments and a pitch of N, omb_paths_eval refuses what this refuses (out = res)
          if (res || N > 0)
            expect(check_paths_eval(nullptr, n_obj, Xc, N, N, res, inf), want, "check_paths_eval against check_paths_min");
        }
  }
  printf("omb_mes_check: %ld calls, %ld mismatches\n", calls, bad);
  return bad ? 1 : 0;
}
