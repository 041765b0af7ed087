// Stand-alone driver (ASan + UBSan, CPU only) of the sample paths' host side (omb_host.cpp): check_paths_set and
// check_paths_eval swept over the edge values of every argument, return codes against the header's contract, in its
// order — OMB_EINVAL (obj / n_obj, S, m outside their ranges; a null pointer; noise negative or not finite; N < 0;
// ld < N), then OMB_ESTATE (an objective without a GP, without paths, or with another S than objective 0), then
// OMB_EUNSUP (n_var > 64, n_train > OMB_MAX_TRAIN_DENSE) — and paths_pack into exactly-sized heap buffers at the tile
// edges of m, d and S, every element against the layout the header states.
// Built by `make -C optimobo_amd/csrc asan` as build/asan/omb_paths_check.
#include <limits.h>
#include <math.h>
#include <stdio.h>

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

static void sweep_set() {
  std::string err;
  static double buf[2];
  const void* ptrs[] = {nullptr, buf};
  const int objs[] = {INT_MIN, -1, 0, OMB_MAX_OBJ - 1, OMB_MAX_OBJ, INT_MAX};
  const int Ss[] = {INT_MIN, -1, 0, 1, 3, 16, 17, INT_MAX};
  const int ms[] = {INT_MIN, -1, 0, 1, 17, 65536, 65537, INT_MAX};
  const double noises[] = {-INFINITY, -1.0, -0.0, 0.0, 1e-4, 1.79769313486231570815e308, INFINITY, NAN};
  const int sets[] = {0, 1};
  const int dims[] = {1, 64, 65, OMB_MAX_DIM};
  const int ns[] = {1, OMB_MAX_TRAIN_DENSE, OMB_MAX_TRAIN_DENSE + 1, INT_MAX};
  for (int obj : objs)
    for (int S : Ss)
      for (int m : ms)
        for (double noise : noises)
          for (int mask = 0; mask < 8; ++mask)
            for (int set : sets)
              for (int d : dims)
                for (int n : ns) {
                  const void *om = ptrs[mask & 1], *ph = ptrs[(mask >> 1) & 1], *w = ptrs[(mask >> 2) & 1];
                  const PathsObjInfo info{set, d, n, 0};
                  int want = OMB_OK;
                  if (obj < 0 || obj >= OMB_MAX_OBJ || S < 1 || S > 16 || m < 1 || m > 65536) want = OMB_EINVAL;
                  else if (mask != 7) want = OMB_EINVAL;
                  else if (!(noise >= 0.0) || isinf(noise)) want = OMB_EINVAL;
                  else if (!set) want = OMB_ESTATE;
                  else if (d > 64 || n > OMB_MAX_TRAIN_DENSE) want = OMB_EUNSUP;
                  err.clear();
                  expect(check_paths_set(&err, obj, S, m, om, ph, w, noise, &info), want, "check_paths_set");
                  expect(check_paths_set(nullptr, obj, S, m, om, ph, w, noise, &info), want,
                         "check_paths_set (no message)");
                  if (want != OMB_OK && err.empty()) {
                    ++bad;
                    fprintf(stderr, "MISMATCH check_paths_set: failure without a message\n");
                  }
                }
  const PathsObjInfo ok{1, 2, 10, 0};
  expect(check_paths_set(&err, 0, 1, 1, buf, buf, buf, 0.0, nullptr), OMB_EINVAL, "check_paths_set (no state)");
  expect(check_paths_set(&err, 0, 1, 1, buf, buf, buf, 0.0, &ok), OMB_OK, "check_paths_set (plain)");
}

static void sweep_eval() {
  std::string err;
  static double buf[2];
  const void* ptrs[] = {nullptr, buf};
  const int n_objs[] = {INT_MIN, -1, 0, 1, 2, OMB_MAX_OBJ, OMB_MAX_OBJ + 1, INT_MAX};
  const int64_t Ns[] = {INT64_MIN, -1, 0, 1, 17, INT64_MAX};
  const int64_t lds[] = {INT64_MIN, -1, 0, 1, 16, 17, 20, INT64_MAX};
  // the last objective of the call: {set, S}, objective 0 holding 3 paths
  const int states[][2] = {{0, 0}, {0, 3}, {1, 0}, {1, -1}, {1, 3}, {1, 4}, {1, 16}};
  const int dims[] = {1, 64, 65};
  const int ns[] = {1, OMB_MAX_TRAIN_DENSE, OMB_MAX_TRAIN_DENSE + 1};
  for (int n_obj : n_objs)
    for (int64_t N : Ns)
      for (int64_t ld : lds)
        for (int mask = 0; mask < 4; ++mask)
          for (const auto& st : states)
            for (int d : dims)
              for (int n : ns) {
                const void *Xc = ptrs[mask & 1], *out = ptrs[(mask >> 1) & 1];
                PathsObjInfo info[OMB_MAX_OBJ];
                for (int o = 0; o < OMB_MAX_OBJ; ++o) info[o] = PathsObjInfo{1, 2, 10, 3};
                const bool in_range = n_obj >= 1 && n_obj <= OMB_MAX_OBJ;
                if (in_range) info[n_obj - 1] = PathsObjInfo{st[0], d, n, st[1]};
                int want = OMB_OK;
                if (!in_range || N < 0 || ld < N) want = OMB_EINVAL;
                else if (N > 0 && mask != 3) want = OMB_EINVAL;
                else if (!st[0] || st[1] < 1) want = OMB_ESTATE;
                else if (n_obj > 1 && st[1] != 3) want = OMB_ESTATE;
                else if (d > 64 || n > OMB_MAX_TRAIN_DENSE) want = OMB_EUNSUP;
                err.clear();
                expect(check_paths_eval(&err, n_obj, Xc, N, ld, out, info), want, "check_paths_eval");
                expect(check_paths_eval(nullptr, n_obj, Xc, N, ld, out, info), want, "check_paths_eval (no message)");
                if (want != OMB_OK && err.empty()) {
                  ++bad;
                  fprintf(stderr, "MISMATCH check_paths_eval: failure without a message\n");
                }
              }
  expect(check_paths_eval(&err, 1, buf, 1, 1, buf, nullptr), OMB_EINVAL, "check_paths_eval (no state)");
}

static void sweep_pack() {
  const int ms[] = {1, 4, 15, 16, 17, 33};
  const int ds[] = {1, 2, 3, 6, 8, 9, 30, 64};
  const int Ss[] = {1, 3, 16};
  for (int m : ms)
    for (int d : ds)
      for (int S : Ss) {
        const int DP = pad_dim(d), ksf = paths_ksf(DP);
        expect(4 * ksf > d, 1, "paths_ksf covers [x, 1]");
        std::vector<double> om((size_t)m * d), ph(m), w((size_t)m * S);
        for (size_t i = 0; i < om.size(); ++i) om[i] = 1.0 + (double)i;
        for (int i = 0; i < m; ++i) ph[i] = -1.0 - i;
        for (size_t i = 0; i < w.size(); ++i) w[i] = 0.5 + (double)i;
        std::vector<double> Of((size_t)paths_of_doubles(m, DP), NAN), Wf((size_t)paths_wf_doubles(m), NAN);
        paths_pack(m, d, DP, S, om.data(), ph.data(), w.data(), 2.0, Of.data(), Wf.data());
        const int MT = (m + 15) / 16;
        long wrong = 0;
        for (int T = 0; T < MT; ++T) {
          for (int s = 0; s < ksf; ++s)
            for (int l = 0; l < 64; ++l) {
              const int i = 16 * T + (l & 15), j = 4 * s + (l >> 4);
              const double want = i >= m ? 0.0 : (j < d ? om[(size_t)i * d + j] : (j == d ? ph[i] : 0.0));
              wrong += Of[((size_t)T * ksf + s) * 64 + l] != want;
            }
          for (int e = 0; e < 4; ++e)
            for (int l = 0; l < 64; ++l) {
              const int i = 16 * T + 4 * e + (l >> 4), p = l & 15;
              const double want = (i < m && p < S) ? 2.0 * w[(size_t)i * S + p] : 0.0;
              wrong += Wf[((size_t)4 * T + e) * 64 + l] != want;
            }
        }
        expect(wrong, 0, "paths_pack layout");
      }
}

int main() {
  sweep_set();
  sweep_eval();
  sweep_pack();
  printf("omb_paths_check: %ld calls, %ld mismatches\n", calls, bad);
  return bad ? 1 : 0;
}
