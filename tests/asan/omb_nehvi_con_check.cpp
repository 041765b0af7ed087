// Stand-alone driver (ASan + UBSan, CPU only) of omb_hvi_paths_con / omb_plan_hvi_paths_con's argument checks
// (check_hvi_paths_con in omb_host.cpp), return codes against the header's contract, in its order: omb_hvi_paths' own
// refusals in its order (a null out is none of them here); then OMB_EINVAL for n_con < 0, eta negative or not finite,
// flag bits other than OMB_CON_VIOLATION, that flag with eta > 0, out and u both null with N > 0, u off its 8-byte
// alignment; then OMB_EUNSUP for k + n_con > OMB_MAX_OBJ (the sum in 64 bits); N = 0 passes.  Wherever the added
// arguments are in order and out is set, the code is check_hvi_paths' own.  The offsets live in a heap array of exactly
// S + 1 ints, so a check that reads past it is a sanitizer report.
// Built by `make -C optimobo_amd/csrc asan` as build/asan/omb_nehvi_con_check.
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

static void sweep() {
  std::string err;
  alignas(16) static char buf[32];
  const void* ptrs[] = {nullptr, buf, buf + 4};   // null, aligned, off by 4
  const int ks[] = {0, 1, 2, OMB_MAX_OBJ, INT_MAX};
  const int Ss[] = {0, 1, 3, kPathsMaxS, kPathsMaxS + 1};
  const int Cs[] = {1, 2};
  const int64_t Ns[] = {-1, 0, 33};
  const int64_t lds[] = {32, 33};
  const int cons[] = {INT_MIN, -1, 0, OMB_MAX_OBJ - 1, OMB_MAX_OBJ, INT_MAX};
  const double etas[] = {0.0, -0.0, 0.5, -1e-300, INFINITY, NAN, 1.7976931348623157e308};
  const unsigned flagss[] = {0u, OMB_CON_VIOLATION, 2u, 3u, 0x80000000u};
  for (int S : Ss) {
    const int n_off = (S >= 1 && S <= kPathsMaxS) ? S + 1 : 1;
    int32_t* good = new int32_t[n_off];
    int32_t* empty = new int32_t[n_off];
    for (int s = 0; s < n_off; ++s) {
      good[s] = 2 * s;
      empty[s] = s ? 2 * s - 2 : 0;   // list 0 is empty
    }
    for (int k : ks)
      for (int C : Cs)
        for (int64_t N : Ns)
          for (int64_t ld : lds)
            for (int oi = 0; oi < 3; ++oi)
              for (int mask = 0; mask < 27; ++mask) {
                const int iy = mask % 3, io = (mask / 3) % 3, iu = mask / 9;
                const void *y = ptrs[iy], *out = ptrs[io], *u = ptrs[iu];
                const int32_t* off = oi == 0 ? good : (oi == 1 ? empty : nullptr);
                // omb_hvi_paths' own answer, out's absence aside
                const int base = check_hvi_paths(nullptr, k, S, y, ld, N, buf, C, off, buf, io == 0 ? buf : out);
                for (int n_con : cons)
                  for (double eta : etas)
                    for (unsigned flags : flagss) {
                      int want = base;
                      if (want == OMB_OK) {
                        if (n_con < 0) want = OMB_EINVAL;
                        else if (!(eta >= 0.0) || isinf(eta)) want = OMB_EINVAL;
                        else if (flags & ~OMB_CON_VIOLATION) want = OMB_EINVAL;
                        else if ((flags & OMB_CON_VIOLATION) && eta > 0.0) want = OMB_EINVAL;
                        else if (N > 0 && io == 0 && iu == 0) want = OMB_EINVAL;
                        else if (iu == 2) want = OMB_EINVAL;
                        else if ((long long)k + n_con > OMB_MAX_OBJ) want = OMB_EUNSUP;
                      }
                      err.clear();
                      expect(check_hvi_paths_con(&err, k, S, n_con, y, ld, N, buf, C, off, buf, eta, flags, out, u), want,
                             "check_hvi_paths_con");
                      expect(check_hvi_paths_con(nullptr, k, S, n_con, y, ld, N, buf, C, off, buf, eta, flags, out, u),
                             want, "check_hvi_paths_con (no message)");
                      if (want != OMB_OK && err.empty()) {
                        ++bad;
                        fprintf(stderr, "MISMATCH check_hvi_paths_con: failure without a message\n");
                      }
                      // with nothing added and out set: check_hvi_paths' code
                      if (n_con == 0 && eta == 0.0 && flags == 0u && iu == 0 && io != 0)
                        expect(check_hvi_paths_con(nullptr, k, S, 0, y, ld, N, buf, C, off, buf, 0.0, 0u, out, nullptr),
                               check_hvi_paths(nullptr, k, S, y, ld, N, buf, C, off, buf, out), "n_con = 0");
                    }
              }
    delete[] good;
    delete[] empty;
  }
}

// the order itself: each refusal with everything after it in the header's order wrong as well
static void order() {
  alignas(16) static char buf[32];
  const int32_t off[] = {0, 1, 2, 3};
  const void *al = buf, *off4 = buf + 4;
  const double nan = NAN;
  auto call = [&](int k, int C, int n_con, double eta, unsigned flags, const void* out, const void* u) {
    return check_hvi_paths_con(nullptr, k, 3, n_con, al, 8, 8, al, C, off, al, eta, flags, out, u);
  };
  expect(call(0, 1, -1, nan, 2u, nullptr, off4), OMB_EINVAL, "k first");
  expect(call(2, 1, -1, nan, 2u, nullptr, off4), OMB_EUNSUP, "omb_hvi_paths' OMB_EUNSUP before the added checks");
  expect(call(2, 4, -1, nan, 2u, nullptr, off4), OMB_EINVAL, "n_con");
  expect(call(2, 4, 7, -1.0, 2u, nullptr, off4), OMB_EINVAL, "eta before the slot count");
  expect(call(2, 4, 7, 0.0, 2u, nullptr, off4), OMB_EINVAL, "flags before the slot count");
  expect(call(2, 4, 7, 0.5, 1u, nullptr, off4), OMB_EINVAL, "violation with eta > 0");
  expect(call(2, 4, 7, 0.0, 1u, nullptr, nullptr), OMB_EINVAL, "both outputs null");
  expect(call(2, 4, 7, 0.0, 1u, al, off4), OMB_EINVAL, "misaligned u");
  expect(call(2, 4, 7, 0.0, 1u, off4, al), OMB_EINVAL, "misaligned out");
  expect(call(2, 4, 7, 0.0, 1u, al, al), OMB_EUNSUP, "k + n_con = 9");
  expect(call(2, 4, 6, 0.0, 1u, nullptr, al), OMB_OK, "u alone");
  expect(call(2, 4, 6, 0.5, 0u, al, nullptr), OMB_OK, "out alone");
  expect(call(1, 4, 7, 0.0, 0u, al, al), OMB_OK, "k = 1, n_con = 7");
  // the plan entry's form: no device pointers, N = 0
  expect(check_hvi_paths_con(nullptr, 2, 3, 1, nullptr, 0, 0, al, 4, off, al, 0.0, 0u, nullptr, nullptr), OMB_OK, "plan");
}

int main() {
  sweep();
  order();
  printf("omb_nehvi_con_check: %ld calls, %ld mismatches\n", calls, bad);
  return bad ? 1 : 0;
}
