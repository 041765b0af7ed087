// Stand-alone driver (ASan + UBSan, CPU only) of omb_hvi_boxes' argument checks (check_hvi_boxes in omb_host.cpp)
// swept over the edge values of k, C, B, N, ld and the four pointers, return codes against the header's contract, in
// its order: OMB_EINVAL for k outside [2, OMB_MAX_OBJ], N < 0, B < 1, a null grid / box list, a null y / out with
// N > 0, a pointer off its alignment (8 bytes; the box list 4) or ld < N; then OMB_EUNSUP for C < 2, k·C > 8192 (the
// product in 64 bits: 8·INT_MAX in int would be a sanitizer report) or B > 2^24; N = 0 passes.
// Built by `make -C optimobo_amd/csrc asan` as build/asan/omb_hvi_check.
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
  alignas(16) static char buf[32];
  // per pointer: null, aligned, off by 4 (misaligned for doubles, fine for the box list), off by 2
  const void* ptrs[] = {nullptr, buf, buf + 4, buf + 2};
  const int ks[] = {INT_MIN, -1, 0, 1, 2, 3, OMB_MAX_OBJ, OMB_MAX_OBJ + 1, INT_MAX};
  const int Cs[] = {INT_MIN, -1, 0, 1, 2, 1024, 1025, 2730, 2731, 4096, 4097, INT_MAX};
  const int64_t Bs[] = {INT64_MIN, -1, 0, 1, 1 << 24, (1 << 24) + 1, INT_MAX, INT64_MAX};
  const int64_t Ns[] = {INT64_MIN, -1, 0, 1, 33, INT64_MAX};
  const int64_t lds[] = {INT64_MIN, -1, 0, 1, 32, 33, INT64_MAX};
  for (int k : ks)
    for (int C : Cs)
      for (int64_t B : Bs)
        for (int64_t N : Ns)
          for (int64_t ld : lds)
            for (int mask = 0; mask < 256; ++mask) {
              const int iy = mask & 3, ic = (mask >> 2) & 3, ib = (mask >> 4) & 3, io = (mask >> 6) & 3;
              const void *y = ptrs[iy], *coords = ptrs[ic], *boxes = ptrs[ib], *out = ptrs[io];
              int want = OMB_OK;
              if (k < 2 || k > OMB_MAX_OBJ || N < 0 || B < 1) want = OMB_EINVAL;
              else if (ic == 0 || ib == 0) want = OMB_EINVAL;
              else if (N > 0 && (iy == 0 || io == 0)) want = OMB_EINVAL;
              else if (iy >= 2 || ic >= 2 || io >= 2 || ib == 3) want = OMB_EINVAL;
              else if (ld < N) want = OMB_EINVAL;
              else if (C < 2 || (long long)k * C > 8192 || B > (1 << 24)) want = OMB_EUNSUP;
              err.clear();
              expect(check_hvi_boxes(&err, k, y, ld, N, coords, C, boxes, B, out), want, "check_hvi_boxes");
              expect(check_hvi_boxes(nullptr, k, y, ld, N, coords, C, boxes, B, out), want,
                     "check_hvi_boxes (no message)");
              if (want != OMB_OK && err.empty()) {
                ++bad;
                fprintf(stderr, "MISMATCH check_hvi_boxes: failure without a message\n");
              }
              if (want == OMB_EUNSUP && err.find("8192") == std::string::npos &&
                  err.find("16777216") == std::string::npos) {
                ++bad;
                fprintf(stderr, "MISMATCH check_hvi_boxes: OMB_EUNSUP message names no cap: %s\n", err.c_str());
              }
            }
  printf("omb_hvi_check: %ld calls, %ld mismatches\n", calls, bad);
  return bad ? 1 : 0;
}
