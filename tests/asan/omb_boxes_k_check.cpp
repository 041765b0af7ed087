// Stand-alone driver (ASan + UBSan, CPU only) of the k-D exact-EHVI argument checks in omb_host.cpp:
// check_boxes_k's ranges with hostile sizes, and check_box_list over exactly-sized heap box lists, so that a
// read past the list or a 32-bit size product is a sanitizer report.  Return codes against the header's contract.
// Built by `make -C optimobo_amd/csrc asan` as build/asan/omb_boxes_k_check.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../optimobo_amd/csrc/omb_host.h"

using namespace omb;

static long calls = 0, bad = 0;

static void expect(int got, int want, const char* what) {
  ++calls;
  if (got != want) {
    ++bad;
    fprintf(stderr, "MISMATCH %s: got %d want %d\n", what, got, want);
  }
}

static int want_boxes_k(int k, int C, int64_t B) {
  if (k < 2 || k > OMB_MAX_OBJ) return OMB_EINVAL;
  if (C < 2 || 3 * (int64_t)k * C + 2 * k + 4 > kMaxLdsDoubles) return OMB_EUNSUP;
  if (B < 1) return OMB_EINVAL;
  if (B > kMaxBoxesK) return OMB_EUNSUP;
  return OMB_OK;
}

int main() {
  std::string err;
  const int ks[] = {INT_MIN, -1, 0, 1, 2, 3, 4, 5, 8, 9, 64, INT_MAX};
  const int Cs[] = {INT_MIN, -1, 0, 1, 2, 11, 62, 340, 341, 681, 682, 1364, 1365, 65535, 65536, INT_MAX / 3, INT_MAX};
  const int64_t Bs[] = {INT64_MIN, -1, 0, 1, 134, kMaxBoxesK, (int64_t)kMaxBoxesK + 1, INT_MAX, INT64_MAX};
  for (int k : ks)
    for (int C : Cs)
      for (int64_t B : Bs) {
        expect(check_boxes_k(&err, k, C, B), want_boxes_k(k, C, B), "check_boxes_k");
        expect(check_boxes_k(nullptr, k, C, B), want_boxes_k(k, C, B), "check_boxes_k (no message)");
      }
  // the stated limit is the largest C that passes
  for (int k = 2; k <= OMB_MAX_OBJ; ++k) {
    const int c_max = (kMaxLdsDoubles - 2 * k - 4) / (3 * k);
    expect(check_boxes_k(&err, k, c_max, 1), OMB_OK, "C at the limit");
    expect(check_boxes_k(&err, k, c_max + 1, 1), OMB_EUNSUP, "C past the limit");
    if (err.find(std::to_string(c_max)) == std::string::npos) {
      ++bad;
      fprintf(stderr, "MISMATCH message without the limit %d: %s\n", c_max, err.c_str());
    }
  }
  // box lists, exactly sized on the heap
  unsigned seed = 12345;
  auto rnd = [&](unsigned n) {
    seed = seed * 1664525u + 1013904223u;
    return (seed >> 8) % n;
  };
  for (int k = 2; k <= OMB_MAX_OBJ; ++k)
    for (int C : {2, 3, 11, 681 / k * 2, 65535}) {
      for (int64_t B : {(int64_t)1, (int64_t)7, (int64_t)1000}) {
        std::vector<uint16_t>* v = new std::vector<uint16_t>((size_t)(2 * k * B));
        for (int64_t b = 0; b < B; ++b)
          for (int j = 0; j < k; ++j) {
            const unsigned hi = 1 + rnd((unsigned)C - 1), lo = rnd(hi);
            (*v)[2 * k * b + 2 * j] = (uint16_t)lo;
            (*v)[2 * k * b + 2 * j + 1] = (uint16_t)hi;
          }
        expect(check_box_list(&err, k, C, v->data(), B), OMB_OK, "valid list");
        const size_t at = (size_t)(2 * k * (B - 1) + 2 * (k - 1));     // the last box's last objective
        const uint16_t lo = (*v)[at], hi = (*v)[at + 1];
        (*v)[at + 1] = (uint16_t)C;                                      // hi index ≥ C
        expect(check_box_list(&err, k, C, v->data(), B), OMB_EINVAL, "hi >= C");
        (*v)[at + 1] = hi;
        (*v)[at] = hi;                                                   // lo == hi
        expect(check_box_list(&err, k, C, v->data(), B), OMB_EINVAL, "lo == hi");
        (*v)[at] = lo;
        (*v)[0] = (*v)[1];                                               // the first box
        expect(check_box_list(nullptr, k, C, v->data(), B), OMB_EINVAL, "first box lo == hi");
        delete v;
      }
    }
  expect(check_box_list(&err, 4, 11, nullptr, 0), OMB_OK, "empty list is never read");
  printf("omb_boxes_k_check: %ld calls, %ld mismatches\n", calls, bad);
  return bad ? 1 : 0;
}
