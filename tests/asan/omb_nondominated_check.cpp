// Stand-alone driver (ASan + UBSan, CPU only) of omb_nondominated's argument checks (check_nondominated in
// omb_host.cpp), return codes against the header's contract, in its order: OMB_EINVAL for k outside
// [1, OMB_MAX_OBJ], S outside [1, OMB_NONDOM_SETS], N < 0, ld < N or ldm < N, a null count, a null y / mask with
// N > 0, y or count off 8-byte alignment; then OMB_EUNSUP for N > OMB_NONDOM_POINTS; N = 0 passes with null y / mask.
// The sieve's round rule (nd_another_round) and the final pass's workgroup count (nd_final_blocks) are swept too.
// Built by `make -C optimobo_amd/csrc asan` as build/asan/omb_nondominated_check.
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

// A pitch against N: the smallest value, N − 1, N, N + 3 (N itself where the neighbour does not exist).
static int64_t pitch(int64_t N, int which) {
  if (which == 0) return INT64_MIN;
  if (which == 1) return N == INT64_MIN ? N : N - 1;
  if (which == 2) return N;
  return N > INT64_MAX - 3 ? N : N + 3;
}

static void sweep() {
  std::string err;
  alignas(16) static char buf[32];
  const void* ptrs[] = {nullptr, buf, buf + 4, buf + 1};   // null, aligned, off by 4, off by 1
  const int ks[] = {INT_MIN, -1, 0, 1, 2, OMB_MAX_OBJ, OMB_MAX_OBJ + 1, INT_MAX};
  const int Ss[] = {INT_MIN, -1, 0, 1, 3, OMB_NONDOM_SETS, OMB_NONDOM_SETS + 1, INT_MAX};
  const int64_t Ns[] = {INT64_MIN, -1, 0, 1, 33, OMB_NONDOM_POINTS, (int64_t)OMB_NONDOM_POINTS + 1, INT64_MAX};
  const int offs[] = {0, 1, 2, 3};                         // pitch()'s choices
  for (int k : ks)
    for (int S : Ss)
      for (int64_t N : Ns)
        for (int lo : offs)
          for (int mo : offs)
            for (int iy = 0; iy < 4; ++iy)
              for (int im = 0; im < 4; ++im)
                for (int ic = 0; ic < 4; ++ic) {
                  const int64_t ld = pitch(N, lo), ldm = pitch(N, mo);
                  const void *y = ptrs[iy], *mask = ptrs[im], *count = ptrs[ic];
                  int want = OMB_OK;
                  if (k < 1 || k > OMB_MAX_OBJ) want = OMB_EINVAL;
                  else if (S < 1 || S > OMB_NONDOM_SETS) want = OMB_EINVAL;
                  else if (N < 0) want = OMB_EINVAL;
                  else if (ld < N || ldm < N) want = OMB_EINVAL;
                  else if (ic == 0) want = OMB_EINVAL;
                  else if (N > 0 && (iy == 0 || im == 0)) want = OMB_EINVAL;
                  else if (iy >= 2 || ic >= 2) want = OMB_EINVAL;         // the mask is bytes: any address
                  else if (N > OMB_NONDOM_POINTS) want = OMB_EUNSUP;
                  err.clear();
                  expect(check_nondominated(&err, k, S, y, ld, N, mask, ldm, count), want, "check_nondominated");
                  expect(check_nondominated(nullptr, k, S, y, ld, N, mask, ldm, count), want,
                         "check_nondominated (no message)");
                  if (want != OMB_OK && err.empty()) {
                    ++bad;
                    fprintf(stderr, "MISMATCH check_nondominated: failure without a message\n");
                  }
                }
}

// the order itself: each refusal with everything after it in the header's order wrong as well
static void order() {
  alignas(16) static char buf[32];
  const void *al = buf, *off4 = buf + 4;
  const int64_t big = (int64_t)OMB_NONDOM_POINTS + 1;
  expect(check_nondominated(nullptr, 0, 0, off4, 0, -1, nullptr, 0, nullptr), OMB_EINVAL, "k first");
  expect(check_nondominated(nullptr, 9, 1, al, big, big, al, big, al), OMB_EINVAL, "k before the size");
  expect(check_nondominated(nullptr, 2, 17, al, big, big, al, big, al), OMB_EINVAL, "S before the size");
  expect(check_nondominated(nullptr, 2, 1, al, big - 1, big, al, big, al), OMB_EINVAL, "ld before the size");
  expect(check_nondominated(nullptr, 2, 1, al, big, big, al, big - 1, al), OMB_EINVAL, "ldm before the size");
  expect(check_nondominated(nullptr, 2, 1, al, big, big, al, big, nullptr), OMB_EINVAL, "count before the size");
  expect(check_nondominated(nullptr, 2, 1, nullptr, big, big, al, big, al), OMB_EINVAL, "y before the size");
  expect(check_nondominated(nullptr, 2, 1, al, big, big, nullptr, big, al), OMB_EINVAL, "mask before the size");
  expect(check_nondominated(nullptr, 2, 1, off4, big, big, al, big, al), OMB_EINVAL, "y's alignment before the size");
  expect(check_nondominated(nullptr, 2, 1, al, big, big, al, big, off4), OMB_EINVAL, "count's alignment before the size");
  expect(check_nondominated(nullptr, 2, 1, al, big, big, buf + 1, big, al), OMB_EUNSUP, "the size");
  expect(check_nondominated(nullptr, 2, 1, al, big - 1, big - 1, buf + 1, big - 1, al), OMB_OK, "2^24 points");
  expect(check_nondominated(nullptr, 1, 16, nullptr, 0, 0, nullptr, 0, al), OMB_OK, "N = 0 with null y and mask");
  expect(check_nondominated(nullptr, 1, 16, nullptr, 0, 0, nullptr, 0, nullptr), OMB_EINVAL, "N = 0 needs the count");
  expect(check_nondominated(nullptr, 1, 16, off4, 0, 0, nullptr, 0, al), OMB_EINVAL, "N = 0, y off its alignment");
}

static void rounds() {
  // another tile pass only while the list is longer than a tile, the last pass halved it and fewer than four ran
  expect(nd_another_round(1, 1 << 20, 1 << 20), 0, "an antichain goes straight to the final pass");
  expect(nd_another_round(1, 1 << 20, 8000), 1, "a pass that shrank the list");
  expect(nd_another_round(1, 1 << 20, kNdTile), 0, "one tile left");
  expect(nd_another_round(1, 1 << 20, kNdTile + 1), 1, "one tile and a point");
  expect(nd_another_round(2, 8000, 4001), 0, "less than halved");
  expect(nd_another_round(2, 8000, 4000), 1, "halved");
  expect(nd_another_round(kNdMaxRounds, 1 << 20, 8000), 0, "the bound on the passes");
  expect(nd_another_round(1, 1, 0), 0, "nothing left");
  expect(nd_final_blocks(0), 1, "an empty list still writes its count");
  expect(nd_final_blocks(1), 1, "one survivor");
  expect(nd_final_blocks(kNdTile), 1, "one tile");
  expect(nd_final_blocks(kNdTile + 1), 2, "one tile and a point");
  expect(nd_final_blocks(kNdMaxN), kNdMaxN / kNdTile, "2^24 survivors");
}

int main() {
  sweep();
  order();
  rounds();
  printf("omb_nondominated_check: %ld calls, %ld mismatches\n", calls, bad);
  return bad ? 1 : 0;
}
