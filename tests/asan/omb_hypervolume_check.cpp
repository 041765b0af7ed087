// Stand-alone driver (ASan + UBSan, CPU only) of omb_hypervolume / omb_hypervolume_contrib's argument checks
// (check_hypervolume in omb_host.cpp), return codes against the header's contract, in its order: OMB_EINVAL for k
// outside [1, OMB_MAX_OBJ], S outside [1, OMB_NONDOM_SETS], N < 0, ld < N or ldm < N, a null or non-finite reference
// point, a null output, a null y with N > 0, y or an output off 8-byte alignment; then OMB_EUNSUP for
// N > OMB_NONDOM_POINTS.  The work cap (check_hv_work, hv_cells) is swept over hostile headers — kept counts and grid
// sizes no preparation leaves, and cell products that overflow 64 bits — and the launch sizes (hv_cell_blocks,
// hv_reduce_blocks) at their edges.  Built by `make -C optimobo_amd/csrc asan` as build/asan/omb_hypervolume_check.
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

// A pitch against N: the smallest value, N − 1, N, N + 3 (N itself where the neighbour does not exist).
static int64_t pitch(int64_t N, int which) {
  if (which == 0) return INT64_MIN;
  if (which == 1) return N == INT64_MIN ? N : N - 1;
  if (which == 2) return N;
  return N > INT64_MAX - 3 ? N : N + 3;
}

static const double kFinite[OMB_MAX_OBJ] = {1.1, -3.0, 0.0, 1e300, -1e300, 5e-324, 2.0, 7.0};

// the reference point of choice `ir` for k objectives: null, finite, NaN / +inf / −inf in the last coordinate that
// the check may read (coordinate min(k, OMB_MAX_OBJ) − 1), +inf past it (must not be read)
static const double* ref_point(int ir, int k, double* store, bool* finite) {
  for (int j = 0; j < OMB_MAX_OBJ; ++j) store[j] = kFinite[j];
  const int last = (k < 1 ? 1 : (k > OMB_MAX_OBJ ? OMB_MAX_OBJ : k)) - 1;
  *finite = true;
  if (ir == 0) return nullptr;
  if (ir == 2) store[last] = NAN, *finite = false;
  if (ir == 3) store[last] = INFINITY, *finite = false;
  if (ir == 4) store[0] = -INFINITY, *finite = false;
  if (ir == 5 && last + 1 < OMB_MAX_OBJ) store[last + 1] = INFINITY;
  return store;
}

static void sweep() {
  std::string err;
  alignas(16) static char buf[32];
  const void* ptrs[] = {nullptr, buf, buf + 4, buf + 1};   // null, aligned, off by 4, off by 1
  const int ks[] = {INT_MIN, -1, 0, 1, 2, 3, OMB_MAX_OBJ, OMB_MAX_OBJ + 1, INT_MAX};
  const int Ss[] = {INT_MIN, 0, 1, 3, OMB_NONDOM_SETS, OMB_NONDOM_SETS + 1, INT_MAX};
  const int64_t Ns[] = {INT64_MIN, -1, 0, 1, 33, OMB_NONDOM_POINTS, (int64_t)OMB_NONDOM_POINTS + 1, INT64_MAX};
  double store[OMB_MAX_OBJ];
  for (int contrib = 0; contrib < 2; ++contrib)
    for (int k : ks)
      for (int S : Ss)
        for (int64_t N : Ns)
          for (int lo = 0; lo < 4; ++lo)
            for (int mo = 0; mo < 4; ++mo)
              for (int ir = 0; ir < 6; ++ir)
                for (int iy = 0; iy < 4; ++iy)
                  for (int ih = 0; ih < 4; ++ih)
                    for (int io = 0; io < 4; ++io) {
                      if (!contrib && io != 0 && io != 2) continue;   // out is not looked at: null and misaligned do
                      const int64_t ld = pitch(N, lo), ldm = pitch(N, mo);
                      bool finite;
                      const double* r = ref_point(ir, k, store, &finite);
                      const void *y = ptrs[iy], *hv = ptrs[ih], *out = ptrs[io], *mask = ptrs[(iy + ih) & 3];
                      int want = OMB_OK;
                      if (k < 1 || k > OMB_MAX_OBJ) want = OMB_EINVAL;
                      else if (S < 1 || S > OMB_NONDOM_SETS) want = OMB_EINVAL;
                      else if (N < 0) want = OMB_EINVAL;
                      else if (ld < N || ldm < N) want = OMB_EINVAL;
                      else if (!r || !finite) want = OMB_EINVAL;
                      else if (ih == 0 || (contrib && io == 0)) want = OMB_EINVAL;
                      else if (N > 0 && iy == 0) want = OMB_EINVAL;
                      else if (iy >= 2 || ih >= 2 || (contrib && io >= 2)) want = OMB_EINVAL;
                      else if (N > OMB_NONDOM_POINTS) want = OMB_EUNSUP;
                      err.clear();
                      expect(check_hypervolume(&err, k, S, y, ld, N, mask, ldm, r, hv, contrib, out), want,
                             "check_hypervolume");
                      expect(check_hypervolume(nullptr, k, S, y, ld, N, mask, ldm, r, hv, contrib, out), want,
                             "check_hypervolume (no message)");
                      if (want != OMB_OK && err.empty()) {
                        ++bad;
                        fprintf(stderr, "MISMATCH check_hypervolume: failure without a message\n");
                      }
                    }
}

// the order itself: each refusal with everything after it in the header's order wrong as well
static void order() {
  alignas(16) static char buf[32];
  const void *al = buf, *off4 = buf + 4;
  const int64_t big = (int64_t)OMB_NONDOM_POINTS + 1;
  const double ok[OMB_MAX_OBJ] = {1, 1, 1, 1, 1, 1, 1, 1}, nan2[OMB_MAX_OBJ] = {1, NAN, 1, 1, 1, 1, 1, 1};
  expect(check_hypervolume(nullptr, 0, 0, off4, 0, -1, nullptr, 0, nullptr, nullptr, 1, nullptr), OMB_EINVAL, "k first");
  expect(check_hypervolume(nullptr, 9, 1, al, big, big, al, big, ok, al, 0, nullptr), OMB_EINVAL, "k before the size");
  expect(check_hypervolume(nullptr, 2, 17, al, big, big, al, big, ok, al, 0, nullptr), OMB_EINVAL, "S before the size");
  expect(check_hypervolume(nullptr, 2, 1, al, big - 1, big, al, big, ok, al, 0, nullptr), OMB_EINVAL, "ld before the size");
  expect(check_hypervolume(nullptr, 2, 1, al, big, big, al, big - 1, ok, al, 0, nullptr), OMB_EINVAL, "ldm before the size");
  expect(check_hypervolume(nullptr, 2, 1, al, big, big, al, big, nullptr, al, 0, nullptr), OMB_EINVAL, "r before the size");
  expect(check_hypervolume(nullptr, 2, 1, al, big, big, al, big, nan2, al, 0, nullptr), OMB_EINVAL, "r_j before the size");
  expect(check_hypervolume(nullptr, 1, 1, al, big - 1, big - 1, al, big - 1, nan2, al, 0, nullptr), OMB_OK,
         "r_1 is not read at k = 1");
  expect(check_hypervolume(nullptr, 2, 1, al, big, big, al, big, ok, nullptr, 0, nullptr), OMB_EINVAL, "hv before the size");
  expect(check_hypervolume(nullptr, 2, 1, al, big, big, al, big, ok, al, 1, nullptr), OMB_EINVAL, "contrib before the size");
  expect(check_hypervolume(nullptr, 2, 1, nullptr, big, big, al, big, ok, al, 0, nullptr), OMB_EINVAL, "y before the size");
  expect(check_hypervolume(nullptr, 2, 1, off4, big, big, al, big, ok, al, 0, nullptr), OMB_EINVAL, "y's alignment before the size");
  expect(check_hypervolume(nullptr, 2, 1, al, big, big, al, big, ok, off4, 0, nullptr), OMB_EINVAL, "hv's alignment before the size");
  expect(check_hypervolume(nullptr, 2, 1, al, big, big, al, big, ok, al, 1, off4), OMB_EINVAL, "contrib's alignment before the size");
  expect(check_hypervolume(nullptr, 2, 1, al, big, big, buf + 1, big, ok, al, 1, al), OMB_EUNSUP, "the size");
  expect(check_hypervolume(nullptr, 2, 1, al, big, big, nullptr, big, ok, al, 0, off4), OMB_EUNSUP, "the size, out ignored");
  expect(check_hypervolume(nullptr, 2, 1, al, big - 1, big - 1, nullptr, big - 1, ok, al, 0, nullptr), OMB_OK, "2^24 rows, no mask");
  expect(check_hypervolume(nullptr, 8, 16, nullptr, 0, 0, nullptr, 0, ok, al, 0, nullptr), OMB_OK, "N = 0 with a null y");
  expect(check_hypervolume(nullptr, 8, 16, nullptr, 0, 0, nullptr, 0, ok, nullptr, 0, nullptr), OMB_EINVAL, "N = 0 needs hv");
  expect(check_hypervolume(nullptr, 8, 16, off4, 0, 0, nullptr, 0, ok, al, 0, nullptr), OMB_EINVAL, "N = 0, y off its alignment");
}

static void set_hdr(int32_t* h, int32_t n, int32_t g0, int32_t g1, int32_t g2, int32_t g3, int32_t g4, int32_t g5) {
  const int32_t v[kHvHdr] = {n, g0, g1, g2, g3, g4, g5, INT32_MIN};   // the spare is never read
  for (int i = 0; i < kHvHdr; ++i) h[i] = v[i];
}

static void work() {
  std::string err;
  int32_t hdr[kHvMaxS * kHvHdr];
  int64_t mc = -1;
  const int32_t M = INT32_MAX;
  // hv_cells: products in 64 bits, saturating
  const int32_t big6[6] = {M, M, M, M, M, M}, mid[6] = {1024, 1024, 1024, 1024, 1024, 1024}, neg[6] = {5, -1, 5, 5, 5, 5};
  expect(hv_cells(0, big6), 1, "no grid objective: one cell");
  expect(hv_cells(2, big6), (long long)M * M, "2^62 fits");
  expect(hv_cells(3, big6), INT64_MAX, "2^93 saturates");
  expect(hv_cells(6, big6), INT64_MAX, "2^186 saturates");
  expect(hv_cells(6, mid), 1ll << 60, "1024^6");
  expect(hv_cells(6, neg), 0, "a grid size below 1");
  // one set at the limits of the contract
  set_hdr(hdr, 1024, 1024, 1024, 1024, 1024, 1024, 1024);
  expect(check_hv_work(&err, 1, 1, hdr, 0, &mc), OMB_OK, "k = 1 reads no grid");
  expect(mc, 1, "k = 1: one cell");
  expect(check_hv_work(&err, 3, 1, hdr, 0, &mc), OMB_OK, "k = 3, 1024 points: 2^20 tests");
  expect(mc, 1024, "k = 3: 1024 cells");
  expect(check_hv_work(&err, 3, 1, hdr, 1, &mc), OMB_OK, "k = 3 contributions: 2^30 tests");
  expect(check_hv_work(&err, 5, 1, hdr, 0, &mc), (1ll << 40) > OMB_HV_MAX_WORK ? OMB_EUNSUP : OMB_OK, "k = 5, 1024 points");
  expect(check_hv_work(&err, 8, 1, hdr, 1, &mc), OMB_EUNSUP, "k = 8, 1024 points: 2^80 saturates and is refused");
  expect(check_hv_work(nullptr, 8, 1, hdr, 1, &mc), OMB_EUNSUP, "the same without a message");
  set_hdr(hdr, 1025, 1, 1, 1, 1, 1, 1);
  expect(check_hv_work(&err, 8, 1, hdr, 0, &mc), OMB_EUNSUP, "1025 kept rows");
  set_hdr(hdr, M, M, M, M, M, M, M);
  expect(check_hv_work(&err, 8, 1, hdr, 1, &mc), OMB_EUNSUP, "a count of INT32_MAX is 'too many rows'");
  // headers that no preparation leaves: refused before anything is sized from them
  set_hdr(hdr, -1, 1, 1, 1, 1, 1, 1);
  expect(check_hv_work(&err, 4, 1, hdr, 0, &mc), OMB_EHIP, "a negative count");
  set_hdr(hdr, INT32_MIN, 1, 1, 1, 1, 1, 1);
  expect(check_hv_work(&err, 4, 1, hdr, 1, &mc), OMB_EHIP, "INT32_MIN rows");
  set_hdr(hdr, 30, 30, 31, 1, 1, 1, 1);
  expect(check_hv_work(&err, 4, 1, hdr, 0, &mc), OMB_EHIP, "more grid values than rows");
  expect(check_hv_work(&err, 3, 1, hdr, 0, &mc), OMB_OK, "the same header at k = 3 never reads that size");
  set_hdr(hdr, 30, 30, 0, 1, 1, 1, 1);
  expect(check_hv_work(&err, 4, 1, hdr, 0, &mc), OMB_EHIP, "an empty grid of a non-empty set");
  set_hdr(hdr, 30, 30, M, M, M, M, M);
  expect(check_hv_work(&err, 8, 1, hdr, 0, &mc), OMB_EHIP, "grid sizes of INT32_MAX");
  set_hdr(hdr, 0, M, -7, M, INT32_MIN, M, M);
  expect(check_hv_work(&err, 8, 1, hdr, 1, &mc), OMB_OK, "an empty set's grid sizes are not read");
  expect(mc, 0, "an empty set has no cell");
  // several sets: the work adds up, the largest set sizes the launch, the first refusal wins
  for (int s = 0; s < kHvMaxS; ++s) set_hdr(hdr + s * kHvHdr, 30, 30, 30, 30, 30, 30, 30);
  const long long per_set = 30ll * 30 * 30 * 30 * 30 * 30 * 30;   // k = 8: 30^6 cells × 30 rows ≈ 2.2e10
  expect(check_hv_work(&err, 8, 1, hdr, 0, &mc), per_set > OMB_HV_MAX_WORK ? OMB_EUNSUP : OMB_OK, "one set of 30^6 cells");
  expect(mc, 729000000, "30^6 cells");
  expect(check_hv_work(&err, 8, kHvMaxS, hdr, 0, &mc), 16 * per_set > OMB_HV_MAX_WORK ? OMB_EUNSUP : OMB_OK, "16 of them");
  expect(check_hv_work(&err, 8, 1, hdr, 1, &mc), 31 * per_set > OMB_HV_MAX_WORK ? OMB_EUNSUP : OMB_OK, "one, per point");
  set_hdr(hdr + 2 * kHvHdr, 5, 5, 5, 1, 1, 1, 1);
  set_hdr(hdr + 1 * kHvHdr, 2, 1, 2, 1, 1, 1, 1);
  set_hdr(hdr, 0, 0, 0, 0, 0, 0, 0);
  expect(check_hv_work(&err, 4, 3, hdr, 0, &mc), OMB_OK, "three small sets");
  expect(mc, 25, "the largest of 0, 2 and 25 cells");
  set_hdr(hdr + 2 * kHvHdr, 1025, 5, 5, 1, 1, 1, 1);
  set_hdr(hdr + 1 * kHvHdr, -1, 1, 2, 1, 1, 1, 1);
  expect(check_hv_work(&err, 4, 3, hdr, 0, &mc), OMB_EHIP, "the first bad set decides");
  expect(check_hv_work(&err, 4, 1, hdr, 0, &mc), OMB_OK, "sets past S are not read");
  // launch sizes
  expect(hv_cell_blocks(0), 1, "no cell still writes its zero");
  expect(hv_cell_blocks(1), 1, "one cell");
  expect(hv_cell_blocks(kHvBlockCells), 1, "one workgroup of cells");
  expect(hv_cell_blocks(kHvBlockCells + 1), 2, "and one more");
  expect(hv_cell_blocks(INT64_MAX), (INT64_MAX - 1) / kHvBlockCells + 1, "a saturated product");
  expect(hv_cell_blocks(OMB_HV_MAX_WORK) <= INT32_MAX, 1, "the cap's workgroups fit a launch");
  expect(hv_reduce_blocks(0), 1, "nothing to add still writes");
  expect(hv_reduce_blocks(1), 1, "one partial sum");
  expect(hv_reduce_blocks(2 * kHvReduceLanes), 1, "one workgroup of partial sums");
  expect(hv_reduce_blocks(2 * kHvReduceLanes + 1), 2, "and one more");
  expect(hv_reduce_blocks(INT64_MAX), (INT64_MAX - 1) / (2 * kHvReduceLanes) + 1, "the largest count");
}

int main() {
  sweep();
  order();
  work();
  printf("omb_hypervolume_check: %ld calls, %ld mismatches\n", calls, bad);
  return bad ? 1 : 0;
}
