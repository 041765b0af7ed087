// Stand-alone driver (ASan + UBSan, CPU only) of omb_hvi_paths / omb_plan_hvi_paths' argument checks (check_hvi_paths
// and check_box_lists in omb_host.cpp), return codes against the header's contract, in its order: OMB_EINVAL for k
// outside [1, OMB_MAX_OBJ], S outside [1, 16], N < 0, a null grid / box list / offsets, offsets that do not start at 0,
// decrease or leave a list empty, a null y / out with N > 0, a pointer off its alignment (8 bytes; the box list 4) or
// ld < N; then OMB_EUNSUP for C < 2, k·C > 8192 (the product in 64 bits) or box_off[S] > 2^24; N = 0 passes.  The
// offsets live in heap arrays of exactly S + 1 ints and the box lists in heap arrays of exactly box_off[S] rows, so a
// check that reads past either is a sanitizer report.
// Built by `make -C optimobo_amd/csrc asan` as build/asan/omb_nehvi_check.
#include <limits.h>
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

// offsets of S lists: exactly S + 1 ints on the heap (S < 1 or past the limit: one int, which no check may pass)
struct Offsets {
  const char* name;
  bool valid;      // starts at 0, strictly increasing
  int32_t* p;
  int S;
  Offsets(const char* n, bool v, int S_, const std::vector<int32_t>& o) : name(n), valid(v), p(new int32_t[o.size()]), S(S_) {
    for (size_t i = 0; i < o.size(); ++i) p[i] = o[i];
  }
};

static std::vector<Offsets> offsets_for(int S) {
  std::vector<Offsets> out;
  if (S < 1 || S > kPathsMaxS) {
    out.emplace_back("one int", true, S, std::vector<int32_t>{0});
    return out;
  }
  std::vector<int32_t> inc(S + 1), big(S + 1), top(S + 1), dec(S + 1), flat(S + 1), from1(S + 1), neg(S + 1), wrap(S + 1);
  for (int s = 0; s <= S; ++s) {
    inc[s] = 3 * s;
    big[s] = s == S ? (1 << 24) + 1 : s;                 // ends past 2^24
    top[s] = s == S ? (1 << 24) : s;                     // ends at the limit
    dec[s] = s == S ? S - 2 : s;                         // the last offset decreases
    flat[s] = s == 0 ? 0 : (s == 1 ? 1 : s - 1);         // list 1 is empty (S >= 2), else increasing
    from1[s] = s + 1;                                    // does not start at 0
    neg[s] = s == 0 ? 0 : -s;                            // decreasing below 0
    wrap[s] = s == 0 ? 0 : (s == S ? INT_MIN : INT_MAX - S + s);   // "overflowed" past INT_MAX
  }
  out.emplace_back("increasing", true, S, inc);
  out.emplace_back("to 2^24 + 1", true, S, big);
  out.emplace_back("to 2^24", true, S, top);
  out.emplace_back("decreasing", false, S, dec);
  out.emplace_back("empty list", S < 2, S, flat);
  out.emplace_back("from 1", false, S, from1);
  out.emplace_back("negative", false, S, neg);
  out.emplace_back("wrapped", false, S, wrap);
  return out;
}

static void sweep_checks() {
  std::string err;
  alignas(16) static char buf[32];
  const void* ptrs[] = {nullptr, buf, buf + 4, buf + 2};   // null, aligned, off by 4 (fine for the box list), off by 2
  const int ks[] = {INT_MIN, 0, 1, 2, OMB_MAX_OBJ, OMB_MAX_OBJ + 1, INT_MAX};
  const int Ss[] = {INT_MIN, -1, 0, 1, 2, kPathsMaxS, kPathsMaxS + 1, INT_MAX};
  const int Cs[] = {INT_MIN, 0, 1, 2, 4096, 4097, 8192, 8193, INT_MAX};
  const int64_t Ns[] = {INT64_MIN, -1, 0, 33, INT64_MAX};
  const int64_t lds[] = {INT64_MIN, 0, 32, 33};
  for (int S : Ss) {
    std::vector<Offsets> offs = offsets_for(S);
    for (int k : ks)
      for (int C : Cs)
        for (int64_t N : Ns)
          for (int64_t ld : lds)
            for (size_t oi = 0; oi <= offs.size(); ++oi)       // the last round: null offsets
              for (int mask = 0; mask < 256; ++mask) {
                const int iy = mask & 3, ic = (mask >> 2) & 3, ib = (mask >> 4) & 3, io = (mask >> 6) & 3;
                const void *y = ptrs[iy], *coords = ptrs[ic], *boxes = ptrs[ib], *out = ptrs[io];
                const Offsets* o = oi < offs.size() ? &offs[oi] : nullptr;
                const int32_t* off = o ? o->p : nullptr;
                int want = OMB_OK;
                if (k < 1 || k > OMB_MAX_OBJ || S < 1 || S > kPathsMaxS || N < 0) want = OMB_EINVAL;
                else if (ic == 0 || ib == 0 || !off) want = OMB_EINVAL;
                else if (!o->valid) want = OMB_EINVAL;
                else if (N > 0 && (iy == 0 || io == 0)) want = OMB_EINVAL;
                else if (iy >= 2 || ic >= 2 || io >= 2 || ib == 3) want = OMB_EINVAL;
                else if (ld < N) want = OMB_EINVAL;
                else if (C < 2 || (long long)k * C > 8192 || off[S] > (1 << 24)) want = OMB_EUNSUP;
                err.clear();
                expect(check_hvi_paths(&err, k, S, y, ld, N, coords, C, off, boxes, out), want,
                       o ? o->name : "null offsets");
                expect(check_hvi_paths(nullptr, k, S, y, ld, N, coords, C, off, boxes, out), want, "no message");
                if (want != OMB_OK && err.empty()) {
                  ++bad;
                  fprintf(stderr, "MISMATCH check_hvi_paths: failure without a message\n");
                }
                if (want == OMB_EUNSUP && err.find("8192") == std::string::npos &&
                    err.find("16777216") == std::string::npos) {
                  ++bad;
                  fprintf(stderr, "MISMATCH check_hvi_paths: OMB_EUNSUP message names no cap: %s\n", err.c_str());
                }
              }
    for (Offsets& o : offs) delete[] o.p;
  }
}

// check_box_lists over exactly-sized heap lists: valid lists pass, one bad box anywhere (first row of the first list,
// last row of the last) is OMB_EINVAL naming its list
static void sweep_lists() {
  std::string err;
  for (int k : {1, 2, 3, OMB_MAX_OBJ})
    for (int S : {1, 3, kPathsMaxS})
      for (int C : {2, 3, 65535}) {
        std::vector<int32_t> off(S + 1);
        for (int s = 0; s <= S; ++s) off[s] = s * (s + 1) / 2 + s;       // lists of 2, 3, 4, … boxes
        const size_t rows = (size_t)off[S];
        uint16_t* b = new uint16_t[rows * 2 * k];
        for (size_t r = 0; r < rows; ++r)
          for (int j = 0; j < k; ++j) {
            b[2 * k * r + 2 * j] = (uint16_t)(C - 2);
            b[2 * k * r + 2 * j + 1] = (uint16_t)(C - 1);
          }
        expect(check_box_lists(&err, k, S, C, off.data(), b), OMB_OK, "valid lists");
        const size_t spots[] = {0, rows - 1, (size_t)off[S - 1]};
        const int lists[] = {0, S - 1, S - 1};
        for (int t = 0; t < 3; ++t)
          for (int kind = 0; kind < 3; ++kind) {
            uint16_t* row = b + 2 * k * spots[t] + 2 * (k - 1);
            const uint16_t lo = row[0], hi = row[1];
            if (kind == 0) row[1] = (uint16_t)C;             // an index past the grid (C = 65535: the largest uint16)
            else if (kind == 1) row[0] = row[1];             // lo == hi
            else { row[0] = hi; row[1] = lo; }               // lo > hi
            err.clear();
            expect(check_box_lists(&err, k, S, C, off.data(), b), OMB_EINVAL, "bad box");
            expect(check_box_lists(nullptr, k, S, C, off.data(), b), OMB_EINVAL, "bad box (no message)");
            char name[32];
            snprintf(name, sizeof(name), "list %d,", lists[t]);
            if (err.find(name) == std::string::npos) {
              ++bad;
              fprintf(stderr, "MISMATCH check_box_lists: message does not name list %d: %s\n", lists[t], err.c_str());
            }
            row[0] = lo;
            row[1] = hi;
          }
        delete[] b;
      }
}

int main() {
  sweep_checks();
  sweep_lists();
  printf("omb_nehvi_check: %ld calls, %ld mismatches\n", calls, bad);
  return bad ? 1 : 0;
}
