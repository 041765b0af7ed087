// Stand-alone driver (ASan + UBSan, CPU only) of the two gradient entry points' host checks (omb_host.cpp):
// check_paths_grad (omb_paths_grad) and check_hvi_paths_grad (omb_hvi_paths_grad) swept over the edge values of every
// argument, return codes against the header's contract, in its order.
//   check_paths_grad: check_paths_eval's refusals — OMB_EINVAL (n_obj, N < 0, ld < N, a null pointer with N > 0, the
//     gradient output among them), then OMB_ESTATE, then OMB_EUNSUP.
//   check_hvi_paths_grad: check_hvi_paths' OMB_EINVAL refusals, then OMB_EINVAL for d outside [1, 64], a null dy /
//     grad with N > 0, exactly one of t / tgrad null, one of the four off its 8-byte alignment, then check_hvi_paths'
//     OMB_EUNSUP refusals — and, wherever the added arguments are in order, check_hvi_paths' own code.
// Built by `make -C optimobo_amd/csrc build/asan/omb_paths_grad_check`.
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

static void sweep_paths_grad() {
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
        for (int mask = 0; mask < 8; ++mask)
          for (const auto& st : states)
            for (int d : dims)
              for (int n : ns) {
                const void *Xc = ptrs[mask & 1], *out = ptrs[(mask >> 1) & 1], *grad = ptrs[(mask >> 2) & 1];
                PathsObjInfo info[OMB_MAX_OBJ];
                for (int o = 0; o < OMB_MAX_OBJ; ++o) info[o] = PathsObjInfo{1, 2, 10, 3};
                const bool in_range = n_obj >= 1 && n_obj <= OMB_MAX_OBJ;
                if (in_range) info[n_obj - 1] = PathsObjInfo{st[0], d, n, st[1]};
                int want = OMB_OK;
                if (!in_range || N < 0 || ld < N) want = OMB_EINVAL;
                else if (N > 0 && mask != 7) want = OMB_EINVAL;
                else if (!st[0] || st[1] < 1) want = OMB_ESTATE;
                else if (n_obj > 1 && st[1] != 3) want = OMB_ESTATE;
                else if (d > 64 || n > OMB_MAX_TRAIN_DENSE) want = OMB_EUNSUP;
                err.clear();
                expect(check_paths_grad(&err, n_obj, Xc, N, ld, out, grad, info), want, "check_paths_grad");
                expect(check_paths_grad(nullptr, n_obj, Xc, N, ld, out, grad, info), want,
                       "check_paths_grad (no message)");
                if (want != OMB_OK && err.empty()) {
                  ++bad;
                  fprintf(stderr, "MISMATCH check_paths_grad: failure without a message\n");
                }
                // with a gradient output in order it is check_paths_eval
                if (grad || N <= 0)
                  expect(check_paths_grad(&err, n_obj, Xc, N, ld, out, grad, info),
                         check_paths_eval(&err, n_obj, Xc, N, ld, out, info), "check_paths_grad = check_paths_eval");
              }
  expect(check_paths_grad(&err, 1, buf, 1, 1, buf, buf, nullptr), OMB_EINVAL, "check_paths_grad (no state)");
}

static void sweep_hvi_paths_grad() {
  std::string err;
  alignas(8) static char mem[64];
  const void* const al = mem;          // 8-byte aligned
  const void* const off4 = mem + 4;    // 4-byte aligned only
  const int ks[] = {INT_MIN, 0, 1, 2, OMB_MAX_OBJ, OMB_MAX_OBJ + 1};
  const int Ss[] = {-1, 0, 1, 3, 16, 17};
  const int ds[] = {INT_MIN, 0, 1, 64, 65, INT_MAX};
  const int64_t Ns[] = {-1, 0, 17};
  const int64_t lds[] = {0, 17, 20};
  const int Cs[] = {1, 2, kMaxLdsDoubles, kMaxLdsDoubles + 1};
  // offsets: in order, not from 0, an empty list, past the box budget
  std::vector<std::vector<int32_t>> offs;
  for (int kind = 0; kind < 4; ++kind) {
    std::vector<int32_t> o(kPathsMaxS + 2);
    for (int s = 0; s < (int)o.size(); ++s) o[s] = 2 * s + (kind == 1 ? 1 : 0);
    if (kind == 2) o[1] = o[0];
    if (kind == 3)
      for (int s = 1; s < (int)o.size(); ++s) o[s] = kMaxBoxesK + s;
    offs.push_back(o);
  }
  const void* yptrs[] = {nullptr, al, off4};
  for (int k : ks)
    for (int S : Ss)
      for (int d : ds)
        for (int64_t N : Ns)
          for (int64_t ld : lds)
            for (int C : Cs)
              for (size_t ok = 0; ok <= offs.size(); ++ok)
                for (int mask = 0; mask < 3 * 3 * 3 * 3; ++mask) {
                  const int32_t* off = ok < offs.size() ? offs[ok].data() : nullptr;
                  const void* dy = yptrs[mask % 3];
                  const void* grad = yptrs[(mask / 3) % 3];
                  const void* t = yptrs[(mask / 9) % 3];
                  const void* tg = yptrs[(mask / 27) % 3];
                  const void *y = al, *coords = al, *boxes = al, *out = al;
                  const int base = check_hvi_paths(nullptr, k, S, y, ld, N, coords, C, off, boxes, out);
                  int want;
                  if (base == OMB_EINVAL) want = OMB_EINVAL;
                  else if (d < 1 || d > 64) want = OMB_EINVAL;
                  else if (N > 0 && (!dy || !grad)) want = OMB_EINVAL;
                  else if ((t == nullptr) != (tg == nullptr)) want = OMB_EINVAL;
                  else if (dy == off4 || grad == off4 || t == off4 || tg == off4) want = OMB_EINVAL;
                  else want = base;
                  err.clear();
                  expect(check_hvi_paths_grad(&err, k, S, d, y, dy, ld, N, coords, C, off, boxes, out, grad, t, tg),
                         want, "check_hvi_paths_grad");
                  expect(check_hvi_paths_grad(nullptr, k, S, d, y, dy, ld, N, coords, C, off, boxes, out, grad, t, tg),
                         want, "check_hvi_paths_grad (no message)");
                  if (want != OMB_OK && err.empty()) {
                    ++bad;
                    fprintf(stderr, "MISMATCH check_hvi_paths_grad: failure without a message\n");
                  }
                }
  // check_hvi_paths' own pointers: a null or misaligned y / out / grid / list is its OMB_EINVAL, before the added ones
  const int32_t* off = offs[0].data();
  expect(check_hvi_paths_grad(&err, 2, 3, 0, nullptr, al, 4, 4, al, 8, off, al, al, al, al, al), OMB_EINVAL, "null y");
  expect(check_hvi_paths_grad(&err, 2, 3, 6, al, al, 4, 4, al, 8, off, al, nullptr, al, al, al), OMB_EINVAL, "null out");
  expect(check_hvi_paths_grad(&err, 2, 3, 6, al, al, 4, 4, nullptr, 8, off, al, al, al, al, al), OMB_EINVAL, "null grid");
  expect(check_hvi_paths_grad(&err, 2, 3, 6, off4, al, 4, 4, al, 8, off, al, al, al, al, al), OMB_EINVAL, "y off 8");
  expect(check_hvi_paths_grad(&err, 2, 3, 6, al, al, 4, 4, al, 8, off, mem + 2, al, al, al, al), OMB_EINVAL,
         "boxes off 4");
  expect(check_hvi_paths_grad(&err, 2, 3, 6, al, al, 4, 4, al, 8, off, off4, al, al, al, al), OMB_OK, "boxes on 4");
  expect(check_hvi_paths_grad(&err, 2, 3, 6, al, al, 4, 4, al, 8, off, al, al, al, nullptr, nullptr), OMB_OK,
         "no per-path outputs");
  expect(check_hvi_paths_grad(&err, 2, 3, 6, nullptr, nullptr, 0, 0, al, 8, off, al, nullptr, nullptr, nullptr, nullptr),
         OMB_OK, "N = 0 without device pointers");
}

int main() {
  sweep_paths_grad();
  sweep_hvi_paths_grad();
  printf("omb_paths_grad_check: %ld calls, %ld mismatches\n", calls, bad);
  return bad ? 1 : 0;
}
