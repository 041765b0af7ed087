// Stand-alone driver (ASan + UBSan, CPU only) of the log-space entry points' argument checks in omb_host.cpp:
// check_plan_log (omb_plan_log) and check_log_ei (omb_log_ei) swept over their boundary values, return codes against
// the header's contract — check_plan_log: OMB_ESTATE with no plan, then OMB_EINVAL for `on` outside {0, 1}, then
// OMB_EUNSUP (naming the plan) for a plan without a log form; check_log_ei: check_ei's OMB_EINVAL first, then
// OMB_EUNSUP for OMB_EI_PARETO.
// Built by `make -C optimobo_amd/csrc asan` as build/asan/omb_logacq_check.
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

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
  const int ons[] = {INT_MIN, -1, 0, 1, 2, INT_MAX};
  const char* names[] = {nullptr, "EHVI-2D", ""};
  for (int has : {0, 1})
    for (int on : ons)
      for (const char* refused : names) {
        int want = OMB_OK;
        if (!has) want = OMB_ESTATE;
        else if (on != 0 && on != 1) want = OMB_EINVAL;
        else if (refused) want = OMB_EUNSUP;
        err.clear();
        expect(check_plan_log(&err, has, on, refused), want, "check_plan_log");
        expect(check_plan_log(nullptr, has, on, refused), want, "check_plan_log (no message)");
        if (want != OMB_OK && err.empty()) {
          ++bad;
          fprintf(stderr, "MISMATCH check_plan_log: failure without a message\n");
        }
        if (want == OMB_EUNSUP && refused[0] && err.find(refused) == std::string::npos) {
          ++bad;
          fprintf(stderr, "MISMATCH check_plan_log: the message does not name the plan\n");
        }
      }
  const double epss[] = {-INFINITY, -1.0, -0.0, 0.0, 4.9e-324, 1e-6, INFINITY, NAN};
  const int kinds[] = {INT_MIN, -1, OMB_EI_PLAIN, OMB_EI_PARETO, OMB_EI_CONSTRAINED, 3, INT_MAX};
  const int ks[] = {INT_MIN, -1, 0, 1, 2, 3, OMB_MAX_OBJ, OMB_MAX_OBJ + 1, INT_MAX};
  for (int kind : kinds)
    for (int k : ks)
      for (double ve : epss)
        for (double pe : epss) {
          const bool shape = (kind == OMB_EI_PLAIN && k == 1) || (kind == OMB_EI_PARETO && k == 2) ||
                             (kind == OMB_EI_CONSTRAINED && k >= 2 && k <= OMB_MAX_OBJ);
          int want = OMB_OK;
          if (!shape || !(ve >= 0.0) || !(pe >= 0.0)) want = OMB_EINVAL;
          else if (kind == OMB_EI_PARETO) want = OMB_EUNSUP;
          expect(check_log_ei(&err, kind, k, ve, pe), want, "check_log_ei");
          expect(check_log_ei(nullptr, kind, k, ve, pe), want, "check_log_ei (no message)");
          // where the linear entry accepts, the log entry differs for the Pareto kind alone
          expect(check_ei(nullptr, kind, k, ve, pe) == OMB_OK, want != OMB_EINVAL, "check_ei against check_log_ei");
        }
  printf("omb_logacq_check: %ld calls, %ld mismatches\n", calls, bad);
  return bad ? 1 : 0;
}
