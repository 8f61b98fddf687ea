// recurrence_probe.cpp -- term_rules.h's recurrence rule behind a C interface, for tests/test_recurrence_rule.py: plain g++, no device.
#include "../../osqp-python_amd/csrc/term_rules.h"

using namespace osqp_hip;

extern "C" {
// runs the rule over errs[0 .. count): returns the step (1-based) at which recurrence_ends first answers true, 0 if it never does; best / worse: the state then
int rr_run(const double *errs, int count, double gain, int min_steps, int max_steps, double *best_out, int *worse_out) {
  double best = INFINITY;
  int worse = 0, ended = 0;
  for (int s = 0; s < count && !ended; s++)
    if (recurrence_ends(errs[s], gain, s + 1, min_steps, max_steps, &best, &worse)) ended = s + 1;
  *best_out = best; *worse_out = worse;
  return ended;
}
double rr_err(double pri_s, double dua_s, double qn_s, double z_s) { return recurrence_err_rhs(pri_s, dua_s, qn_s, z_s); }
}
