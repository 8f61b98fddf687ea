// polish_err_probe.cpp -- term_rules.h's error measure of the polish recurrence behind a C interface, for tests/test_polish_err_rule.py: plain g++, no device.
#include "../../osqp-python_amd/csrc/term_rules.h"

using namespace osqp_hip;

extern "C" {
double pe_err(double pri_s, double ax_s, double z_s, double dua_s, double aty_s, double px_s, double qn_s) {
  return recurrence_err_polish(pri_s, ax_s, z_s, dua_s, aty_s, px_s, qn_s);
}
}
