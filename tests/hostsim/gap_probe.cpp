// gap_probe.cpp -- the duality-gap rules of the batch family (term_rules.h: term_dual_obj, term_gap_ok, batch_check_gap, batch_record_gap) and the
// support term they are fed (step_rules.h support_finite) behind a C ABI, for tests/test_batch_gap_rules.py.  Plain g++, no device: a block goes through
// the calls in the order k_batch_admm and k_ls_decide make them -- term_info, term_dual_obj, the subtraction, batch_check_gap.
#include "../../osqp-python_amd/csrc/step_rules.h"
#include "../../osqp-python_amd/csrc/term_rules.h"

using namespace osqp_hip;

namespace {
TermSet gp_set(const double *v) { return {v[0], v[1], v[2], v[3], v[4], v[5], (int)v[6], (int)v[7], (int)v[8]}; }
TermRes gp_res(const double *v) {
  TermRes R;
  R.pri_u = v[0]; R.ax_u = v[1]; R.z_u = v[2]; R.pri_s = v[3]; R.ax_s = v[4]; R.z_s = v[5]; R.dy_u = v[6]; R.dy_s = v[7]; R.pinf_lhs = v[8];
  R.dua_u = v[9]; R.px_u = v[10]; R.aty_u = v[11]; R.dua_s = v[12]; R.px_s = v[13]; R.aty_s = v[14]; R.dxn_u = v[15]; R.dxn_s = v[16]; R.qn_u = v[17]; R.qn_s = v[18];
  R.xpx = v[19]; R.qx = v[20]; R.qdx = v[21];
  return R;
}
}  // namespace

extern "C" {
// one check with the setting gap_on and the support sum supp; out: obj (after the status conventions), prim_res, dual_res, second stages asked for
// (bit 0 A' dy, 1 P dx, 2 A dx), the A dx threshold, dual_obj, gap
int gp_check(const double *set9, const double *R22, int iter, int max_iter, int at_check, const double *stage2, int gap_on, double supp, double *out) {
  const TermSet s = gp_set(set9); const TermRes R = gp_res(R22);
  int asked = 0; double thr = NAN;
  term_info(s, R, &out[0], &out[1], &out[2]);
  const double dual_obj = gap_on ? term_dual_obj(s, R, supp) : 0.0, gap = gap_on ? out[0] - dual_obj : 0.0;
  const int st = batch_check_gap(s, R, out[1], out[2], iter, max_iter, at_check != 0,
                                 [&](double &u, double &v) { asked |= 1; u = stage2[0]; v = stage2[1]; }, [&](double &u, double &v) { asked |= 2; u = stage2[2]; v = stage2[3]; },
                                 [&](double t) { asked |= 4; thr = t; return stage2[4] != 0.0; }, &out[0], gap_on != 0, dual_obj, gap);
  out[3] = asked; out[4] = thr; out[5] = dual_obj; out[6] = gap;
  return st;
}
// the check without the setting, as every caller made it before there was one: batch_check
int gp_check_plain(const double *set9, const double *R22, int iter, int max_iter, int at_check, const double *stage2, double *out) {
  const TermSet s = gp_set(set9); const TermRes R = gp_res(R22);
  int asked = 0; double thr = NAN;
  term_info(s, R, &out[0], &out[1], &out[2]);
  const int st = batch_check(s, R, out[1], out[2], iter, max_iter, at_check != 0,
                             [&](double &u, double &v) { asked |= 1; u = stage2[0]; v = stage2[1]; }, [&](double &u, double &v) { asked |= 2; u = stage2[2]; v = stage2[3]; },
                             [&](double t) { asked |= 4; thr = t; return stage2[4] != 0.0; }, &out[0]);
  out[3] = asked; out[4] = thr;
  return st;
}
int gp_gap_ok(const double *set9, double obj, double dual_obj, double gap, int approx) { return term_gap_ok(gp_set(set9), obj, dual_obj, gap, approx != 0); }
// batch_record, then column 11 the way the kernels write it
void gp_record(double *rc12, int status, double gap) {
  batch_record(rc12, status, 75, -2.5, 1e-7, 2e-7, 0.3, 2, 410.0, 0.25);
  batch_record_gap(rc12, status, gap);
}
// sum_i support_finite(l_i, u_i, y_i) in index order
double gp_supp(int m, const double *l, const double *u, const double *y) {
  double s = 0.0;
  for (int i = 0; i < m; i++) s += support_finite(l[i], u[i], y[i]);
  return s;
}
}
