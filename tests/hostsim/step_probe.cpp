// TEST INFRASTRUCTURE: the rules of osqp-python_amd/csrc/step_rules.h (one text, compiled for the batch kernels, the single-QP kernels and the host driver)
// behind a C ABI, so that the CPU tier can exercise each rule on its own (tests/test_step_rules.py).  Built with -ffp-contract=off: what a rule returns
// is compared with == against a restatement with the same order of operations.  Never part of the product.
#include "../../osqp-python_amd/csrc/step_rules.h"

using namespace osqp_hip;

extern "C" {
// consts4: kRowLooseFrac, kRowEqTol, kRowRhoLoose, kRowEqWeight
void sr_consts(double *c) { c[0] = kRowLooseFrac; c[1] = kRowEqTol; c[2] = kRowRhoLoose; c[3] = kRowEqWeight; }
double sr_nanmax(double r, double a) { return nanmax(r, a); }
int sr_row_class(double l, double u, int rho_is_vec) { return row_class(l, u, rho_is_vec); }
double sr_row_rho(int cls, double rho_bar, double rho_eq) { return row_rho(cls, rho_bar, rho_eq); }
double sr_eq_weight(int no_inequality_row, double mixed) { return eq_weight(no_inequality_row != 0, mixed); }
int sr_upper_is_finite(double u) { return upper_is_finite(u); }
int sr_lower_is_finite(double l) { return lower_is_finite(l); }
int sr_adx_violates(double a, double l, double u, double thr) { return adx_violates(a, l, u, thr); }
double sr_support_term(double l, double u, double dy) { return support_term(l, u, dy); }
double sr_support_finite(double l, double u, double y) { return support_finite(l, u, y); }
double sr_clamp_lower(double l) { return clamp_lower(l); }
double sr_clamp_upper(double u) { return clamp_upper(u); }
double sr_in_q(double c, double Dj, double q) { return in_q(c, Dj, q); }
double sr_in_l(double Ei, double l) { return in_l(Ei, l); }
double sr_in_u(double Ei, double u) { return in_u(Ei, u); }
double sr_in_x(double x, double Dinvj) { return in_x(x, Dinvj); }
double sr_in_y(double y, double Einvi, double c) { return in_y(y, Einvi, c); }
// out3: z, y, dy
void sr_step_row(double alpha, double a, double rho, double z, double y, double l, double u, double *out3) {
  const StepRow s = step_row(alpha, a, rho, z, y, l, u);
  out3[0] = s.z; out3[1] = s.y; out3[2] = s.dy;
}
// out2: x, dx
void sr_step_col(double alpha, double xs, double x, double *out2) { const StepCol s = step_col(alpha, xs, x); out2[0] = s.x; out2[1] = s.dx; }
// The residual rows of a dense problem, rows folded in index order by ONE accumulator each and stored: A m x n and P n x n row-major; R22: the fields of
// TermRes in their order.  The products are formed as the kernels form them: sp = ((P + sigma I) x)_j, sa = (A' y)_j.
void sr_residuals(int m, int n, const double *A, const double *P, double sigma, const double *x, const double *z, const double *y, const double *dx, const double *dy,
                  const double *q, const double *l, const double *u, const double *D, const double *E, double *R22) {
  ResRowsA ra; ResRowsB rb;
  for (int i = 0; i < m; i++) {
    double ax = 0.0;
    for (int j = 0; j < n; j++) ax += A[i * n + j] * x[j];
    res_row_a(ra, ax, z[i], dy[i], l[i], u[i], E[i], 1.0 / E[i]);
  }
  for (int j = 0; j < n; j++) {
    double sp = 0.0, sa = 0.0;
    for (int k = 0; k < n; k++) sp += (P[j * n + k] + (k == j ? sigma : 0.0)) * x[k];
    for (int i = 0; i < m; i++) sa += A[i * n + j] * y[i];
    res_row_b(rb, sp, sa, sigma, x[j], q[j], dx[j], D[j], 1.0 / D[j]);
  }
  TermRes R;
  res_store(R, ra, rb);
  static_assert(sizeof(TermRes) == 22 * sizeof(double), "TermRes: 22 doubles");
  __builtin_memcpy(R22, &R, sizeof(R));
}
// bit 0: low, bit 1: upp
int sr_polish_active(double z, double l, double u, double y) { const RowActive a = polish_active(z, l, u, y); return (a.low ? 1 : 0) | (a.upp ? 2 : 0); }
int sr_adjoint_active(double z, double l, double u, double y) { const RowActive a = adjoint_active(z, l, u, y); return (a.low ? 1 : 0) | (a.upp ? 2 : 0); }
// out2: z, y
void sr_normal_cone(double t, double l, double u, double *out2) { const ConeRow c = normal_cone(t, l, u); out2[0] = c.z; out2[1] = c.y; }
int sr_polish_accept(double pri, double dua, double pri0, double dua0) { return polish_accept(pri, dua, pri0, dua0); }
}
