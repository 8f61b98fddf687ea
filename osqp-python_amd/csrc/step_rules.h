// step_rules.h -- the body of an ADMM iteration as plain functions on scalars: the class and the rho of a constraint row, what counts as a finite bound,
// how a problem's vectors are scaled on the way in, the z / y and x steps, what one row of A and one row of B = [P + sigma I | A'] add to the residual
// norms, and the active-set / normal-cone / accept rules of polish and of the adjoint.  ONE text for the places that state one of them: the batch family
// (batch_hip.hip k_batch_admm / k_batch_wave / k_batch_adjoint, lockstep_hip.hip), the single-QP path's rho, bound-scaling, normal-cone and A dx kernels
// and the support terms of its residual kernel (backend_hip.hip, adjoint_hip.hip) and the host driver (engine.cpp, engine_api.cpp;
// tests/hostsim/backend_host.cpp).  Not here: the single-QP hot kernels (pcg_hip.hip, woodbury_hip.hip, wbdirect_hip.hip), which multiply by a stored
// 1 / rho where step_row divides; the residual rows of k_batch_admm and k_batch_wave and the rho line of k_batch_admm, kept in those kernels' own text
// for the reasons given there (profiles/step_rules_ab.txt); the eight maxima of the single-QP residual kernel (its own accumulators and partial slots).
// Compiles for host and device and under plain g++ (tests/hostsim/step_probe.cpp, tests/test_step_rules.py); nothing here knows a parameter block, a
// vector, LDS or a lane.  The order of the floating-point operations in every expression is part of the contract: the routes are compared bit for bit.
#pragma once
#include "term_rules.h"

namespace osqp_hip {

// the maximum that lets a NaN through (fmax drops it): every max-norm of the residuals is folded with it, so a NaN iterate ends as OSQP_NON_CVX
OSQP_HDI double nanmax(double r, double a) { return (a > r || a != a) ? a : r; }

// ---------------------------------------------------------------------------------------------------------------- rows: class, rho, finite sides
constexpr double kRowLooseFrac = 1e-4;            // MIN_SCALING: a bound beyond OSQP_INFTY times this is no bound (_osqp.py:44, :508-509)
constexpr double kRowEqTol = 1e-4;                // RHO_TOL: u - l below this is an equality (_osqp.py:28, :512)
constexpr double kRowRhoLoose = 1e-6;             // RHO_MIN: rho of a loose row, whatever rho_bar is (_osqp.py:25, :520)
constexpr double kRowEqWeight = 1e3;              // RHO_EQ_OVER_RHO_INEQ (_osqp.py:27, :521)

OSQP_HDI bool upper_is_finite(double u) { return u < OSQP_INFTY * kRowLooseFrac; }           // _osqp.py:861-872, :811-813
OSQP_HDI bool lower_is_finite(double l) { return l > -OSQP_INFTY * kRowLooseFrac; }
// constraint class of a row from its SCALED bounds: -1 loose, 1 equality, 0 inequality (_osqp.py:505-518); without rho_is_vec every row is an inequality
OSQP_HDI int row_class(double l, double u, int rho_is_vec) {
  const int ty = (l < -OSQP_INFTY * kRowLooseFrac && u > OSQP_INFTY * kRowLooseFrac) ? -1 : ((u - l < kRowEqTol) ? 1 : 0);
  return rho_is_vec ? ty : 0;
}
// rho of a row (_osqp.py:520-522); rho_eq = (equality weight) * rho_bar is formed by the caller: a kernel that keeps three values per problem instead of
// a rho vector forms it once
OSQP_HDI double row_rho(int cls, double rho_bar, double rho_eq) { return cls == -1 ? kRowRhoLoose : (cls == 1 ? rho_eq : rho_bar); }
// equality weight of a problem: the reference's where no inequality row exists, else the caller's mixed factor (engine.cpp classify_constraints)
OSQP_HDI double eq_weight(bool no_inequality_row, double mixed) { return no_inequality_row ? kRowEqWeight : mixed; }
// a row of A dx lies beyond thr on a finite side of its bounds (is_dual_infeasible, _osqp.py:855-872)
OSQP_HDI bool adx_violates(double a, double l, double u, double thr) { return (upper_is_finite(u) && a > thr) || (lower_is_finite(l) && a < -thr); }
// a row's term of  u' max(dy, 0) + l' min(dy, 0)  (is_primal_infeasible, _osqp.py:811-813)
OSQP_HDI double support_term(double l, double u, double dy) { return u * fmax(dy, 0.0) + l * fmin(dy, 0.0); }
// a row's term of the support function of [l, u] at y over the finite sides (dual objective, _osqp.py:811-813 on y); 0 where the side is infinite
OSQP_HDI double support_finite(double l, double u, double y) {
  return (y > 0.0 && upper_is_finite(u)) ? u * y : ((y < 0.0 && lower_is_finite(l)) ? l * y : 0.0);
}

// ---------------------------------------------------------------------------------------------------------------- load rules
// A problem's vectors arrive unscaled (update_lin_cost _osqp.py:1328, update_bounds :1357-1358, warm_start :1505-1506):
//   q <- c D q,  l, u <- E clamp(l, u),  x <- Dinv x,  y <- c Einv y   -- the products in exactly this order
OSQP_HDI double clamp_lower(double l) { return fmax(l, -OSQP_INFTY); }
OSQP_HDI double clamp_upper(double u) { return fmin(u, OSQP_INFTY); }
OSQP_HDI double in_q(double c, double Dj, double q) { return c * Dj * q; }
OSQP_HDI double in_l(double Ei, double l) { return Ei * clamp_lower(l); }
OSQP_HDI double in_u(double Ei, double u) { return Ei * clamp_upper(u); }
OSQP_HDI double in_x(double x, double Dinvj) { return x * Dinvj; }
OSQP_HDI double in_y(double y, double Einvi, double c) { return y * Einvi * c; }

// ---------------------------------------------------------------------------------------------------------------- step rules
// z, y of a row from a = (A x~)_i (update_z / update_y, _osqp.py:678-703), the batch family's dividing form  zr + y / rho.
// The relaxed value is a sum of two products: which of them a compiler contracts into an FMA depends on what surrounds the call, so the FMA is WRITTEN
// here (alpha a exact, (1 - alpha) z rounded: what every batch kernel has always computed) -- as in step_col.  No other expression of this file has two
// products in one sum, except support_term, whose callers (lockstep_hip.hip FResM, backend_hip.hip EKr1) compile to one form.
struct StepRow { double z, y, dy; };
OSQP_HDI StepRow step_row(double alpha, double a, double rho, double z, double y, double l, double u) {
  const double zr = fma(alpha, a, (1.0 - alpha) * z);
  const double zn = fmin(fmax(zr + y / rho, l), u);
  const double dy = rho * (zr - zn);
  return {zn, y + dy, dy};
}
// x of a column from x~ (update_x, _osqp.py:660-668): (1 - alpha) x exact, alpha x~ rounded
struct StepCol { double x, dx; };
OSQP_HDI StepCol step_col(double alpha, double xs, double x) {
  const double xn = fma(1.0 - alpha, x, alpha * xs);
  return {xn, xn - x};
}

// ---------------------------------------------------------------------------------------------------------------- residual rows
// What the rows of A (ResRowsA) and of B = [P + sigma I | A'] (ResRowsB) fold to: the max-type fields first, then the sums; TermRes's names.  A caller
// folds its rows into one of these with res_row_a / res_row_b, reduces every field over its threads in its own way (all start from 0, the identity of
// the sums and of the maxima of magnitudes), fills a pair with the reduced values and hands it to res_store.  Named fields: indexed accumulators end in scratch.
struct ResRowsA { double pri_u = 0, ax_u = 0, z_u = 0, pri_s = 0, ax_s = 0, z_s = 0, dy_u = 0, dy_s = 0, pinf_lhs = 0; };
struct ResRowsB { double dua_u = 0, px_u = 0, aty_u = 0, dua_s = 0, px_s = 0, aty_s = 0, dxn_u = 0, dxn_s = 0, qn_s = 0, qn_u = 0, xpx = 0, qx = 0, qdx = 0; };
// row i of A: ax = (A x)_i; Ei, Einvi: the equilibration's entries (_osqp.py:728-751, :796-813)
OSQP_HDI void res_row_a(ResRowsA &r, double ax, double z, double dy, double l, double u, double Ei, double Einvi) {
  const double pr = ax - z;
  r.pri_u = nanmax(r.pri_u, fabs(Einvi * pr)); r.ax_u = nanmax(r.ax_u, fabs(Einvi * ax)); r.z_u = nanmax(r.z_u, fabs(Einvi * z));
  r.pri_s = nanmax(r.pri_s, fabs(pr)); r.ax_s = nanmax(r.ax_s, fabs(ax)); r.z_s = nanmax(r.z_s, fabs(z));
  r.dy_u = nanmax(r.dy_u, fabs(Ei * dy)); r.dy_s = nanmax(r.dy_s, fabs(dy));
  r.pinf_lhs += support_term(l, u, dy);
}
// row j of B: sp = ((P + sigma I) x)_j, sa = (A' y)_j; Dj, Dinvj: the equilibration's entries (_osqp.py:766-794, :836, :705-712, :846)
OSQP_HDI void res_row_b(ResRowsB &r, double sp, double sa, double sigma, double x, double q, double dx, double Dj, double Dinvj) {
  const double px = sp - sigma * x, dr = px + q + sa;
  r.dua_u = nanmax(r.dua_u, fabs(Dinvj * dr)); r.px_u = nanmax(r.px_u, fabs(Dinvj * px)); r.aty_u = nanmax(r.aty_u, fabs(Dinvj * sa));
  r.dua_s = nanmax(r.dua_s, fabs(dr)); r.px_s = nanmax(r.px_s, fabs(px)); r.aty_s = nanmax(r.aty_s, fabs(sa));
  r.dxn_u = nanmax(r.dxn_u, fabs(Dj * dx)); r.dxn_s = nanmax(r.dxn_s, fabs(dx)); r.qn_s = nanmax(r.qn_s, fabs(q)); r.qn_u = nanmax(r.qn_u, fabs(Dinvj * q));
  r.xpx += x * px; r.qx += q * x; r.qdx += q * dx;
}
// the REDUCED values as the termination rules read them
OSQP_HDI void res_store(TermRes &R, const ResRowsA &a, const ResRowsB &b) {
  R.pri_u = a.pri_u; R.ax_u = a.ax_u; R.z_u = a.z_u; R.pri_s = a.pri_s; R.ax_s = a.ax_s; R.z_s = a.z_s; R.dy_u = a.dy_u; R.dy_s = a.dy_s; R.pinf_lhs = a.pinf_lhs;
  R.dua_u = b.dua_u; R.px_u = b.px_u; R.aty_u = b.aty_u; R.dua_s = b.dua_s; R.px_s = b.px_s; R.aty_s = b.aty_s; R.dxn_u = b.dxn_u; R.dxn_s = b.dxn_s;
  R.qn_s = b.qn_s; R.qn_u = b.qn_u; R.xpx = b.xpx; R.qx = b.qx; R.qdx = b.qdx;
}

// ---------------------------------------------------------------------------------------------------------------- polish / adjoint rules
// active rows guessed from (z, y) (_osqp.py:1719-1720); a row active on both sides enters once, at its lower bound
struct RowActive { bool low, upp; };
OSQP_HDI RowActive polish_active(double z, double l, double u, double y) {
  const bool low = z - l < -y;
  return {low, !low && (u - z < y)};
}
// the adjoint's override: an equality row (unscaled l == u) is always active, on the side its multiplier points to
OSQP_HDI RowActive adjoint_active(double z, double l, double u, double y) {
  RowActive a = polish_active(z, l, u, y);
  if (l == u) { a.low = y < 0.0; a.upp = !a.low; }
  return a;
}
// normal-cone projection of (z, y) from t = z + y (project_normalcone, _osqp.py:670-674, :1773-1780)
struct ConeRow { double z, y; };
OSQP_HDI ConeRow normal_cone(double z_plus_y, double l, double u) {
  const double zc = fmin(fmax(z_plus_y, l), u);
  return {zc, z_plus_y - zc};
}
// polish is kept when it improved both residuals, or one while the other was already negligible (_osqp.py:1786-1793)
OSQP_HDI bool polish_accept(double pri, double dua, double pri0, double dua0) {
  return (pri < pri0 && dua < dua0) || (pri < pri0 && dua0 < 1e-10) || (dua < dua0 && pri0 < 1e-10);
}

}  // namespace osqp_hip
