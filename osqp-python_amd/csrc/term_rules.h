// term_rules.h -- when a QP is finished, what its rho should be and what its caller gets back, as plain functions on scalars: ONE text for every
// place that decides it.  policy.h (the single-QP driver: host + backend_hip.hip k_decide) builds its Ctl rules from the first part -- the host driver
// (engine.cpp, engine_api.cpp) keeps no text of its own: the approximate pass at max_iter, the info fields of a polished point and the statuses'
// objective values are these rules too (profiles/host_rules_ab.txt: bit for bit what its former transcriptions gave); the batch family
// (batch_hip.hip k_batch_admm / k_batch_wave, lockstep_hip.hip k_ls_decide / k_ls_store_*) calls the second part.  Compiles for host and device and under
// plain g++ (tests/hostsim/policy_probe.cpp, tests/test_batch_rules.py); nothing here knows a Ctl, a parameter block, a vector or LDS.  The order of the
// floating-point operations in every expression is part of the contract: results are compared bit for bit across the kernels.
#pragma once
#include <math.h>

#include "../../include/osqp_hip.h"

#if defined(__HIPCC__)
#define OSQP_HD __host__ __device__
#else
#define OSQP_HD
#endif
#ifndef OSQP_HDI
#define OSQP_HDI OSQP_HD inline __attribute__((always_inline))
#endif

namespace osqp_hip {

constexpr double kPolRhoMin = 1e-6, kPolRhoMax = 1e6;            // _osqp.py:25-26
constexpr double kPolCgTolAbsMin = 1e-13;
OSQP_HDI double pol_clamp_rho(double r) { return fmin(fmax(r, kPolRhoMin), kPolRhoMax); }

// ---------------------------------------------------------------------------------------------------------------- the rules proper
// What the residual passes reduce to (_u: unscaled, _s: scaled; infinity norms unless noted)
struct TermRes {
  double pri_u, ax_u, z_u, pri_s, ax_s, z_s;        // A x - z, A x, z                                  (_osqp.py:728-751)
  double dy_u, dy_s, pinf_lhs;                      // dy;  u' max(dy, 0) + l' min(dy, 0)               (:796-813)
  double dua_u, px_u, aty_u, dua_s, px_s, aty_s;    // P x + q + A' y, P x, A' y                        (:766-794)
  double dxn_u, dxn_s, qn_u, qn_s;                  // dx;  q (qn_u: Dinv q)                            (:836)
  double xpx, qx, qdx;                              // x' P x, q' x, q' dx (sums)                       (:705-712, :846)
};
struct TermSet {
  double eps_abs, eps_rel, eps_pinf, eps_dinf, c, cinv;
  int m, unscaled, scaling;                         // unscaled: scaling && !scaled_termination
};
struct TermSide { bool ok, need; double nd; };              // one residual test: passed; else need: the first stage of that side's infeasibility test
                                                            // passed and its second stage decides, nd: ||dy|| / ||dx|| of the pending test
struct TermStage1 { bool non_cvx, pri_ok, dua_ok, need_pinf, need_dinf; double nd_p, nd_d; };

// info fields of a check (_osqp.py:705-764)
OSQP_HDI void term_info(const TermSet &s, const TermRes &R, double *obj, double *prim_res, double *dual_res) {
  *obj = (0.5 * R.xpx + R.qx) * (s.scaling ? s.cinv : 1.0);
  *prim_res = (s.m == 0) ? 0.0 : (s.unscaled ? R.pri_u : R.pri_s);
  *dual_res = s.unscaled ? s.cinv * R.dua_u : R.dua_s;
}
// rel_kkt_error of a check: the largest of the three relative errors, each over its normalisation + 1e-10 (pn: max(||A x||, ||z||), dn: max(||P x||,
// ||A' y||, ||q||); gap = obj - dual_obj is the CALLER's subtraction: policy.h ctl_info says why).  Only fabs, fmax, the add of a constant and divisions:
// nothing here can be contracted into an FMA, so host and device give the same bits (profiles/host_rules_ab.txt)
OSQP_HDI double term_rel_kkt(int m, double prim_res, double pn, double dual_res, double dn, double gap, double obj, double dual_obj) {
  const double tiny = 1e-10, gn = fmax(fabs(obj), fabs(dual_obj));
  return fmax(fmax(m == 0 ? 0.0 : prim_res / (pn + tiny), dual_res / (dn + tiny)), fabs(gap) / (gn + tiny));
}
// the x10 of the approximate pass (_osqp.py:1012-1016)
OSQP_HDI double term_eps(double eps, bool approx) { return (approx ? 10.0 : 1.0) * eps; }
// The duality gap of a check, for the batch family (settings.check_dualgap; the single-QP driver keeps policy.h ctl_info / ctl_stage1's own text, for the
// reason given there).  supp: sum_i support_finite(l_i, u_i, y_i) on the scaled bounds and dual (step_rules.h).  The gap is the CALLER's subtraction
// obj - dual_obj on the two stored values; the test is ctl_stage1's: |gap| < eps_abs + eps_rel max(|obj|, |dual_obj|), x10 on the approximate pass.  A NaN
// in supp makes dual_obj and the gap NaN and the comparison false: never "solved".
OSQP_HDI double term_dual_obj(const TermSet &s, const TermRes &R, double supp) { return (-0.5 * R.xpx - supp) * (s.scaling ? s.cinv : 1.0); }
OSQP_HDI bool term_gap_ok(const TermSet &s, double obj, double dual_obj, double gap, bool approx) {
  return fabs(gap) < term_eps(s.eps_abs, approx) + term_eps(s.eps_rel, approx) * fmax(fabs(obj), fabs(dual_obj));
}

// check_termination (_osqp.py:998-1077) as far as it goes without another SpMV: the NON_CVX guard (:1025-1028), the residual tests with their
// normalisations (:728-751, :766-794) and the FIRST stage of is_primal_infeasible (:796-813) / is_dual_infeasible (:822-846)
OSQP_HDI bool term_non_cvx(double prim_res, double dual_res) { return prim_res > OSQP_INFTY || dual_res > OSQP_INFTY || prim_res != prim_res || dual_res != dual_res; }
OSQP_HDI TermSide term_pri_side(const TermSet &s, const TermRes &R, double prim_res, bool approx) {
  const double ea = term_eps(s.eps_abs, approx), er = term_eps(s.eps_rel, approx), epi = term_eps(s.eps_pinf, approx);
  if (s.m == 0) return {true, false, 0.0};
  if (prim_res < ea + er * (s.unscaled ? fmax(R.ax_u, R.z_u) : fmax(R.ax_s, R.z_s))) return {true, false, 0.0};
  const double nd = s.unscaled ? R.dy_u : R.dy_s;
  return {false, nd > epi && R.pinf_lhs < -epi * nd, nd};
}
OSQP_HDI TermSide term_dua_side(const TermSet &s, const TermRes &R, double dual_res, bool approx) {
  const double ea = term_eps(s.eps_abs, approx), er = term_eps(s.eps_rel, approx), edi = term_eps(s.eps_dinf, approx);
  const double mx = s.unscaled ? s.cinv * fmax(fmax(R.aty_u, R.px_u), R.qn_u) : fmax(fmax(R.aty_s, R.px_s), R.qn_s);
  if (dual_res < ea + er * mx) return {true, false, 0.0};
  const double nd = s.unscaled ? R.dxn_u : R.dxn_s, sc = s.unscaled ? s.c : 1.0;
  return {false, nd > edi && R.qdx < -sc * edi * nd, nd};
}
OSQP_HDI TermStage1 term_stage1(const TermSet &s, const TermRes &R, double prim_res, double dual_res, bool approx) {
  if (term_non_cvx(prim_res, dual_res)) return {true, false, false, false, false, 0.0, 0.0};
  const TermSide p = term_pri_side(s, R, prim_res, approx), d = term_dua_side(s, R, dual_res, approx);
  return {false, p.ok, d.ok, p.need, d.need, p.need ? p.nd : 0.0, d.need ? d.nd : 0.0};
}
// second stage of is_primal_infeasible (:815-818): ||A' dy|| against eps_prim_inf ||dy||
OSQP_HDI bool term_pinf_holds(const TermSet &s, bool approx, double nd_p, double atdy_u, double atdy_s) {
  return (s.unscaled ? atdy_u : atdy_s) < term_eps(s.eps_pinf, approx) * nd_p;
}
// second stage of is_dual_infeasible (:846-872): ||P dx|| against c eps_dual_inf ||dx||, then every row of A dx against term_adx_thr on its finite side
OSQP_HDI bool term_dinf_pdx_ok(const TermSet &s, bool approx, double nd_d, double pdx_u, double pdx_s) {
  const double sc = s.unscaled ? s.c : 1.0;
  return (s.unscaled ? pdx_u : pdx_s) < sc * term_eps(s.eps_dinf, approx) * nd_d;
}
OSQP_HDI double term_adx_thr(const TermSet &s, bool approx, double nd_d) { return term_eps(s.eps_dinf, approx) * nd_d; }

// compute_rho_estimate (_osqp.py:880-908, scaled quantities), clamped to [RHO_MIN, RHO_MAX]
OSQP_HDI double term_rho_estimate(double rho_bar, const TermRes &R) {
  const double pr = R.pri_s / (fmax(R.ax_s, R.z_s) + 1e-10), du = R.dua_s / (fmax(fmax(R.aty_s, R.px_s), R.qn_s) + 1e-10);
  return pol_clamp_rho(rho_bar * sqrt(pr / (du + 1e-10)));
}

OSQP_HDI bool term_is_pinf(int status) { return status == OSQP_PRIMAL_INFEASIBLE || status == OSQP_PRIMAL_INFEASIBLE_INACCURATE; }
OSQP_HDI bool term_is_dinf(int status) { return status == OSQP_DUAL_INFEASIBLE || status == OSQP_DUAL_INFEASIBLE_INACCURATE; }

// ---------------------------------------------------------------------------------------------------------------- the batch family's layer
// One termination check of a batch problem at ADMM iteration `iter`: the status it ends with, or kBatchGoOn.  The exact pass, then -- at max_iter
// only -- the approximate one (_osqp.py:1264-1266), then OSQP_MAX_ITER_REACHED.  at_check false (a rho adaptation point between checks): nothing is
// tested.  The second-stage quantities come from the caller when a first stage asks for them, and only then:
//   pinf_cb(atdy_u, atdy_s)   ||Dinv A' dy||, ||A' dy||
//   pdx_cb(pdx_u, pdx_s)      ||Dinv P dx||, ||P dx||
//   adx_cb(thr) -> bool       no row of A dx (unscaled: Einv A dx) lies beyond thr on a finite side of its bounds (:855-872)
// k_batch_admm / k_batch_wave run their extra SpMVs and reductions inside them (the decision is uniform over the workgroup / wave: so are the barriers),
// k_ls_decide returns what it has folded already.  *obj follows the status: NAN for OSQP_NON_CVX, +-OSQP_INFTY for the infeasible ones (:1045-1070).
constexpr int kBatchGoOn = 0;
// batch_check_gap: the same check with settings.check_dualgap: gap_on, and then dual_obj (term_dual_obj) and gap = *obj - dual_obj of the point -- "solved"
// additionally needs term_gap_ok on that pass (policy.h ctl_stage1's rule: the infeasibility tests are untouched, they ask for a residual test that FAILED).
// batch_check is batch_check_gap with gap_on false.
template <class PinfCb, class PdxCb, class AdxCb>
OSQP_HDI int batch_check_gap(const TermSet &s, const TermRes &R, double prim_res, double dual_res, int iter, int max_iter, bool at_check, PinfCb &&pinf_cb,
                             PdxCb &&pdx_cb, AdxCb &&adx_cb, double *obj, bool gap_on, double dual_obj, double gap) {
  for (int approx = 0; approx < 2 && at_check; approx++) {
    if (approx && iter < max_iter) break;
    if (term_non_cvx(prim_res, dual_res)) { *obj = NAN; return OSQP_NON_CVX; }
    bool pinf = false, dinf = false;
    const TermSide p = term_pri_side(s, R, prim_res, approx);
    if (p.need) {
      double au = 0.0, as = 0.0;
      pinf_cb(au, as);
      pinf = term_pinf_holds(s, approx, p.nd, au, as);
    }
    const TermSide d = term_dua_side(s, R, dual_res, approx);               // (after the primal side's callable: nothing of it is live across that)
    if (d.need) {
      double pu = 0.0, ps = 0.0;
      pdx_cb(pu, ps);
      if (term_dinf_pdx_ok(s, approx, d.nd, pu, ps)) dinf = adx_cb(term_adx_thr(s, approx, d.nd));
    }
    if (p.ok && d.ok && (!gap_on || term_gap_ok(s, *obj, dual_obj, gap, approx))) return approx ? OSQP_SOLVED_INACCURATE : OSQP_SOLVED;
    if (pinf) { *obj = OSQP_INFTY; return approx ? OSQP_PRIMAL_INFEASIBLE_INACCURATE : OSQP_PRIMAL_INFEASIBLE; }
    if (dinf) { *obj = -OSQP_INFTY; return approx ? OSQP_DUAL_INFEASIBLE_INACCURATE : OSQP_DUAL_INFEASIBLE; }
  }
  return iter >= max_iter ? (int)OSQP_MAX_ITER_REACHED : kBatchGoOn;
}
template <class PinfCb, class PdxCb, class AdxCb>
OSQP_HDI int batch_check(const TermSet &s, const TermRes &R, double prim_res, double dual_res, int iter, int max_iter, bool at_check, PinfCb &&pinf_cb,
                         PdxCb &&pdx_cb, AdxCb &&adx_cb, double *obj) {
  return batch_check_gap(s, R, prim_res, dual_res, iter, max_iter, at_check, pinf_cb, pdx_cb, adx_cb, obj, false, 0.0, 0.0);
}

// adapt_rho (_osqp.py:910-930) with the reference's plain factor test (the single-QP path's square-root / persistence rule is policy.h ctl_rho_rule)
OSQP_HDI bool batch_rho_rule(double rho_bar, double rho_tol, const TermRes &R, double *rho_new) {
  *rho_new = term_rho_estimate(rho_bar, R);
  return *rho_new > rho_tol * rho_bar || *rho_new < rho_bar / rho_tol;
}

// adapt_rho with the single-QP path's test (policy.h ctl_rho_rule is this text on a Ctl; the direct lockstep route runs it per problem, so that a batch
// element takes the path update(q, l, u) + solve() on the handle takes): an update costs that path no refactorisation worth the reference's factor-5
// guard, so `tol` is the setting's tolerance on a square-root scale (the caller's pow), and an estimate that falls on the same side of rho by more than
// sqrt(tol) at two CONSECUTIVE adaptation points is applied as well.  *last_side: the side seen at the previous adaptation point.
OSQP_HDI bool single_rho_rule(double rho_bar, double tol, int persist, const TermRes &R, int *last_side, double *rho_new) {
  const double rn = term_rho_estimate(rho_bar, R);
  *rho_new = rn;
  const double st = sqrt(tol);
  const int side = rn > st * rho_bar ? 1 : (rn < rho_bar / st ? -1 : 0);
  const bool big = rn > tol * rho_bar || rn < rho_bar / tol;
  const bool persistent = persist && side != 0 && side == *last_side;
  *last_side = (big || persistent) ? 0 : side;
  return big || persistent;
}

// PCG tolerance of the batch family's PCG variants: a fraction of the scaled dual residual, absolute (rel_rule: relative to ||rhs||, for a start whose
// dual residual gives no usable value), never loosening, floor 1e-13; a non-finite value leaves the state as it is
OSQP_HDI void batch_tol_init(double cg_frac, double dua_s, double *eps_prev, double *eps_cg, bool *rel_rule) {
  *eps_cg = cg_frac * dua_s; *eps_prev = INFINITY;
  *rel_rule = !(*eps_cg > kPolCgTolAbsMin) || !isfinite(*eps_cg);
}
OSQP_HDI void batch_tol_rule(double cg_frac, double dua_s, double *eps_prev, double *eps_cg, bool *rel_rule) {
  const double e2 = fmax(fmin(cg_frac * dua_s, *eps_prev), kPolCgTolAbsMin);
  if (isfinite(e2)) { *eps_prev = e2; *eps_cg = e2; *rel_rule = false; }
}

// The progress rule of the recurrence polish and the adjoint derivatives run (engine.cpp Engine::run_recurrence on the host; lockstep_hip.hip
// k_ls_adj_decide / k_ls_pol_decide per problem on the device).  recurrence_err_rhs: the reduced system's scaled residuals against its right-hand side (the
// adjoint's measure).  recurrence_err_polish: polish's measure, each residual relative to the products it is the difference of.  recurrence_ends:
// `steps` steps have been taken and the last one left the error `err`; a step that does not bring the error below gain * best counts as no progress;
// the recurrence ends after at least min_steps when the error is negligible or two steps in a row showed no progress, and at max_steps at the latest.
// Comparisons, one product and one quotient: host and device give the same bits.
OSQP_HDI double recurrence_err_rhs(double pri_s, double dua_s, double qn_s, double z_s) {
  return (pri_s < dua_s ? dua_s : pri_s) / ((qn_s < z_s ? z_s : qn_s) + 1e-30);        // (std::max's selects: a NaN goes where it always went)
}
OSQP_HDI double recurrence_err_polish(double pri_s, double ax_s, double z_s, double dua_s, double aty_s, double px_s, double qn_s) {
  const double pn = ax_s < z_s ? z_s : ax_s, d1 = aty_s < px_s ? px_s : aty_s, dn = d1 < qn_s ? qn_s : d1;        // (std::max's selects, as above)
  const double ep = pri_s / (pn + 1e-30), ed = dua_s / (dn + 1e-30);
  return ep < ed ? ed : ep;
}
OSQP_HDI bool recurrence_ends(double err, double gain, int steps, int min_steps, int max_steps, double *best, int *worse) {
  if (!(err < gain * *best)) *worse += 1; else *worse = 0;
  *best = err < *best ? err : *best;
  return (steps >= min_steps && (err < 1e-13 || *worse >= 2)) || steps >= max_steps;
}

// The record of a batch problem (backend.h kBatchRec = 12 doubles; include/osqp_hip.h OSQP_HIP_BATCH_REC): status, iter, obj, prim_res, dual_res, rho,
// rho_updates, pcg_iters, status_polish, polish seconds, rho_estimate (_osqp.py:1275, at the ADMM point), duality_gap (check_dualgap only).  The polish fields
// and the gap are zeroed: the polishing variants, batch_record_gap and the OSQP_HIP_KTRACE build overwrite theirs afterwards.
OSQP_HDI void batch_record(double *rc, int status, int iter, double obj, double prim_res, double dual_res, double rho_bar, int rho_updates, double pcg,
                           double rho_est) {
  rc[0] = status; rc[1] = iter; rc[2] = obj; rc[3] = prim_res; rc[4] = dual_res; rc[5] = rho_bar; rc[6] = rho_updates; rc[7] = pcg;
  rc[8] = 0.0; rc[9] = 0.0; rc[10] = rho_est; rc[11] = 0.0;
}
// Column 11 with settings.check_dualgap, written AFTER batch_record (and again after an accepted polish, with the polished point's gap): the duality gap of
// the point the record describes; NAN where the record describes no point (x or y is a certificate, or the iterates are not finite).
OSQP_HDI void batch_record_gap(double *rc, int status, double gap) { rc[11] = (term_is_pinf(status) || term_is_dinf(status) || status == OSQP_NON_CVX) ? NAN : gap; }

// What a batch problem's caller reads in x / y: x = D x, y = cinv E y (_osqp.py:1110-1112); for an infeasible problem the certificate (dx for dual, dy
// for primal infeasibility: :815-820, :870-878) in one and NAN in the other.  Dj, Ei: the equilibration's entries; xj, dxj, yi, dyi: scaled iterates.
OSQP_HDI double batch_out_x(int status, int unscaled, int scaling, double Dj, double xj, double dxj) {
  return term_is_dinf(status) ? (unscaled ? Dj * dxj : dxj) : (term_is_pinf(status) ? NAN : (scaling ? Dj * xj : xj));
}
OSQP_HDI double batch_out_y(int status, int unscaled, int scaling, double cinv, double Ei, double yi, double dyi) {
  return term_is_pinf(status) ? (unscaled ? Ei * dyi : dyi) : (term_is_dinf(status) ? NAN : (scaling ? cinv * Ei * yi : yi));
}

}  // namespace osqp_hip
