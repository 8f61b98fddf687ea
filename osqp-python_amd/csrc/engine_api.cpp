// engine_api.cpp -- the rest of the C-API surface of the engine: cold / warm start, data and settings updates, the LinSysSolver slot, the batch
// and small-problem paths (one-workgroup-per-QP kernels), statistics and probes.  See engine.hpp.
#include "engine_internal.hpp"

namespace osqp_hip {

// ------------------------------------------------------------------------------------------------ updates
int Engine::cold_start() {                                                               // _osqp.py:636-642
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  be::activate(d_);
  be::zero(d_, d_.x, sizeof(double) * n); be::zero(d_, d_.z, sizeof(double) * m); be::zero(d_, d_.y, sizeof(double) * m);
  be::init_iterates(d_, 1);
  return OSQP_NO_ERROR;
}

int Engine::warm_start(const double *x, const double *y, bool keep_z) {                  // _osqp.py:1493-1545
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  be::activate(d_);
  settings.warm_starting = 1;
  std::vector<double> xi, yi;
  if (reordered_) { if (x) { xi = to_internal_n(x); x = xi.data(); } if (y) { yi = to_internal_m(y); y = yi.data(); } }
  if (be::device_vec_updates()) {                      // raw vectors go up as they are; x = Dinv x, y = c Einv y on the device
    double *sx = d_.w, *sy = d_.t;                     // PCG work vectors are free between solves
    if (x) be::copy_in(d_, sx, x, sizeof(double) * n, 0);
    if (y) be::copy_in(d_, sy, y, sizeof(double) * m, 0);
    be::scale_warm(d_, x ? sx : nullptr, y ? sy : nullptr, c_);
  } else {
    if (x) {
      std::vector<double> xs(n);
      for (int j = 0; j < n; j++) xs[j] = x[j] * Dinv_[j];
      be::h2d(d_, d_.x, xs.data(), sizeof(double) * n);
    }
    if (y) {
      std::vector<double> ys(m);
      for (int i = 0; i < m; i++) ys[i] = y[i] * Einv_[i] * c_;   // inverse of y = cinv E y_scaled (:1112); the C core includes c
      be::h2d(d_, d_.y, ys.data(), sizeof(double) * m);
    }
  }
  be::init_iterates(d_, keep_z ? 2 : 1);                            // z = A x (:1509); keep_z: the caller has put the z iterate in place
  return OSQP_NO_ERROR;
}

int Engine::warm_start_device(const double *x, const double *y, void *stream) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!be::device_vec_updates()) return OSQP_FUNC_NOT_IMPLEMENTED;
  be::activate(d_);
  be::ext_wait(d_);                                 // a batch kernel on a caller's stream may still read this solver's vectors
  settings.warm_starting = 1;
  be::stream_wait(d_, stream);
  if (reordered_) {                                 // the caller's numbering -> the engine's, on the device (PCG work vectors are free between solves)
    if (x) { be::gather(d_, d_.w, x, d_pc_, n); x = d_.w; }
    if (y) { be::gather(d_, d_.t, y, d_pr_, m); y = d_.t; }
  }
  be::scale_warm(d_, x, y, c_);
  be::init_iterates(d_, 1);
  return OSQP_NO_ERROR;
}

int Engine::update_data_vec(const double *q, const double *l, const double *u) {          // _osqp.py:1312-1367
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  be::activate(d_);
  be::ext_wait(d_);                                 // a batch kernel on a caller's stream may still read the bounds / q
  double t0 = now_s();
  std::vector<double> qi, li_, ui_;
  if (reordered_) {
    if (q) { qi = to_internal_n(q); q = qi.data(); }
    if (l) { li_ = to_internal_m(l); l = li_.data(); }
    if (u) { ui_ = to_internal_m(u); u = ui_.data(); }
  }
  if (l || u) {
    if (raw_stale_) ensure_host_vectors();
    for (int i = 0; i < m; i++) {
      double li = l ? l[i] : l0_[i], ui = u ? u[i] : u0_[i];
      if (!(li <= ui)) return OSQP_DATA_VALIDATION_ERROR;                                // :1348-1349
    }
  }
  const bool dev = be::device_vec_updates();
  if (q) { q0_.assign(q, q + n); if (dev) be::copy_in(d_, d_.qraw, q, sizeof(double) * n, 0); else upload_q(); }
  if (l) { l0_.assign(l, l + m); if (dev) be::copy_in(d_, d_.lraw, l, sizeof(double) * m, 0); }
  if (u) { u0_.assign(u, u + m); if (dev) be::copy_in(d_, d_.uraw, u, sizeof(double) * m, 0); }
  if (dev) device_scale_vectors(q != nullptr, l || u);
  else if (l || u) upload_bounds_and_types();                                           // update_rho_vec :526-562
  if (l || u) {
    be::set_rho(d_, rho_bar_);
    be::precond(d_, settings.cg_precond == OSQP_DIAGONAL_PRECONDITIONER);
  }
  set_status(OSQP_UNSOLVED);                                                             // reset_info :932-941
  if (!dev) be::sync(d_);                           // (device path: everything is stream-ordered; the next solve waits for it)
  update_time_acc_ += now_s() - t0;
  return OSQP_NO_ERROR;
}

// q / l / u given by DEVICE pointer (parametric re-solve with the data produced on the GPU, nn/torch.py:136-140): one device-to-device
// copy per vector, then the same kernels.  The bounds are validated on the device BEFORE anything changes (one 4-byte read-back).
int Engine::update_data_vec_device(const double *q, const double *l, const double *u, void *stream) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!be::device_vec_updates()) return OSQP_FUNC_NOT_IMPLEMENTED;
  be::activate(d_);
  be::ext_wait(d_);
  double t0 = now_s();
  be::stream_wait(d_, stream);
  if (reordered_ && (l || u) && !(l && u)) {        // one bound in the caller's numbering against the resident other one: bring it over first
    double *tmp = d_.t;                               // (a rejected call leaves the resident vectors untouched: staged in a PCG work vector)
    be::gather(d_, tmp, l ? l : u, d_pr_, m);
    if (be::count_bad_bounds(d_, l ? tmp : d_.lraw, u ? tmp : d_.uraw) > 0) return OSQP_DATA_VALIDATION_ERROR;
  } else
  if ((l || u) && be::count_bad_bounds(d_, l ? l : d_.lraw, u ? u : d_.uraw) > 0) return OSQP_DATA_VALIDATION_ERROR;
  if (reordered_) {                                 // the resident raw vectors are kept in the engine's numbering: gathers instead of copies
    if (q) be::gather(d_, d_.qraw, q, d_pc_, n);
    if (l) be::gather(d_, d_.lraw, l, d_pr_, m);
    if (u) be::gather(d_, d_.uraw, u, d_pr_, m);
  } else {
    if (q) be::copy_in(d_, d_.qraw, q, sizeof(double) * n, 1);
    if (l) be::copy_in(d_, d_.lraw, l, sizeof(double) * m, 1);
    if (u) be::copy_in(d_, d_.uraw, u, sizeof(double) * m, 1);
  }
  if (q || l || u) raw_stale_ = true;
  device_scale_vectors(q != nullptr, l || u);
  if (l || u) {
    be::set_rho(d_, rho_bar_);
    be::precond(d_, settings.cg_precond == OSQP_DIAGONAL_PRECONDITIONER);
  }
  set_status(OSQP_UNSOLVED);
  update_time_acc_ += now_s() - t0;
  return OSQP_NO_ERROR;
}

int Engine::update_data_mat(const double *Px, const int *Px_idx, int P_n, const double *Ax, const int *Ax_idx, int A_n) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  be::activate(d_);
  be::ext_wait(d_);
  double t0 = now_s();
  const int nzP = P_.nnz(), nzA = A_.nnz();
  // bindings.cpp.in:240-281: idx == NULL means all entries in order.  Both arguments are validated BEFORE anything is changed:
  // a rejected call leaves the host copies (and therefore the next upload) untouched.
  if (Px) {
    if (Px_idx) { for (int k = 0; k < P_n; k++) if (Px_idx[k] < 0 || Px_idx[k] >= nzP) return OSQP_DATA_VALIDATION_ERROR; }
    else if (P_n != nzP && P_n != 0) return OSQP_DATA_VALIDATION_ERROR;
  }
  if (Ax) {
    if (Ax_idx) { for (int k = 0; k < A_n; k++) if (Ax_idx[k] < 0 || Ax_idx[k] >= nzA) return OSQP_DATA_VALIDATION_ERROR; }
    else if (A_n != nzA && A_n != 0) return OSQP_DATA_VALIDATION_ERROR;
  }
  // (reordered problem: the caller's positions in its own CSC arrays -> where those entries live in the permuted ones)
  mat_epoch_ += 1;
  if (Px) for (int k = 0; k < (Px_idx ? P_n : nzP); k++) { const int c = Px_idx ? Px_idx[k] : k; P_.x[reordered_ ? PvalMap_[c] : c] = Px[k]; }
  if (Ax) for (int k = 0; k < (Ax_idx ? A_n : nzA); k++) { const int c = Ax_idx ? Ax_idx[k] : k; A_.x[reordered_ ? AvalMap_[c] : c] = Ax[k]; }
  if (be::device_assembly()) {                                                           // _osqp.py:1443,:1463 on the device
    if (Px) be::h2d(d_, d_.Praw, P_.x.data(), sizeof(double) * nzP);
    if (Ax) be::h2d(d_, d_.Araw, A_.x.data(), sizeof(double) * nzA);
    be::assemble(d_, 1, c_, 1);
    be::f1_refresh(d_); be::wb_refresh(d_); be::wbx_refresh(d_);
  } else {
    std::vector<double> Pxs, Axs;
    scale_matrix_values(Pxs, Axs);
    fill_matrix_values(Pxs, Axs);
  }
  be::precond(d_, settings.cg_precond == OSQP_DIAGONAL_PRECONDITIONER);                   // the "refactor" of :1446,:1466,:1488
  be::init_iterates(d_, 0);                                                              // z~, t0 depend on A; iterates untouched
  set_status(OSQP_UNSOLVED);
  be::sync(d_);
  update_time_acc_ += now_s() - t0;
  return OSQP_NO_ERROR;
}

int Engine::update_rho(double rho) {                                                     // _osqp.py:1579-1597
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  be::activate(d_);
  if (!(rho > 0)) return OSQP_SETTINGS_VALIDATION_ERROR;
  rho_bar_ = clamp_rho(rho); settings.rho = rho_bar_;
  be::set_rho(d_, rho_bar_);
  be::precond(d_, settings.cg_precond == OSQP_DIAGONAL_PRECONDITIONER);
  return OSQP_NO_ERROR;
}

int Engine::update_settings(const OSQPSettings *s) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  be::activate(d_);
  int err = validate_settings(s, false);
  if (err) return err;
  // settings that can change after setup (the reference: "These can be changed without running setup", _osqp.py:128-143)
  settings.max_iter = s->max_iter; settings.eps_abs = s->eps_abs; settings.eps_rel = s->eps_rel;
  settings.eps_prim_inf = s->eps_prim_inf; settings.eps_dual_inf = s->eps_dual_inf; settings.alpha = s->alpha;
  settings.scaled_termination = s->scaled_termination; settings.check_termination = s->check_termination;
  settings.check_dualgap = s->check_dualgap; settings.time_limit = s->time_limit; settings.warm_starting = s->warm_starting;
  settings.verbose = s->verbose; settings.polishing = s->polishing; settings.delta = s->delta;
  settings.polish_refine_iter = s->polish_refine_iter; settings.adaptive_rho = s->adaptive_rho;
  settings.adaptive_rho_interval = s->adaptive_rho_interval; settings.adaptive_rho_fraction = s->adaptive_rho_fraction;
  settings.adaptive_rho_tolerance = s->adaptive_rho_tolerance; settings.cg_max_iter = s->cg_max_iter;
  settings.cg_tol_reduction = s->cg_tol_reduction; settings.cg_tol_fraction = s->cg_tol_fraction;
  if (s->cg_precond != settings.cg_precond) { settings.cg_precond = s->cg_precond; be::precond(d_, settings.cg_precond == OSQP_DIAGONAL_PRECONDITIONER); }
  if (d_.alpha != settings.alpha) { d_.alpha = settings.alpha; drop_graphs(); }     // alpha is baked into captured launches
  have_tol_ = false; cg_budget_ = 0;
  return OSQP_NO_ERROR;
}

// Batch of nbatch QPs that share this solver's (P, A, scaling, settings) and differ in q / l / u -- the reference's
// update-style batching (nn/torch.py:136-164: update(q,l,u) + solve() per element) as ONE kernel launch.
// q: nbatch x n, l/u: nbatch x m (row-major; NULL = this solver's current vector for every problem);
// x: nbatch x n, y: nbatch x m (in: unscaled warm start if warm != 0; out: solution, or certificate for infeasible ones);
// rec: nbatch x kBatchRec = {status_val, iter, obj_val, prim_res, dual_res, rho, rho_updates, pcg_iters, status_polish, polish_time, rho_estimate, reserved}.


// ------------------------------------------------------------------------------------------------ LinSysSolver slot
// The reduced-KKT PCG as a stand-alone linear solver (include/osqp_hip.h), built from the same backend
// operations as the ADMM loop:  kb_rhs  forms  rhs = sigma x - q + A' v  and the PCG start residual, so with  x = 0,
// q = -rhs_x,  v = rho .* rhs_z  it forms exactly the right-hand side of the reduced system;  k1/k2/kv  are the PCG
// iterations (three-kernel form: a solve may be continued past its first budget);  init_iterates(0)  leaves  z~ = A x~.
int Engine::ls_setup(const OSQPCscMatrix *P, const OSQPCscMatrix *A, const double *rho_vec, const OSQPSettings *s) {
  if (!P || !A || !rho_vec || !s) return OSQP_DATA_VALIDATION_ERROR;
  OSQPSettings st = *s;
  st.scaling = 0; st.linsys_solver = OSQP_INDIRECT_SOLVER; st.verbose = 0; st.polishing = 0;   // the matrices arrive scaled
  const int nn = P->n, mm = A->m;
  std::vector<double> q(nn, 0.0), l(mm, -OSQP_INFTY), u(mm, OSQP_INFTY);
  no_reorder_ = true;                                 // (the slot's vectors -- rhs, rho_vec, warm start -- are exchanged in the caller's numbering)
  int err = setup(P, q.data(), A, l.data(), u.data(), mm, nn, &st);
  if (err) return err;
  d_.fused = 0; d_.f1.on = 0; d_.kf.on = 0; d_.wb.on = 0;
  return ls_set_rho_vec(rho_vec);
}

int Engine::ls_set_rho_vec(const double *rho_vec) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!rho_vec) return OSQP_DATA_VALIDATION_ERROR;
  be::activate(d_);
  ls_rho_.assign(rho_vec, rho_vec + m);
  std::vector<double> rinv(m);
  for (int i = 0; i < m; i++) { if (!(ls_rho_[i] > 0)) return OSQP_DATA_VALIDATION_ERROR; rinv[i] = 1.0 / ls_rho_[i]; }
  be::h2d(d_, d_.rho, ls_rho_.data(), sizeof(double) * m);
  be::h2d(d_, d_.rho_inv, rinv.data(), sizeof(double) * m);
  be::precond(d_, settings.cg_precond == OSQP_DIAGONAL_PRECONDITIONER);
  be::init_iterates(d_, 0);                        // t0 = rho .* (A x~) must match the new rho
  be::sync(d_);
  return OSQP_NO_ERROR;
}

int Engine::ls_warm_start(const double *x) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!x) return OSQP_DATA_VALIDATION_ERROR;
  be::activate(d_);
  be::h2d(d_, d_.xs, x, sizeof(double) * n);
  be::init_iterates(d_, 0);
  be::sync(d_);
  return OSQP_NO_ERROR;
}

int Engine::ls_solve(double *b, double tol_rel, double tol_abs, int *iters) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!b) return OSQP_DATA_VALIDATION_ERROR;
  be::activate(d_);
  std::vector<double> nq(n), v(m);
  for (int j = 0; j < n; j++) nq[j] = -b[j];
  for (int i = 0; i < m; i++) v[i] = ls_rho_[i] * b[n + i];
  be::h2d(d_, d_.q, nq.data(), sizeof(double) * n);
  be::h2d(d_, d_.v, v.data(), sizeof(double) * m);
  be::zero(d_, d_.x, sizeof(double) * n);
  be::set_pcg_tol(d_, tol_rel, tol_abs);
  be::kb_rhs(d_);
  const int cap = std::min(settings.cg_max_iter, kMaxCg);
  int flags[F_COUNT] = {0};
  int done = 0;
  for (int i0 = 0; i0 < cap && !done;) {           // budget: what the previous solve needed + 2, then doubling
    const int bud = std::min(cap - i0, std::max(4, i0 == 0 ? cg_budget_ + 2 : i0));
    for (int i = i0; i < i0 + bud; i++) { be::k1(d_, i); be::k2(d_, i); be::kv(d_, i); }
    i0 += bud;
    be::k1(d_, i0 < cap ? i0 : cap);               // the stopping test of the last update (its SpMV is wasted only if the cap was hit)
    be::fetch_flags(d_, flags);
    done = flags[F_DONE];
    if (!done && i0 >= cap) break;
    if (!done) { be::k2(d_, i0); be::kv(d_, i0); i0++; }
  }
  cg_budget_ = done ? flags[F_ITERS] : cap;
  if (iters) *iters = cg_budget_;
  be::init_iterates(d_, 0);                        // z~ = A x~ ; t0 for the next solve's start residual
  be::d2h(d_, b, d_.xs, sizeof(double) * n);
  if (m > 0) be::d2h(d_, b + n, d_.zt, sizeof(double) * m);
  return OSQP_NO_ERROR;
}

// ------------------------------------------------------------------------------------------------ batch path, direct solve
// Symbolic preparation of the banded-Cholesky linear solve of the batch kernel (batch_hip.hip): the pattern of
// K = P + sigma I + A' diag(rho) A, a reverse Cuthill-McKee ordering of it, the band slot of every P entry, and for
// every band slot the list of products A_ia A_ib that rho_i multiplies.  The reference's builtin algebra factorises the
// KKT matrix with QDLDL after an AMD ordering; for QPs small enough to live in one workgroup's LDS the
// reduced matrix K (n x n, SPD) under a BANDWIDTH-reducing ordering is the better fit: no indirect addressing in the
// factor, fixed trip counts.
void Engine::free_batch_direct() {
  void *ptrs[] = {bd_.perm, bd_.bp_slot, bd_.ke_slot, bd_.ke_ptr, bd_.kp_row, bd_.kp_a, bd_.kp_b, bd_.tri, bd_.kp_val};
  for (void *p : ptrs) if (p) be::dfree(d_, p);
  bd_ = BatchDirect();
}

// ------------------------------------------------------------------------------------------------ batch path, one wave per problem
// engine.hpp BatchWave / backend.h BatchParams::wv_*.  Rows of A sorted by length (descending, stable): sorted position p -> lane p % 64, slot p / 64; a group
// of 64 positions takes as many ELL steps as its longest (= first) row has entries.  A' (B's entries with column >= n) in the natural order of the variables.
constexpr int kBatchWaveMin = 2048, kBatchWaveMinOrdered = 1280;      // smallest batches that take the wave-per-problem kernel by default (without / with a launch order)
void Engine::free_batch_wave() {
  void *ptrs[] = {bwv_.Aidx, bwv_.Acol, bwv_.Tidx, bwv_.Tcol, bwv_.row, bwv_.queue};
  for (void *p : ptrs) if (p) be::dfree(d_, p);
  bwv_ = BatchWave();
}
void Engine::prepare_batch_wave() {
  if (bwv_.tried) return;
  bwv_.tried = true;
  if (n < 1 || n > kBatchSpecN || m < 1 || m > 256 || reordered_) return;
  std::vector<int> pos(m);
  for (int i = 0; i < m; i++) pos[i] = i;
  std::stable_sort(pos.begin(), pos.end(), [&](int a, int b) { return Arp_[a + 1] - Arp_[a] > Arp_[b + 1] - Arp_[b]; });
  int aend[4] = {0, 0, 0, 0}, tend[2] = {0, 0}, acc = 0;
  for (int g = 0; g < 4; g++) { if (g * 64 < m) { const int r = pos[g * 64]; acc += Arp_[r + 1] - Arp_[r]; } aend[g] = acc; }
  if (acc > kBatchWaveSA) return;
  std::vector<int> Aidx((size_t)std::max(acc, 1) * 64, -1), Acol((size_t)std::max(acc, 1) * 64, 0), row(256, -1);
  for (int p = 0; p < m; p++) {
    const int r = pos[p], lane = p % 64, g = p / 64, s0 = g ? aend[g - 1] : 0;
    row[p] = r;
    for (int k = Arp_[r]; k < Arp_[r + 1]; k++) { Aidx[(size_t)(s0 + k - Arp_[r]) * 64 + lane] = k; Acol[(size_t)(s0 + k - Arp_[r]) * 64 + lane] = Arj_[k]; }
  }
  int tacc = 0;
  std::vector<int> tcnt(n, 0);
  for (int j = 0; j < n; j++) for (int k = Brp_[j]; k < Brp_[j + 1]; k++) tcnt[j] += Bj_[k] >= n;
  for (int g = 0; g < 2; g++) { int mx = 0; for (int j = g * 64; j < std::min(n, g * 64 + 64); j++) mx = std::max(mx, tcnt[j]); tacc += mx; tend[g] = tacc; }
  if (tacc > kBatchWaveST) return;
  std::vector<int> Tidx((size_t)std::max(tacc, 1) * 64, -1), Tcol((size_t)std::max(tacc, 1) * 64, 0);
  for (int j = 0; j < n; j++) {
    const int lane = j % 64, g = j / 64, s0 = g ? tend[g - 1] : 0;
    int e = 0;
    for (int k = Brp_[j]; k < Brp_[j + 1]; k++) if (Bj_[k] >= n) { Tidx[(size_t)(s0 + e) * 64 + lane] = k; Tcol[(size_t)(s0 + e) * 64 + lane] = Bj_[k] - n; e++; }
  }
  if (!be::batch_wave_lds_bytes(n, m, acc + tacc)) return;
  auto up = [&](const std::vector<int> &v) { int *dptr = dev_vec<int>(d_, v.size()); be::h2d(d_, dptr, v.data(), sizeof(int) * v.size()); return dptr; };
  bwv_.Aidx = up(Aidx); bwv_.Acol = up(Acol); bwv_.Tidx = up(Tidx); bwv_.Tcol = up(Tcol); bwv_.row = up(row);
  bwv_.queue = dev_vec<int>(d_, 1);
  for (int g = 0; g < 4; g++) bwv_.aend[g] = aend[g];
  bwv_.tend[0] = tend[0]; bwv_.tend[1] = tend[1];
  bwv_.ok = true;
}
// (behind attach_batch_direct: the form needs the spectral decomposition)
void Engine::attach_batch_wave(BatchParams &p, int nbatch) {
  // OSQPHipPolicy::batch_wave; automatic = where it measured faster (tools/batch_size_sweep.py): large batches, smaller ones only with a launch order
  // (k_batch_wave has no duality-gap test: with check_dualgap the whole batch stays on k_batch_admm, which has, as with polish)
  if (!p.sp_V || pol_.batch_wave < 0 || p.mat_on || p.polish || p.check_dualgap) return;
  if (pol_.batch_wave == 0 && nbatch < (p.order ? kBatchWaveMinOrdered : kBatchWaveMin)) return;
  prepare_batch_wave();
  if (!bwv_.ok) return;
  p.wv_on = 1;
  for (int g = 0; g < 4; g++) p.wv_aend[g] = bwv_.aend[g];
  p.wv_tend[0] = bwv_.tend[0]; p.wv_tend[1] = bwv_.tend[1];
  // the longest-expected problems to the workgroup kernel (be::batch_solve applies it when there is a launch order): wv_cus CUs are left free for it
  // and take wv_split problems, several each, one after the other
  // (tools/batch_size_sweep.py under OSQP_HIP_WAVE_SPLIT / OSQP_HIP_WAVE_CUS, MPC batch: 2048 QPs 2.21 ms with 32 / 32, 2.84 with 64 / 16; 4096 QPs 3.26 ms
  //  with 48 / 16, 3.41 with 32 / 32; 8192 QPs 5.66 against 6.18 -- a large batch is bound by the wave kernel's throughput and wants its CUs back)
  const BatchEnv &env = batch_env();
  p.wv_cus = env.wave_cus >= 0 ? env.wave_cus : (nbatch < 3072 ? 32 : 16);
  p.wv_split = env.wave_split >= 0 ? env.wave_split : (nbatch < 3072 ? 32 : 48);
  p.wv_Aidx = bwv_.Aidx; p.wv_Acol = bwv_.Acol; p.wv_Tidx = bwv_.Tidx; p.wv_Tcol = bwv_.Tcol; p.wv_row = bwv_.row; p.wv_queue = bwv_.queue;
}

// ------------------------------------------------------------------------------------------------ batch path, spectral form of the direct solve
// engine.hpp BatchSpectral.  Dense work on the host, n <= kBatchSpecN: the SCALED matrices (c D P D + sigma I, E A D: what the kernels hold) are
// rebuilt from the host copies, K_ref and M1 assembled, K_ref = L L' (Cholesky), C = L^-1 M1 L^-T, C = Q Lambda Q' (cyclic Jacobi sweeps: C is
// symmetric PSD with eigenvalues in [0, 1 / rho_ref]), V = L^-T Q.  Checked before use: || V' K_ref V - I ||_max and || V' M1 V - Lambda ||_max.
constexpr int kBatchSpectralMin = 32;      // smallest batch that has the spectral form prepared for it (Engine::attach_batch_direct)
void Engine::free_batch_spectral() {
  void *ptrs[] = {bs_.V, bs_.lam, bs_.d_ctype, bs_.K0};
  for (void *p : ptrs) if (p) be::dfree(d_, p);
  bs_ = BatchSpectral();
}
bool Engine::prepare_batch_spectral(double rho_ref, double eqf, bool allow_build) {
  const int N = kBatchSpecN;
  if (n > N || m == 0 || !be::device_assembly() || reordered_) { bs_.ok = false; return false; }
  // the reference classes: those of the solver's own bounds, classified as the kernel classifies a problem's (batch_hip.hip, _osqp.py:505-518)
  std::vector<int> ct(m);
  for (int i = 0; i < m; i++) ct[i] = row_class(in_l(E_[i], l0_[i]), in_u(E_[i], u0_[i]), settings.rho_is_vec);
  if ((bs_.ok || bs_.failed) && bs_.mat_epoch == mat_epoch_ && bs_.eqf == eqf && bs_.sigma == settings.sigma && bs_.rho_is_vec == settings.rho_is_vec && bs_.ctype == ct) return bs_.ok;
  if (!allow_build) return false;                          // (what exists was built for other matrices / classes; this caller does not pay for a new one)
  const double rref = bs_.ok ? bs_.rho_ref : rho_ref;       // (any reference works: K(rho) = K_ref + (rho - rho_ref) M1; the first call's rho stays)
  free_batch_spectral();
  // a rejected attempt (pivot <= 0, sweeps not converged, check missed) is remembered under the same key: every later call would redo O(n^3 x sweeps)
  // host work for the same verdict.  Cleared by whatever changes the key (matrix update, other classes, sigma).
  auto reject = [&]() { bs_.ok = false; bs_.failed = true; bs_.ctype = ct; bs_.eqf = eqf; bs_.sigma = settings.sigma; bs_.rho_is_vec = settings.rho_is_vec; bs_.mat_epoch = mat_epoch_; };
  std::vector<double> K((size_t)n * n, 0.0), M1((size_t)n * n, 0.0);
  for (int j = 0; j < n; j++) {
    for (int k = P_.p[j]; k < P_.p[j + 1]; k++) {
      const int i = P_.i[k];
      const double v = c_ * D_[i] * P_.x[k] * D_[j];
      K[(size_t)i * n + j] += v; if (i != j) K[(size_t)j * n + i] += v;
    }
    K[(size_t)j * n + j] += settings.sigma;
  }
  { // A' W A by rows of A (CSC -> per-row lists)
    std::vector<std::vector<std::pair<int, double>>> rows(m);
    for (int j = 0; j < n; j++) for (int k = A_.p[j]; k < A_.p[j + 1]; k++) rows[A_.i[k]].push_back({j, E_[A_.i[k]] * A_.x[k] * D_[j]});
    for (int i = 0; i < m; i++) {
      const int ty = ct[i];
      for (auto &a : rows[i]) for (auto &b : rows[i]) {
        const double v = a.second * b.second;
        if (ty == -1) K[(size_t)a.first * n + b.first] += kRowRhoLoose * v;         // loose rows keep their rho whatever rho_bar is (_osqp.py:520)
        else M1[(size_t)a.first * n + b.first] += (ty == 1 ? eqf : 1.0) * v;
      }
    }
  }
  std::vector<double> Kref(K);
  for (size_t e = 0; e < Kref.size(); e++) Kref[e] += rref * M1[e];
  // Cholesky Kref = L L' (lower, in place in Lm)
  std::vector<double> Lm(Kref);
  for (int c = 0; c < n; c++) {
    double dg = Lm[(size_t)c * n + c];
    for (int k = 0; k < c; k++) dg -= Lm[(size_t)c * n + k] * Lm[(size_t)c * n + k];
    if (!(dg > 0.0)) { reject(); return false; }
    dg = std::sqrt(dg); Lm[(size_t)c * n + c] = dg;
    for (int r = c + 1; r < n; r++) {
      double v = Lm[(size_t)r * n + c];
      for (int k = 0; k < c; k++) v -= Lm[(size_t)r * n + k] * Lm[(size_t)c * n + k];
      Lm[(size_t)r * n + c] = v / dg;
    }
  }
  auto fwd = [&](std::vector<double> &X) {                    // X <- L^-1 X  (X: n x n row-major, column by column)
    for (int col = 0; col < n; col++) for (int r = 0; r < n; r++) {
      double v = X[(size_t)r * n + col];
      for (int k = 0; k < r; k++) v -= Lm[(size_t)r * n + k] * X[(size_t)k * n + col];
      X[(size_t)r * n + col] = v / Lm[(size_t)r * n + r];
    }
  };
  auto transpose = [&](std::vector<double> &X) { for (int a = 0; a < n; a++) for (int b = a + 1; b < n; b++) std::swap(X[(size_t)a * n + b], X[(size_t)b * n + a]); };
  std::vector<double> C(M1);
  fwd(C); transpose(C); fwd(C);                              // L^-1 M1 L^-T  (symmetric)
  for (int a = 0; a < n; a++) for (int b = a + 1; b < n; b++) { const double v = 0.5 * (C[(size_t)a * n + b] + C[(size_t)b * n + a]); C[(size_t)a * n + b] = C[(size_t)b * n + a] = v; }
  // cyclic Jacobi: C = Q diag(lam) Q'
  std::vector<double> Q((size_t)n * n, 0.0);
  for (int a = 0; a < n; a++) Q[(size_t)a * n + a] = 1.0;
  bool jacobi_converged = false;
  for (int sweep = 0; sweep < 60; sweep++) {
    double off = 0.0, dsum = 0.0;
    for (int a = 0; a < n; a++) { dsum += C[(size_t)a * n + a] * C[(size_t)a * n + a]; for (int b = a + 1; b < n; b++) off += C[(size_t)a * n + b] * C[(size_t)a * n + b]; }
    if (off <= 1e-32 * (dsum + 1e-300)) { jacobi_converged = true; break; }
    for (int p_ = 0; p_ < n - 1; p_++) for (int q_ = p_ + 1; q_ < n; q_++) {
      const double apq = C[(size_t)p_ * n + q_];
      if (apq == 0.0) continue;
      const double theta = (C[(size_t)q_ * n + q_] - C[(size_t)p_ * n + p_]) / (2.0 * apq);
      const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0)), cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
      for (int k = 0; k < n; k++) { const double ckp = C[(size_t)k * n + p_], ckq = C[(size_t)k * n + q_]; C[(size_t)k * n + p_] = cs * ckp - sn * ckq; C[(size_t)k * n + q_] = sn * ckp + cs * ckq; }
      for (int k = 0; k < n; k++) { const double cpk = C[(size_t)p_ * n + k], cqk = C[(size_t)q_ * n + k]; C[(size_t)p_ * n + k] = cs * cpk - sn * cqk; C[(size_t)q_ * n + k] = sn * cpk + cs * cqk; }
      for (int k = 0; k < n; k++) { const double qkp = Q[(size_t)k * n + p_], qkq = Q[(size_t)k * n + q_]; Q[(size_t)k * n + p_] = cs * qkp - sn * qkq; Q[(size_t)k * n + q_] = sn * qkp + cs * qkq; }
    }
  }
  // V = L^-T Q  (back substitution per column)
  std::vector<double> V(Q);
  for (int col = 0; col < n; col++) for (int r = n - 1; r >= 0; r--) {
    double v = V[(size_t)r * n + col];
    for (int k = r + 1; k < n; k++) v -= Lm[(size_t)k * n + r] * V[(size_t)k * n + col];
    V[(size_t)r * n + col] = v / Lm[(size_t)r * n + r];
  }
  std::vector<double> lam(n);
  for (int k = 0; k < n; k++) lam[k] = std::max(C[(size_t)k * n + k], 0.0);
  // check, EVERY entry (two n^3 products: cheap next to the sweeps): V' Kref V = I, V' M1 V = Lambda -- a V that is wrong anywhere would serve as K^-1 for a whole batch
  double err = jacobi_converged ? 0.0 : 1.0;
  { std::vector<double> T((size_t)n * n);
    for (int pass = 0; pass < 2 && err < 1e-9; pass++) {
      const std::vector<double> &X = pass ? M1 : Kref;
      for (int i = 0; i < n; i++) for (int b = 0; b < n; b++) { double t = 0; for (int j = 0; j < n; j++) t += X[(size_t)i * n + j] * V[(size_t)j * n + b]; T[(size_t)i * n + b] = t; }      // T = X V
      for (int a = 0; a < n; a++) for (int b = 0; b < n; b++) {
        double s_ = 0; for (int i = 0; i < n; i++) s_ += V[(size_t)i * n + a] * T[(size_t)i * n + b];
        err = std::max(err, pass ? std::fabs(s_ - (a == b ? lam[a] : 0.0)) / (1.0 + std::max(lam[a], lam[b])) : std::fabs(s_ - (a == b ? 1.0 : 0.0)));
      }
    } }
  if (!(err < 1e-9)) { reject(); return false; }
  std::vector<double> Vp((size_t)N * N, 0.0), lp(N, 0.0);
  for (int k = 0; k < n; k++) { lp[k] = lam[k]; for (int j = 0; j < n; j++) Vp[(size_t)k * N + j] = V[(size_t)j * n + k]; }      // column-major, zero-padded
  bs_.V = dev_vec<double>(d_, Vp.size()); be::h2d(d_, bs_.V, Vp.data(), sizeof(double) * Vp.size());
  bs_.lam = dev_vec<double>(d_, N); be::h2d(d_, bs_.lam, lp.data(), sizeof(double) * N);
  bs_.d_ctype = dev_vec<int>(d_, m); be::h2d(d_, bs_.d_ctype, ct.data(), sizeof(int) * m);
  bs_.Vh = Vp; bs_.lamh = lp; bs_.k0_ok = false;
  bs_.ctype = ct; bs_.rho_ref = rref; bs_.eqf = eqf; bs_.sigma = settings.sigma; bs_.rho_is_vec = settings.rho_is_vec; bs_.mat_epoch = mat_epoch_;
  bs_.ok = true;
  return true;
}

// K^-1(rho0) = V diag(1 / (1 + (rho0 - rho_ref) lambda)) V' in the register layout batch_hip.hip's threads hold it in (the result layout of the f64 matrix
// instruction), formed once for the whole batch: a problem loads its first K^-1 instead of building it.
void Engine::prepare_batch_k0(double rho0) {
  if (!bs_.ok) return;
  if (bs_.k0_ok && bs_.k0_rho == rho0) return;
  const int N = kBatchSpecN, T = 256;
  const double dl = rho0 - bs_.rho_ref;
  std::vector<double> dk(N), K0((size_t)64 * T);
  for (int k = 0; k < N; k++) dk[k] = 1.0 / (1.0 + dl * bs_.lamh[k]);
  const double *V = bs_.Vh.data();                            // V[k * N + j] = V(j, k)
  // (layout: batch_hip.hip kacc -- thread tid = 64 w + l holds, for tile t = tr * 8 + tc and register r, element (32 w + 16 tr + l / 16 + 4 r, 16 tc + l % 16))
  for (int tid = 0; tid < T; tid++) {
    const int wv = tid >> 6, l = tid & 63, lj = l & 15, lk = l >> 4;
    for (int t = 0; t < 16; t++) for (int r = 0; r < 4; r++) {
      const int i = 32 * wv + 16 * (t / 8) + lk + 4 * r, j = 16 * (t % 8) + lj;
      double acc = 0.0;
      for (int k = 0; k < n; k++) acc = std::fma(V[(size_t)k * N + i] * dk[k], V[(size_t)k * N + j], acc);
      K0[(size_t)(t * 4 + r) * T + tid] = acc;
    }
  }
  if (!bs_.K0) bs_.K0 = dev_vec<double>(d_, K0.size());
  be::h2d(d_, bs_.K0, K0.data(), sizeof(double) * K0.size());
  bs_.k0_rho = rho0; bs_.k0_ok = true;
}

void Engine::prepare_batch_direct() {
  if (bd_.tried) return;
  bd_.tried = true;
  const int nzA = (int)Arj_.size(), nzB = (int)Bj_.size();
  // adjacency of K (excluding the diagonal)
  double pairs = 0;
  for (int i = 0; i < m; i++) { const double len = Arp_[i + 1] - Arp_[i]; pairs += len * (len + 1) / 2; }
  if (pairs > 4e6 || n > 4096) { bd_.bw_symbolic = -2; return; }   // dense rows: K would be (nearly) dense -- PCG path
  std::vector<std::vector<int>> adj(n);
  for (int j = 0; j < n; j++)
    for (int k = Brp_[j]; k < Brp_[j + 1]; k++) { const int c = Bj_[k]; if (c < n && c != j) adj[j].push_back(c); }
  for (int i = 0; i < m; i++)
    for (int a = Arp_[i]; a < Arp_[i + 1]; a++)
      for (int b = Arp_[i]; b < Arp_[i + 1]; b++) if (a != b) adj[Arj_[a]].push_back(Arj_[b]);
  for (auto &v : adj) { std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end()); }
  // reverse Cuthill-McKee, component by component, each started from a pseudo-peripheral node
  std::vector<int> order; order.reserve(n);
  std::vector<char> seen(n, 0);
  std::vector<int> level(n, -1), frontier, next;
  auto bfs_far = [&](int start, int &ecc) {                  // farthest node of minimum degree from start (within its component)
    std::vector<int> touched;
    frontier.assign(1, start); level[start] = 0; touched.push_back(start);
    int last = start; ecc = 0;
    while (!frontier.empty()) {
      next.clear();
      int best = frontier[0];
      for (int v : frontier) if (adj[v].size() < adj[best].size()) best = v;
      last = best; ecc = level[best];
      for (int v : frontier) for (int w : adj[v]) if (level[w] < 0) { level[w] = level[v] + 1; next.push_back(w); touched.push_back(w); }
      frontier.swap(next);
    }
    for (int v : touched) level[v] = -1;
    return last;
  };
  for (int s0 = 0; s0 < n; s0++) {
    if (seen[s0]) continue;
    int start = s0, ecc = -1;
    for (int rounds = 0; rounds < 8; rounds++) {            // pseudo-peripheral node (George-Liu)
      int e2; const int far = bfs_far(start, e2);
      if (e2 <= ecc) break;
      ecc = e2; start = far;
    }
    size_t head = order.size();
    order.push_back(start); seen[start] = 1;
    while (head < order.size()) {
      const int v = order[head++];
      std::vector<int> nb;
      for (int w : adj[v]) if (!seen[w]) { seen[w] = 1; nb.push_back(w); }
      std::sort(nb.begin(), nb.end(), [&](int a, int b) { return adj[a].size() != adj[b].size() ? adj[a].size() < adj[b].size() : a < b; });
      order.insert(order.end(), nb.begin(), nb.end());
    }
  }
  std::reverse(order.begin(), order.end());
  std::vector<int> iperm(n);
  for (int k = 0; k < n; k++) iperm[order[k]] = k;
  int bw = 0;
  for (int j = 0; j < n; j++) for (int c : adj[j]) bw = std::max(bw, std::abs(iperm[j] - iperm[c]));
  bd_.bw_symbolic = bw;
  if (bw > kBatchDirectMaxBw || !be::batch_direct_lds_bytes(n, m, std::max(nzA, nzB), bw)) return;
  // band slot (band_ldl.h: column-major lower band, row >= col, permuted indices) of the P + sigma I entries of B
  std::vector<int> bp_slot(nzB, -1);
  for (int j = 0; j < n; j++)
    for (int k = Brp_[j]; k < Brp_[j + 1]; k++) {
      const int c = Bj_[k];
      if (c >= n) continue;
      const int pr = iperm[j], pc = iperm[c];
      if (pr >= pc) bp_slot[k] = band_slot(bw, pc, pr);
    }
  // products of A' rho A, grouped by slot
  struct Prod { int slot, row, a, b; };
  std::vector<Prod> prods; prods.reserve((size_t)pairs);
  for (int i = 0; i < m; i++)
    for (int a = Arp_[i]; a < Arp_[i + 1]; a++)
      for (int b = a; b < Arp_[i + 1]; b++) {
        const int pa = iperm[Arj_[a]], pb = iperm[Arj_[b]];
        const int r = std::max(pa, pb), c = std::min(pa, pb);
        prods.push_back({band_slot(bw, c, r), i, a, b});
      }
  std::stable_sort(prods.begin(), prods.end(), [](const Prod &x, const Prod &y) { return x.slot < y.slot; });
  std::vector<int> ke_slot, ke_ptr, kp_row(prods.size()), kp_a(prods.size()), kp_b(prods.size());
  for (size_t p = 0; p < prods.size(); p++) {
    if (p == 0 || prods[p].slot != prods[p - 1].slot) { ke_slot.push_back(prods[p].slot); ke_ptr.push_back((int)p); }
    kp_row[p] = prods[p].row; kp_a[p] = prods[p].a; kp_b[p] = prods[p].b;
  }
  ke_ptr.push_back((int)prods.size());
  const std::vector<int> tri = band_tri_pairs(bw);
  auto up = [&](const std::vector<int> &h) { int *p = dev_vec<int>(d_, h.size()); if (!h.empty()) be::h2d(d_, p, h.data(), sizeof(int) * h.size()); return p; };
  bd_.perm = up(order); bd_.bp_slot = up(bp_slot); bd_.ke_slot = up(ke_slot); bd_.ke_ptr = up(ke_ptr);
  bd_.kp_row = up(kp_row); bd_.kp_a = up(kp_a); bd_.kp_b = up(kp_b); bd_.tri = up(tri);
  bd_.kp_val = dev_vec<double>(d_, prods.size());
  bd_.bw = bw; bd_.nents = (int)ke_slot.size(); bd_.nprod = (int)prods.size(); bd_.ntri = (int)tri.size();
  bd_.ok = true;
}

void Engine::fill_batch_settings(BatchSettings &p, int warm) {
  p.c = c_; p.cinv = cinv_; p.sigma = settings.sigma; p.alpha = settings.alpha; p.rho0 = clamp_rho(settings.rho); p.eq_factor = eq_factor_mixed_;
  p.eps_abs = settings.eps_abs; p.eps_rel = settings.eps_rel; p.eps_pinf = settings.eps_prim_inf; p.eps_dinf = settings.eps_dual_inf;
  p.cg_frac = settings.cg_tol_fraction; p.rho_tol = settings.adaptive_rho_tolerance;
  p.max_iter = settings.max_iter; p.check = settings.check_termination; p.rho_interval = settings.adaptive_rho ? auto_rho_interval() : 0;
  p.cg_max = settings.cg_max_iter; p.unscaled = settings.scaling && !settings.scaled_termination; p.scaling = settings.scaling;
  p.precond = settings.cg_precond == OSQP_DIAGONAL_PRECONDITIONER; p.rho_is_vec = settings.rho_is_vec; p.warm = warm;
  p.check_dualgap = settings.check_dualgap != 0;
}
void Engine::fill_batch_params(BatchParams &p, int nbatch, int warm) {
  fill_batch_settings(p, warm);
  p.n = n; p.m = m; p.nbatch = nbatch; p.A = d_.A; p.B = d_.B; p.D = d_.D; p.Dinv = d_.Dinv; p.E = d_.E; p.Einv = d_.Einv;
  p.polish = settings.polishing; p.refine = settings.polish_refine_iter; p.delta = settings.delta;      // (honoured by the direct variants)
  p.variant = pol_.batch_variant; p.wide_rounds = batch_env().wide_rounds;
}

void Engine::attach_batch_direct(BatchParams &p, bool spectral) {
  if (!bd_.ok) return;
  p.eq_factor_direct = eq_factor_set_ ? eq_factor_mixed_ : kRowEqWeight;
  // the spectral form of the same solve, where it applies (never with polish: that factorises another matrix in the band) -- and where the caller is a
  // batch that pays for the host-side decomposition (dense Cholesky + Jacobi sweeps: tens to hundreds of ms for a kernel that runs about one): a
  // single osqp_solve of a small QP and small batches keep the banded kernel unless a batch has prepared the form for this key before
  if (pol_.batch_variant == 0 && !settings.polishing && n <= kBatchSpecN) {
    if (raw_stale_) ensure_host_vectors();             // (the solver's own bounds define the reference classes)
    int n_ineq = 0;
    for (int i = 0; i < m; i++) n_ineq += row_class(in_l(E_[i], l0_[i]), in_u(E_[i], u0_[i]), settings.rho_is_vec) == 0;
    if (prepare_batch_spectral(p.rho0, eq_weight(n_ineq == 0, p.eq_factor_direct), spectral)) {
      p.sp_V = bs_.V; p.sp_lam = bs_.lam; p.sp_ctype = bs_.d_ctype; p.sp_rho_ref = bs_.rho_ref; p.sp_eqf = bs_.eqf;
      prepare_batch_k0(p.rho0);
      if (bs_.k0_ok) { p.sp_K0 = bs_.K0; p.sp_K0_rho = bs_.k0_rho; }
    }
  }
  p.bw = bd_.bw; p.nents = bd_.nents; p.ntri = bd_.ntri; p.perm = bd_.perm; p.bp_slot = bd_.bp_slot; p.ke_slot = bd_.ke_slot;
  p.ke_ptr = bd_.ke_ptr; p.kp_row = bd_.kp_row; p.kp_val = bd_.kp_val; p.tri = bd_.tri;
}

// ------------------------------------------------------------------------------------------------ small problems
// A QP small enough for the batch kernel's DIRECT variant (iterates, matrices and the banded LDL' factor of the reduced
// KKT matrix in one workgroup's LDS) is solved by ONE launch of that kernel with a batch of one: the whole ADMM loop runs
// on the device with exact linear solves and the reference's rho rule, i.e. the algorithm of the reference's direct path
// (same iteration counts as the oracle), instead of thousands of graph-replayed multi-kernel iterations with inexact
// inner solves -- on small LPs / rank-deficient QPs the latter can need 10x more ADMM iterations (fuzz).
// With `polishing`, a SOLVED problem is polished in the same launch (reduced KKT system on the active set, factorised in LDS,
// polish_refine_iter refinement steps: the reference's algorithm, _osqp.py:1710-1828).  Not taken with a time limit or when
// OSQP_HIP_SMALL_DIRECT=0.  `verbose` does not change the path: the whole loop is one launch, so the table holds its last line only.
bool Engine::small_direct_applicable() {
  if (!pol_.small_direct || !be::device_assembly() || settings.time_limit < 1e9 || reordered_ || d_.dk.on) return false;      // (a handle with the dense KKT mode on runs that mode)
  if (settings.check_dualgap) return false;            // the one-launch kernel has no duality-gap test: the host-driven loop honours the setting
  if (!be::batch_lds_bytes(n, m)) return false;
  prepare_batch_direct();
  if (!bd_.ok) return false;
  BatchParams p{};
  fill_batch_params(p, 1, 0);
  attach_batch_direct(p, false);
  return be::batch_direct_selected(p);
}

int Engine::solve_small_direct(double t0) {
  const int warm = settings.warm_starting ? 1 : 0;
  std::vector<double> x(n, 0.0), y(std::max(m, 1), 0.0);       // (m = 0: batch_solve still wants a non-null y)
  if (warm) {                                                   // continue from the device iterates (x, y; z = A x as in warm_start)
    be::d2h(d_, x.data(), d_.x, sizeof(double) * n);
    if (m > 0) be::d2h(d_, y.data(), d_.y, sizeof(double) * m);
    for (int j = 0; j < n; j++) x[j] *= D_[j];
    for (int i = 0; i < m; i++) y[i] *= cinv_ * E_[i];
  }
  double rec[kBatchRec] = {0};
  // (the handle's own scaled z goes in and out by device pointer: a continued solve keeps its z iterate, _osqp.py:1197-1204)
  const int err = batch_solve(1, nullptr, nullptr, nullptr, x.data(), y.data(), rec, warm, m > 0 ? d_.z : nullptr);
  if (err) return err;
  const int st = (int)rec[0];
  set_status(st);
  info.iter = (int)rec[1]; info.obj_val = rec[2]; info.prim_res = rec[3]; info.dual_res = rec[4];
  info.rho_updates = (int)rec[6]; info.rho_estimate = rec[10];                 // (_osqp.py:1275)
  info.status_polish = (int)rec[8]; info.polish_time = rec[9];      // polished inside the kernel (reduced KKT on the factor in LDS)
  if (rec[5] != rho_bar_) {                                     // adaptive rho moved: keep the handle's state in step (_osqp.py:923-930)
    rho_bar_ = clamp_rho(rec[5]); settings.rho = rho_bar_;
    be::set_rho(d_, rho_bar_);
    be::precond(d_, settings.cg_precond == OSQP_DIAGONAL_PRECONDITIONER);
  }
  const bool pinf = term_is_pinf(st), dinf = term_is_dinf(st);
  std::fill(sol_pc_.begin(), sol_pc_.end(), kNaN); std::fill(sol_dc_.begin(), sol_dc_.end(), kNaN);
  const bool finite_xy = std::isfinite(rec[2]) && st != OSQP_NON_CVX;
  if (!pinf && !dinf) {
    std::copy(x.begin(), x.end(), sol_x_.begin()); std::copy(y.begin(), y.begin() + m, sol_y_.begin());   // (solution.x/y point into these)
    if (finite_xy) {
      const int keep = settings.warm_starting;
      warm_start(x.data(), m > 0 ? y.data() : nullptr, /*keep_z=*/true);   // device x, y follow; z is the kernel's own (a later solve continues from them)
      settings.warm_starting = keep;
      // the v1 gap fields (policy.h ctl_info) from the unscaled data on the host -- the kernel's record carries no residual block: a few hundred entries
      ensure_host_vectors();
      std::vector<double> px(n, 0.0), ax(m, 0.0), aty(n, 0.0);
      for (int j = 0; j < n; j++)
        for (int k = P_.p[j]; k < P_.p[j + 1]; k++) { const int i = P_.i[k]; px[i] += P_.x[k] * x[j]; if (i != j) px[j] += P_.x[k] * x[i]; }
      for (int j = 0; j < n; j++)
        for (int k = A_.p[j]; k < A_.p[j + 1]; k++) { ax[A_.i[k]] += A_.x[k] * x[j]; aty[j] += A_.x[k] * y[A_.i[k]]; }
      double xpx = 0, sup = 0, nax = 0, nz = 0, npx = 0, naty = 0, nq = 0;
      for (int j = 0; j < n; j++) { xpx += x[j] * px[j]; npx = std::max(npx, std::fabs(px[j])); naty = std::max(naty, std::fabs(aty[j])); nq = std::max(nq, std::fabs(q0_[j])); }
      for (int i = 0; i < m; i++) {
        sup += support_finite(l0_[i], u0_[i], y[i]);
        nax = std::max(nax, std::fabs(ax[i])); nz = std::max(nz, std::fabs(std::min(std::max(ax[i], l0_[i]), u0_[i])));
      }
      info.dual_obj_val = -0.5 * xpx - sup;
      info.duality_gap = info.obj_val - info.dual_obj_val;
      info.rel_kkt_error = term_rel_kkt(m, info.prim_res, std::max(nax, nz), info.dual_res, std::max(std::max(npx, naty), nq), info.duality_gap, info.obj_val, info.dual_obj_val);
    } else {
      cold_start();                                             // NaN iterates (non-convex problem) are no warm start
      info.dual_obj_val = info.duality_gap = info.rel_kkt_error = kNaN;
    }
  } else {
    std::fill(sol_x_.begin(), sol_x_.end(), kNaN); std::fill(sol_y_.begin(), sol_y_.end(), kNaN);
    if (pinf) std::copy(y.begin(), y.begin() + m, sol_pc_.begin()); else std::copy(x.begin(), x.end(), sol_dc_.begin());                    // the kernel returns the certificate in place of y / x
    cold_start();
  }
  stats_.pcg_iters_total = stats_.pcg_iters_max = stats_.pcg_unconverged = 0;
  stats_.kernel_launches = 1; stats_.graph_launches = 0;
  be::sync(d_);
  info.solve_time = std::max(now_s() - t0 - info.polish_time, 0.0);
  info.run_time = (first_run_ ? info.setup_time : info.update_time) + info.solve_time + info.polish_time;
  if (settings.verbose) {                          // (one launch ran the whole loop: the table holds its last line, _osqp.py:1259-1261)
    say("iter   objective    pri res    dua res    rho       time\n");
    print_summary_line(info.iter, info.obj_val, info.prim_res, info.dual_res, rho_bar_, t0);
    if (info.status_polish) say("plsh  %11.4e   %8.2e   %8.2e   --------  %8.2es\n", info.obj_val, info.prim_res, info.dual_res, info.run_time);
    print_footer();
  }
  first_run_ = false; clear_update_time_ = true;
  return OSQP_NO_ERROR;
}

// Per-problem matrices (BatchParams::mat_on): one scratch block [Aval | Bval | D | Dinv | E | Einv | c | products], filled by be::batch_prepare on `stream`
// (assembly + the reference's equilibration per problem).  The spectral form (one V for the whole batch) is switched off for such a call.
int Engine::attach_batch_matrices(BatchParams &p, const double *Px_dev, const double *Ax_dev, void *stream) {
  if (!be::device_assembly()) return OSQP_FUNC_NOT_IMPLEMENTED;
  const size_t nb = (size_t)p.nbatch, nzA = (size_t)d_.A.nnz, nzB = (size_t)d_.B.nnz, np = bd_.ok ? (size_t)bd_.nprod : 0;
  const size_t need = nb * (nzA + nzB + 2 * (size_t)n + 2 * (size_t)m + 1 + np);
  if (need > bmat_cap_) { be::ext_wait(d_); if (bmat_) be::dfree(d_, bmat_); bmat_ = dev_vec<double>(d_, need); bmat_cap_ = need; be::sync(d_); }
  p.Aval_b = bmat_; p.Bval_b = p.Aval_b + nb * nzA; p.D_b = p.Bval_b + nb * nzB; p.Dinv_b = p.D_b + nb * n; p.E_b = p.Dinv_b + nb * n; p.Einv_b = p.E_b + nb * m;
  p.c_b = p.Einv_b + nb * m; p.kp_val_b = np ? p.c_b + nb : nullptr; p.nprod = (int)np; p.kp_a = bd_.kp_a; p.kp_b = bd_.kp_b;
  p.mat_on = 1; p.sp_V = nullptr; p.sp_K0 = nullptr;
  return be::batch_prepare(d_, p, Px_dev, Ax_dev, settings.scaling, stream);
}

// The launch-order buffer holds at least nbatch positions (growing it drops the device path's iteration counts as well)
void Engine::reserve_batch_order(int nbatch) {
  if ((size_t)nbatch <= batch_order_cap_) return;
  if (d_batch_order_) be::dfree(d_, d_batch_order_);
  if (d_batch_iters_) { be::dfree(d_, d_batch_iters_); d_batch_iters_ = nullptr; }
  d_batch_order_ = dev_vec<int>(d_, nbatch); batch_order_cap_ = nbatch; d_batch_iters_n_ = 0;
}

// The common tail of batch_solve and batch_solve_device, in this order:
//   1. on the solver's stream: the direct form's symbolic data, the refresh of its products (A's values may have changed since the last call), the
//      direct / spectral / wave forms attached to p;
//   2. wait_solver: the device path waits for the solver's stream here (its launches go on the caller's stream; the host path's uploads were waited for);
//   3. on `stream` (nullptr: the solver's): the per-problem matrices (be::batch_prepare), then be::batch_solve -- synchronous for nullptr.
// OSQPHipStats::batch_wave_split reports what be::batch_solve launched.
int Engine::launch_batch(BatchParams &p, int nbatch, const double *Px, const double *Ax, void *stream, bool wait_solver) {
  prepare_batch_direct();
  if (bd_.ok) {
    be::batch_products(d_, bd_.nprod, bd_.kp_a, bd_.kp_b, bd_.kp_val);
    attach_batch_direct(p, nbatch >= kBatchSpectralMin && !Px && !Ax);
    if (!Px && !Ax) attach_batch_wave(p, nbatch);
  }
  if (wait_solver) be::sync(d_);
  int err = (Px || Ax) ? attach_batch_matrices(p, Px, Ax, stream) : OSQP_NO_ERROR;
  if (!err) err = be::batch_solve(d_, p, stream);
  batch_wave_last_ = err ? -1 : d_.batch_wave_ran;
  return err;
}

// ---- what the batch entry points share
bool Engine::batch_applies() { return be::batch_lds_bytes(n, m) && !reordered_; }      // (a reordered handle is a large single QP: the batch kernel is for QPs that fit one workgroup)
bool Engine::batch_applies_prepared() { prepare_batch_direct(); return batch_applies(); }      // (the symbolic part runs on every backend: tests read the bandwidth)
bool Engine::lockstep_applies() { return be::lockstep_chunk && be::device_vec_updates() && !d_.wb.on; }

// How every batch entry point begins: the handle is ready, the arguments are there, the route (`applies`) holds this handle; then the device is
// this handle's and nothing on a caller's stream still reads what the call is about to overwrite (the scratch block, the shared vectors, kp_val).
// query (the device-pointer entry points): nbatch == 0 asks whether the route applies -- a rank whose share of a sharded batch is empty; the answer
// depends on the handle alone, so every rank of a job reaches the same decision before its first collective (osqp_amd/sharded.py).
// Returns kBatchEnter to go on, else what the entry point returns.
constexpr int kBatchEnter = -1;
int Engine::batch_enter(int nbatch, bool query, const double *x, const double *y, const double *rec, Applies applies) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (query && nbatch == 0) return (this->*applies)() ? OSQP_NO_ERROR : OSQP_FUNC_NOT_IMPLEMENTED;
  if (nbatch <= 0 || !x || !y || !rec) return OSQP_DATA_VALIDATION_ERROR;
  if (!(this->*applies)()) return OSQP_FUNC_NOT_IMPLEMENTED;
  be::activate(d_);
  be::ext_wait(d_);
  return kBatchEnter;
}

// Host staging of a batch given as host arrays (batch_solve, solve_lockstep_host).  in: batch_enter, l <= u for every member, the device scratch
// block bbuf_ = [q | l | u | x | y | rec | tail] (kept for the next call), the uploads; out: the downloads.  What the two routes do differently:
//   own_row   where row i of the caller's numbering sits in l0_ / u0_, the host copies of the handle's own bounds (nullptr: at i).  The lockstep route
//             passes ipr_ on a reordered handle -- the copies are kept in the engine's numbering; the workgroup route refuses reordered handles;
//   wg        the workgroup route appends [q0 | l0 | u0 | Px | Ax]: the handle's own vectors for the arguments given as NULL, uploaded where they
//             are not resident (!be::device_vec_updates(); dq0 .. du0 point at the resident ones otherwise), and the per-problem matrix values.  The
//             lockstep route reads d_.qraw .. itself; its per-problem matrix values (LockstepSolveIO::mat) follow the records directly.
struct Engine::BatchStage {
  Engine &e; int nbatch;
  Applies applies;                                    // the route
  const int *own_row; bool wg;
  size_t N = 0, M = 0;
  double *dq = nullptr, *dl = nullptr, *du = nullptr, *dx = nullptr, *dy = nullptr, *drec = nullptr, *dq0 = nullptr, *dl0 = nullptr, *du0 = nullptr, *dPx = nullptr, *dAx = nullptr;
  double t[3] = {0, 0, 0};                            // in() began / validated / uploaded (batch_timing)
  int in(const double *q, const double *l, const double *u, const double *x, const double *y, const double *rec, int warm, const double *Px = nullptr, const double *Ax = nullptr) {
    const int err = e.batch_enter(nbatch, false, x, y, rec, applies);
    if (err != kBatchEnter) return err;
    const int n = e.n, m = e.m;
    Dev &d = e.d_;
    t[0] = now_s();
    N = (size_t)nbatch * n; M = (size_t)nbatch * m;
    if ((l || u) && !(l && u)) e.ensure_host_vectors();
    for (int b = 0; b < nbatch && (l || u); b++)                                                       // _osqp.py:1348-1349
      for (int i = 0; i < m; i++) {
        const int ii = own_row ? own_row[i] : i;
        const double li = l ? l[(size_t)b * m + i] : e.l0_[ii], ui = u ? u[(size_t)b * m + i] : e.u0_[ii];
        if (!(li <= ui)) return OSQP_DATA_VALIDATION_ERROR;
      }
    t[1] = now_s();
    const size_t NP = Px ? (size_t)nbatch * e.P_.nnz() : 0, NA = Ax ? (size_t)nbatch * e.A_.nnz() : 0;
    const size_t need = 2 * N + 3 * M + (size_t)nbatch * kBatchRec + (wg ? n + 2 * (size_t)m : 0) + NP + NA;
    if (need > e.bbuf_cap_) { if (e.bbuf_) be::dfree(d, e.bbuf_); e.bbuf_ = dev_vec<double>(d, need); e.bbuf_cap_ = need; }
    dq = e.bbuf_; dl = dq + N; du = dl + M; dx = du + M; dy = dx + N; drec = dy + M;
    if (wg) {
      dq0 = drec + (size_t)nbatch * kBatchRec; dl0 = dq0 + n; du0 = dl0 + m; dPx = du0 + m; dAx = dPx + NP;
      const bool devv = be::device_vec_updates();       // then the solver's own q, l, u are resident (unscaled): no upload for NULL arguments
      if (!q) { if (devv) dq0 = d.qraw; else be::h2d(d, dq0, e.q0_.data(), sizeof(double) * n); }
      if (!l) { if (devv) dl0 = d.lraw; else be::h2d(d, dl0, e.l0_.data(), sizeof(double) * m); }
      if (!u) { if (devv) du0 = d.uraw; else be::h2d(d, du0, e.u0_.data(), sizeof(double) * m); }
    }
    else { dPx = drec + (size_t)nbatch * kBatchRec; dAx = dPx + NP; }
    if (Px) be::h2d(d, dPx, Px, sizeof(double) * NP);
    if (Ax) be::h2d(d, dAx, Ax, sizeof(double) * NA);
    if (q) be::h2d(d, dq, q, sizeof(double) * N);
    if (l) be::h2d(d, dl, l, sizeof(double) * M);
    if (u) be::h2d(d, du, u, sizeof(double) * M);
    if (warm) { be::h2d(d, dx, x, sizeof(double) * N); be::h2d(d, dy, y, sizeof(double) * M); }
    be::sync(d); t[2] = now_s();
    return OSQP_NO_ERROR;
  }
  void out(double *x, double *y, double *rec) const {
    be::d2h(e.d_, x, dx, sizeof(double) * N);
    if (M) be::d2h(e.d_, y, dy, sizeof(double) * M);  // (m == 0: nothing to read, on either route)
    be::d2h(e.d_, rec, drec, sizeof(double) * kBatchRec * nbatch);
  }
};

int Engine::batch_solve(int nbatch, const double *q, const double *l, const double *u, double *x, double *y, double *rec, int warm, double *zs_dev, const double *Px, const double *Ax) {
  BatchStage s{*this, nbatch, &Engine::batch_applies_prepared, /*own_row=*/nullptr, /*wg=*/true};
  if (const int err = s.in(q, l, u, x, y, rec, warm, Px, Ax)) return err;
  BatchParams p{};
  fill_batch_params(p, nbatch, warm);
  p.q = q ? s.dq : nullptr; p.l = l ? s.dl : nullptr; p.u = u ? s.du : nullptr; p.q0 = s.dq0; p.l0 = s.dl0; p.u0 = s.du0; p.x = s.dx; p.y = s.dy; p.rec = s.drec;
  p.zs = zs_dev;
  // Launch order: the problems that took most iterations in the PREVIOUS call of the same size go first (parametric batches -- MPC
  // steps, training epochs -- repeat their hard problems; with index order the last round of workgroups waits for stragglers:
  // 4096 MPC QPs 13.3 -> 11 ms).  Scheduling only: every problem is solved by its own workgroup exactly as before.
  const bool reorder = pol_.batch_reorder != 0;
  if (reorder && nbatch > 1 && (int)batch_order_.size() == nbatch) {
    reserve_batch_order(nbatch);
    be::h2d(d_, d_batch_order_, batch_order_.data(), sizeof(int) * nbatch);
    p.order = d_batch_order_;
  }
  d_batch_iters_n_ = 0;                            // (the device-pointer path's history does not describe this call)
  const int err = launch_batch(p, nbatch, Px ? s.dPx : nullptr, Ax ? s.dAx : nullptr, nullptr, false);
  const double t_ran = now_s();
  if (!err) {
    s.out(x, y, rec);
    if (reorder && nbatch > 1) {
      batch_order_.resize(nbatch);
      for (int b = 0; b < nbatch; b++) batch_order_[b] = b;
      std::stable_sort(batch_order_.begin(), batch_order_.end(), [&](int a, int b) { return rec[(size_t)a * kBatchRec + 1] > rec[(size_t)b * kBatchRec + 1]; });
    }
  }
  stats_.gpu_solve_ms = 1e3 * (t_ran - s.t[2]);
  if (pol_.batch_timing) std::fprintf(stderr, "osqp_hip batch: validate %.2f ms, H2D %.2f ms, kernel %.2f ms, D2H %.2f ms\n", 1e3 * (s.t[1] - s.t[0]), 1e3 * (s.t[2] - s.t[1]), 1e3 * (t_ran - s.t[2]), 1e3 * (now_s() - t_ran));
  return err;
}


// Device-resident variant: q, l, u, x, y, rec are device pointers on this solver's device; the kernel is
// enqueued on the caller's stream and not waited for (stream == nullptr: the solver's stream, synchronous).
int Engine::batch_solve_device(int nbatch, const double *q, const double *l, const double *u, double *x, double *y, double *rec, int warm, void *stream, const double *Px, const double *Ax) {
  const int enter = batch_enter(nbatch, true, x, y, rec, &Engine::batch_applies);
  if (enter != kBatchEnter) return enter;
  // shared vectors (for the arguments given as NULL): the solver's own resident unscaled q, l, u
  double *dq0 = d_.qraw, *dl0 = d_.lraw, *du0 = d_.uraw;
  BatchParams p{};
  fill_batch_params(p, nbatch, warm);
  p.q = q; p.l = l; p.u = u; p.q0 = dq0; p.l0 = dl0; p.u0 = du0; p.x = x; p.y = y; p.rec = rec;
  // launch order as in batch_solve, entirely on the device: the kernel leaves every problem's iteration count, a rank kernel turns
  // the previous call's counts into this call's order (both on the caller's stream: ordered with the batch kernels themselves)
  const bool reorder = pol_.batch_reorder != 0;
  if (reorder && nbatch > 1) {
    reserve_batch_order(nbatch);                     // (both buffers have the same capacity)
    if (!d_batch_iters_) { d_batch_iters_ = dev_vec<int>(d_, batch_order_cap_); d_batch_iters_n_ = 0; }
    be::sync(d_);                                    // (allocations / zero fills ran on the solver's stream)
    if (d_batch_iters_n_ == nbatch) { be::batch_order(d_, nbatch, d_batch_iters_, d_batch_order_, stream); p.order = d_batch_order_; }
    p.iters_out = d_batch_iters_;
    d_batch_iters_n_ = nbatch;
    batch_order_.clear();                            // (the host path's order does not describe this call)
  }
  const int err = launch_batch(p, nbatch, Px, Ax, stream, true);
  if (!err) be::ext_record(d_, stream);           // later calls that overwrite or free what this kernel reads wait for it (ext_wait)
  return err;
}

// ------------------------------------------------------------------------------------------------ lockstep routes
// Chunks of kLsW problems, one after the other, each from its transposes in to its transposes out.  The axes (engine.hpp): the route -- PCG on block
// vectors (be::lockstep_chunk), or direct: the Woodbury formula per problem in its place (lockstep_hip.hip "lockstep DIRECT") --, shared or per-problem
// matrices, solve or adjoint, host or device arrays.  One chunk loop per direction (run_lockstep_solve, run_lockstep_adjoint) and one body per kind of
// arrays serve every entry point.  The handle's iterates, rho, info, solution, graphs and history are not touched: each route has its own blocks (lsr_).
static_assert(OSQP_HIP_LOCKSTEP_LAST_REC == 8 && OSQP_HIP_LOCKSTEP_POLISH_LAST_REC == 8 && OSQP_HIP_LOCKSTEP_MAT_LAST_REC == 8 && OSQP_HIP_LOCKSTEP_DIRECT_LAST_REC == 8 &&
              OSQP_HIP_LOCKSTEP_DIRECT_MAT_LAST_REC == 8 && OSQP_HIP_LOCKSTEP_ADJOINT_LAST_REC == 8 && OSQP_HIP_LOCKSTEP_MAT_ADJOINT_LAST_REC == 8 &&
              OSQP_HIP_LOCKSTEP_DIRECT_ADJOINT_LAST_REC == 8 && OSQP_HIP_LOCKSTEP_DIRECT_MAT_ADJOINT_LAST_REC == 8, "one table (Engine::ls_last_) and one record text for every lockstep record");
constexpr int kLsRecLen = 8;

// what every lockstep route takes from the handle: the matrices, the scalings, the shared vectors, the permutations of a reordered handle
void Engine::fill_lockstep_handle(LockstepParams &p) {
  p.n = n; p.m = m; p.A = d_.A; p.B = d_.B; p.D = d_.D; p.Dinv = d_.Dinv; p.E = d_.E; p.Einv = d_.Einv;
  p.q0 = d_.qraw; p.l0 = d_.lraw; p.u0 = d_.uraw; p.pc = reordered_ ? d_pc_ : nullptr; p.pr = reordered_ ? d_pr_ : nullptr;
}
// The parameters of a forward chunk that do not change from chunk to chunk, for run_lockstep_solve and for the diagnostic entry (test_lockstep), which
// therefore launches on what a solve launches on: the route's work block (allocated by the first call), the settings snapshot of the batch path, the
// handle; with per-problem matrices the route's matrix block (allocated by the first such call, solve or adjoint), the value maps of a reordered handle
// (PCG route; the direct route's position maps are its caller's) and the equilibration's iteration count.
void Engine::fill_lockstep_solve(LsRoute &rt, LockstepParams &p, bool direct, bool mat, int warm, size_t need, size_t mneed) {
  if (!rt.ws) { rt.ws = dev_vec<double>(d_, need); be::sync(d_); }
  fill_batch_settings(p, warm);
  fill_lockstep_handle(p);
  p.ws = rt.ws;
  if (!mat) return;
  bool fresh = false;
  if (!direct) { fresh = ensure_value_maps(); p.pvmap = reordered_ ? d_pvmap_ : nullptr; p.avmap = reordered_ ? d_avmap_ : nullptr; }
  if (!rt.mat_ws) { rt.mat_ws = dev_vec<double>(d_, mneed); fresh = true; }
  if (fresh) be::sync(d_);
  p.mat_ws = rt.mat_ws; p.mat_iters = std::max(0, (int)settings.scaling);
}
// Polish of a chunk's solved problems: the recurrence of Engine::run_recurrence as Engine::polish calls it -- rho_bar = 1 / delta_eff, at least
// 1 + polish_refine_iter steps; on the PCG route the inner systems to polish_pcg_tol within kMaxCg iterations.  The work block is one per handle.
void Engine::fill_lockstep_polish(LockstepParams &p, bool direct) {
  if (!lspw_) { lspw_ = dev_vec<double>(d_, lockstep_polish_ws_doubles(n, m)); be::sync(d_); }
  const double de = std::max(settings.delta, pol_.polish_delta_floor);
  p.polish = 1; p.pol_rho = clamp_rho(1.0 / de); p.pol_min_steps = 1 + std::max(0, (int)settings.polish_refine_iter);
  p.pol_ws = lspw_;
  if (direct) p.pol_prod2 = batch_env().ls_pol_prod2;
  else { p.pol_cg_max = kMaxCg; p.pol_pcg_rel = pol_.polish_pcg_tol; }
}
// The parameters of a backward chunk that do not change from chunk to chunk, for run_lockstep_adjoint and the diagnostic entry (test_lockstep_back): the
// direction's work block and, with mat, the route's matrix block (each allocated by the first call that needs it), the value maps of a reordered handle, the
// settings snapshot, the handle, the recurrence's settings (the direct route has no PCG) and the entry maps of the gradients.  p.v: filled by the caller.
void Engine::fill_lockstep_adjoint(LsRoute &rt, LockstepDirectAdjointParams &p, bool direct, bool mat, size_t need, size_t mneed) {
  bool fresh = ensure_value_maps();
  if (!rt.adj_ws) { rt.adj_ws = dev_vec<double>(d_, need); fresh = true; }
  if (mat && !rt.mat_ws) { rt.mat_ws = dev_vec<double>(d_, mneed); fresh = true; }
  if (mat && direct) { prepare_lockstep_direct_wtpos(); p.v.wtpos = lsd_wtpos_; p.v.vsrc = lsd_vsrc_; }
  if (fresh) be::sync(d_);
  fill_batch_settings(p, 0);
  fill_lockstep_handle(p);
  p.ws = rt.adj_ws;
  const double de = std::max(settings.delta, pol_.polish_delta_floor);
  p.alpha = 1.0; p.rho0 = clamp_rho(1.0 / de); p.eq_factor = 1.0; p.cg_max = direct ? 0 : kMaxCg; p.pcg_rel = direct ? 0.0 : pol_.polish_pcg_tol;
  p.min_steps = 1 + std::max(0, (int)settings.polish_refine_iter); p.max_steps = 60; p.gain = 0.9;
  p.nzP = d_.nzP; p.nzA = d_.nzA; p.Pi = d_.Pi; p.Pj = d_.Pj; p.Ai = d_.Ai; p.Aj = d_.Aj; p.Pmap = reordered_ ? d_pvmap_ : nullptr; p.Amap = reordered_ ? d_avmap_ : nullptr;
  if (mat) {
    p.mat_ws = rt.mat_ws; p.mat_iters = std::max(0, (int)settings.scaling); p.pvmap = p.Pmap; p.avmap = p.Amap;
    if (!direct) lsm_last_count_ = 0;                 // (the block is being overwritten)
  }
}
// device copies of PvalMap_ / AvalMap_ (reordered handle; per-problem matrices and the adjoint read them); true: something was uploaded, sync before use
bool Engine::ensure_value_maps() {
  bool fresh = false;
  if (reordered_ && !d_pvmap_ && d_.nzP > 0) { d_pvmap_ = dev_vec<int>(d_, d_.nzP); be::h2d(d_, d_pvmap_, PvalMap_.data(), sizeof(int) * d_.nzP); fresh = true; }
  if (reordered_ && !d_avmap_ && d_.nzA > 0) { d_avmap_ = dev_vec<int>(d_, d_.nzA); be::h2d(d_, d_avmap_, AvalMap_.data(), sizeof(int) * d_.nzA); fresh = true; }
  return fresh;
}
// what the *_last_record getters share
int Engine::last_record(const double *src, int cnt, double *rec) const {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!rec) return OSQP_DATA_VALIDATION_ERROR;
  std::copy(src, src + cnt, rec);
  return OSQP_NO_ERROR;
}
int Engine::lockstep_last(LsRec which, double *rec) const { return last_record(ls_last_[which], kLsRecLen, rec); }

// ---- which handles the routes take
// The direct route: a handle in the small Woodbury mode whose K0 setup found structurally diagonal (prepare_wb: wb_k0diag_), as numbered by the caller: a
// reordered handle declines.
bool Engine::lockstep_direct_applies() {
  return be::lockstep_direct_chunk && be::lockstep_direct_values && be::device_vec_updates() && d_.wb.on && !d_.wb.large && d_.wb.r >= 1 && d_.wb.r <= kWbMaxRows && wb_k0diag_ && !reordered_;
}
// Per-problem matrices, on either route (include/osqp_hip.h osqp_hip_batch_solve_lockstep_mat): a handle without device assembly and a handle whose stored
// upper triangle of P holds a repeated (j, j) entry (the single-handle assembly sums those with a floating-point atomic; the chunk's assembly has one
// writer per entry) are declined.
bool Engine::mat_assembly_applies() {
  if (!be::device_assembly() || !d_.Praw || !d_.Araw) return false;
  for (int j = 0; j < n; j++) {
    int diag = 0;
    for (int k = P_.p[j]; k < P_.p[j + 1]; k++) diag += P_.i[k] == j;
    if (diag > 1) return false;
  }
  return true;
}
bool Engine::lockstep_mat_applies() { return lockstep_applies() && mat_assembly_applies(); }
bool Engine::lockstep_direct_mat_applies() { return lockstep_direct_applies() && mat_assembly_applies(); }
bool Engine::lockstep_adjoint_applies() { return be::lockstep_adjoint_chunk && be::device_assembly() && be::device_vec_updates() && !d_.wb.on; }
bool Engine::lockstep_direct_adjoint_applies() { return lockstep_direct_applies() && be::lockstep_direct_adjoint_chunk && be::device_assembly(); }
Engine::Applies Engine::solve_applies(bool direct, bool mat) {
  static constexpr Applies table[2][2] = {{&Engine::lockstep_applies, &Engine::lockstep_mat_applies}, {&Engine::lockstep_direct_applies, &Engine::lockstep_direct_mat_applies}};
  return table[direct][mat];
}

// ---- the direct route's view of A and position map
int Engine::prepare_lockstep_direct_view() {
  if (lsd_vrp_) return OSQP_NO_ERROR;
  // the view of A: a one-entry row keeps its entry (vsrc: where it sits in A.val), long row a becomes the entry 1.0 at column n + a
  std::vector<int> vrp(m + 1, 0), vcol, vsrc;
  int a = 0;
  for (int i = 0; i < m; i++) {
    if (Arp_[i + 1] - Arp_[i] > kLongRow) { vcol.push_back(n + a++); vsrc.push_back(-1); }
    else for (int k = Arp_[i]; k < Arp_[i + 1]; k++) { vcol.push_back(Arj_[k]); vsrc.push_back(k); }
    vrp[i + 1] = (int)vcol.size();
  }
  if (a != d_.wb.r) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  lsd_nv_ = (int)vcol.size();
  lsd_vrp_ = dev_vec<int>(d_, m + 1); lsd_vcol_ = dev_vec<int>(d_, vcol.size()); lsd_vsrc_ = dev_vec<int>(d_, vsrc.size()); lsd_vval_ = dev_vec<double>(d_, vcol.size());
  be::h2d(d_, lsd_vrp_, vrp.data(), sizeof(int) * (m + 1)); be::h2d(d_, lsd_vcol_, vcol.data(), sizeof(int) * vcol.size()); be::h2d(d_, lsd_vsrc_, vsrc.data(), sizeof(int) * vsrc.size());
  be::sync(d_);
  return OSQP_NO_ERROR;
}

// The direct view of both directions of the direct route: built on first use, filled, its values refreshed from A's current ones on `stream`
int Engine::fill_lockstep_direct_view(LockstepDirectView &v, void *stream) {
  if (const int err = prepare_lockstep_direct_view()) return err;
  v.r = d_.wb.r; v.WT = d_.wb.WT; v.rows = d_.wb.rows; v.islong = d_.wb.islong;
  v.Av = d_.A; v.Av.ncols = n + v.r; v.Av.nnz = lsd_nv_; v.Av.rowptr = lsd_vrp_; v.Av.col = lsd_vcol_; v.Av.val = lsd_vval_;
  return be::lockstep_direct_values(d_, lsd_nv_, lsd_vsrc_, lsd_vval_, stream);      // (A's values may have changed since the last call)
}

// where entry (long row a, column j) of A sits in the engine's A.val, at j r + a (-1: no entry): what fills a chunk's own dense rows.  Once per handle.
void Engine::prepare_lockstep_direct_wtpos() {
  if (lsd_wtpos_) return;
  const int r = d_.wb.r;
  std::vector<int> pos((size_t)n * r, -1);
  int a = 0;
  for (int i = 0; i < m; i++) {
    if (Arp_[i + 1] - Arp_[i] <= kLongRow) continue;
    for (int k = Arp_[i]; k < Arp_[i + 1]; k++) pos[(size_t)Arj_[k] * r + a] = k;
    a++;
  }
  lsd_wtpos_ = dev_vec<int>(d_, pos.size());
  be::h2d(d_, lsd_wtpos_, pos.data(), sizeof(int) * pos.size());
  be::sync(d_);
}

// ---- solve: the chunk loop of both routes.  Every array of `a` is a DEVICE array in the caller's numbering; the settings are read once, in front of the
// first chunk.  What the routes do differently is said here, once:
//   PCG     the value maps of a reordered handle and lsm_last_count_ (with mat), the PCG rule of polish's recurrence;
//   direct  the view of A (and, with mat, the position map of the dense rows), the single-QP rho rule, the call's seconds in slot 7 of its record.
int Engine::run_lockstep_solve(bool direct, int nbatch, const LockstepSolveIO &a, void *stream) {
  const bool mat = a.mat;
  const int nzP = d_.nzP, nzA = d_.nzA;
  LsRoute &rt = lsr_[direct];
  LockstepDirectParams p;                             // (the PCG route takes its LockstepParams base)
  // direct: the view before any allocation -- its value refresh is a launch on `stream`
  if (direct) if (const int err = fill_lockstep_direct_view(p.v, stream)) return err;
  const size_t need = direct ? lockstep_direct_ws_doubles(n, m, d_.wb.r) : lockstep_ws_doubles(n, m);
  const size_t mneed = direct ? lockstep_direct_mat_ws_doubles(n, m, d_.wb.r, d_.A.nnz, d_.B.nnz, lsd_nv_) : lockstep_mat_ws_doubles(n, m, d_.A.nnz, d_.B.nnz);
  double mst[kLsMatStat] = {0, 0}, mtot = 0;
  if (mat && direct) { prepare_lockstep_direct_wtpos(); p.v.wtpos = lsd_wtpos_; p.v.vsrc = lsd_vsrc_; }
  fill_lockstep_solve(rt, p, direct, mat, a.warm, need, mneed);
  if (mat) p.mat_stat = mst;
  // polish (settings.polishing; with per-problem matrices too: the chunk polishes on its own matrix block): the recurrence of Engine::run_recurrence as
  // Engine::polish calls it, per problem on block vectors -- rho_bar = 1 / delta_eff, at least 1 + polish_refine_iter steps; on the PCG route the inner
  // systems to polish_pcg_tol within kMaxCg iterations, on the direct route the Woodbury solve with S_b inverted once per problem.  The work block is one
  // per handle, shared by both routes, allocated by the first such call.  The polish record: a PCG call always writes it; a direct call writes it when
  // the handle polishes, and once more -- zeros -- when polishing has been switched off since the direct call that wrote it (the record is then no
  // longer that of the last direct call); any other direct call leaves it exactly as it was.
  double pst[kLsPolStat] = {0, 0, 0, 0, 0, 0, 0}, ptot[kLsPolStat] = {0, 0, 0, 0, 0, 0, 0};
  const size_t pneed = lockstep_polish_ws_doubles(n, m);
  const bool pol_record = !direct || settings.polishing || ls_pol_direct_;
  if (settings.polishing) { fill_lockstep_polish(p, direct); p.pol_stat = pst; }
  // direct, adaptive rho as the handle's own solve decides it (ctl_setup: the tolerance on the square-root scale where P has a quadratic part, the
  // persistence test), not as the batch family does: an element then takes the path update(q, l, u) + solve() takes from the same rho
  if (direct) { p.rho_tol_single = pol_rho_tol(settings.adaptive_rho_tolerance, has_quad(), pol_.rho_tol_exp); p.rho_persist = pol_.rho_persist; }
  const double t0 = now_s(), limit = settings.time_limit > 0 && settings.time_limit < 1e9 ? settings.time_limit : 0.0;
  double tot[4] = {0, 0, 0, 0};
  int chunks = 0;
  if (pol_record) std::fill(ls_last_[kLsRecPolish], ls_last_[kLsRecPolish] + kLsRecLen, 0.0);
  for (int b0 = 0; b0 < nbatch; b0 += kLsW, chunks++) {
    p.count = std::min(kLsW, nbatch - b0);
    p.q = a.q ? a.q + (size_t)b0 * n : nullptr; p.l = a.l ? a.l + (size_t)b0 * m : nullptr; p.u = a.u ? a.u + (size_t)b0 * m : nullptr;
    p.x = a.x + (size_t)b0 * n; p.y = a.y + (size_t)b0 * m; p.rec = a.rec + (size_t)b0 * kBatchRec;
    p.Px = (mat && a.Px) ? a.Px + (size_t)b0 * nzP : nullptr; p.Ax = (mat && a.Ax) ? a.Ax + (size_t)b0 * nzA : nullptr;
    p.time_limit = limit > 0 ? std::max(limit - (now_s() - t0), 1e-9) : 0.0;
    double st[4] = {0, 0, 0, 0};
    std::fill(pst, pst + kLsPolStat, 0.0);
    if (mat && !direct) lsm_last_count_ = 0;          // (the block is being overwritten)
    const int err = direct ? be::lockstep_direct_chunk(d_, p, stream, st) : be::lockstep_chunk(d_, p, stream, st);
    if (err) return err;
    if (mat && !direct) lsm_last_count_ = p.count;
    tot[0] = std::max(tot[0], st[0]); tot[1] += st[1]; tot[2] += st[2]; tot[3] += st[3]; mtot += mst[0];
    for (int k = 0; k < kLsPolStat; k++) ptot[k] = k == 3 ? std::max(ptot[k], pst[k]) : ptot[k] + pst[k];
  }
  // the records: the route's own (a PCG call with mat writes it as well), the mat record, the polish record (a PCG call, and a direct call that polishes)
  const double r[kLsRecLen] = {(double)chunks, (double)kLsW, tot[0], tot[1], tot[2], tot[3], (double)(need * sizeof(double)), direct ? now_s() - t0 : 0.0};
  std::copy(r, r + kLsRecLen, ls_last_[direct ? kLsRecDirect : kLsRecSolve]);
  if (mat) {
    const double rm[kLsRecLen] = {(double)chunks, (double)kLsW, tot[0], tot[1], tot[2], tot[3], (double)(mneed * sizeof(double)), mtot};
    std::copy(rm, rm + kLsRecLen, ls_last_[direct ? kLsRecDirectMat : kLsRecMat]);
  }
  if (pol_record) {
    ls_pol_direct_ = direct && settings.polishing;
    std::copy(ptot, ptot + kLsPolStat, ls_last_[kLsRecPolish]);
    ls_last_[kLsRecPolish][kLsPolStat] = settings.polishing ? (double)(pneed * sizeof(double)) : 0.0;
  }
  return OSQP_NO_ERROR;
}

// the host-array entry of both routes, staged like batch_solve.  The PCG route serves a reordered handle, whose own bounds are kept in the engine's numbering.
int Engine::solve_lockstep_host(bool direct, int nbatch, const LockstepSolveIO &h) {
  BatchStage s{*this, nbatch, solve_applies(direct, h.mat), /*own_row=*/(!direct && reordered_) ? ipr_.data() : nullptr, /*wg=*/false};
  const double *Px = h.mat ? h.Px : nullptr, *Ax = h.mat ? h.Ax : nullptr;
  if (const int err = s.in(h.q, h.l, h.u, h.x, h.y, h.rec, h.warm, Px, Ax)) return err;
  const LockstepSolveIO dv{h.q ? s.dq : nullptr, h.l ? s.dl : nullptr, h.u ? s.du : nullptr, s.dx, s.dy, s.drec, h.warm, h.mat, Px ? s.dPx : nullptr, Ax ? s.dAx : nullptr};
  const int err = run_lockstep_solve(direct, nbatch, dv, nullptr);
  if (!err) s.out(h.x, h.y, h.rec);
  return err;
}

// the device-array entry of both routes
int Engine::solve_lockstep_device(bool direct, int nbatch, const LockstepSolveIO &a, void *stream) {
  const int enter = batch_enter(nbatch, true, a.x, a.y, a.rec, solve_applies(direct, a.mat));
  if (enter != kBatchEnter) return enter;
  be::sync(d_);                                       // the solver's own stream first: pending updates of the resident q / l / u, the matrices, the raw matrix values
  return run_lockstep_solve(direct, nbatch, a, stream);
}

// D, E, c of problem b of the last chunk the last PCG-route solve with per-problem matrices processed, in the caller's numbering: read back from the matrix
// block and the chunk's scalar state (row kLsMatScalC), where lockstep_layout.h's carves put them
int Engine::lockstep_mat_scaling(int b, double *D, double *E, double *c) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!D || (m > 0 && !E) || !c) return OSQP_DATA_VALIDATION_ERROR;
  const LsRoute &rt = lsr_[0];
  if (!rt.mat_ws || !rt.ws || b < 0 || b >= lsm_last_count_) return OSQP_DATA_NOT_INITIALIZED;
  be::activate(d_);
  be::ext_wait(d_);
  const size_t nW = (size_t)n * kLsW, mW = (size_t)m * kLsW;
  LsCursor cm{rt.mat_ws};
  LsMatVecs t;
  lockstep_carve_mat(cm, t, n, m, d_.A.nnz, d_.B.nnz);
  const double *dD = t.D, *dE = t.E;
  std::vector<double> h(std::max(nW, mW));
  be::d2h(d_, h.data(), dD, sizeof(double) * nW);
  for (int j = 0; j < n; j++) D[reordered_ ? pc_[j] : j] = h[(size_t)j * kLsW + b];
  if (m > 0) {
    be::d2h(d_, h.data(), dE, sizeof(double) * mW);
    for (int i = 0; i < m; i++) E[reordered_ ? pr_[i] : i] = h[(size_t)i * kLsW + b];
  }
  double cs[kLsW];
  be::d2h(d_, cs, rt.ws + lockstep_sc_offset(n, m) + (size_t)kLsMatScalC * kLsW, sizeof(cs));
  *c = cs[b];
  return OSQP_NO_ERROR;
}

// ---- adjoint: the chunk loop of both routes (lockstep_hip.hip lockstep_adjoint_chunk / lockstep_direct_adjoint_chunk), chunk after chunk like
// run_lockstep_solve.  Every array is a DEVICE array in the caller's numbering (dP / dA: the caller's CSC order).  The recurrence's settings are those of
// Engine::run_recurrence as the single-QP adjoint calls it: rho_bar = 1 / delta_eff on the active rows with equality factor 1, alpha = 1, PCG to
// polish_pcg_tol within kMaxCg (direct: no PCG -- the recurrence's rho is fixed, so S_b is inverted once per problem), progress rule {rhs_norm, 0.9, 60}
// after at least 1 + polish_refine_iter steps.  The work block (adj_ws) is the direction's own; the direct route's view of A is the forward's (read only,
// its values refreshed per call); the forward's workspace and records are not written.  a.mat: every chunk assembles and equilibrates its problems' own
// matrices in the route's matrix block, which this call therefore overwrites -- lockstep_mat_scaling answers OSQP_DATA_NOT_INITIALIZED until the next
// forward call.  A forward call prepares its block anew, so its results do not depend on this one.
int Engine::run_lockstep_adjoint(bool direct, int nbatch, const LockstepAdjointIO &a, void *stream) {
  const int nzP = d_.nzP, nzA = d_.nzA;
  const bool mat = a.mat;
  LsRoute &rt = lsr_[direct];
  const size_t need = direct ? lockstep_direct_adjoint_ws_doubles(n, m, d_.wb.r) : lockstep_adjoint_ws_doubles(n, m);
  LockstepDirectAdjointParams p;                      // (the PCG route takes its LockstepAdjointParams base)
  if (direct) if (const int err = fill_lockstep_direct_view(p.v, stream)) return err;
  const size_t mneed = direct ? lockstep_direct_mat_ws_doubles(n, m, d_.wb.r, d_.A.nnz, d_.B.nnz, lsd_nv_) : lockstep_mat_ws_doubles(n, m, d_.A.nnz, d_.B.nnz);
  fill_lockstep_adjoint(rt, p, direct, mat, need, mneed);
  double mst[kLsMatStat] = {0, 0}, mtot = 0;
  if (mat) p.mat_stat = mst;
  double tot[4] = {0, 0, 0, 0};
  int chunks = 0;
  auto at = [](auto *v, size_t off) { return v ? v + off : nullptr; };
  for (int b0 = 0; b0 < nbatch; b0 += kLsW, chunks++) {
    const size_t b = (size_t)b0;
    p.count = std::min(kLsW, nbatch - b0);
    p.l = at(a.l, b * m); p.u = at(a.u, b * m); p.sx = a.x + b * n; p.sy = at(a.y, b * m); p.gx = a.dx + b * n; p.gy = at(a.dy, b * m);
    p.dP = at(a.dP, b * nzP); p.dq = at(a.dq, b * n); p.dA = at(a.dA, b * nzA); p.dl = at(a.dl, b * m); p.du = at(a.du, b * m); p.arec = at(a.arec, b * kAdjointRec);
    if (mat) { p.Px = at(a.Px, b * nzP); p.Ax = at(a.Ax, b * nzA); }
    double st[4] = {0, 0, 0, 0};
    const int err = direct ? be::lockstep_direct_adjoint_chunk(d_, p, stream, st) : be::lockstep_adjoint_chunk(d_, p, stream, st);
    if (err) return err;
    tot[0] = std::max(tot[0], st[0]); tot[1] += st[1]; tot[2] += st[2]; tot[3] += st[3]; mtot += mst[0];
  }
  const double r[kLsRecLen] = {(double)chunks, (double)kLsW, tot[0], tot[1], tot[2], tot[3], (double)(need * sizeof(double)), 0.0};
  std::copy(r, r + kLsRecLen, ls_last_[direct ? kLsRecDirectAdjoint : kLsRecAdjoint]);
  if (mat) {
    const double rm[kLsRecLen] = {(double)chunks, (double)kLsW, tot[0], tot[1], tot[2], tot[3], (double)(mneed * sizeof(double)), mtot};
    std::copy(rm, rm + kLsRecLen, ls_last_[direct ? kLsRecDirectMatAdjoint : kLsRecMatAdjoint]);
  }
  return OSQP_NO_ERROR;
}

// the host-array entry of both routes: one device scratch block per route, kept for the next call
int Engine::adjoint_lockstep_host(bool direct, int nbatch, const LockstepAdjointIO &h) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (nbatch <= 0 || !h.x || (!h.y && m > 0) || !h.dx) return OSQP_DATA_VALIDATION_ERROR;
  be::activate(d_);
  if (!(direct ? lockstep_direct_adjoint_applies() : lockstep_adjoint_applies()) || (h.mat && !(this->*solve_applies(direct, true))())) return OSQP_FUNC_NOT_IMPLEMENTED;
  be::ext_wait(d_);
  DevScratch &sc = lsr_[direct].adj_buf;
  const size_t nb = (size_t)nbatch, N = nb * n, M = nb * m, NP = nb * (size_t)d_.nzP, NA = nb * (size_t)d_.nzA;
  const size_t MP = (h.mat && h.Px) ? NP : 0, MA = (h.mat && h.Ax) ? NA : 0;
  // [l | u | x | y | dx | dy | dP | dq | dA | dl | du | arec | Px | Ax]   (the last two: per-problem matrices, where given)
  const size_t need = 3 * N + 6 * M + NP + NA + nb * kAdjointRec + MP + MA;
  if (need > sc.cap) { if (sc.buf) be::dfree(d_, sc.buf); sc.cap = 0; sc.buf = dev_vec<double>(d_, need); sc.cap = need; }
  double *d_l = sc.buf, *d_u = d_l + M, *d_x = d_u + M, *d_y = d_x + N, *d_dx = d_y + M, *d_dy = d_dx + N;
  double *o_dP = d_dy + M, *o_dq = o_dP + NP, *o_dA = o_dq + N, *o_dl = o_dA + NA, *o_du = o_dl + M, *o_rec = o_du + M;
  double *d_Px = o_rec + nb * kAdjointRec, *d_Ax = d_Px + MP;
  auto up = [&](double *dst, const double *src, size_t cnt) { if (src && cnt) be::h2d(d_, dst, src, sizeof(double) * cnt); };
  up(d_l, h.l, M); up(d_u, h.u, M); up(d_x, h.x, N); up(d_y, h.y, M); up(d_dx, h.dx, N); up(d_dy, h.dy, M); up(d_Px, h.Px, MP); up(d_Ax, h.Ax, MA);
  be::sync(d_);
  const LockstepAdjointIO dv{h.l ? d_l : nullptr, h.u ? d_u : nullptr, d_x, d_y, d_dx, h.dy ? d_dy : nullptr, h.dP ? o_dP : nullptr, h.dq ? o_dq : nullptr,
                             h.dA ? o_dA : nullptr, h.dl ? o_dl : nullptr, h.du ? o_du : nullptr, h.arec ? o_rec : nullptr,
                             h.mat, MP ? d_Px : nullptr, MA ? d_Ax : nullptr};
  if (const int err = run_lockstep_adjoint(direct, nbatch, dv, nullptr)) return err;
  auto down = [&](double *dst, const double *src, size_t cnt) { if (dst && cnt) be::d2h(d_, dst, src, sizeof(double) * cnt); };
  down(h.dP, o_dP, NP); down(h.dq, o_dq, N); down(h.dA, o_dA, NA); down(h.dl, o_dl, M); down(h.du, o_du, M); down(h.arec, o_rec, nb * kAdjointRec);
  return OSQP_NO_ERROR;
}

// the device-array entry of both routes
int Engine::adjoint_lockstep_device(bool direct, int nbatch, const LockstepAdjointIO &a, void *stream) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (nbatch < 0) return OSQP_DATA_VALIDATION_ERROR;
  be::activate(d_);
  if (!(direct ? lockstep_direct_adjoint_applies() : lockstep_adjoint_applies()) || (a.mat && !(this->*solve_applies(direct, true))())) return OSQP_FUNC_NOT_IMPLEMENTED;
  if (nbatch == 0) return OSQP_NO_ERROR;              // (the applicability query, as osqp_hip_batch_solve_lockstep_device answers it)
  if (!a.x || (!a.y && m > 0) || !a.dx) return OSQP_DATA_VALIDATION_ERROR;
  be::ext_wait(d_);
  be::sync(d_);                                       // the solver's own stream first: pending updates of the resident l / u, the matrices
  return run_lockstep_adjoint(direct, nbatch, a, stream);
}

// ------------------------------------------------------------------------------------------------ adjoint derivatives
// The backward pass of the batch path (batch_hip.hip k_batch_adjoint).  A problem is eligible when the forward's direct variant holds it (banded factor
// under the engine's ordering: prepare_batch_direct) and the adjoint kernel's own LDS fits; the batch entry points answer OSQP_FUNC_NOT_IMPLEMENTED for
// everything else.  osqp_adjoint_derivative_compute goes on to the PCG route for a single handle (adjoint_compute_pcg below).
bool Engine::adjoint_applicable() {
  if (!be::batch_adjoint || !be::device_assembly() || !be::device_vec_updates() || reordered_ || !be::batch_lds_bytes(n, m)) return false;
  prepare_batch_direct();
  return bd_.ok && batch_adjoint_lds_bytes(n, m, d_.A.nnz, d_.B.nnz, bd_.bw) != 0;
}

void Engine::fill_adjoint_params(AdjointParams &p, int nbatch) {
  p.n = n; p.m = m; p.nbatch = nbatch; p.nzP = d_.nzP; p.nzA = d_.nzA; p.A = d_.A; p.B = d_.B; p.Praw = d_.Praw; p.Araw = d_.Araw;
  p.Pi = d_.Pi; p.Pj = d_.Pj; p.Pm1 = d_.Pm1; p.Pm2 = d_.Pm2; p.Ai = d_.Ai; p.Aj = d_.Aj; p.AmA = d_.AmA; p.AmB = d_.AmB;
  p.l0 = d_.lraw; p.u0 = d_.uraw; p.delta = settings.delta; p.refine = settings.polish_refine_iter;
  p.bw = bd_.bw; p.nents = bd_.nents; p.ntri = bd_.ntri; p.perm = bd_.perm; p.bp_slot = bd_.bp_slot; p.ke_slot = bd_.ke_slot; p.ke_ptr = bd_.ke_ptr;
  p.kp_row = bd_.kp_row; p.kp_a = bd_.kp_a; p.kp_b = bd_.kp_b; p.tri = bd_.tri;
}

int Engine::batch_adjoint(int nbatch, const double *Px, const double *Ax, const double *l, const double *u, const double *x, const double *y, const double *dx, const double *dy,
                          double *dP, double *dq, double *dA, double *dl, double *du, double *arec) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (nbatch <= 0 || !x || !y || !dx) return OSQP_DATA_VALIDATION_ERROR;
  be::activate(d_);
  if (!adjoint_applicable()) return OSQP_FUNC_NOT_IMPLEMENTED;
  be::ext_wait(d_);
  const size_t nb = (size_t)nbatch, N = nb * n, M = nb * m, NP = nb * (size_t)d_.nzP, NA = nb * (size_t)d_.nzA;
  // one device scratch block, kept for the next call: [Px | Ax | l | u | x | y | dx | dy | dP | dq | dA | dl | du | arec]
  const size_t need = 2 * NP + 2 * NA + 3 * N + 6 * M + nb * kAdjointRec;
  if (need > abuf_cap_) { if (abuf_) be::dfree(d_, abuf_); abuf_ = dev_vec<double>(d_, need); abuf_cap_ = need; }
  double *dPx = abuf_, *dAx = dPx + NP, *d_l = dAx + NA, *d_u = d_l + M, *d_x = d_u + M, *d_y = d_x + N, *d_dx = d_y + M, *d_dy = d_dx + N;
  double *o_dP = d_dy + M, *o_dq = o_dP + NP, *o_dA = o_dq + N, *o_dl = o_dA + NA, *o_du = o_dl + M, *o_rec = o_du + M;
  auto up = [&](double *dst, const double *src, size_t cnt) { if (src && cnt) be::h2d(d_, dst, src, sizeof(double) * cnt); };
  up(dPx, Px, NP); up(dAx, Ax, NA); up(d_l, l, M); up(d_u, u, M); up(d_x, x, N); up(d_y, y, M); up(d_dx, dx, N); up(d_dy, dy, M);
  AdjointParams p{};
  fill_adjoint_params(p, nbatch);
  p.Px_b = Px ? dPx : nullptr; p.Ax_b = Ax ? dAx : nullptr; p.l = l ? d_l : nullptr; p.u = u ? d_u : nullptr;
  p.x = d_x; p.y = d_y; p.dx = d_dx; p.dy = dy ? d_dy : nullptr;
  p.dP = dP ? o_dP : nullptr; p.dq = dq ? o_dq : nullptr; p.dA = dA ? o_dA : nullptr; p.dl = dl ? o_dl : nullptr; p.du = du ? o_du : nullptr; p.arec = arec ? o_rec : nullptr;
  be::sync(d_);
  const int err = be::batch_adjoint(d_, p, nullptr);
  if (err) return err;
  auto down = [&](double *dst, const double *src, size_t cnt) { if (dst && cnt) be::d2h(d_, dst, src, sizeof(double) * cnt); };
  down(dP, o_dP, NP); down(dq, o_dq, N); down(dA, o_dA, NA); down(dl, o_dl, M); down(du, o_du, M); down(arec, o_rec, nb * kAdjointRec);
  return OSQP_NO_ERROR;
}

int Engine::batch_adjoint_device(int nbatch, const double *Px, const double *Ax, const double *l, const double *u, const double *x, const double *y, const double *dx, const double *dy,
                                 double *dP, double *dq, double *dA, double *dl, double *du, double *arec, void *stream) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (nbatch < 0) return OSQP_DATA_VALIDATION_ERROR;
  be::activate(d_);
  if (!adjoint_applicable()) return OSQP_FUNC_NOT_IMPLEMENTED;
  if (nbatch == 0) return OSQP_NO_ERROR;                     // (the applicability query, as osqp_hip_batch_solve_device answers it)
  if (!x || !y || !dx) return OSQP_DATA_VALIDATION_ERROR;
  be::ext_wait(d_);
  AdjointParams p{};
  fill_adjoint_params(p, nbatch);
  p.Px_b = Px; p.Ax_b = Ax; p.l = l; p.u = u; p.x = x; p.y = y; p.dx = dx; p.dy = dy;
  p.dP = dP; p.dq = dq; p.dA = dA; p.dl = dl; p.du = du; p.arec = arec;
  be::sync(d_);                                              // as batch_solve_device (launch_batch, wait_solver): the kernel goes on the CALLER's stream and reads what the solver's own stream may still be writing -- the symbolic data's uploads, a pending update of the resident P / A / l / u
  const int err = be::batch_adjoint(d_, p, stream);
  if (!err) be::ext_record(d_, stream);                      // the kernel reads the solver's own matrices and bounds
  return err;
}

// The PCG path's adjoint (adjoint_hip.hip) holds every handle whose solve runs the multi-kernel PCG form with a Jacobi-family preconditioner.  A handle
// with a Woodbury-corrected preconditioner (dense rows; the portfolio one-launch form is one of its modes) is taken with OSQPHipPolicy::adjoint_woodbury
// only: the route changes the constraint classes on the device, past the host classification that keeps the correction's bookkeeping in step for
// polish, so adjoint_compute_pcg saves and restores that bookkeeping itself (WbSave below).  The default stays OSQP_FUNC_NOT_IMPLEMENTED.
bool Engine::adjoint_pcg_applicable() const {
  return be::adjoint_load && be::adjoint_residual && be::adjoint_gradients && be::device_assembly() && be::device_vec_updates() && (!d_.wb.on || pol_.adjoint_woodbury != 0);
}

void Engine::wb_save(WbSave &s) const {
  const DevWb &w = d_.wb;
  s.exact = w.exact; s.slots = w.x.slots; s.rho_key = w.rho_key; s.Sinv = w.Sinv;
  for (int k = 0; k < DevWb::kCache; k++) { s.cache_buf[k] = w.cache_buf[k]; s.cache_rho[k] = w.cache_rho[k]; }
  s.cache_used = w.cache_used; s.cache_next = w.cache_next; s.cache_hits = w.cache_hits;
}
// Large form: the adjoint's classes give another rho vector under a rho_bar the handle may have seen, so no cached inverse may be looked up (with the
// probe off nothing would notice), and the factorisation must not evict the inverse the solve is using.  For the length of the recurrence the table
// holds one free buffer of the call's own and no entry.
void Engine::wb_enter_adjoint() {
  DevWb &w = d_.wb;
  if (!w.large) return;
  const size_t ord = w.dual ? (size_t)w.cd : (size_t)w.r, need = ord * ord;
  if (need > adj_sinv_cap_) { if (adj_sinv_) be::dfree(d_, adj_sinv_); adj_sinv_cap_ = 0; adj_sinv_ = dev_vec<double>(d_, need); adj_sinv_cap_ = need; }
  w.cache_buf[0] = adj_sinv_; w.cache_rho[0] = -1.0;
  for (int k = 1; k < DevWb::kCache; k++) { w.cache_buf[k] = nullptr; w.cache_rho[k] = -1.0; }
  w.cache_used = 1; w.cache_next = 0;
}
void Engine::wb_restore_state(const WbSave &s) {
  DevWb &w = d_.wb;
  w.exact = s.exact; w.x.slots = s.slots; w.Sinv = s.Sinv;
  for (int k = 0; k < DevWb::kCache; k++) { w.cache_buf[k] = s.cache_buf[k]; w.cache_rho[k] = s.cache_rho[k]; }
  w.cache_used = s.cache_used; w.cache_next = s.cache_next;
}
void Engine::wb_restore_keys(const WbSave &s) {
  DevWb &w = d_.wb;
  w.rho_key = s.rho_key; w.cache_hits = s.cache_hits; w.cache_next = s.cache_next;
}

// osqp_adjoint_derivative_compute: needs the solution of a solve that ended OSQP_SOLVED on the current data (every data update resets the status);
// OSQP_DATA_NOT_INITIALIZED otherwise.  The batch kernel where it holds the problem, the PCG route otherwise.
int Engine::adjoint_compute(const double *dx, const double *dy) { return adjoint_compute_at(nullptr, nullptr, dx, dy); }

// The same at a solution the CALLER holds (x, y in the caller's numbering; nullptr: the handle's last solution, which then has to be OSQP_SOLVED on
// the current data): the derivative is a function of (P, A, l, u, x, y) alone, so a caller that kept (x, y) of an earlier solve -- the torch layer's
// backward, one element after the other on one handle -- needs the data on the handle, not another solve.
int Engine::adjoint_compute_at(const double *x, const double *y, const double *dx, const double *dy) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  adj_ok_ = false;
  for (double &v : adj_rec_) v = 0.0;
  be::activate(d_);
  const bool batch = adjoint_applicable();
  if (!batch && !adjoint_pcg_applicable()) return OSQP_FUNC_NOT_IMPLEMENTED;
  if (!x != !y && m > 0) return OSQP_DATA_VALIDATION_ERROR;
  if (!x) { if (info.status_val != OSQP_SOLVED) return OSQP_DATA_NOT_INITIALIZED; x = sol_x_.data(); y = sol_y_.data(); }
  std::vector<double> zero;
  if (!dx) { zero.assign(n, 0.0); dx = zero.data(); }
  adj_dP_.assign(P_.nnz(), 0.0); adj_dA_.assign(A_.nnz(), 0.0); adj_dq_.assign(n, 0.0); adj_dl_.assign(m, 0.0); adj_du_.assign(m, 0.0);
  if (!batch) return adjoint_compute_pcg(x, y, dx, m > 0 ? dy : nullptr);
  std::vector<double> yv(std::max(m, 1), 0.0);
  if (m > 0) std::copy(y, y + m, yv.begin());
  double arec[kAdjointRec] = {0, 0, 0, 0};
  const int err = batch_adjoint(1, nullptr, nullptr, nullptr, nullptr, x, yv.data(), dx, m > 0 ? dy : nullptr,
                                adj_dP_.empty() ? nullptr : adj_dP_.data(), adj_dq_.data(), adj_dA_.empty() ? nullptr : adj_dA_.data(),
                                m > 0 ? adj_dl_.data() : nullptr, m > 0 ? adj_du_.data() : nullptr, arec);
  adj_ok_ = err == OSQP_NO_ERROR;
  for (int k = 0; k < 3; k++) adj_rec_[k] = arec[k];
  return err;
}

// The PCG route: classify the rows on the device, load q~ = c D dx and the bounds b~ = -E dy of the active rows, run polish's recurrence from a
// zero start, unscale, evaluate the unregularised residual, run the gradient kernels.  Everything the recurrence touches -- q, the bounds and
// classes, the iterates and the PCG's starting vectors, rho, alpha, the predictions and statistics -- is saved first and put back bit for bit: a
// solve after this call runs as if the call had not been made.  info, solution and the history feed are never written.
// On a handle with a Woodbury-corrected preconditioner (wb): run_recurrence's set_rho + precond re-form D0, the weights and S (or T) from the device
// rho vector of the adjoint's classes, in every mode; a direct mode whose check (small form) or probe (large form) does not hold there -- the lasso's
// row pairs lose their equal weights -- runs as the PCG's preconditioner.  WbSave is put back around recurrence_restore_rho, which re-forms the
// correction at the solve's rho: launches in the small form, a look-up of the solve's own cached inverse in the large form (a second factorisation
// where the cache is off).  A Woodbury system that is not positive definite at the adjoint's rho ends the call with status 3, the correction kept.
int Engine::adjoint_compute_pcg(const double *x, const double *y, const double *dx, const double *dy) {
  const double t_begin = now_s();
  be::ext_wait(d_);
  const size_t N = (size_t)n, M = (size_t)m, NP = (size_t)d_.nzP, NA = (size_t)d_.nzA, MI = (M + 1) / 2;      // MI: doubles that hold m ints
  // one device block, kept for the next call: saved state | inputs | work | results
  const size_t need = 6 * N + 9 * M + MI + 2 * N + 2 * M + N + M + MI + NP + NA + 2 * M + kAdjointPcgRec;
  if (need > adjw_cap_) { if (adjw_) be::dfree(d_, adjw_); adjw_cap_ = 0; adjw_ = dev_vec<double>(d_, need); adjw_cap_ = need; }
  double *p = adjw_;
  auto take = [&p](size_t cnt) { double *r = p; p += cnt; return r; };
  struct Kept { double *dev, *copy; size_t bytes; };
  std::vector<Kept> kept;
  for (double *v : {d_.x, d_.xs, d_.xg, d_.xsp, d_.dx, d_.q}) kept.push_back({v, take(N), sizeof(double) * N});
  for (double *v : {d_.z, d_.y, d_.zt, d_.ztg, d_.t0, d_.v, d_.dy, d_.l, d_.u}) kept.push_back({v, take(M), sizeof(double) * M});
  kept.push_back({reinterpret_cast<double *>(d_.ctype), take(MI), sizeof(int) * M});
  double *i_x = take(N), *i_dx = take(N), *i_y = take(M), *i_dy = take(M);
  double *w_rx = take(N), *w_ry = take(M); int *w_code = reinterpret_cast<int *>(take(MI));
  double *o_dP = take(NP), *o_dA = take(NA), *o_dl = take(M), *o_du = take(M), *o_rec = take(kAdjointPcgRec);
  for (const Kept &k : kept) be::copy_in(d_, k.copy, k.dev, k.bytes, 1);
  // the stored solution and the incoming gradients, in the engine's numbering
  {
    std::vector<double> t;
    auto up_n = [&](double *dst, const double *src) { if (reordered_) { t = to_internal_n(src); src = t.data(); } be::h2d(d_, dst, src, sizeof(double) * N); };
    auto up_m = [&](double *dst, const double *src) { if (!M) return; if (reordered_) { t = to_internal_m(src); src = t.data(); } be::h2d(d_, dst, src, sizeof(double) * M); };
    up_n(i_x, x); up_n(i_dx, dx); up_m(i_y, y); if (dy) up_m(i_dy, dy);
  }
  AdjointPcg a;
  a.x = i_x; a.y = i_y; a.dx = i_dx; a.dy = dy ? i_dy : nullptr; a.code = w_code; a.rx = w_rx; a.ry = w_ry;
  a.dP = o_dP; a.dA = o_dA; a.dl = o_dl; a.du = o_du; a.rec = o_rec; a.c = c_; a.cinv = cinv_; a.rho_is_vec = settings.rho_is_vec;
  const OSQPInfo info0 = info;
  RecurrenceSave keep;
  recurrence_save(keep);
  const bool wb = d_.wb.on != 0;
  WbSave wkeep{};
  if (wb) wb_save(wkeep);
  auto put_back = [&]() {
    recurrence_restore_launch(keep);
    for (const Kept &k : kept) if (k.dev == d_.l || k.dev == d_.u || k.dev == reinterpret_cast<double *>(d_.ctype)) be::copy_in(d_, k.dev, k.copy, k.bytes, 1);
    d_.rho_eq_factor = keep.eq_factor;
    if (wb) wb_restore_state(wkeep);
    recurrence_restore_rho(keep);                   // rho, the preconditioner (and K's values) from the solve's classes again ...
    if (wb) wb_restore_keys(wkeep);
    for (const Kept &k : kept) be::copy_in(d_, k.dev, k.copy, k.bytes, 1);      // ... then every vector as the solve left it (set_rho rewrites v, t0 and the PCG's start)
    info = info0;
    be::sync(d_);
  };
  double rec[kAdjointPcgRec] = {0, 0, 0, 0};
  int steps = 0;
  double t_rec = 0, t_grad = 0, pcg = 0;
  bool singular = false, not_spd = false;
  try {
    if (wb) wb_enter_adjoint();
    be::adjoint_load(d_, a);
    be::d2h(d_, rec, o_rec, sizeof(double));
    singular = rec[0] > (double)n;                  // more active rows than variables: K_a is singular, nothing to iterate on
    if (!singular) {
      double res[R_COUNT];
      const double t0 = now_s();
      // from a zero start the recurrence has to converge, not correct: it ends when two steps in a row gain less than 10 %, within twice polish's
      // cap (under polish's rule the n = 100k banded QP with a random dy ended at 3.2e-5 after 12 steps; with this one at 5.4e-10 after 23:
      // DESIGN.md section 6)
      steps = run_recurrence(RecurrenceRule{true, 0.9, 60}, res);
      pcg = recurrence_pcg_;
      t_rec = now_s() - t0;
      be::adjoint_residual(d_, a);
      be::sync(d_);
      const double t1 = now_s();
      be::adjoint_gradients(d_, a);
      be::sync(d_);
      t_grad = now_s() - t1;
      be::d2h(d_, rec, o_rec, sizeof(double) * kAdjointPcgRec);
    }
  } catch (const NotPositiveDefinite &) {           // the correction at the adjoint's rho vector: the handle keeps it for its solves, the call reports "not solved"
    if (!wb) { put_back(); throw; }
    not_spd = true;
  } catch (...) {
    put_back();
    throw;
  }
  const double resid = (singular || not_spd) ? INFINITY : (rec[2] > 0.0 ? rec[1] / rec[2] : (rec[1] > 0.0 ? INFINITY : 0.0));
  const int status = singular ? 2 : (resid < kAdjointTol ? 0 : 3);
  if (status == 0) {
    std::vector<double> t;
    auto down = [&](std::vector<double> &dst, const double *src, const std::vector<int> *perm) {      // perm: engine position -> caller's
      if (dst.empty()) return;
      if (!perm) { be::d2h(d_, dst.data(), src, sizeof(double) * dst.size()); return; }
      t.resize(dst.size());
      be::d2h(d_, t.data(), src, sizeof(double) * dst.size());
      for (size_t k = 0; k < dst.size(); k++) dst[(*perm)[k]] = t[k];
    };
    const bool ro = reordered_;
    down(adj_dq_, w_rx, ro ? &pc_ : nullptr); down(adj_dl_, o_dl, ro ? &pr_ : nullptr); down(adj_du_, o_du, ro ? &pr_ : nullptr);
    if (!ro) { down(adj_dP_, o_dP, nullptr); down(adj_dA_, o_dA, nullptr); }
    else {                                          // PvalMap_ / AvalMap_: caller's position -> the engine's
      auto gather = [&](std::vector<double> &dst, const double *src, const std::vector<int> &map) {
        if (dst.empty()) return;
        t.resize(dst.size());
        be::d2h(d_, t.data(), src, sizeof(double) * dst.size());
        for (size_t k = 0; k < dst.size(); k++) dst[k] = t[map[k]];
      };
      gather(adj_dP_, o_dP, PvalMap_); gather(adj_dA_, o_dA, AvalMap_);
    }
  }
  put_back();
  adj_rec_[0] = status; adj_rec_[1] = rec[0]; adj_rec_[2] = resid; adj_rec_[3] = steps;
  adj_rec_[4] = t_rec; adj_rec_[5] = t_grad; adj_rec_[6] = now_s() - t_begin; adj_rec_[7] = pcg;
  adj_ok_ = status == 0;
  return adj_ok_ ? OSQP_NO_ERROR : OSQP_LINSYS_SOLVER_INIT_ERROR;
}

int Engine::adjoint_last_record(double *rec) const { return last_record(adj_rec_, OSQP_HIP_ADJOINT_LAST_REC, rec); }

int Engine::adjoint_get_mat(OSQPCscMatrix *dP, OSQPCscMatrix *dA) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!adj_ok_) return (adjoint_applicable() || adjoint_pcg_applicable()) ? OSQP_DATA_NOT_INITIALIZED : OSQP_FUNC_NOT_IMPLEMENTED;
  // the caller passes the patterns of P's upper triangle and of A as given at setup; the values arrive in that order
  if (dP) { if (!dP->x || dP->n != n || !dP->p || dP->p[n] != P_.nnz()) return OSQP_DATA_VALIDATION_ERROR; std::copy(adj_dP_.begin(), adj_dP_.end(), dP->x); }
  if (dA) { if (!dA->x || dA->n != n || dA->m != m || !dA->p || dA->p[n] != A_.nnz()) return OSQP_DATA_VALIDATION_ERROR; std::copy(adj_dA_.begin(), adj_dA_.end(), dA->x); }
  return OSQP_NO_ERROR;
}

int Engine::adjoint_get_vec(double *dq, double *dl, double *du) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!adj_ok_) return (adjoint_applicable() || adjoint_pcg_applicable()) ? OSQP_DATA_NOT_INITIALIZED : OSQP_FUNC_NOT_IMPLEMENTED;
  if (dq) std::copy(adj_dq_.begin(), adj_dq_.end(), dq);
  if (dl) std::copy(adj_dl_.begin(), adj_dl_.end(), dl);
  if (du) std::copy(adj_du_.begin(), adj_du_.end(), du);
  return OSQP_NO_ERROR;
}

int Engine::get_stats(OSQPHipStats *out) {
  if (!out) return OSQP_DATA_VALIDATION_ERROR;
  *out = stats_; out->pcg_fused = (d_.f1.on && use_slots_) ? 2.0 : ((d_.kf.on && use_slots_) ? 3.0 : (be::pcg_fused(d_) ? 1.0 : 0.0)); out->batch_direct_bw = bd_.bw_symbolic;
  out->f1_replicas = d_.f1.on ? d_.f1.D : 0;
  out->kform_nnz = d_.kf.on ? (double)d_.kf.K.nnz : 0.0;
  out->batch_wave_split = (double)batch_wave_last_;
  out->woodbury_dual_cols = (d_.wb.on && d_.wb.dual) ? (double)d_.wb.cd : 0.0;
  out->woodbury_fused_iteration = be::wbf_active(d_) ? (d_.wb.dense ? (d_.wb.thin ? 3.0 : 2.0) : 1.0) : 0.0;
  out->woodbury_one_launch = (be::wbx_active(d_) && d_.wb.x.one && !d_.wb.x.slots) ? 1.0 : 0.0;
  out->woodbury_rows = d_.wb.on ? d_.wb.r : 0; out->woodbury_direct = (d_.wb.on && d_.wb.exact) ? ((d_.wb.x.on) ? 2 : 1) : 0;
  out->windowed_blocks = d_.A.nwin + d_.B.nwin; out->row_blocks = d_.A.nblk + d_.B.nblk;
  out->reordered = reordered_ ? 1.0 : 0.0; out->reorder_ms = reorder_ms_;
  out->f1_far_columns = d_.f1.on && d_.f1.mix ? (double)d_.f1.nsp : 0.0;
  // which preconditioner the PCG of this handle runs with RIGHT NOW (the setting cg_precond = diagonal selects the Jacobi family; the
  // Woodbury correction for dense rows is the engine's addition: OSQPHipPolicy::woodbury / woodbury_large switch it off)
  out->preconditioner = settings.cg_precond != OSQP_DIAGONAL_PRECONDITIONER ? OSQP_HIP_PRECOND_NONE
                        : !d_.wb.on ? OSQP_HIP_PRECOND_JACOBI : (d_.wb.large ? OSQP_HIP_PRECOND_JACOBI_WOODBURY_DENSE : OSQP_HIP_PRECOND_JACOBI_WOODBURY);
  return OSQP_NO_ERROR;
}
int Engine::time_kernel(int which, int reps, double *ms) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  be::activate(d_);
  if (which < 0 || which > 25 || reps <= 0 || !ms) return OSQP_DATA_VALIDATION_ERROR;
  if (which >= 24 && !dk_direct(d_.dk)) return OSQP_FUNC_NOT_IMPLEMENTED;      // 24 / 25: the dense KKT mode's hot path, on a handle that solves direct
  if (which == 25) {
    // one ADMM iteration of the dense KKT mode (KB, K^-1 r_0, KA) as a solve runs it: a REPLAYED chunk of `reps` iterations between the solve's event pair,
    // ms per iteration.  The iterates move on (tools/dense_kkt_bench.py solves cold afterwards).
    reps = std::min(reps, 1024);
    sync_graph_scalars();
    run_chunk(reps, 0);                                 // (captures the chunk's graph and warms it)
    be::ev_mark(d_, 0); run_chunk(reps, 0); be::ev_mark(d_, 1);
    *ms = be::ev_ms(d_) / reps;
    int flags[F_COUNT]; be::fetch_flags(d_, flags);     // (the chunk's PCG statistics are not a solve's)
    return OSQP_NO_ERROR;
  }
  *ms = be::time_kernel(d_, which, reps);
  return OSQP_NO_ERROR;
}
int Engine::trace_read(unsigned long long *out, int count) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!out || count <= 0) return OSQP_DATA_VALIDATION_ERROR;
  return be::ktrace_read(d_, out, count) ? OSQP_NO_ERROR : OSQP_FUNC_NOT_IMPLEMENTED;
}
int Engine::test_spmv(int which, const double *in, double *out) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  be::activate(d_);
  const int nin = which == 0 ? n : n + m, nout = which == 0 ? m : n;
  double *din = dev_vec<double>(d_, nin), *dout = dev_vec<double>(d_, nout);
  std::vector<double> hin(in, in + nin), hout(nout);
  if (reordered_) {                                   // (vectors of the caller's numbering, like everything else at the API)
    for (int j = 0; j < n; j++) hin[j] = in[pc_[j]];
    if (which != 0) for (int i = 0; i < m; i++) hin[n + i] = in[n + pr_[i]];
  }
  be::h2d(d_, din, hin.data(), sizeof(double) * nin);
  be::test_spmv(d_, which, din, dout);
  be::d2h(d_, hout.data(), dout, sizeof(double) * nout);
  for (int k = 0; k < nout; k++) out[reordered_ ? (which == 0 ? pr_[k] : pc_[k]) : k] = hout[k];
  be::dfree(d_, din); be::dfree(d_, dout);
  return OSQP_NO_ERROR;
}
int Engine::test_dense(OSQPHipDenseTest *t) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!be::test_dense) return OSQP_FUNC_NOT_IMPLEMENTED;
  if (!t || t->op < 0 || t->op > 2 || t->M < 0 || t->N < 0 || t->K < 0 || !t->C) return OSQP_DATA_VALIDATION_ERROR;
  // every operand inside its buffer: the last element a routine may address, from non-negative strides and offsets (checked here, not in the kernels)
  auto fits = [](long long off, long long r, long long sr, long long c, long long sc, long long len) {
    if (off < 0 || sr < 0 || sc < 0 || len < 0) return false;
    if (r == 0 || c == 0) return off <= len;
    return off + (r - 1) * sr + (c - 1) * sc < len;
  };
  const bool square = t->op != 0;
  if (square && (t->cs_i < t->N || !fits(t->c_off, t->N, t->cs_i, t->N, 1, t->c_len))) return OSQP_DATA_VALIDATION_ERROR;
  if (!square && !fits(t->c_off, t->M, t->cs_i, t->N, t->cs_j, t->c_len)) return OSQP_DATA_VALIDATION_ERROR;
  const int rows = t->op == 0 ? t->M : t->N;
  if (t->op != 2 && ((t->a_len > 0 && !t->A) || (t->b_len > 0 && !t->B) || !fits(t->a_off, rows, t->as_i, t->K, t->as_k, t->a_len) || !fits(t->b_off, t->K, t->bs_k, t->N, t->bs_j, t->b_len)))
    return OSQP_DATA_VALIDATION_ERROR;
  be::activate(d_);
  struct Buf { Dev &d; double *p; ~Buf() { if (p) be::dfree(d, p); } };      // (the routine may throw: an operand without a unit stride)
  const size_t na = t->op != 2 ? (size_t)t->a_len : 0, nb = t->op != 2 ? (size_t)t->b_len : 0, nc = (size_t)t->c_len;
  Buf a{d_, dev_vec<double>(d_, na)}, b{d_, dev_vec<double>(d_, nb)}, c{d_, dev_vec<double>(d_, nc)};
  be::h2d(d_, a.p, t->A, sizeof(double) * na);
  be::h2d(d_, b.p, t->B, sizeof(double) * nb);
  be::h2d(d_, c.p, t->C, sizeof(double) * nc);
  const be::DenseProbe p{t->op, t->M, t->N, t->K, t->alpha, t->beta, (long)t->as_i, (long)t->as_k, (long)t->bs_k, (long)t->bs_j, (long)t->cs_i, (long)t->cs_j,
                         a.p + t->a_off, b.p + t->b_off, c.p + t->c_off};
  t->minpiv = be::test_dense(d_, p);
  be::d2h(d_, t->C, c.p, sizeof(double) * nc);
  return OSQP_NO_ERROR;
}
int Engine::test_band(OSQPHipBandTest *t) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!be::test_band) return OSQP_FUNC_NOT_IMPLEMENTED;
  // everything the kernel indexes with is checked here: the kernel itself checks nothing
  if (!t || t->n < 1 || t->bw < 0 || t->bw > kBatchDirectMaxBw || t->bw > t->n - 1 || t->nrhs < 0 || t->nrhs > 8) return OSQP_DATA_VALIDATION_ERROR;
  if (!(t->threads == 64 || t->threads == 256) || !(t->guard == 0 || t->guard == 1) || (t->threads == 64 && t->guard == 1)) return OSQP_DATA_VALIDATION_ERROR;
  if (!be::test_band_lds_bytes(t->n, t->bw)) return OSQP_DATA_VALIDATION_ERROR;                 // (also bounds n: every length below fits an int)
  const int n = t->n, bw = t->bw, nrhs = t->nrhs;
  const size_t nband = (size_t)n * (bw + 1), nx = (size_t)nrhs * n + 16, nimg = band_doubles(n, bw);
  if (t->band_len != (long long)nband || t->perm_len != n || t->rhs_len != (long long)nrhs * n || t->x_len != (long long)nx || t->image_len != (long long)nimg || t->dinv_len != n)
    return OSQP_DATA_VALIDATION_ERROR;
  if (!t->band || !t->perm || (nrhs > 0 && !t->rhs) || !t->x || !t->image || !t->dinv) return OSQP_DATA_VALIDATION_ERROR;
  std::vector<char> seen(n, 0);
  for (int k = 0; k < n; k++) {
    const int v = t->perm[k];
    if (v < 0 || v >= n || seen[v]) return OSQP_DATA_VALIDATION_ERROR;
    seen[v] = 1;
  }
  be::activate(d_);
  const std::vector<int> tri = band_tri_pairs(bw);
  struct Buf { Dev &d; void *p; ~Buf() { if (p) be::dfree(d, p); } };
  Buf band{d_, dev_vec<double>(d_, nband)}, perm{d_, dev_vec<int>(d_, n)}, dtri{d_, dev_vec<int>(d_, tri.size())}, rhs{d_, dev_vec<double>(d_, (size_t)nrhs * n)};
  Buf x{d_, dev_vec<double>(d_, nx)}, image{d_, dev_vec<double>(d_, nimg)}, dinv{d_, dev_vec<double>(d_, n)}, bad{d_, dev_vec<int>(d_, 1)};
  be::h2d(d_, band.p, t->band, sizeof(double) * nband);
  be::h2d(d_, perm.p, t->perm, sizeof(int) * n);
  if (!tri.empty()) be::h2d(d_, dtri.p, tri.data(), sizeof(int) * tri.size());
  if (nrhs > 0) be::h2d(d_, rhs.p, t->rhs, sizeof(double) * nrhs * n);
  be::h2d(d_, x.p, t->x, sizeof(double) * nx);
  const be::BandProbe p{n, bw, t->threads, t->guard, nrhs, (int)tri.size(), t->pivot_floor, static_cast<const double *>(band.p), static_cast<const int *>(perm.p),
                        static_cast<const int *>(dtri.p), static_cast<const double *>(rhs.p), static_cast<double *>(x.p), static_cast<double *>(image.p),
                        static_cast<double *>(dinv.p), static_cast<int *>(bad.p)};
  const int st = be::test_band(d_, p);
  if (st != OSQP_NO_ERROR) return st;
  int hbad = 0;
  be::d2h(d_, t->x, x.p, sizeof(double) * nx);
  be::d2h(d_, t->image, image.p, sizeof(double) * nimg);
  be::d2h(d_, t->dinv, dinv.p, sizeof(double) * n);
  be::d2h(d_, &hbad, bad.p, sizeof(int));
  t->bad = hbad;
  return OSQP_NO_ERROR;
}
int Engine::test_woodbury(OSQPHipWoodburyTest *t) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!be::test_woodbury || !d_.wb.on) return OSQP_FUNC_NOT_IMPLEMENTED;
  // every length is checked here: the backend copies exactly these counts
  if (!t || !(t->parity == 0 || t->parity == 1) || !(t->direct == 0 || t->direct == 1)) return OSQP_DATA_VALIDATION_ERROR;
  const DevWb &w = d_.wb;
  const long long nn = n, mm = m, ord = w.dual ? w.cd : w.r, tail = 16;
  if (t->r_len != nn || t->x0_len != (t->direct ? nn : 0) || t->u_len != nn + tail || t->xs_len != nn + tail || t->dinv0_len != nn + tail ||
      t->s_len != ord * ord + tail || t->sinv_len != ord * ord + tail || t->rho_len != mm + tail || t->idx_len != ord + tail)
    return OSQP_DATA_VALIDATION_ERROR;
  if (!t->r || (t->direct && !t->x0) || !t->u || !t->xs || !t->dinv0 || !t->S || !t->Sinv || !t->rho || !t->idx) return OSQP_DATA_VALIDATION_ERROR;
  be::activate(d_);
  std::vector<double> hr(n), hx0(t->direct ? n : 0), hu(n), hxs(n), hd(n), hrho(m);
  for (int j = 0; j < n; j++) { const int c = reordered_ ? pc_[j] : j; hr[j] = t->r[c]; if (t->direct) hx0[j] = t->x0[c]; }
  std::vector<int> hidx((size_t)ord);
  be::d2h(d_, hidx.data(), w.dual ? w.dcol : w.rows, sizeof(int) * (size_t)ord);
  be::WbProbe p{t->refactor != 0, t->parity, t->direct, hr.data(), hx0.data(), hu.data(), hxs.data(), hd.data(), t->S, t->Sinv, hrho.data(), 0, {0, 0}, 0, 0, 0.0, 0.0};
  const int st = be::test_woodbury(d_, p);
  if (st != OSQP_NO_ERROR) return st;
  for (int j = 0; j < n; j++) { const int c = reordered_ ? pc_[j] : j; t->u[c] = hu[j]; t->xs[c] = hxs[j]; t->dinv0[c] = hd[j]; }
  for (int i = 0; i < m; i++) t->rho[reordered_ ? pr_[i] : i] = hrho[i];
  for (long long k = 0; k < ord; k++) t->idx[k] = reordered_ ? (w.dual ? pc_[hidx[k]] : pr_[hidx[k]]) : hidx[k];
  t->form = w.dual ? 2 : (w.large ? 1 : 0); t->order = (int)ord; t->rows = w.r; t->exact = p.exact; t->info[0] = p.info[0]; t->info[1] = p.info[1];
  t->done = p.done; t->iters = p.iters; t->gamma = p.gamma; t->rnorm = p.rnorm;
  return OSQP_NO_ERROR;
}
// Dense KKT mode (include/osqp_hip.h osqp_hip_dense_kkt; backend.h DevDk; densekkt_hip.hip).  A handle the mode declines is left exactly as it was.
static_assert(OSQP_HIP_DENSE_KKT_MAX_N == kDkMaxN, "include/osqp_hip.h states the mode's size cap");
int Engine::dense_kkt(int on) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!(on == 0 || on == 1)) return OSQP_DATA_VALIDATION_ERROR;
  if (!on) {
    if (!d_.dk.on) return OSQP_NO_ERROR;
    be::activate(d_);
    be::ext_wait(d_); be::sync(d_); drop_graphs();        // (captured launches hold the inverse's address)
    be::dk_release(d_);
    dk_solve_nfac_ = 0; dk_solve_ms_ = 0;
    return OSQP_NO_ERROR;
  }
  if (!be::dk_enable || !be::dk_release || !be::dk_factor || !be::dk_apply) return OSQP_FUNC_NOT_IMPLEMENTED;      // the host simulator
  if (d_.wb.on || !be::device_assembly() || !d_.Araw || !ls_rho_.empty()) return OSQP_FUNC_NOT_IMPLEMENTED;        // Woodbury handles have their own direct modes
  if (m == 0 || n > kDkMaxN || (long long)m * n > kDkMaxW) return OSQP_FUNC_NOT_IMPLEMENTED;
  if (d_.dk.on) return OSQP_NO_ERROR;
  be::activate(d_);
  be::ext_wait(d_); be::sync(d_); drop_graphs();
  const int err = be::dk_enable(d_);
  if (err != OSQP_NO_ERROR) return err;
  try { be::dk_factor(d_); }
  catch (...) { be::dk_release(d_); throw; }
  dk_solve_nfac_ = 0; dk_solve_ms_ = 0;
  return OSQP_NO_ERROR;
}
int Engine::dense_kkt_last_record(double *rec) const {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!rec) return OSQP_DATA_VALIDATION_ERROR;
  const DevDk &k = d_.dk;
  const double r[OSQP_HIP_DENSE_KKT_REC] = {(double)(k.on ? k.state : 0), (double)(k.on ? n : 0), (double)dk_solve_nfac_, dk_solve_ms_, k.probe, k.minpiv, k.bytes, (double)k.nfac};
  std::copy(r, r + OSQP_HIP_DENSE_KKT_REC, rec);
  return OSQP_NO_ERROR;
}
// The mode's diagnostic entry: every length and pointer is checked here (the backend copies exactly n, m, n^2 values); host code that only checks and copies.
int Engine::test_dense_kkt(OSQPHipDenseKktTest *t) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!be::test_dense_kkt || !d_.dk.on) return OSQP_FUNC_NOT_IMPLEMENTED;
  if (!t || t->op < OSQP_HIP_DK_FORM || t->op > OSQP_HIP_DK_PROBE) return OSQP_DATA_VALIDATION_ERROR;
  const long long nn = n, mm = m, tail = 16;
  const bool form = t->op == OSQP_HIP_DK_FORM, apply = t->op == OSQP_HIP_DK_APPLY;
  if (t->k_len != (form ? nn * nn + tail : 0) || t->rho_len != (form ? mm + tail : 0) || t->r_len != (apply ? nn : 0) || t->xg_len != (apply ? nn : 0) ||
      t->xs_len != (apply ? nn + tail : 0) || t->u_len != (apply ? nn + tail : 0)) return OSQP_DATA_VALIDATION_ERROR;
  if ((form && (!t->K || !t->rho)) || (apply && (!t->r || !t->xg || !t->xs || !t->u))) return OSQP_DATA_VALIDATION_ERROR;
  if (apply && d_.dk.state != 1) return OSQP_FUNC_NOT_IMPLEMENTED;      // (no accepted inverse to apply)
  be::activate(d_);
  be::ext_wait(d_);
  be::DkProbe p{t->op, t->r, t->xg, t->K, t->rho, t->xs, t->u, 0, 0, 0, 0.0, 0.0};
  const int st = be::test_dense_kkt(d_, p);
  if (st != OSQP_NO_ERROR) return st;
  t->state = p.state; t->order = n; t->done = p.done; t->iters = p.iters; t->probe = p.probe; t->minpiv = p.minpiv;
  return OSQP_NO_ERROR;
}
// What both lockstep diagnostic entries stage a caller's array with: a device copy for the duration of the call (nullptr: the array is absent), freed on
// every way out.
namespace {
struct LsStaged { Dev &d; double *p; ~LsStaged() { if (p) be::dfree(d, p); } };
double *ls_stage(Dev &d, const double *src, long long len) {
  if (!src) return nullptr;
  double *dst = dev_vec<double>(d, (size_t)len);
  be::h2d(d, dst, src, sizeof(double) * (size_t)len);
  return dst;
}
}  // namespace
// Single launches of the lockstep kernels on the caller's blocks (include/osqp_hip.h osqp_hip_test_lockstep).  The sizes first, then EVERY check, then the
// parameters as run_lockstep_solve builds them, the staging of the caller's arrays, the blocks up, be::test_lockstep, the blocks down.
int Engine::test_lockstep(OSQPHipLockstepTest *t) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!t) return OSQP_DATA_VALIDATION_ERROR;
  const long long nn = n, mm = m, nnzA = d_.A.nnz, nnzB = d_.B.nnz, nzP = d_.nzP, nzA = d_.nzA;
  t->n = n; t->m = m; t->nnzA = d_.A.nnz; t->nnzB = d_.B.nnz; t->nzP = d_.nzP; t->nzA = d_.nzA; t->G = lockstep_grid(n, m);
  t->ws_need = (long long)lockstep_ws_doubles(n, m); t->mat_need = (long long)lockstep_mat_ws_doubles(n, m, d_.A.nnz, d_.B.nnz);
  t->r = t->GC = t->cb = t->nv = 0; t->dws_need = t->dmat_need = 0;
  if (!be::test_lockstep) return OSQP_FUNC_NOT_IMPLEMENTED;
  // the direct route's sizes, where it takes the handle: the view is built as its first solve builds it (host work and uploads, no launch)
  const bool dapplies = lockstep_direct_applies() && prepare_lockstep_direct_view() == OSQP_NO_ERROR;
  const long long rr = dapplies ? d_.wb.r : 0, nv = dapplies ? lsd_nv_ : 0;
  if (dapplies) {
    t->r = d_.wb.r; t->GC = lockstep_direct_colblocks(n); t->cb = lockstep_direct_colblock(n); t->nv = lsd_nv_;
    t->dws_need = (long long)lockstep_direct_ws_doubles(n, m, d_.wb.r); t->dmat_need = (long long)lockstep_direct_mat_ws_doubles(n, m, d_.wb.r, d_.A.nnz, d_.B.nnz, lsd_nv_);
  }
  const bool direct = t->route == 1;
  const long long need = direct ? t->dws_need : t->ws_need, mneed = direct ? t->dmat_need : t->mat_need;
  // ---- every check
  if (!(t->route == 0 || t->route == 1) || !(t->mat == 0 || t->mat == 1) || !(t->warm == 0 || t->warm == 1)) return OSQP_DATA_VALIDATION_ERROR;
  if (t->count < 1 || t->count > kLsW || t->nops < 1 || t->nops > 64 || !t->ops) return OSQP_DATA_VALIDATION_ERROR;
  const bool mat = t->mat != 0;
  if (direct && !dapplies) return OSQP_FUNC_NOT_IMPLEMENTED;                    // (the direct route's lengths exist only where it takes the handle)
  for (int k = 0; k < t->nops; k++) {
    const int op = t->ops[k];
    if (op < 0 || op >= OSQP_HIP_LS_OP_COUNT) return OSQP_DATA_VALIDATION_ERROR;
    const bool mat_op = (op >= OSQP_HIP_LS_BEGIN && op <= OSQP_HIP_LS_FINISH) || op == OSQP_HIP_LS_VALS || op == OSQP_HIP_LS_WT;
    if (mat_op && !mat) return OSQP_DATA_VALIDATION_ERROR;
    if (!direct && op >= OSQP_HIP_LS_D0 && op != OSQP_HIP_LS_SUPP) return OSQP_DATA_VALIDATION_ERROR;
    // the direct route has no PCG (and no Kp): of the PCG route's kernels it launches the transposes, the state, rhs, upd, the residuals, initz and setrho
    const bool pcg_only = op == OSQP_HIP_LS_MINV || op == OSQP_HIP_LS_T || op == OSQP_HIP_LS_KP || op == OSQP_HIP_LS_CGUPD || op == OSQP_HIP_LS_CGP ||
                          op == OSQP_HIP_LS_CGINIT || op == OSQP_HIP_LS_CGALPHA || op == OSQP_HIP_LS_CGBETA;
    if (direct && pcg_only) return OSQP_DATA_VALIDATION_ERROR;
    if ((op == OSQP_HIP_LS_ASM_A && nzA == 0) || (op == OSQP_HIP_LS_ASM_P && nzP == 0)) return OSQP_DATA_VALIDATION_ERROR;
    const bool m_only = op == OSQP_HIP_LS_LOAD_M || op == OSQP_HIP_LS_STORE_M || op == OSQP_HIP_LS_INITZ || op == OSQP_HIP_LS_T || op == OSQP_HIP_LS_RESM || op == OSQP_HIP_LS_SETRHO || op == OSQP_HIP_LS_SUPP;
    if (m_only && m == 0) return OSQP_DATA_VALIDATION_ERROR;
  }
  const long long cnt = t->count;
  // an optional array: absent (NULL, length 0) or there with exactly `len`; a required one: there with exactly `len` (an empty one may be NULL)
  auto optional = [](const void *p, long long have, long long len) { return p ? have == len : have == 0; };
  auto required = [](const void *p, long long have, long long len) { return have == len && (p || len == 0); };
  if (!optional(t->q, t->q_len, cnt * nn) || !optional(t->l, t->l_len, cnt * mm) || !optional(t->u, t->u_len, cnt * mm)) return OSQP_DATA_VALIDATION_ERROR;
  if (!required(t->x, t->x_len, cnt * nn) || !required(t->y, t->y_len, cnt * mm) || !required(t->rec, t->rec_len, cnt * kBatchRec)) return OSQP_DATA_VALIDATION_ERROR;
  if (!optional(t->Px, t->px_len, mat ? cnt * nzP : 0) || !optional(t->Ax, t->ax_len, mat ? cnt * nzA : 0)) return OSQP_DATA_VALIDATION_ERROR;
  if (!required(t->ws, t->ws_len, need) || !t->ws) return OSQP_DATA_VALIDATION_ERROR;
  if (mat ? (!t->mat_ws || t->mat_len != mneed) : (t->mat_ws || t->mat_len != 0)) return OSQP_DATA_VALIDATION_ERROR;
  // the handle's arrays: a group is wanted as a whole or not at all
  auto group = [](long long have, long long len, std::initializer_list<const void *> ptrs) {
    bool any = false, all = true;
    for (const void *p : ptrs) { any = any || p; all = all && p; }
    return have == 0 ? (len == 0 || !any) : (have == len && all);      // (an array that is empty on this handle -- m = 0 -- may have any pointer)
  };
  if (!group(t->arp_len, mm + 1, {t->A_rowptr}) || !group(t->anz_len, nnzA, {t->A_col, t->A_val}) || !group(t->brp_len, nn + 1, {t->B_rowptr}) ||
      !group(t->bnz_len, nnzB, {t->B_col, t->B_val}) || !group(t->n_len, nn, {t->D, t->Dinv}) || !group(t->m_len, mm, {t->E, t->Einv}) ||
      !group(t->pmap_len, nzP, {t->Pm1, t->Pm2, t->pvmap, t->Praw}) || !group(t->amap_len, nzA, {t->AmA, t->AmB, t->avmap, t->Araw}) || !group(t->bdiag_len, nn, {t->Bdiag}))
    return OSQP_DATA_VALIDATION_ERROR;
  if ((t->pmap_len || t->amap_len || t->bdiag_len) && !(d_.Praw && d_.Araw && d_.Bdiag)) return OSQP_DATA_VALIDATION_ERROR;      // (a backend without device assembly keeps no maps)
  // the direct route's view: with route 1 only (the lengths are then known: the route takes the handle, or the call is declined below with nothing written)
  const bool view_wanted = t->avrp_len || t->av_len || t->wt_len || t->rows_len || t->islong_len || t->Av_rowptr || t->Av_col || t->Av_val || t->vsrc || t->WT || t->wtpos || t->rows || t->islong;
  if (view_wanted && !direct) return OSQP_DATA_VALIDATION_ERROR;
  if (direct && (!group(t->avrp_len, mm + 1, {t->Av_rowptr}) || !group(t->av_len, nv, {t->Av_col, t->Av_val, t->vsrc}) || !group(t->wt_len, nn * rr, {t->WT, t->wtpos}) ||
                             !group(t->rows_len, rr, {t->rows}) || !group(t->islong_len, mm, {t->islong})))
    return OSQP_DATA_VALIDATION_ERROR;
  // ---- the route
  if (!(this->*solve_applies(direct, mat))()) return OSQP_FUNC_NOT_IMPLEMENTED;
  be::activate(d_);
  be::ext_wait(d_);
  // ---- the parameters of a chunk, as run_lockstep_solve builds them
  LsRoute &rt = lsr_[direct];
  be::LsProbe pr{};
  pr.direct = direct;
  LockstepDirectParams &p = pr.p;
  if (direct) if (const int err = fill_lockstep_direct_view(p.v, nullptr)) return err;
  if ((direct && mat) || t->wt_len) prepare_lockstep_direct_wtpos();
  if (direct && mat) { p.v.wtpos = lsd_wtpos_; p.v.vsrc = lsd_vsrc_; }
  fill_lockstep_solve(rt, p, direct, mat, t->warm, (size_t)need, (size_t)mneed);
  p.count = t->count;
  if (mat && !direct) lsm_last_count_ = 0;                                    // (the block is being overwritten)
  // ---- the caller's arrays, staged on the device for the duration of the call
  using Buf = LsStaged;
  auto stage = [&](const double *src, long long len) { return ls_stage(d_, src, len); };
  Buf bq{d_, stage(t->q, t->q_len)}, bl{d_, stage(t->l, t->l_len)}, bu{d_, stage(t->u, t->u_len)}, bx{d_, stage(t->x, t->x_len)}, by{d_, stage(t->y, t->y_len)};
  Buf brec{d_, stage(t->rec, t->rec_len)}, bPx{d_, stage(t->Px, t->px_len)}, bAx{d_, stage(t->Ax, t->ax_len)};
  Buf by0{d_, (!by.p) ? dev_vec<double>(d_, 1) : nullptr};                     // (m = 0: a solve's y is a valid pointer that no kernel follows)
  p.q = bq.p; p.l = bl.p; p.u = bu.p; p.x = bx.p; p.y = by.p ? by.p : by0.p; p.rec = brec.p; p.Px = bPx.p; p.Ax = bAx.p;
  be::h2d(d_, rt.ws, t->ws, sizeof(double) * (size_t)need);
  if (mat) be::h2d(d_, rt.mat_ws, t->mat_ws, sizeof(double) * (size_t)mneed);
  be::sync(d_);
  pr.nops = t->nops; pr.ops = t->ops;
  const int st = be::test_lockstep(d_, pr);
  if (st != OSQP_NO_ERROR) return st;
  be::d2h(d_, t->ws, rt.ws, sizeof(double) * (size_t)need);
  if (mat) be::d2h(d_, t->mat_ws, rt.mat_ws, sizeof(double) * (size_t)mneed);
  if (t->x_len) be::d2h(d_, t->x, bx.p, sizeof(double) * (size_t)t->x_len);
  if (t->y_len) be::d2h(d_, t->y, by.p, sizeof(double) * (size_t)t->y_len);
  be::d2h(d_, t->rec, brec.p, sizeof(double) * (size_t)t->rec_len);
  // ---- what the references need of the handle
  auto ints = [&](int *dst, const int *src, long long len) { if (dst && len) be::d2h(d_, dst, src, sizeof(int) * (size_t)len); };
  auto dbls = [&](double *dst, const double *src, long long len) { if (dst && len) be::d2h(d_, dst, src, sizeof(double) * (size_t)len); };
  ints(t->A_rowptr, d_.A.rowptr, t->arp_len); ints(t->A_col, d_.A.col, t->anz_len); dbls(t->A_val, d_.A.val, t->anz_len);
  ints(t->B_rowptr, d_.B.rowptr, t->brp_len); ints(t->B_col, d_.B.col, t->bnz_len); dbls(t->B_val, d_.B.val, t->bnz_len);
  dbls(t->D, d_.D, t->n_len); dbls(t->Dinv, d_.Dinv, t->n_len); dbls(t->E, d_.E, t->m_len); dbls(t->Einv, d_.Einv, t->m_len);
  ints(t->Pm1, d_.Pm1, t->pmap_len); ints(t->Pm2, d_.Pm2, t->pmap_len); dbls(t->Praw, d_.Praw, t->pmap_len);
  ints(t->AmA, d_.AmA, t->amap_len); ints(t->AmB, d_.AmB, t->amap_len); dbls(t->Araw, d_.Araw, t->amap_len);
  ints(t->Bdiag, d_.Bdiag, t->bdiag_len);
  for (long long k = 0; k < t->pmap_len; k++) t->pvmap[k] = reordered_ ? PvalMap_[k] : (int)k;
  for (long long k = 0; k < t->amap_len; k++) t->avmap[k] = reordered_ ? AvalMap_[k] : (int)k;
  t->c = c_;
  if (direct) {
    ints(t->Av_rowptr, lsd_vrp_, t->avrp_len); ints(t->Av_col, lsd_vcol_, t->av_len); dbls(t->Av_val, lsd_vval_, t->av_len); ints(t->vsrc, lsd_vsrc_, t->av_len);
    dbls(t->WT, d_.wb.WT, t->wt_len); ints(t->wtpos, lsd_wtpos_, t->wt_len); ints(t->rows, d_.wb.rows, t->rows_len);
    if (t->islong_len) {
      std::vector<unsigned char> fl((size_t)m);
      be::d2h(d_, fl.data(), d_.wb.islong, (size_t)m);
      for (int i = 0; i < m; i++) t->islong[i] = fl[i];
    }
  }
  return OSQP_NO_ERROR;
}
// The same for the kernels of the backward pass and of polish (include/osqp_hip.h osqp_hip_test_lockstep_back).  The sizes first, then EVERY check, then the
// parameters as run_lockstep_adjoint (mode 0) or a polishing run_lockstep_solve (mode 1) builds them, the staging, the blocks up, be::test_lockstep_back, the
// blocks and every staged output array down.
int Engine::test_lockstep_back(OSQPHipLockstepBackTest *t) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!t) return OSQP_DATA_VALIDATION_ERROR;
  const long long nn = n, mm = m, nzP = d_.nzP, nzA = d_.nzA;
  t->n = n; t->m = m; t->nzP = d_.nzP; t->nzA = d_.nzA; t->G = lockstep_grid(n, m); t->r = 0;
  t->ws_need = (long long)lockstep_ws_doubles(n, m); t->adj_need = (long long)lockstep_adjoint_ws_doubles(n, m);
  t->mat_need = (long long)lockstep_mat_ws_doubles(n, m, d_.A.nnz, d_.B.nnz); t->pol_need = (long long)lockstep_polish_ws_doubles(n, m);
  t->dws_need = t->dadj_need = t->dmat_need = 0;
  if (!be::test_lockstep_back) return OSQP_FUNC_NOT_IMPLEMENTED;
  const bool dapplies = lockstep_direct_applies() && prepare_lockstep_direct_view() == OSQP_NO_ERROR;
  if (dapplies) {
    t->r = d_.wb.r; t->dws_need = (long long)lockstep_direct_ws_doubles(n, m, d_.wb.r); t->dadj_need = (long long)lockstep_direct_adjoint_ws_doubles(n, m, d_.wb.r);
    t->dmat_need = (long long)lockstep_direct_mat_ws_doubles(n, m, d_.wb.r, d_.A.nnz, d_.B.nnz, lsd_nv_);
  }
  // ---- every check
  if (!(t->mode == 0 || t->mode == 1) || !(t->route == 0 || t->route == 1) || !(t->mat == 0 || t->mat == 1)) return OSQP_DATA_VALIDATION_ERROR;
  if (t->count < 1 || t->count > kLsW || t->nops < 1 || t->nops > 64 || !t->ops) return OSQP_DATA_VALIDATION_ERROR;
  const bool polish = t->mode == 1, direct = t->route == 1, mat = t->mat != 0;
  if (direct && !dapplies) return OSQP_FUNC_NOT_IMPLEMENTED;                    // (the direct route's lengths exist only where it takes the handle)
  const long long need = polish ? (direct ? t->dws_need : t->ws_need) : (direct ? t->dadj_need : t->adj_need), mneed = direct ? t->dmat_need : t->mat_need;
  for (int k = 0; k < t->nops; k++) {
    const int op = t->ops[k];
    if (op < 0 || op >= OSQP_HIP_LSB_OP_COUNT) return OSQP_DATA_VALIDATION_ERROR;
    const bool adj_op = op <= OSQP_HIP_LSB_ADJ_GRAD_A, lwa_op = op >= OSQP_HIP_LSB_LWA_SETL_X && op <= OSQP_HIP_LSB_LWA_ZERO, pol_op = op >= OSQP_HIP_LSB_POL_BEGIN;
    if ((adj_op && polish) || (pol_op && !polish) || (lwa_op && !direct)) return OSQP_DATA_VALIDATION_ERROR;
    const bool m_only = op == OSQP_HIP_LSB_ADJ_LOAD_M || op == OSQP_HIP_LSB_ADJ_CLASS || op == OSQP_HIP_LSB_ADJ_RESM || op == OSQP_HIP_LSB_ADJ_OUT_M || op == OSQP_HIP_LSB_POL_CONE;
    if (m_only && m == 0) return OSQP_DATA_VALIDATION_ERROR;
    if ((op == OSQP_HIP_LSB_ADJ_GRAD_P && (nzP == 0 || !t->dP)) || (op == OSQP_HIP_LSB_ADJ_GRAD_A && (nzA == 0 || !t->dA))) return OSQP_DATA_VALIDATION_ERROR;
    if ((op == OSQP_HIP_LSB_ADJ_OUT_N && !t->dq) || (op == OSQP_HIP_LSB_ADJ_OUT_M && !t->dl && !t->du)) return OSQP_DATA_VALIDATION_ERROR;
  }
  const long long cnt = t->count, an = polish ? 0 : cnt * nn, am = polish ? 0 : cnt * mm, pn = polish ? cnt * nn : 0, pm = polish ? cnt * mm : 0;
  auto optional = [](const void *p, long long have, long long len) { return p ? have == len : have == 0; };
  auto required = [](const void *p, long long have, long long len) { return have == len && (p || len == 0); };
  if (!required(t->sx, t->sx_len, an) || !required(t->gx, t->gx_len, an) || !required(t->sy, t->sy_len, am)) return OSQP_DATA_VALIDATION_ERROR;
  if (!optional(t->gy, t->gy_len, am) || !optional(t->l, t->l_len, am) || !optional(t->u, t->u_len, am)) return OSQP_DATA_VALIDATION_ERROR;
  if (!optional(t->dq, t->dq_len, an) || !optional(t->dl, t->dl_len, am) || !optional(t->du, t->du_len, am) || !optional(t->dP, t->dp_len, polish ? 0 : cnt * nzP) ||
      !optional(t->dA, t->da_len, polish ? 0 : cnt * nzA) || !optional(t->arec, t->arec_len, polish ? 0 : cnt * kAdjointRec))
    return OSQP_DATA_VALIDATION_ERROR;
  if (!required(t->x, t->x_len, pn) || !required(t->y, t->y_len, pm) || !required(t->rec, t->rec_len, polish ? cnt * kBatchRec : 0)) return OSQP_DATA_VALIDATION_ERROR;
  if (polish ? (!t->x || !t->rec) : (t->x || t->y || t->rec)) return OSQP_DATA_VALIDATION_ERROR;
  if (!t->ws || t->ws_len != need) return OSQP_DATA_VALIDATION_ERROR;
  if (mat ? (!t->mat_ws || t->mat_len != mneed) : (t->mat_ws || t->mat_len != 0)) return OSQP_DATA_VALIDATION_ERROR;
  if (polish ? (!t->pol_ws || t->pol_len != t->pol_need) : (t->pol_ws || t->pol_len != 0)) return OSQP_DATA_VALIDATION_ERROR;
  // ---- the route
  if (!(this->*solve_applies(direct, mat))()) return OSQP_FUNC_NOT_IMPLEMENTED;
  if (!polish && !(direct ? lockstep_direct_adjoint_applies() : lockstep_adjoint_applies())) return OSQP_FUNC_NOT_IMPLEMENTED;
  be::activate(d_);
  be::ext_wait(d_);
  // ---- the parameters of a chunk
  LsRoute &rt = lsr_[direct];
  be::LsBackProbe pr{};
  pr.polish = polish; pr.direct = direct; pr.nops = t->nops; pr.ops = t->ops; pr.secs = t->secs;
  using Buf = LsStaged;
  auto stage = [&](const double *src, long long len) { return ls_stage(d_, src, len); };
  double *block = nullptr;
  if (polish) {
    LockstepDirectParams &p = pr.p;
    if (direct) if (const int err = fill_lockstep_direct_view(p.v, nullptr)) return err;
    if (direct && mat) { prepare_lockstep_direct_wtpos(); p.v.wtpos = lsd_wtpos_; p.v.vsrc = lsd_vsrc_; }
    fill_lockstep_solve(rt, p, direct, mat, 0, (size_t)need, (size_t)mneed);
    fill_lockstep_polish(p, direct);
    p.count = t->count;
    if (mat && !direct) lsm_last_count_ = 0;                                  // (the block is being overwritten)
    block = rt.ws;
  } else {
    LockstepDirectAdjointParams &p = pr.a;
    if (direct) if (const int err = fill_lockstep_direct_view(p.v, nullptr)) return err;
    fill_lockstep_adjoint(rt, p, direct, mat, (size_t)need, (size_t)mneed);
    p.count = t->count;
    block = rt.adj_ws;
  }
  Buf bsx{d_, stage(t->sx, t->sx_len)}, bsy{d_, stage(t->sy, t->sy_len)}, bgx{d_, stage(t->gx, t->gx_len)}, bgy{d_, stage(t->gy, t->gy_len)}, bl{d_, stage(t->l, t->l_len)}, bu{d_, stage(t->u, t->u_len)};
  Buf bdq{d_, stage(t->dq, t->dq_len)}, bdl{d_, stage(t->dl, t->dl_len)}, bdu{d_, stage(t->du, t->du_len)}, bdP{d_, stage(t->dP, t->dp_len)}, bdA{d_, stage(t->dA, t->da_len)};
  Buf barec{d_, stage(t->arec, t->arec_len)}, bx{d_, stage(t->x, t->x_len)}, by{d_, stage(t->y, t->y_len)}, brec{d_, stage(t->rec, t->rec_len)};
  Buf by0{d_, (polish && !by.p) ? dev_vec<double>(d_, 1) : nullptr};            // (m = 0: a solve's y is a valid pointer that no kernel follows)
  if (polish) { pr.p.x = bx.p; pr.p.y = by.p ? by.p : by0.p; pr.p.rec = brec.p; }
  else {
    LockstepAdjointParams &p = pr.a;
    p.sx = bsx.p; p.sy = bsy.p; p.gx = bgx.p; p.gy = bgy.p; p.l = bl.p; p.u = bu.p;
    p.dq = bdq.p; p.dl = bdl.p; p.du = bdu.p; p.dP = bdP.p; p.dA = bdA.p; p.arec = barec.p;
  }
  be::h2d(d_, block, t->ws, sizeof(double) * (size_t)need);
  if (mat) be::h2d(d_, rt.mat_ws, t->mat_ws, sizeof(double) * (size_t)mneed);
  if (polish) be::h2d(d_, lspw_, t->pol_ws, sizeof(double) * (size_t)t->pol_need);
  be::sync(d_);
  const int st = be::test_lockstep_back(d_, pr);
  if (st != OSQP_NO_ERROR) return st;
  be::d2h(d_, t->ws, block, sizeof(double) * (size_t)need);
  if (mat) be::d2h(d_, t->mat_ws, rt.mat_ws, sizeof(double) * (size_t)mneed);
  if (polish) be::d2h(d_, t->pol_ws, lspw_, sizeof(double) * (size_t)t->pol_need);
  auto down = [&](double *dst, const double *src, long long len) { if (dst && src && len) be::d2h(d_, dst, src, sizeof(double) * (size_t)len); };
  down(t->dq, bdq.p, t->dq_len); down(t->dl, bdl.p, t->dl_len); down(t->du, bdu.p, t->du_len); down(t->dP, bdP.p, t->dp_len); down(t->dA, bdA.p, t->da_len);
  down(t->arec, barec.p, t->arec_len); down(t->x, bx.p, t->x_len); down(t->y, by.p, t->y_len); down(t->rec, brec.p, t->rec_len);
  // ---- the scalars the references need
  t->gain = pr.a.gain; t->min_steps = pr.a.min_steps; t->max_steps = pr.a.max_steps; t->rho0 = pr.a.rho0;
  t->pol_rho = pr.p.pol_rho; t->pol_min_steps = pr.p.pol_min_steps; t->pol_max_steps = pr.pol_max_steps; t->check_dualgap = polish ? pr.p.check_dualgap : pr.a.check_dualgap;
  t->adjoint_tol = kAdjointTol;
  return OSQP_NO_ERROR;
}
// A few ADMM iterations of the PCG path from the caller's iterates, through the handle's own launch path (include/osqp_hip.h osqp_hip_test_admm): every
// check first, then POKE (the four vectors up, the refresh of init_iterates(0), which also clears the PCG start's history), RUN (run_chunk, or run_slots with the
// pairs the chunk needs plus one spare, and ONE synchronising fetch), PEEK.  Host code over operations that exist: it runs on the host simulator too.
int Engine::test_admm(OSQPHipAdmmTest *t) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!t) return OSQP_DATA_VALIDATION_ERROR;
  if (t->iters < 1 || t->iters > 8 || t->cap < 0 || t->cap > 16) return OSQP_DATA_VALIDATION_ERROR;
  if (!std::isfinite(t->tol_rel) || !std::isfinite(t->tol_abs) || t->tol_rel < 0.0 || t->tol_abs < 0.0) return OSQP_DATA_VALIDATION_ERROR;
  if (t->n_len != (long long)n || t->m_len != (long long)m || t->hist_len != 3LL * t->cap) return OSQP_DATA_VALIDATION_ERROR;
  if (!t->x_in || !t->xt_in || !t->x || !t->xt || !t->dx || !t->xg || !t->Minv || (t->cap > 0 && !t->hist)) return OSQP_DATA_VALIDATION_ERROR;
  if (m > 0 && (!t->z_in || !t->y_in || !t->z || !t->y || !t->zt || !t->dy || !t->v || !t->t0 || !t->rho)) return OSQP_DATA_VALIDATION_ERROR;
  if (d_.wb.on) return OSQP_FUNC_NOT_IMPLEMENTED;                       // (the Woodbury correction has its own tier: osqp_hip_test_woodbury)
  be::activate(d_);
  be::ext_wait(d_);
  const int iters = t->iters, cap = t->cap;
  const size_t nb = sizeof(double) * (size_t)n, mb = sizeof(double) * (size_t)m;
  // ---- POKE
  {
    std::vector<double> hx(n), hxt(n), hz(m), hy(m);
    for (int j = 0; j < n; j++) { const int c = reordered_ ? pc_[j] : j; hx[j] = t->x_in[c]; hxt[j] = t->xt_in[c]; }
    for (int i = 0; i < m; i++) { const int r = reordered_ ? pr_[i] : i; hz[i] = t->z_in[r]; hy[i] = t->y_in[r]; }
    be::h2d(d_, d_.x, hx.data(), nb); be::h2d(d_, d_.xs, hxt.data(), nb);
    if (m > 0) { be::h2d(d_, d_.z, hz.data(), mb); be::h2d(d_, d_.y, hy.data(), mb); }
  }
  be::init_iterates(d_, 0);
  be::set_pcg_tol(d_, t->tol_rel, t->tol_abs);
  int flags[F_COUNT] = {0};
  be::fetch_flags(d_, flags);                                           // (clears the statistics an earlier chunk may have left)
  // ---- RUN
  sync_graph_scalars();
  const bool slots = slot_form();
  const double launches0 = stats_.kernel_launches;
  if (!slots) run_chunk(iters, cap);
  else run_slots(iters, (int)std::ceil(0.5 * iters * be::slot_launches(d_, cap)) + 1, cap);
  be::fetch_flags(d_, flags);
  t->launches = (int)(stats_.kernel_launches - launches0);
  t->form = !slots ? (be::pcg_fused(d_) ? 1 : 0) : (d_.f1.on ? 3 : (d_.kf.on ? 4 : 2));
  t->f1_D = d_.f1.on ? d_.f1.D : 0; t->f1_mix = d_.f1.on ? d_.f1.mix : 0;
  if (slots && be::slot_done(d_) < iters) return OSQP_ALGEBRA_LOAD_ERROR;      // the string was too short for the chunk: nothing is topped up here
  // ---- PEEK
  std::vector<double> hn(n), hm(m);
  auto peek_n = [&](double *dst, const double *src) { be::d2h(d_, hn.data(), src, nb); for (int j = 0; j < n; j++) dst[reordered_ ? pc_[j] : j] = hn[j]; };
  auto peek_m = [&](double *dst, const double *src) { if (m == 0) return; be::d2h(d_, hm.data(), src, mb); for (int i = 0; i < m; i++) dst[reordered_ ? pr_[i] : i] = hm[i]; };
  peek_n(t->x, d_.x); peek_n(t->xt, d_.xs); peek_n(t->dx, d_.dx); peek_n(t->xg, d_.xg); peek_n(t->Minv, d_.Minv);
  peek_m(t->z, d_.z); peek_m(t->y, d_.y); peek_m(t->zt, d_.zt); peek_m(t->dy, d_.dy); peek_m(t->v, d_.v); peek_m(t->t0, d_.t0); peek_m(t->rho, d_.rho);
  t->stat_sum = flags[F_STAT_SUM]; t->stat_max = flags[F_STAT_MAX]; t->stat_unconv = flags[F_STAT_UNCONV]; t->stat_n = flags[F_STAT_N];
  t->pcg_iters = flags[F_ITERS]; t->pcg_done = flags[F_DONE];
  double sc[2] = {0.0, 0.0};
  be::d2h(d_, &sc[0], d_.scal + S_TOL_NOW, sizeof(double)); be::d2h(d_, &sc[1], d_.scal + S_RN0, sizeof(double));
  t->tol_now = sc[0]; t->rn0 = sc[1];
  for (int q = 0; q < 3 && cap > 0; q++) be::d2h(d_, t->hist + (size_t)q * cap, d_.scal + S_HIST + (size_t)q * (kMaxCg + 1), sizeof(double) * (size_t)cap);
  return OSQP_NO_ERROR;
}
// The order of Dev::res (backend.h ResId) by name, for the tests' reference (include/osqp_hip.h osqp_hip_res_name)
const char *Engine::res_name(int q) {
  static const char *const names[] = {
    "R_PRI_U", "R_AX_U", "R_Z_U", "R_PRI_S", "R_AX_S", "R_Z_S", "R_DY_U", "R_DY_S", "R_PINF_LHS", "R_SUPP",
    "R_DUA_U", "R_PX_U", "R_ATY_U", "R_DUA_S", "R_PX_S", "R_ATY_S", "R_DX_U", "R_DX_S", "R_XPX", "R_QX", "R_QDX",
    "R_QN_S", "R_QN_U",
    "R_ATDY_U", "R_ATDY_S", "R_PDX_U", "R_PDX_S", "R_ADX_VIOL"};
  static_assert(sizeof(names) / sizeof(names[0]) == R_COUNT, "one name per entry of Dev::res");
  static_assert(OSQP_HIP_RES_COUNT == R_COUNT, "include/osqp_hip.h states the length of Dev::res");
  static_assert(R_PRI_U == 0 && R_SUPP == 9 && R_DUA_U == 10 && R_QDX == 20 && R_QN_U == 22 && R_ATDY_U == 23 && R_ADX_VIOL == 27, "the names follow ResId's order");
  return (q >= 0 && q < R_COUNT) ? names[q] : nullptr;
}
namespace {
OSQPHipBoundaryCtl boundary_fields(const Ctl &c) {
  OSQPHipBoundaryCtl o;
  o.status = c.status; o.osqp_status = c.osqp_status; o.need = c.need; o.stage2 = c.stage2; o.rho_flag = c.rho_flag; o.rho_updates = c.rho_updates;
  o.iter = c.iter; o.boundaries = c.boundaries; o.ch_next = c.ch_next; o.ch_at_check = c.ch_at_check; o.ch_kind = c.ch_kind; o.ch_tight = c.ch_tight;
  o.budget[0] = c.budget[0]; o.budget[1] = c.budget[1];
  o.rho_bar = c.rho_bar; o.rho_estimate = c.rho_estimate; o.tol_rel = c.tol_rel; o.tol_abs = c.tol_abs;
  o.obj_val = c.obj_val; o.prim_res = c.prim_res; o.dual_res = c.dual_res; o.dual_obj_val = c.dual_obj_val; o.duality_gap = c.duality_gap; o.rel_kkt_error = c.rel_kkt_error;
  o.inf_nd_p = c.inf_nd_p; o.inf_nd_d = c.inf_nd_d; o.inf_thr_d = c.inf_thr_d; o.inf_unscaled = c.inf_unscaled;
  return o;
}
// what ONE boundary group does to the state block, on the host: backend_hip.hip k_decide's two stages around policy.h's rules, with the residual block
// and the chunk statistics the device had
void boundary_twin_group(Ctl &c, const double *res, const int *flags) {
  if (c.status != CTL_RUNNING) return;
  if (!c.chunk_done) { c.rho_flag = 0; return; }
  c.chunk_done = 0;
  if (c.boundaries >= 0 && c.boundaries < kCtlHist) c.hist[c.boundaries] = c.seq_end - c.seq_begin;
  for (int q = 0; q < F_COUNT; q++) c.last_flags[q] = flags[q];
  int st = ctl_boundary(c, res, flags);
  if (st == CTL_RUNNING && c.stage2) st = ctl_boundary_stage2(c, res, c.last_flags);
  c.status = st;
}
}  // namespace
// The chunk boundary on the caller's vectors (include/osqp_hip.h osqp_hip_test_boundary): every check first, then POKE (seven vectors up, nothing
// refreshed), RUN (mode 0: the host-synchronous launches of a boundary; mode 1: the device-driven group, as admm_core / run_device_driven set it up and
// enqueue it), PEEK.  Mode 0 is host code over operations that exist: it runs on the host simulator too.
int Engine::test_boundary(OSQPHipBoundaryTest *t) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!t) return OSQP_DATA_VALIDATION_ERROR;
  auto bit = [](int v) { return v == 0 || v == 1; };
  if (!bit(t->mode) || !bit(t->unscaled) || !bit(t->keep) || t->need < 0 || t->need > (NEED_PINF | NEED_DINF)) return OSQP_DATA_VALIDATION_ERROR;
  if (!std::isfinite(t->thr) || t->thr < 0.0) return OSQP_DATA_VALIDATION_ERROR;
  if (t->mode == 1 && (!bit(t->at_check) || !bit(t->chunk_done) || t->groups < 1 || t->groups > 2 || t->iter < 0 || t->status_in < CTL_RUNNING || t->status_in > CTL_NEED_HOST)) return OSQP_DATA_VALIDATION_ERROR;
  if (t->n_len != (long long)n || t->m_len != (long long)m || t->res_len != (long long)R_COUNT) return OSQP_DATA_VALIDATION_ERROR;
  if (!t->x_in || !t->dx_in || !t->xt_in || !t->res || !t->xg || !t->xsp || !t->Minv) return OSQP_DATA_VALIDATION_ERROR;
  if (m > 0 && (!t->z_in || !t->y_in || !t->dy_in || !t->zt_in || !t->rho || !t->rho_inv || !t->v || !t->t0 || !t->ztg)) return OSQP_DATA_VALIDATION_ERROR;
  const bool slots = slot_form();
  if (t->mode == 1 && (!slots || !be::ctl_supported(d_) || d_.wb.on)) return OSQP_FUNC_NOT_IMPLEMENTED;
  be::activate(d_);
  be::ext_wait(d_);
  const size_t nb = sizeof(double) * (size_t)n, mb = sizeof(double) * (size_t)m;
  // ---- POKE
  {
    std::vector<double> hn(n), hm(m);
    auto poke_n = [&](double *dst, const double *src) { for (int j = 0; j < n; j++) hn[j] = src[reordered_ ? pc_[j] : j]; be::h2d(d_, dst, hn.data(), nb); };
    auto poke_m = [&](double *dst, const double *src) { if (m == 0) return; for (int i = 0; i < m; i++) hm[i] = src[reordered_ ? pr_[i] : i]; be::h2d(d_, dst, hm.data(), mb); };
    poke_n(d_.x, t->x_in); poke_n(d_.dx, t->dx_in); poke_n(d_.xs, t->xt_in);
    poke_m(d_.z, t->z_in); poke_m(d_.y, t->y_in); poke_m(d_.dy, t->dy_in); poke_m(d_.zt, t->zt_in);
  }
  // ---- RUN
  sync_graph_scalars();
  const double launches0 = stats_.kernel_launches;
  t->form = !slots ? (be::pcg_fused(d_) ? 1 : 0) : (d_.f1.on ? 3 : (d_.kf.on ? 4 : 2));
  double res[R_COUNT];
  if (t->mode == 0) {
    be::residuals(d_); stats_.kernel_launches += 3;
    if (t->need & NEED_PINF) { be::infeas_primal(d_); stats_.kernel_launches += 2; }
    if (t->need & NEED_DINF) { be::infeas_dual(d_, t->thr, t->unscaled); stats_.kernel_launches += 3; }
    be::fetch_res(d_, res);
  } else {
    Ctl &c = ctl_;
    ctl_setup();
    int flags[F_COUNT] = {0};
    be::fetch_flags(d_, flags);                                         // (clears the statistics an earlier chunk may have left)
    for (int q = 0; q < F_COUNT; q++) flags[q] = 0;
    {
      double r0[R_COUNT];
      be::residuals(d_); be::fetch_res(d_, r0);
      ctl_init_tol(c, r0);
    }
    ctl_next_chunk(c);
    c.ch_next = t->iter; c.ch_at_check = t->at_check; c.chunk_done = t->chunk_done; c.status = t->status_in; c.rho_flag = 0; c.stage2 = 0;
    Ctl twin = c;
    be::ctl_upload(d_, c);
    be::zero(d_, d_.res, sizeof(double) * R_COUNT);
    const int diagonal = settings.cg_precond == OSQP_DIAGONAL_PRECONDITIONER;
    for (int g = 0; g < t->groups; g++) run_group(diagonal);
    Ctl dn;
    be::ctl_download(d_, &dn);
    be::fetch_res(d_, res);
    for (int g = 0; g < t->groups; g++) boundary_twin_group(twin, res, flags);
    t->dev = boundary_fields(dn); t->host = boundary_fields(twin);
    c = dn;
  }
  t->launches = (int)(stats_.kernel_launches - launches0);
  // ---- PEEK
  for (int q = 0; q < R_COUNT; q++) t->res[q] = res[q];
  std::vector<double> hn(n), hm(m);
  auto peek_n = [&](double *dst, const double *src) { be::d2h(d_, hn.data(), src, nb); for (int j = 0; j < n; j++) dst[reordered_ ? pc_[j] : j] = hn[j]; };
  auto peek_m = [&](double *dst, const double *src) { if (m == 0) return; be::d2h(d_, hm.data(), src, mb); for (int i = 0; i < m; i++) dst[reordered_ ? pr_[i] : i] = hm[i]; };
  peek_n(t->xg, d_.xg); peek_n(t->xsp, d_.xsp); peek_n(t->Minv, d_.Minv);
  peek_m(t->rho, d_.rho); peek_m(t->rho_inv, d_.rho_inv); peek_m(t->v, d_.v); peek_m(t->t0, d_.t0); peek_m(t->ztg, d_.ztg);
  double sc[2] = {0.0, 0.0};
  be::d2h(d_, sc, d_.scal + S_TOL_REL, sizeof(double) * 2);
  static_assert(S_TOL_ABS == S_TOL_REL + 1, "the two tolerance scalars are read in one copy");
  t->tol_rel = sc[0]; t->tol_abs = sc[1];
  // ---- afterwards
  if (t->mode == 1) {
    if (t->keep && ctl_.rho_bar != rho_bar_) { rho_bar_ = ctl_.rho_bar; settings.rho = rho_bar_; }      // (applied on the device, as run_device_driven adopts it)
    else apply_rho(rho_bar_);
    be::sync(d_);
  }
  return OSQP_NO_ERROR;
}
int Engine::get_reordering(int *perm_cols, int *perm_rows) const {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!perm_cols || (m > 0 && !perm_rows)) return OSQP_DATA_VALIDATION_ERROR;
  for (int j = 0; j < n; j++) perm_cols[j] = reordered_ ? pc_[j] : j;
  for (int i = 0; i < m; i++) perm_rows[i] = reordered_ ? pr_[i] : i;
  return OSQP_NO_ERROR;
}
int Engine::get_scaling(double *D, double *E, double *c) {
  if (!dev_ready_) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  for (int j = 0; j < n; j++) D[reordered_ ? pc_[j] : j] = D_[j];
  for (int i = 0; i < m; i++) E[reordered_ ? pr_[i] : i] = E_[i];
  *c = c_;
  return OSQP_NO_ERROR;
}


}  // namespace osqp_hip
