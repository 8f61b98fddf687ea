// tests/hostsim/backend_host.cpp -- TEST INFRASTRUCTURE ONLY.
//
// Plain-loop implementation of the device-op interface (osqp-python_amd/csrc/backend.h).  Linked with the product's
// host driver (engine.cpp, api.cpp) into tests/_build/libosqp_hostsim.so by tests/hostsim_build.py so the driver logic
// can be exercised in CI containers that have no GPU.  The product library libosqp_hip.so links backend_hip.hip only,
// has no CPU path, and never loads this file.
#include <chrono>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../osqp-python_amd/csrc/backend.h"
#include "../../osqp-python_amd/csrc/step_rules.h"
#include "../../include/osqp_hip.h"

namespace osqp_hip {
namespace be {

namespace {
inline double *gam(Dev &d) { return d.scal + S_HIST; }
inline double *alp(Dev &d) { return d.scal + S_HIST + kMaxCg + 1; }
struct Impl { double gamma_next = 0, rnorm = 0, bnorm = 0, delta = 0; };
inline Impl &im(Dev &d) { return *static_cast<Impl *>(d.impl); }
}  // namespace

const char *name() { return "hostsim"; }
int init(Dev &d, int) { d.impl = new Impl(); return 0; }
void destroy(Dev &d) { delete static_cast<Impl *>(d.impl); d.impl = nullptr; }
void *alloc(Dev &, size_t bytes) { return std::calloc(1, bytes); }
void dfree(Dev &, void *p) { std::free(p); }
void h2d(Dev &, void *dst, const void *src, size_t b) { if (b) std::memcpy(dst, src, b); }      // (b == 0: an empty vector's data() may be null, which memcpy must not be given)
void d2h(Dev &, void *dst, const void *src, size_t b) { if (b) std::memcpy(dst, src, b); }
void zero(Dev &, void *dst, size_t b) { std::memset(dst, 0, b); }
void sync(Dev &) {}
static thread_local double g_ev[2];
void ev_mark(Dev &, int which) { g_ev[which ? 1 : 0] = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
double ev_ms(Dev &) { return 1e3 * (g_ev[1] - g_ev[0]); }
void activate(Dev &) {}
#ifdef HOSTSIM_LS_ENTRY_PROBE              // (tests/hostsim/ls_entry_probe.cpp alone: the lockstep routes take a handle whose vectors are resident, so that the host side of osqp_hip_test_lockstep reaches its backend call; the probe solves nothing)
bool device_vec_updates() { return true; }
#else
bool device_vec_updates() { return false; }
#endif
void copy_in(Dev &, void *dst, const void *src, size_t bytes, int) { if (bytes) std::memcpy(dst, src, bytes); }
void stream_wait(Dev &, void *) {}
void scale_q(Dev &, double) {}
void scale_bounds(Dev &, int) {}
int count_bad_bounds(Dev &, const double *, const double *) { return 0; }
bool wbx_supported() { return false; }
void wbx_init(Dev &) {}
void wbx_refresh(Dev &) {}
void wbx_factor(Dev &, int) {}
void wbx_slot_pair(Dev &) {}
void wbx_chunk(Dev &, int) {}
void gather(Dev &, double *dst, const double *src, const int *idx, int cnt) { for (int k = 0; k < cnt; k++) dst[k] = src[idx[k]]; }
void scale_warm(Dev &, const double *, const double *, double) {}
bool slots_supported(const Dev &) { return false; }
void slot_begin(Dev &, int, int) {}
void slot_pair(Dev &) {}
int slot_done(Dev &) { return 0; }
int slot_seq(Dev &) { return 0; }
void slot_poll(Dev &, int *seq, int *done) { *seq = 0; *done = 0; }
void f1_refresh(Dev &) {}
bool kf_supported() { return false; }
void wbf_iteration(Dev &) {}
void kf_values(Dev &, int) {}
#ifdef HOSTSIM_WB_ENTRY_PROBE              // (tests/hostsim/wb_entry_probe.cpp alone: Engine::prepare_wb builds the symbolic plan, so that the host side of osqp_hip_test_woodbury has a handle to validate against)
bool wb_supported() { return true; }
bool wb_large_supported() { return true; }
#else
bool wb_supported() { return false; }
bool wb_large_supported() { return false; }
#endif
void wb_refresh(Dev &) {}
void wb_apply(Dev &, int, int) {}
void wb_direct(Dev &) {}
bool ctl_supported(const Dev &) { return false; }
void ctl_upload(Dev &, const Ctl &) {}
void ctl_begin(Dev &) {}
void ctl_group(Dev &, int) {}
void ctl_poll(Dev &, Ctl *, int *seq, int *done) { *seq = 0; *done = 0; }
void ctl_download(Dev &, Ctl *) {}
void ext_record(Dev &, void *) {}
void ext_wait(Dev &) {}

void kb_rhs(Dev &d) {
  Impl &s = im(d);
  double g = 0, rn = 0, bn = 0;
  for (int j = 0; j < d.n; j++) {
    double sA = 0, sK = 0;
    for (int k = d.B.rowptr[j]; k < d.B.rowptr[j + 1]; k++) {
      int c = d.B.col[k]; double v = d.B.val[k];
      if (c < d.n) sK += v * d.xg[c];                       // the PCG starts from the extrapolated point (backend.h Dev::xg)
      else { sA += v * d.v[c - d.n]; sK += v * d.t0[c - d.n]; }
    }
    double rhs = d.sigma * d.x[j] - d.q[j] + sA;
    double r = rhs - sK, u = d.Minv[j] * r;
    d.r[j] = r; d.uu[j] = u;
    g += r * u; rn = nanmax(rn, std::fabs(r)); bn = nanmax(bn, std::fabs(rhs));
  }
  for (int j = 0; j < d.n; j++) d.xs[j] = d.xg[j];
  s.gamma_next = g; s.rnorm = rn; s.bnorm = bn;
  d.scal[S_RN0] = rn;
  d.flags[F_DONE] = 0; d.flags[F_ITERS] = 0;
}

void k1(Dev &d, int i) {
  if (d.flags[F_DONE]) return;
  Impl &s = im(d);
  double tol = std::max(d.scal[S_TOL_REL] * s.bnorm, d.scal[S_TOL_ABS]);
  if (i == 0) d.scal[S_TOL_NOW] = tol;                  // (as k_k1's stopping test records it)
  if (!(s.rnorm > tol)) { d.flags[F_DONE] = 1; d.flags[F_ITERS] = i; return; }
  for (int r = 0; r < d.m; r++) {
    double a = 0;
    for (int k = d.A.rowptr[r]; k < d.A.rowptr[r + 1]; k++) a += d.A.val[k] * d.uu[d.A.col[k]];
    d.t[r] = d.rho[r] * a;
  }
}

void k2(Dev &d, int) {
  if (d.flags[F_DONE]) return;
  double dl = 0;
  for (int j = 0; j < d.n; j++) {
    double a = 0;
    for (int k = d.B.rowptr[j]; k < d.B.rowptr[j + 1]; k++) { int c = d.B.col[k]; a += d.B.val[k] * (c < d.n ? d.uu[c] : d.t[c - d.n]); }
    d.w[j] = a; dl += a * d.uu[j];
  }
  im(d).delta = dl;
}

void kv(Dev &d, int i) {
  if (d.flags[F_DONE]) return;
  Impl &s = im(d);
  double gamma = s.gamma_next, delta = s.delta, alpha, beta;
  if (i == 0) { beta = 0; alpha = gamma / delta; }
  else { beta = gamma / gam(d)[i - 1]; alpha = gamma / (delta - beta * gamma / alp(d)[i - 1]); }
  gam(d)[i] = gamma; alp(d)[i] = alpha;
  double g = 0, rn = 0;
  for (int j = 0; j < d.n; j++) {
    double p = i == 0 ? d.uu[j] : d.uu[j] + beta * d.p[j];
    double sv = i == 0 ? d.w[j] : d.w[j] + beta * d.s[j];
    d.p[j] = p; d.s[j] = sv;
    d.xs[j] += alpha * p;
    double r = d.r[j] - alpha * sv, u = d.Minv[j] * r;
    d.r[j] = r; d.uu[j] = u;
    g += r * u; rn = nanmax(rn, std::fabs(r));
  }
  s.gamma_next = g; s.rnorm = rn;
}

void ka(Dev &d, int budget) {
  double theta = d.theta;
  if (!d.flags[F_DONE] && budget > 0) theta = 0.0;     // after a cut-off solve the next one starts from x~ itself (backend_hip.hip cutoff_theta)
  for (int i = 0; i < d.m; i++) {
    double zt = 0;
    for (int k = d.A.rowptr[i]; k < d.A.rowptr[i + 1]; k++) zt += d.A.val[k] * d.xs[d.A.col[k]];
    double zr = d.alpha * zt + (1.0 - d.alpha) * d.z[i];
    double zn = std::fmin(std::fmax(zr + d.rho_inv[i] * d.y[i], d.l[i]), d.u[i]);
    double dy = d.rho[i] * (zr - zn);
    const double zg = zt + theta * (zt - d.zt[i]);
    d.y[i] += dy; d.dy[i] = dy; d.z[i] = zn; d.zt[i] = zt; d.ztg[i] = zg;
    d.v[i] = d.rho[i] * zn - d.y[i]; d.t0[i] = d.rho[i] * zg;
  }
  for (int j = 0; j < d.n; j++) {
    const double xt = d.xs[j];
    double xn = d.alpha * xt + (1.0 - d.alpha) * d.x[j];
    d.dx[j] = xn - d.x[j]; d.x[j] = xn;
    d.xg[j] = xt + theta * (xt - d.xsp[j]); d.xsp[j] = xt;
  }
  int used = d.flags[F_DONE] ? d.flags[F_ITERS] : budget;
  d.flags[F_STAT_SUM] += used; d.flags[F_STAT_SUMSQ] += used * used; d.flags[F_STAT_N] += 1;
  d.flags[F_STAT_MAX] = std::max(d.flags[F_STAT_MAX], used);
  // like k_ka of the HIP backend: a PCG whose LAST budgeted update reached the tolerance is converged, not budget-limited
  bool done = d.flags[F_DONE] != 0;
  if (!done) { Impl &s = im(d); const double tol = std::max(d.scal[S_TOL_REL] * s.bnorm, d.scal[S_TOL_ABS]); done = !(s.rnorm > tol); }
  if (!done) { d.flags[F_STAT_UNCONV] += 1; if (im(d).rnorm > 0.1 * d.scal[S_RN0]) d.flags[F_STAT_STAG] += 1; }
}

void residuals(Dev &d) {
  double *R = d.res;
  for (int q = 0; q <= R_QN_U; q++) R[q] = 0;
  for (int i = 0; i < d.m; i++) {
    double ax = 0;
    for (int k = d.A.rowptr[i]; k < d.A.rowptr[i + 1]; k++) ax += d.A.val[k] * d.x[d.A.col[k]];
    double pr = ax - d.z[i], ei = d.Einv[i];
    R[R_PRI_U] = nanmax(R[R_PRI_U], std::fabs(ei * pr)); R[R_AX_U] = nanmax(R[R_AX_U], std::fabs(ei * ax)); R[R_Z_U] = nanmax(R[R_Z_U], std::fabs(ei * d.z[i]));
    R[R_PRI_S] = nanmax(R[R_PRI_S], std::fabs(pr)); R[R_AX_S] = nanmax(R[R_AX_S], std::fabs(ax)); R[R_Z_S] = nanmax(R[R_Z_S], std::fabs(d.z[i]));
    R[R_DY_U] = nanmax(R[R_DY_U], std::fabs(d.E[i] * d.dy[i])); R[R_DY_S] = nanmax(R[R_DY_S], std::fabs(d.dy[i]));
    R[R_PINF_LHS] += support_term(d.l[i], d.u[i], d.dy[i]);
    R[R_SUPP] += support_finite(d.l[i], d.u[i], d.y[i]);
  }
  for (int j = 0; j < d.n; j++) {
    double sp = 0, sa = 0;
    for (int k = d.B.rowptr[j]; k < d.B.rowptr[j + 1]; k++) { int c = d.B.col[k]; if (c < d.n) sp += d.B.val[k] * d.x[c]; else sa += d.B.val[k] * d.y[c - d.n]; }
    double px = sp - d.sigma * d.x[j], dr = px + d.q[j] + sa, di = d.Dinv[j];
    R[R_DUA_U] = nanmax(R[R_DUA_U], std::fabs(di * dr)); R[R_PX_U] = nanmax(R[R_PX_U], std::fabs(di * px)); R[R_ATY_U] = nanmax(R[R_ATY_U], std::fabs(di * sa));
    R[R_DUA_S] = nanmax(R[R_DUA_S], std::fabs(dr)); R[R_PX_S] = nanmax(R[R_PX_S], std::fabs(px)); R[R_ATY_S] = nanmax(R[R_ATY_S], std::fabs(sa));
    R[R_DX_U] = nanmax(R[R_DX_U], std::fabs(d.D[j] * d.dx[j])); R[R_DX_S] = nanmax(R[R_DX_S], std::fabs(d.dx[j]));
    R[R_XPX] += d.x[j] * px; R[R_QX] += d.q[j] * d.x[j]; R[R_QDX] += d.q[j] * d.dx[j];
    R[R_QN_S] = nanmax(R[R_QN_S], std::fabs(d.q[j])); R[R_QN_U] = nanmax(R[R_QN_U], std::fabs(di * d.q[j]));
  }
}

void infeas_primal(Dev &d) {
  double u = 0, s = 0;
  for (int j = 0; j < d.n; j++) {
    double sa = 0;
    for (int k = d.B.rowptr[j]; k < d.B.rowptr[j + 1]; k++) { int c = d.B.col[k]; if (c >= d.n) sa += d.B.val[k] * d.dy[c - d.n]; }
    u = nanmax(u, std::fabs(d.Dinv[j] * sa)); s = nanmax(s, std::fabs(sa));
  }
  d.res[R_ATDY_U] = u; d.res[R_ATDY_S] = s;
}

void infeas_dual(Dev &d, double thr, int unscaled) {
  double u = 0, s = 0, viol = 0;
  for (int j = 0; j < d.n; j++) {
    double sp = 0;
    for (int k = d.B.rowptr[j]; k < d.B.rowptr[j + 1]; k++) { int c = d.B.col[k]; if (c < d.n) sp += d.B.val[k] * d.dx[c]; }
    sp -= d.sigma * d.dx[j];
    u = nanmax(u, std::fabs(d.Dinv[j] * sp)); s = nanmax(s, std::fabs(sp));
  }
  for (int i = 0; i < d.m; i++) {
    double a = 0;
    for (int k = d.A.rowptr[i]; k < d.A.rowptr[i + 1]; k++) a += d.A.val[k] * d.dx[d.A.col[k]];
    if (unscaled) a *= d.Einv[i];
    if (adx_violates(a, d.l[i], d.u[i], thr)) viol += 1;
  }
  d.res[R_PDX_U] = u; d.res[R_PDX_S] = s; d.res[R_ADX_VIOL] = viol;
}

void fetch_res(Dev &d, double *h) { std::memcpy(h, d.res, sizeof(double) * R_COUNT); }
void fetch_flags(Dev &d, int *h) {
  std::memcpy(h, d.flags, sizeof(int) * F_COUNT);
  d.flags[F_STAT_SUM] = d.flags[F_STAT_MAX] = d.flags[F_STAT_UNCONV] = d.flags[F_STAT_SUMSQ] = d.flags[F_STAT_N] = d.flags[F_STAT_STAG] = 0;
}
void fetch_res_flags(Dev &d, double *hr, int *hf) { fetch_res(d, hr); fetch_flags(d, hf); }

void set_rho(Dev &d, double rb) {
  for (int j = 0; j < d.n; j++) { d.xg[j] = d.xs[j]; d.xsp[j] = d.xs[j]; }      // history cleared (backend_hip.hip set_rho)
  for (int i = 0; i < d.m; i++) {
    double r = row_rho(d.ctype[i], rb, d.rho_eq_factor * rb);
    d.rho[i] = r; d.rho_inv[i] = 1.0 / r;
    d.v[i] = r * d.z[i] - d.y[i]; d.ztg[i] = d.zt[i]; d.t0[i] = r * d.zt[i];
  }
}
void precond(Dev &d, int diagonal) {
  for (int j = 0; j < d.n; j++) {
    if (!diagonal) { d.Minv[j] = 1.0; continue; }
    double s = d.B.val[d.Bdiag[j]];
    for (int k = d.B.rowptr[j]; k < d.B.rowptr[j + 1]; k++) { int c = d.B.col[k]; if (c >= d.n) s += d.rho[c - d.n] * d.B.val[k] * d.B.val[k]; }
    d.Minv[j] = 1.0 / s;
  }
}
void set_pcg_tol(Dev &d, double rel, double ab) { d.scal[S_TOL_REL] = rel; d.scal[S_TOL_ABS] = ab; }

void init_iterates(Dev &d, int full) {
  if (full) for (int j = 0; j < d.n; j++) { d.xs[j] = d.x[j]; d.dx[j] = 0; }
  for (int j = 0; j < d.n; j++) { d.xg[j] = d.xs[j]; d.xsp[j] = d.xs[j]; }
  for (int i = 0; i < d.m; i++) {
    double a = 0;
    for (int k = d.A.rowptr[i]; k < d.A.rowptr[i + 1]; k++) a += d.A.val[k] * d.xs[d.A.col[k]];
    if (full == 1) { d.z[i] = a; d.dy[i] = 0; }                      // (full = 2: x~ = x, z kept)
    d.zt[i] = a; d.ztg[i] = a; d.t0[i] = d.rho[i] * a; d.v[i] = d.rho[i] * d.z[i] - d.y[i];
  }
}

void project_normalcone(Dev &d) {
  for (int i = 0; i < d.m; i++) { const ConeRow c = normal_cone(d.z[i] + d.y[i], d.l[i], d.u[i]); d.z[i] = c.z; d.y[i] = c.y; }
}

size_t batch_lds_bytes(int, int) { return 0; }
size_t batch_direct_lds_bytes(int, int, int, int) { return 0; }
bool batch_direct_selected(const BatchParams &) { return false; }
size_t batch_wave_lds_bytes(int, int, int) { return 0; }
void batch_products(Dev &, int, const int *, const int *, double *) {}
void batch_order(Dev &, int, const int *, int *, void *) {}
int batch_prepare(Dev &, const BatchParams &, const double *, const double *, int, void *) { return OSQP_FUNC_NOT_IMPLEMENTED; }
int batch_solve(Dev &, const BatchParams &, void *) { return OSQP_FUNC_NOT_IMPLEMENTED; }   // GPU-only feature

bool pcg_fused(const Dev &) { return false; }
bool graphs_supported() { return false; }
void graph_begin(Dev &) {}
void *graph_end(Dev &) { return nullptr; }
void graph_launch(Dev &, void *) {}
void graph_free(Dev &, void *) {}

bool ktrace_read(Dev &, unsigned long long *, int) { return false; }
bool device_assembly() { return false; }        // the simulator exercises the driver's host scaling path
void assemble(Dev &, int, double, int) {}
double ruiz(Dev &, int) { return 1.0; }
void test_spmv(Dev &d, int which, const double *in, double *out) {
  const DevCsr &M = which == 0 ? d.A : d.B;
  for (int r = 0; r < M.nrows; r++) { double a = 0; for (int k = M.rowptr[r]; k < M.rowptr[r + 1]; k++) a += M.val[k] * in[M.col[k]]; out[r] = a; }
}
// The dense routines as plain loops (the CPU tier drives the GPU test's canvases, masks and bounds through them: tests/test_dense_ref.py).
namespace {
void host_gemm(const DenseProbe &p, int M, double beta, long cs_i, long cs_j) {
  if (!((p.as_k == 1 || p.as_i == 1) && (p.bs_k == 1 || p.bs_j == 1))) throw DeviceError("osqp_hip: dense_gemm needs a unit stride in every operand");
  for (int i = 0; i < M; i++)
    for (int j = 0; j < p.N; j++) {
      double a = 0;
      for (int k = 0; k < p.K; k++) a += p.A[i * p.as_i + k * p.as_k] * p.B[k * p.bs_k + j * p.bs_j];
      double *c = p.C + i * cs_i + j * cs_j;
      *c = beta == 0.0 ? p.alpha * a : beta * *c + p.alpha * a;
    }
}
// block Gauss-Jordan without pivoting, 64 columns per step, on the whole matrix; the lower triangle is the mirror of the upper one at the end
double host_spd_inverse(double *A, long ld, int n) {
  constexpr int nbk = 64;
  double minpiv = 1e300;
  std::vector<double> P(nbk * nbk), R((size_t)nbk * n), Ck((size_t)n * nbk);
  for (int k0 = 0; k0 < n; k0 += nbk) {
    const int nb = std::min(nbk, n - k0);
    for (int i = 0; i < nb; i++) for (int j = 0; j < nb; j++) P[i * nbk + j] = A[(k0 + i) * ld + k0 + j];
    for (int k = 0; k < nb; k++) {                                       // P = A_kk^-1 in place
      const double piv = P[k * nbk + k], pi = 1.0 / piv;
      if (!(piv >= minpiv)) minpiv = piv;
      for (int j = 0; j < nb; j++) P[k * nbk + j] = (j == k) ? pi : P[k * nbk + j] * pi;
      for (int i = 0; i < nb; i++) {
        if (i == k) continue;
        const double c = P[i * nbk + k];
        for (int j = 0; j < nb; j++) P[i * nbk + j] = (j == k) ? -c * pi : P[i * nbk + j] - c * P[k * nbk + j];
      }
    }
    if (nb < nbk && !(1.0 >= minpiv)) minpiv = 1.0;                      // (the kernel pads a partial block with the identity: pivots 1)
    auto inblk = [&](int j) { return j >= k0 && j < k0 + nb; };
    for (int i = 0; i < n; i++) for (int c = 0; c < nb; c++) Ck[(size_t)i * nbk + c] = inblk(i) ? 0.0 : A[i * ld + k0 + c];
    for (int i = 0; i < nb; i++)                                         // R = P A_k:  (block k's own columns: zero)
      for (int j = 0; j < n; j++) {
        double a = 0;
        if (!inblk(j)) for (int c = 0; c < nb; c++) a += P[i * nbk + c] * A[(k0 + c) * ld + j];
        R[(size_t)i * n + j] = a;
      }
    for (int i = 0; i < n; i++) {
      if (inblk(i)) continue;
      for (int j = 0; j < n; j++) {                                      // A_ij -= A_ik R_j
        if (inblk(j)) continue;
        double a = 0;
        for (int c = 0; c < nb; c++) a += Ck[(size_t)i * nbk + c] * R[(size_t)c * n + j];
        A[i * ld + j] -= a;
      }
      for (int j = 0; j < nb; j++) {                                     // A_ik = -A_ik P
        double a = 0;
        for (int c = 0; c < nb; c++) a += Ck[(size_t)i * nbk + c] * P[c * nbk + j];
        A[i * ld + k0 + j] = -a;
      }
    }
    for (int i = 0; i < nb; i++) for (int j = 0; j < n; j++) A[(k0 + i) * ld + j] = inblk(j) ? P[i * nbk + (j - k0)] : R[(size_t)i * n + j];
  }
  for (int i = 0; i < n; i++) for (int j = 0; j < i; j++) A[i * ld + j] = A[j * ld + i];
  return minpiv;
}
}  // namespace
double test_dense(Dev &, const DenseProbe &p) {
  if (p.op == 0) { host_gemm(p, p.M, p.beta, p.cs_i, p.cs_j); return 0.0; }
  if (p.op == 1) {
    host_gemm(p, p.N, 0.0, p.cs_i, 1);
    for (int i = 0; i < p.N; i++) for (int j = 0; j < i; j++) p.C[i * p.cs_i + j] = p.C[j * p.cs_i + i];
    return 0.0;
  }
  return p.N > 0 ? host_spd_inverse(p.C, p.cs_i, p.N) : 0.0;
}
// The band of band_ldl.h as textbook loops on a dense lower triangle (the CPU tier drives the GPU test's cases, bounds and checks through them:
// tests/test_band_ref.py): K = L^ D L^' row by row, the pivot rule of band_factor's GUARD, two substitutions, and the outputs in the kernel's layout --
// L^ strictly lower at band_slot(), zeros everywhere else in the image, 1 / D.
int test_band(Dev &, const BandProbe &p) {
  const int n = p.n, bw = p.bw;
  std::vector<double> L((size_t)n * n, 0.0), D(n);
  bool bad = false;
  for (int c = 0; c < n; c++) {
    double pv = p.band[(size_t)c * (bw + 1)];
    for (int j = std::max(0, c - bw); j < c; j++) pv -= L[(size_t)c * n + j] * L[(size_t)c * n + j] * D[j];
    if (p.guard && (!(pv > 0.0) || pv > 1e300)) { bad = true; pv = (std::fabs(pv) > p.pivot_floor && std::fabs(pv) <= 1e300) ? std::fabs(pv) : 1.0; }
    D[c] = pv;
    for (int r = c + 1; r <= std::min(n - 1, c + bw); r++) {
      double v = p.band[(size_t)c * (bw + 1) + (r - c)];
      for (int j = std::max(0, r - bw); j < c; j++) v -= L[(size_t)r * n + j] * L[(size_t)c * n + j] * D[j];
      L[(size_t)r * n + c] = v / pv;
    }
  }
  const size_t nimg = band_doubles(n, bw);
  for (size_t s = 0; s < nimg; s++) p.image[s] = 0.0;
  for (int c = 0; c < n; c++) {
    p.dinv[c] = 1.0 / D[c];
    for (int r = c + 1; r <= std::min(n - 1, c + bw); r++) p.image[kBandFront + band_slot(bw, c, r)] = L[(size_t)r * n + c];
  }
  std::vector<double> v(n);
  for (int s = 0; s < p.nrhs; s++) {
    const double *rhs = p.rhs + (size_t)s * n;
    double *out = p.x + (size_t)s * n;
    for (int k = 0; k < n; k++) {
      double a = rhs[p.perm[k]];
      for (int j = std::max(0, k - bw); j < k; j++) a -= L[(size_t)k * n + j] * v[j];
      v[k] = a;
    }
    for (int k = 0; k < n; k++) v[k] /= D[k];
    for (int k = n - 1; k >= 0; k--) {
      double a = v[k];
      for (int j = k + 1; j <= std::min(n - 1, k + bw); j++) a -= L[(size_t)j * n + k] * v[j];
      v[k] = a;
    }
    for (int k = 0; k < n; k++) out[p.perm[k]] = v[k];
  }
  *p.bad = bad ? 1 : 0;
  return OSQP_NO_ERROR;
}
float time_kernel(Dev &, int, int) { return 0.f; }

}  // namespace be
}  // namespace osqp_hip
