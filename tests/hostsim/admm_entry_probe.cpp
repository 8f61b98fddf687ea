// tests/hostsim/admm_entry_probe.cpp -- TEST INFRASTRUCTURE ONLY.  Stand-alone program (own main) for the HOST side of osqp_hip_test_admm: the validation
// of Engine::test_admm, its copies between the caller's canvases and the engine's numbering (a reordered handle included) and the run itself on the host
// simulator, under the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o admm_entry_probe
//       tests/hostsim/admm_entry_probe.cpp tests/hostsim/backend_host.cpp osqp-python_amd/csrc/{engine,engine_setup,engine_api,api}.cpp && ./admm_entry_probe
// Every canvas is a heap block of exactly the listed length, so a copy one past it is a sanitizer report; every rejected call must leave all canvases as
// they were.  Prints what it checked and returns 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "../../include/osqp_hip.h"

namespace {
int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

struct Csc { std::vector<OSQPInt> p, i; std::vector<OSQPFloat> x; OSQPCscMatrix m; };
void finish(Csc &c, int rows, int cols) { c.m = OSQPCscMatrix{rows, cols, c.p.data(), c.i.data(), c.x.data(), (OSQPInt)c.x.size(), -1}; }
// P tridiagonal (upper triangle stored), A: m rows of three entries in a band that wraps; bounds of all three classes
OSQPSolver *make(int n, int m, int reorder) {
  Csc P, A;
  P.p.push_back(0);
  for (int j = 0; j < n; j++) {
    if (j > 0) { P.i.push_back(j - 1); P.x.push_back(-0.1); }
    P.i.push_back(j); P.x.push_back(1.0 + 0.01 * j);
    P.p.push_back((OSQPInt)P.i.size());
  }
  finish(P, n, n);
  std::vector<std::vector<std::pair<int, double>>> cols(n);
  for (int i = 0; i < m; i++)
    for (int k = 0; k < 3; k++) cols[(i * 5 + k * 7) % n].push_back({i, 0.3 + 0.01 * ((i * 13 + k * 29) % 41) - 0.2 * k});
  A.p.push_back(0);
  for (int j = 0; j < n; j++) { for (auto &e : cols[j]) { A.i.push_back(e.first); A.x.push_back(e.second); } A.p.push_back((OSQPInt)A.i.size()); }
  finish(A, m, n);
  std::vector<OSQPFloat> q(n), l(m), u(m);
  for (int j = 0; j < n; j++) q[j] = 0.5 - 0.03 * j;
  for (int i = 0; i < m; i++) { l[i] = -0.4 - 0.01 * i; u[i] = i % 5 == 1 ? l[i] : 0.3 + 0.02 * i; if (i % 7 == 2) { l[i] = -OSQP_INFTY; u[i] = OSQP_INFTY; } }
  OSQPSettings st; osqp_set_default_settings(&st); st.verbose = 0; st.warm_starting = 0;
  OSQPHipPolicy pol; osqp_hip_default_policy(&pol); pol.reorder = reorder; pol.small_direct = 0;
  osqp_hip_set_default_policy(&pol);
  OSQPSolver *s = nullptr;
  const OSQPInt rc = osqp_setup(&s, &P.m, q.data(), &A.m, l.data(), u.data(), m, n, &st);
  osqp_hip_set_default_policy(nullptr);
  if (rc != 0) { std::printf("setup failed: %d\n", (int)rc); std::exit(2); }
  return s;
}
constexpr int kOut = 13;      // x z y xt zt dx dy v t0 xg rho Minv hist
struct Canvas {
  long long n, m, cap;
  double *in[4], *out[kOut];
  static double *mk(long long c, double v) { double *p = (double *)std::malloc(sizeof(double) * (size_t)(c > 0 ? c : 1)); for (long long k = 0; k < c; k++) p[k] = v; return p; }
  long long len(int k) const { static const int isn[kOut] = {1, 0, 0, 1, 0, 1, 0, 0, 0, 1, 0, 1, -1}; return isn[k] < 0 ? 3 * cap : (isn[k] ? n : m); }
  Canvas(long long n_, long long m_, long long cap_) : n(n_), m(m_), cap(cap_) {
    const long long il[4] = {n, m, m, n};
    for (int k = 0; k < 4; k++) { in[k] = mk(il[k], 0.0); for (long long j = 0; j < il[k]; j++) in[k][j] = std::sin(1.0 + 0.37 * j + k); }
    for (int k = 0; k < kOut; k++) out[k] = mk(len(k), -7.0);
  }
  ~Canvas() { for (auto p : in) std::free(p); for (auto p : out) std::free(p); }
  bool untouched() const { for (int k = 0; k < kOut; k++) for (long long j = 0; j < len(k); j++) if (out[k][j] != -7.0) return false; return true; }
  bool written() const { for (int k = 0; k < kOut - 1; k++) for (long long j = 0; j < len(k); j++) if (!std::isfinite(out[k][j]) || out[k][j] == -7.0) return false; return true; }
  OSQPHipAdmmTest fill(int iters, double tol_abs = 0.0) const {
    OSQPHipAdmmTest t;
    std::memset(&t, 0, sizeof(t));
    t.iters = iters; t.cap = (OSQPInt)cap; t.tol_rel = 0.0; t.tol_abs = tol_abs; t.n_len = n; t.m_len = m; t.hist_len = 3 * cap;
    t.x_in = in[0]; t.z_in = m ? in[1] : nullptr; t.y_in = m ? in[2] : nullptr; t.xt_in = in[3];
    OSQPFloat **o[kOut] = {&t.x, &t.z, &t.y, &t.xt, &t.zt, &t.dx, &t.dy, &t.v, &t.t0, &t.xg, &t.rho, &t.Minv, &t.hist};
    for (int k = 0; k < kOut; k++) *o[k] = len(k) ? out[k] : nullptr;
    return t;
  }
};
}  // namespace

int main() {
  const int n = 37, m = 61;
  OSQPSolver *s = make(n, m, 0);
  {                                                  // valid runs: every cap edge, the statistics of a run at tolerance 0
    for (int cap : {0, 1, 3, 16}) {
      Canvas c(n, m, cap);
      OSQPHipAdmmTest t = c.fill(2);
      CHECK(osqp_hip_test_admm(s, &t) == OSQP_NO_ERROR && c.written());
      CHECK(t.form == 0 && t.f1_D == 0 && t.f1_mix == 0 && t.stat_n == 2 && t.stat_sum == 2 * cap && t.stat_max == cap && t.launches == 2 * (2 + 3 * cap));
      for (int k = 0; k < 2 * cap; k++) CHECK(std::isfinite(c.out[12][k]) && c.out[12][k] != -7.0);      // gamma, alpha of the last PCG
    }
    Canvas c(n, m, 16);
    OSQPHipAdmmTest t = c.fill(8, 1e9);              // a start that already meets the tolerance: no PCG iteration at all
    const OSQPInt rc8 = osqp_hip_test_admm(s, &t);
    std::printf("tolerance met at the start: rc %d n %d sum %d unconv %d tol %g done %d iters %d\n", (int)rc8, t.stat_n, t.stat_sum, t.stat_unconv, t.tol_now, t.pcg_done, t.pcg_iters);
    CHECK(rc8 == OSQP_NO_ERROR && t.stat_n == 8 && t.stat_sum == 0 && t.stat_unconv == 0 && t.tol_now == 1e9 && t.pcg_done == 1 && t.pcg_iters == 0);
  }
  {                                                  // everything else is refused before anything is touched
    Canvas c(n, m, 2);
    CHECK(osqp_hip_test_admm(s, nullptr) == OSQP_DATA_VALIDATION_ERROR);
    CHECK(osqp_hip_test_admm(nullptr, nullptr) == OSQP_WORKSPACE_NOT_INIT_ERROR);
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    auto refused = [&](auto &&edit) { OSQPHipAdmmTest t = c.fill(2); edit(t); const OSQPInt rc = osqp_hip_test_admm(s, &t); return rc == OSQP_DATA_VALIDATION_ERROR && c.untouched(); };
    CHECK(refused([](OSQPHipAdmmTest &t) { t.iters = 0; }));
    CHECK(refused([](OSQPHipAdmmTest &t) { t.iters = 9; }));
    CHECK(refused([](OSQPHipAdmmTest &t) { t.cap = -1; t.hist_len = -3; }));
    CHECK(refused([](OSQPHipAdmmTest &t) { t.cap = 17; t.hist_len = 51; }));
    CHECK(refused([&](OSQPHipAdmmTest &t) { t.tol_rel = nan; }));
    CHECK(refused([&](OSQPHipAdmmTest &t) { t.tol_abs = inf; }));
    CHECK(refused([](OSQPHipAdmmTest &t) { t.tol_abs = -1e-9; }));
    CHECK(refused([](OSQPHipAdmmTest &t) { t.n_len -= 1; }));
    CHECK(refused([](OSQPHipAdmmTest &t) { t.n_len += 1; }));
    CHECK(refused([](OSQPHipAdmmTest &t) { t.m_len += 1; }));
    CHECK(refused([](OSQPHipAdmmTest &t) { t.hist_len = 5; }));
    CHECK(refused([](OSQPHipAdmmTest &t) { t.x_in = nullptr; }));
    CHECK(refused([](OSQPHipAdmmTest &t) { t.y_in = nullptr; }));
    CHECK(refused([](OSQPHipAdmmTest &t) { t.xg = nullptr; }));
    CHECK(refused([](OSQPHipAdmmTest &t) { t.t0 = nullptr; }));
    CHECK(refused([](OSQPHipAdmmTest &t) { t.hist = nullptr; }));
  }
  {                                                  // a reordered handle computes the same thing in the caller's numbering
    OSQPSolver *r = make(n, m, 2);
    std::vector<OSQPInt> pc(n), pr(m);
    CHECK(osqp_hip_get_reordering(r, pc.data(), pr.data()) == OSQP_NO_ERROR);
    bool moved = false;
    for (int j = 0; j < n; j++) moved = moved || pc[j] != j;
    Canvas a(n, m, 3), b(n, m, 3);
    OSQPHipAdmmTest ta = a.fill(3), tb = b.fill(3);
    CHECK(osqp_hip_test_admm(s, &ta) == OSQP_NO_ERROR && osqp_hip_test_admm(r, &tb) == OSQP_NO_ERROR && b.written());
    double worst = 0;
    for (int k = 0; k < kOut - 1; k++) for (long long j = 0; j < a.len(k); j++) worst = std::fmax(worst, std::fabs(a.out[k][j] - b.out[k][j]) / (1.0 + std::fabs(a.out[k][j])));
    std::printf("reordered handle (%s): worst deviation %.3e\n", moved ? "permuted" : "identity", worst);
    CHECK(worst <= 1e-9);
    osqp_cleanup(r);
  }
  {                                                  // no constraints: the m-side pointers may be NULL
    OSQPSolver *u = make(n, 0, 0);
    Canvas c(n, 0, 2);
    OSQPHipAdmmTest t = c.fill(2);
    CHECK(osqp_hip_test_admm(u, &t) == OSQP_NO_ERROR && t.stat_sum == 4);
    osqp_cleanup(u);
  }
  osqp_cleanup(s);
  if (fails) { std::printf("%d checks failed\n", fails); return 1; }
  std::printf("admm_entry_probe OK\n");
  return 0;
}
