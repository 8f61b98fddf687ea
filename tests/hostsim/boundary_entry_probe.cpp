// tests/hostsim/boundary_entry_probe.cpp -- TEST INFRASTRUCTURE ONLY.  Stand-alone program (own main) for the HOST side of osqp_hip_test_boundary: the
// validation of Engine::test_boundary, its copies between the caller's canvases and the engine's numbering (a reordered handle included) and mode 0 itself
// on the host simulator, under the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -o boundary_entry_probe
//       tests/hostsim/boundary_entry_probe.cpp tests/hostsim/backend_host.cpp osqp-python_amd/csrc/{engine,engine_setup,engine_api,api}.cpp && ./boundary_entry_probe
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
constexpr int kIn = 7, kOut = 9;      // in: x dx xt z y dy zt; out: res rho rho_inv v t0 ztg xg xsp Minv
struct Canvas {
  long long n, m;
  double *in[kIn], *out[kOut];
  static double *mk(long long c, double v) { double *p = (double *)std::malloc(sizeof(double) * (size_t)(c > 0 ? c : 1)); for (long long k = 0; k < c; k++) p[k] = v; return p; }
  long long ilen(int k) const { return k < 3 ? n : m; }
  long long olen(int k) const { return k == 0 ? OSQP_HIP_RES_COUNT : (k < 6 ? m : n); }
  Canvas(long long n_, long long m_) : n(n_), m(m_) {
    for (int k = 0; k < kIn; k++) { in[k] = mk(ilen(k), 0.0); for (long long j = 0; j < ilen(k); j++) in[k][j] = std::sin(1.0 + 0.37 * j + k); }
    for (int k = 0; k < kOut; k++) out[k] = mk(olen(k), -7.0);
  }
  ~Canvas() { for (auto p : in) std::free(p); for (auto p : out) std::free(p); }
  bool untouched() const { for (int k = 0; k < kOut; k++) for (long long j = 0; j < olen(k); j++) if (out[k][j] != -7.0) return false; return true; }
  bool written() const { for (int k = 0; k < kOut; k++) for (long long j = 0; j < olen(k); j++) if (!std::isfinite(out[k][j]) || out[k][j] == -7.0) return false; return true; }
  OSQPHipBoundaryTest fill(int need) const {
    OSQPHipBoundaryTest t;
    std::memset(&t, 0, sizeof(t));
    t.mode = 0; t.need = need; t.unscaled = 1; t.groups = 1; t.thr = 0.25; t.n_len = n; t.m_len = m; t.res_len = OSQP_HIP_RES_COUNT;
    const OSQPFloat **i[kIn] = {&t.x_in, &t.dx_in, &t.xt_in, &t.z_in, &t.y_in, &t.dy_in, &t.zt_in};
    for (int k = 0; k < kIn; k++) *i[k] = ilen(k) ? in[k] : nullptr;
    OSQPFloat **o[kOut] = {&t.res, &t.rho, &t.rho_inv, &t.v, &t.t0, &t.ztg, &t.xg, &t.xsp, &t.Minv};
    for (int k = 0; k < kOut; k++) *o[k] = olen(k) ? out[k] : nullptr;
    return t;
  }
};
}  // namespace

int main() {
  const int n = 37, m = 61;
  OSQPSolver *s = make(n, m, 0);
  CHECK(osqp_hip_res_name(-1) == nullptr && osqp_hip_res_name(OSQP_HIP_RES_COUNT) == nullptr);
  CHECK(std::strcmp(osqp_hip_res_name(0), "R_PRI_U") == 0 && std::strcmp(osqp_hip_res_name(OSQP_HIP_RES_COUNT - 1), "R_ADX_VIOL") == 0);
  {                                                  // valid runs: every combination of the second-stage bits
    for (int need = 0; need < 4; need++) {
      Canvas c(n, m);
      OSQPHipBoundaryTest t = c.fill(need);
      CHECK(osqp_hip_test_boundary(s, &t) == OSQP_NO_ERROR && c.written());
      CHECK(t.form == 0 && t.launches == 3 + ((need & 1) ? 2 : 0) + ((need & 2) ? 3 : 0));
      CHECK(c.out[0][7] > 0.0 && c.out[0][7] <= 1.0);                         // R_DY_S of the sine canvas
      std::printf("need %d: R_PRI_S %.6f R_DUA_S %.6f R_ATDY_S %.6f R_PDX_S %.6f violations %.0f\n", need, c.out[0][3], c.out[0][13], c.out[0][24], c.out[0][26], c.out[0][27]);
    }
  }
  {                                                  // everything else is refused before anything is touched
    Canvas c(n, m);
    CHECK(osqp_hip_test_boundary(s, nullptr) == OSQP_DATA_VALIDATION_ERROR);
    CHECK(osqp_hip_test_boundary(nullptr, nullptr) == OSQP_WORKSPACE_NOT_INIT_ERROR);
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    auto refused = [&](auto &&edit) { OSQPHipBoundaryTest t = c.fill(3); edit(t); const OSQPInt rc = osqp_hip_test_boundary(s, &t); return rc == OSQP_DATA_VALIDATION_ERROR && c.untouched(); };
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.mode = 2; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.mode = -1; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.need = 4; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.need = -1; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.unscaled = 2; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.keep = -1; }));
    CHECK(refused([&](OSQPHipBoundaryTest &t) { t.thr = nan; }));
    CHECK(refused([&](OSQPHipBoundaryTest &t) { t.thr = inf; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.thr = -1e-9; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.n_len -= 1; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.n_len += 1; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.m_len += 1; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.res_len -= 1; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.res_len += 1; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.x_in = nullptr; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.dx_in = nullptr; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.zt_in = nullptr; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.dy_in = nullptr; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.res = nullptr; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.rho_inv = nullptr; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.xsp = nullptr; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.mode = 1; t.groups = 0; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.mode = 1; t.groups = 3; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.mode = 1; t.at_check = 2; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.mode = 1; t.chunk_done = 2; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.mode = 1; t.status_in = 3; }));
    CHECK(refused([](OSQPHipBoundaryTest &t) { t.mode = 1; t.iter = -1; }));
    OSQPHipBoundaryTest t = c.fill(3);               // the device-driven group does not exist on the host simulator
    t.mode = 1; t.iter = 50; t.at_check = 1; t.chunk_done = 1;
    CHECK(osqp_hip_test_boundary(s, &t) == OSQP_FUNC_NOT_IMPLEMENTED && c.untouched());
  }
  {                                                  // a reordered handle computes the same thing in the caller's numbering
    OSQPSolver *r = make(n, m, 2);
    std::vector<OSQPInt> pc(n), pr(m);
    CHECK(osqp_hip_get_reordering(r, pc.data(), pr.data()) == OSQP_NO_ERROR);
    bool moved = false;
    for (int j = 0; j < n; j++) moved = moved || pc[j] != j;
    Canvas a(n, m), b(n, m);
    OSQPHipBoundaryTest ta = a.fill(3), tb = b.fill(3);
    CHECK(osqp_hip_test_boundary(s, &ta) == OSQP_NO_ERROR && osqp_hip_test_boundary(r, &tb) == OSQP_NO_ERROR && b.written());
    double worst = 0;
    for (int k = 0; k < kOut; k++) for (long long j = 0; j < a.olen(k); j++) worst = std::fmax(worst, std::fabs(a.out[k][j] - b.out[k][j]) / (1.0 + std::fabs(a.out[k][j])));
    std::printf("reordered handle (%s): worst deviation %.3e\n", moved ? "permuted" : "identity", worst);
    CHECK(worst <= 1e-9);
    osqp_cleanup(r);
  }
  {                                                  // no constraints: the m-side pointers may be NULL, the m-side quantities are 0
    OSQPSolver *u = make(n, 0, 0);
    Canvas c(n, 0);
    OSQPHipBoundaryTest t = c.fill(3);
    CHECK(osqp_hip_test_boundary(u, &t) == OSQP_NO_ERROR);
    for (int q = 0; q < 10; q++) CHECK(c.out[0][q] == 0.0);
    CHECK(c.out[0][27] == 0.0 && c.out[0][13] > 0.0);
    osqp_cleanup(u);
  }
  osqp_cleanup(s);
  if (fails) { std::printf("%d checks failed\n", fails); return 1; }
  std::printf("boundary_entry_probe OK\n");
  return 0;
}
