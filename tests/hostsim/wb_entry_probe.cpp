// tests/hostsim/wb_entry_probe.cpp -- TEST INFRASTRUCTURE ONLY.  Stand-alone program (own main) for the HOST side of osqp_hip_test_woodbury: the
// validation of Engine::test_woodbury and its copies between the caller's canvases and the engine's numbering, under the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -DHOSTSIM_WB_ENTRY_PROBE -o wb_entry_probe
//       tests/hostsim/wb_entry_probe.cpp tests/hostsim/backend_host.cpp osqp-python_amd/csrc/{engine,engine_setup,engine_api,api}.cpp && ./wb_entry_probe
// The simulator (built with HOSTSIM_WB_ENTRY_PROBE: the symbolic Woodbury plan is made, nothing numeric) gets a be::test_woodbury of its own here, which
// writes exactly the counts the entry lists into the engine's host vectors.  Every canvas is a heap block of exactly the listed length, so a copy one
// past it is a sanitizer report; every rejected call must leave all canvases as they were.  Prints what it checked and returns 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/osqp_hip.h"
#include "../../osqp-python_amd/csrc/backend.h"

namespace osqp_hip {
namespace be {
int test_woodbury(Dev &d, WbProbe &p) {
  const int n = d.n, m = d.m, ord = d.wb.dual ? d.wb.cd : d.wb.r;
  for (int j = 0; j < n; j++) { p.u[j] = 2.0 * p.r[j]; p.xs[j] = p.direct ? p.x0[j] + p.u[j] : -1.0; p.dinv0[j] = 1.0 + j; }
  for (long k = 0; k < (long)ord * ord; k++) { p.S[k] = (double)k; p.Sinv[k] = -(double)k; }
  for (int i = 0; i < m; i++) p.rho[i] = 0.1 + i;
  p.exact = 1; p.info[0] = 1; p.info[1] = 0; p.done = p.direct; p.iters = p.direct; p.gamma = 3.0; p.rnorm = 4.0;
  return OSQP_NO_ERROR;
}
}  // namespace be
}  // namespace osqp_hip

namespace {
int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

struct Csc { std::vector<OSQPInt> p, i; std::vector<OSQPFloat> x; OSQPCscMatrix m; };
void finish(Csc &c, int rows, int cols) { c.m = OSQPCscMatrix{rows, cols, c.p.data(), c.i.data(), c.x.data(), (OSQPInt)c.x.size(), -1}; }
// A: `longrows` rows over the first `dense` columns (+ `singles` columns of their own each), then one one-entry row per column
OSQPSolver *make(int dense, int longrows, int singles, int *n_out, int *m_out) {
  const int n = dense + longrows * singles + 1, m = longrows + n;
  Csc P, A;
  P.p.push_back(0);
  for (int j = 0; j < n; j++) { P.i.push_back(j); P.x.push_back(1.0 + 0.01 * j); P.p.push_back(j + 1); }
  finish(P, n, n);
  A.p.push_back(0);
  for (int j = 0; j < n; j++) {
    if (j < dense) for (int a = 0; a < longrows; a++) { A.i.push_back(a); A.x.push_back(0.5 + 0.001 * ((a * 31 + j * 17) % 97)); }
    else if (j < n - 1) { A.i.push_back((j - dense) / singles); A.x.push_back(-1.0); }
    A.i.push_back(longrows + j); A.x.push_back(1.0);
    A.p.push_back((OSQPInt)A.i.size());
  }
  finish(A, m, n);
  std::vector<OSQPFloat> q(n, 1.0), l(m, -1.0), u(m, 1.0);
  OSQPSettings st; osqp_set_default_settings(&st); st.verbose = 0; st.scaling = 0;
  OSQPSolver *s = nullptr;
  const OSQPInt rc = osqp_setup(&s, &P.m, q.data(), &A.m, l.data(), u.data(), m, n, &st);
  if (rc != 0) { std::printf("setup failed: %d\n", (int)rc); std::exit(2); }
  *n_out = n; *m_out = m;
  return s;
}
struct Canvas {
  double *u, *xs, *dinv0, *S, *Sinv, *rho; OSQPInt *idx; long long n, m, ord;
  static double *mk(long long c) { double *p = (double *)std::malloc(sizeof(double) * (size_t)c); for (long long k = 0; k < c; k++) p[k] = -7.0; return p; }
  Canvas(long long n_, long long m_, long long o) : n(n_), m(m_), ord(o) {
    u = mk(n + 16); xs = mk(n + 16); dinv0 = mk(n + 16); S = mk(o * o + 16); Sinv = mk(o * o + 16); rho = mk(m + 16);
    idx = (OSQPInt *)std::malloc(sizeof(OSQPInt) * (size_t)(o + 16)); for (long long k = 0; k < o + 16; k++) idx[k] = -1;
  }
  ~Canvas() { std::free(u); std::free(xs); std::free(dinv0); std::free(S); std::free(Sinv); std::free(rho); std::free(idx); }
  bool untouched_from(const double *p, long long from, long long to) const { for (long long k = from; k < to; k++) if (p[k] != -7.0) return false; return true; }
  bool all_untouched() const {
    for (long long k = 0; k < ord + 16; k++) if (idx[k] != -1) return false;
    return untouched_from(u, 0, n + 16) && untouched_from(xs, 0, n + 16) && untouched_from(dinv0, 0, n + 16) && untouched_from(S, 0, ord * ord + 16) && untouched_from(Sinv, 0, ord * ord + 16) && untouched_from(rho, 0, m + 16);
  }
};
OSQPHipWoodburyTest fill(const Canvas &c, const double *r, const double *x0, int direct) {
  OSQPHipWoodburyTest t;
  std::memset(&t, 0, sizeof(t));
  t.refactor = 1; t.parity = 1; t.direct = direct;
  t.r_len = c.n; t.x0_len = direct ? c.n : 0; t.u_len = t.xs_len = t.dinv0_len = c.n + 16; t.s_len = t.sinv_len = c.ord * c.ord + 16; t.rho_len = c.m + 16; t.idx_len = c.ord + 16;
  t.r = r; t.x0 = x0; t.u = c.u; t.xs = c.xs; t.dinv0 = c.dinv0; t.S = c.S; t.Sinv = c.Sinv; t.rho = c.rho; t.idx = c.idx;
  return t;
}
void one_handle(int dense, int longrows, int singles, int form, long long ord) {
  int n = 0, m = 0;
  OSQPSolver *s = make(dense, longrows, singles, &n, &m);
  std::vector<double> r(n), x0(n);
  for (int j = 0; j < n; j++) { r[j] = 1.0 + j; x0[j] = 0.5 * j; }
  for (int direct = 0; direct < 2; direct++) {
    Canvas c(n, m, ord);
    OSQPHipWoodburyTest t = fill(c, r.data(), direct ? x0.data() : nullptr, direct);
    const OSQPInt rc = osqp_hip_test_woodbury(s, &t);
    CHECK(rc == OSQP_NO_ERROR);
    CHECK(t.form == form && t.order == ord && t.rows == longrows && t.exact == 1 && t.done == direct && t.gamma == 3.0 && t.rnorm == 4.0);
    bool ok = true;
    for (int j = 0; j < n; j++) ok = ok && c.u[j] == 2.0 * r[j] && c.dinv0[j] == 1.0 + j && c.xs[j] == (direct ? x0[j] + 2.0 * r[j] : -1.0);
    for (int i = 0; i < m; i++) ok = ok && c.rho[i] == 0.1 + i;
    for (long long k = 0; k < ord; k++) ok = ok && c.idx[k] == (form == 2 ? k : k);      // (long rows 0 .. r-1 / dense columns 0 .. cd-1 of make())
    CHECK(ok);
    CHECK(c.untouched_from(c.u, n, n + 16) && c.untouched_from(c.xs, n, n + 16) && c.untouched_from(c.dinv0, n, n + 16) && c.untouched_from(c.rho, m, m + 16) &&
          c.untouched_from(c.S, ord * ord, ord * ord + 16) && c.untouched_from(c.Sinv, ord * ord, ord * ord + 16));
    for (long long k = ord; k < ord + 16; k++) CHECK(c.idx[k] == -1);
  }
  // rejections: one field wrong at a time, canvases exactly as long as the call CLAIMS where it claims less
  int rejected = 0;
  for (int what = 0; what < 40; what++) {
    Canvas c(n, m, ord);
    OSQPHipWoodburyTest t = fill(c, r.data(), x0.data(), 1);
    long long *lens[] = {&t.r_len, &t.x0_len, &t.u_len, &t.xs_len, &t.dinv0_len, &t.s_len, &t.sinv_len, &t.rho_len, &t.idx_len};
    if (what < 27) *lens[what / 3] += (what % 3 == 0 ? -1 : (what % 3 == 1 ? 1 : -16));
    else if (what == 27) t.parity = 2;
    else if (what == 28) t.parity = -1;
    else if (what == 29) t.direct = 2;
    else if (what == 30) { t.direct = 0; }                       // x0_len = n without direct
    else if (what == 31) t.r = nullptr;
    else if (what == 32) t.x0 = nullptr;
    else if (what == 33) t.u = nullptr;
    else if (what == 34) t.xs = nullptr;
    else if (what == 35) t.dinv0 = nullptr;
    else if (what == 36) t.S = nullptr;
    else if (what == 37) t.Sinv = nullptr;
    else if (what == 38) t.rho = nullptr;
    else t.idx = nullptr;
    const OSQPInt rc = osqp_hip_test_woodbury(s, &t);
    CHECK(rc == OSQP_DATA_VALIDATION_ERROR);
    CHECK(c.all_untouched());
    rejected += rc == OSQP_DATA_VALIDATION_ERROR;
  }
  CHECK(osqp_hip_test_woodbury(s, nullptr) == OSQP_DATA_VALIDATION_ERROR);
  std::printf("form %d: n %d m %d order %lld: 2 calls answered, %d rejected\n", form, n, m, ord, rejected);
  osqp_cleanup(s);
}
}  // namespace

int main() {
  one_handle(130, 2, 0, 0, 2);            // small form: two long rows
  one_handle(130, 129, 0, 1, 129);        // row space: 4 cd > 3 r
  one_handle(130, 180, 1, 2, 130);        // column space: 130 dense columns, a singleton per row
  { // no long row: the correction is off
    int n = 0, m = 0;
    OSQPSolver *s = make(5, 0, 0, &n, &m);
    Canvas c(n, m, 1);
    std::vector<double> r(n, 1.0);
    OSQPHipWoodburyTest t = fill(c, r.data(), nullptr, 0);
    CHECK(osqp_hip_test_woodbury(s, &t) == OSQP_FUNC_NOT_IMPLEMENTED);
    CHECK(c.all_untouched());
    osqp_cleanup(s);
  }
  std::printf(fails ? "%d checks FAILED\n" : "all checks passed\n", fails);
  return fails ? 1 : 0;
}
