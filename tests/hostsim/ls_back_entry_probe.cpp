// tests/hostsim/ls_back_entry_probe.cpp -- TEST INFRASTRUCTURE ONLY.  Stand-alone program (own main) for the HOST side of osqp_hip_test_lockstep_back:
// the validation branches of Engine::test_lockstep_back, the lengths it stages and hands down, and its copies of the blocks, under the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -DHOSTSIM_LS_ENTRY_PROBE -o ls_back_entry_probe
//       tests/hostsim/ls_back_entry_probe.cpp tests/hostsim/backend_host.cpp osqp-python_amd/csrc/{engine,engine_setup,engine_api,api}.cpp && ./ls_back_entry_probe
// As ls_entry_probe.cpp: the simulator gets a be::lockstep_chunk that is never called and a be::test_lockstep_back of its own here, which records what it is
// handed, reads every staged array from its first to its last element and marks the blocks.  Every canvas is a heap block of exactly the length the call
// CLAIMS; every rejected call must leave all canvases as they were.  The simulator does not assemble on the device, so the backward pass's predicate
// declines there: mode 1 (polish) is answered, mode 0 (adjoint) is checked up to the route (every validation branch) and then declined -- its answered
// path runs on the GPU tier.  Prints what it checked and returns 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/osqp_hip.h"
#include "../../osqp-python_amd/csrc/backend.h"

namespace {
struct Seen { int calls = 0, n = 0, m = 0, count = 0, nops = 0, op0 = -1, polish = 0, pol_min = 0; bool mat = false, pol_ws = false; double sum = 0, secs = 0, pol_rho = 0; } seen;
}

namespace osqp_hip {
namespace be {
int lockstep_chunk(Dev &, const LockstepParams &, void *, double *) { return OSQP_FUNC_NOT_IMPLEMENTED; }
int test_lockstep_back(Dev &, LsBackProbe &t) {
  const LockstepParams &p = t.p;
  seen.calls++; seen.n = p.n; seen.m = p.m; seen.count = p.count; seen.nops = t.nops; seen.op0 = t.ops[0]; seen.polish = t.polish; seen.secs = t.secs;
  seen.mat = p.mat_ws; seen.pol_ws = p.pol_ws; seen.pol_rho = p.pol_rho; seen.pol_min = p.pol_min_steps;
  double s = 0;
  auto rd = [&](const double *v, size_t cnt) { for (size_t k = 0; v && k < cnt; k++) s += v[k]; };      // (the staged copies are exactly this long)
  const size_t c = (size_t)p.count;
  rd(p.x, c * p.n); rd(p.y, c * p.m); rd(p.rec, c * kBatchRec);
  seen.sum = s;
  p.ws[0] += 1.0; p.ws[lockstep_ws_doubles(p.n, p.m) - 1] += 2.0;
  p.pol_ws[0] += 3.0; p.pol_ws[lockstep_polish_ws_doubles(p.n, p.m) - 1] += 4.0;
  t.pol_max_steps = 30;
  return OSQP_NO_ERROR;
}
}  // namespace be
}  // namespace osqp_hip

namespace {
int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

struct Csc { std::vector<OSQPInt> p, i; std::vector<OSQPFloat> x; OSQPCscMatrix m; };
void finish(Csc &c, int rows, int cols) { c.m = OSQPCscMatrix{rows, cols, c.p.data(), c.i.data(), c.x.data(), (OSQPInt)c.x.size(), -1}; }
OSQPSolver *make(int n, int m) {       // tridiagonal P, A = [I; a row pair per column]: no long row
  Csc P, A;
  P.p.push_back(0);
  for (int j = 0; j < n; j++) { if (j > 0) { P.i.push_back(j - 1); P.x.push_back(0.1); } P.i.push_back(j); P.x.push_back(2.0 + 0.01 * j); P.p.push_back((OSQPInt)P.i.size()); }
  finish(P, n, n);
  A.p.push_back(0);
  for (int j = 0; j < n; j++) { for (int i = 0; i < m; i++) if (i % n == j || (i + 1) % n == j) { A.i.push_back(i); A.x.push_back(1.0 + 0.1 * i); } A.p.push_back((OSQPInt)A.i.size()); }
  finish(A, m, n);
  std::vector<OSQPFloat> q(n, 1.0), l(m, -1.0), u(m, 1.0);
  OSQPSettings st; osqp_set_default_settings(&st); st.verbose = 0; st.scaling = 0;
  OSQPSolver *s = nullptr;
  const OSQPInt rc = osqp_setup(&s, &P.m, q.data(), &A.m, l.data(), u.data(), m, n, &st);
  if (rc != 0) { std::printf("setup failed: %d\n", (int)rc); std::exit(2); }
  return s;
}
double *mk(long long c) { double *p = (double *)std::malloc(sizeof(double) * (size_t)(c > 0 ? c : 1)); for (long long k = 0; k < c; k++) p[k] = -7.0; return p; }
// every array of a call, each exactly as long as its length field says
struct Canvas {
  OSQPHipLockstepBackTest t;
  std::vector<double *> d; std::vector<long long> dl;
  OSQPInt ops[2];
  double *D(long long c) { d.push_back(mk(c)); dl.push_back(c); return d.back(); }
  Canvas(const OSQPHipLockstepBackTest &sz, int count, bool polish) {
    std::memset(&t, 0, sizeof(t));
    const long long n = sz.n, m = sz.m, c = count;
    ops[0] = polish ? OSQP_HIP_LSB_POL_END : OSQP_HIP_LSB_ADJ_INIT; ops[1] = polish ? OSQP_HIP_LSB_POL_BEGIN : OSQP_HIP_LSB_ADJ_FINAL;
    t.mode = polish; t.count = count; t.nops = 2; t.ops = ops; t.secs = 0.25;
    if (polish) {
      t.x_len = c * n; t.y_len = c * m; t.rec_len = c * OSQP_HIP_BATCH_REC; t.ws_len = sz.ws_need; t.pol_len = sz.pol_need;
      t.x = D(t.x_len); t.y = D(t.y_len); t.rec = D(t.rec_len); t.ws = D(t.ws_len); t.pol_ws = D(t.pol_len);
    } else {
      t.sx_len = t.gx_len = t.dq_len = c * n; t.sy_len = t.gy_len = t.l_len = t.u_len = t.dl_len = t.du_len = c * m; t.dp_len = c * sz.nzP; t.da_len = c * sz.nzA;
      t.arec_len = c * OSQP_HIP_ADJOINT_REC; t.ws_len = sz.adj_need;
      t.sx = D(t.sx_len); t.gx = D(t.gx_len); t.sy = D(t.sy_len); t.gy = D(t.gy_len); t.l = D(t.l_len); t.u = D(t.u_len);
      t.dq = D(t.dq_len); t.dl = D(t.dl_len); t.du = D(t.du_len); t.dP = D(t.dp_len); t.dA = D(t.da_len); t.arec = D(t.arec_len); t.ws = D(t.ws_len);
    }
  }
  ~Canvas() { for (double *p : d) std::free(p); }
  bool untouched() const {
    for (size_t a = 0; a < d.size(); a++) for (long long k = 0; k < dl[a]; k++) if (d[a][k] != -7.0) return false;
    return true;
  }
};

void one_handle(int n, int m) {
  OSQPSolver *s = make(n, m);
  OSQPHipLockstepBackTest sz;
  std::memset(&sz, 0, sizeof(sz));
  CHECK(osqp_hip_test_lockstep_back(s, &sz) == OSQP_DATA_VALIDATION_ERROR);     // (the sizes come back from a rejected call)
  CHECK(sz.n == n && sz.m == m && sz.ws_need > 0 && sz.adj_need > sz.ws_need && sz.mat_need > 0 && sz.pol_need == 64LL * (n + 4 * m) + 64 && sz.G >= 1 && sz.r == 0 && sz.dws_need == 0);
  CHECK(osqp_hip_test_lockstep_back(s, nullptr) == OSQP_DATA_VALIDATION_ERROR);
  // ---- polish: answered calls
  for (int count : {1, 6, 64}) {
    Canvas c(sz, count, true);
    const int calls0 = seen.calls;
    const OSQPInt rc = osqp_hip_test_lockstep_back(s, &c.t);
    CHECK(rc == OSQP_NO_ERROR && seen.calls == calls0 + 1);
    if (rc != OSQP_NO_ERROR) { std::printf("  (count %d answered %d)\n", count, (int)rc); continue; }
    CHECK(seen.n == n && seen.m == m && seen.count == count && seen.nops == 2 && seen.op0 == OSQP_HIP_LSB_POL_END && seen.polish && seen.secs == 0.25 && !seen.mat && seen.pol_ws);
    CHECK(seen.sum == -7.0 * (double)((long long)count * (n + m + OSQP_HIP_BATCH_REC)));
    CHECK(c.t.ws[0] == -6.0 && c.t.ws[sz.ws_need - 1] == -5.0 && c.t.ws[1] == -7.0 && c.t.pol_ws[0] == -4.0 && c.t.pol_ws[sz.pol_need - 1] == -3.0 && c.t.pol_ws[1] == -7.0);
    CHECK(c.t.x[0] == -7.0 && c.t.rec[0] == -7.0);
    CHECK(c.t.pol_max_steps == 30 && c.t.pol_min_steps == seen.pol_min && c.t.pol_rho == seen.pol_rho && c.t.pol_rho > 0 && c.t.adjoint_tol == OSQP_HIP_ADJOINT_TOL);
  }
  // ---- rejections, both modes: one thing wrong at a time
  int rejected = 0;
  for (int polish = 0; polish < 2; polish++) {
    for (int what = 0; what < 70; what++) {
      Canvas c(sz, 3, polish != 0);
      OSQPHipLockstepBackTest &t = c.t;
      long long *lens[] = {&t.sx_len, &t.sy_len, &t.gx_len, &t.gy_len, &t.l_len, &t.u_len, &t.dq_len, &t.dl_len, &t.du_len, &t.dp_len, &t.da_len, &t.arec_len, &t.x_len, &t.y_len,
                           &t.rec_len, &t.ws_len, &t.mat_len, &t.pol_len};
      static OSQPInt op1;
      auto one = [&](OSQPInt op) { op1 = op; t.ops = &op1; t.nops = 1; };
      if (what < 36) { *lens[what / 2] += what % 2 ? 1 : -1; }                   // (a length of -1 where 0 is expected is wrong too)
      else if (what == 36) t.route = 2;
      else if (what == 37) t.mode = 2;
      else if (what == 38) t.mat = 2;
      else if (what == 39) t.count = 0;
      else if (what == 40) t.count = 65;
      else if (what == 41) t.nops = 0;
      else if (what == 42) t.nops = 65;
      else if (what == 43) t.ops = nullptr;
      else if (what == 44) one(OSQP_HIP_LSB_OP_COUNT);
      else if (what == 45) one(-1);
      else if (what == 46) one(polish ? OSQP_HIP_LSB_ADJ_INIT : OSQP_HIP_LSB_POL_BEGIN);      // an op of the other mode
      else if (what == 47) one(OSQP_HIP_LSB_LWA_ZERO);                          // the direct route's op on route 0
      else if (what == 48) t.ws = nullptr;
      else if (what == 49) { t.mat = 1; }                                       // mat without its block
      else if (what == 50) { t.mat_ws = t.ws; }                                 // a matrix block without mat
      else if (what == 51) { if (polish) { t.sx = t.x; t.sx_len = t.x_len; } else { t.x = t.dq; t.x_len = t.dq_len; } }      // an array of the other mode
      else if (what == 52) { if (polish) t.pol_ws = nullptr; else { t.pol_ws = t.ws; } }
      else if (what == 53) { if (polish) t.rec = nullptr; else t.sx = nullptr; }    // a length without its pointer
      else if (what == 54) { if (polish) continue; t.dq = nullptr; t.dq_len = 0; one(OSQP_HIP_LSB_ADJ_OUT_N); }      // an output op without its array
      else if (what == 55) { if (polish) continue; t.dl = t.du = nullptr; t.dl_len = t.du_len = 0; one(OSQP_HIP_LSB_ADJ_OUT_M); }
      else if (what == 56) { if (polish) continue; t.dP = nullptr; t.dp_len = 0; one(OSQP_HIP_LSB_ADJ_GRAD_P); }
      else if (what == 57) { if (polish) continue; t.dA = nullptr; t.da_len = 0; one(OSQP_HIP_LSB_ADJ_GRAD_A); }
      else if (what == 58) { if (m > 0) continue; one(polish ? OSQP_HIP_LSB_POL_CONE : OSQP_HIP_LSB_ADJ_CLASS); }      // an m-side op on an m = 0 handle
      else if (what == 59) { if (m > 0 || polish) continue; one(OSQP_HIP_LSB_ADJ_GRAD_A); }                              // a gradient without stored entries
      else continue;
      const int calls0 = seen.calls;
      const OSQPInt rc = osqp_hip_test_lockstep_back(s, &t);
      CHECK(rc == OSQP_DATA_VALIDATION_ERROR);
      if (rc != OSQP_DATA_VALIDATION_ERROR) std::printf("  (mode %d what = %d answered %d)\n", polish, what, (int)rc);
      CHECK(seen.calls == calls0 && c.untouched());
      rejected++;
    }
  }
  { // declined: the direct route on a handle without long rows, both modes; the backward pass on a backend that does not assemble on the device
    const int calls0 = seen.calls;
    for (int polish = 0; polish < 2; polish++) {
      Canvas c(sz, 3, polish != 0);
      c.t.route = 1;
      CHECK(osqp_hip_test_lockstep_back(s, &c.t) == OSQP_FUNC_NOT_IMPLEMENTED && seen.calls == calls0 && c.untouched());
    }
    Canvas c(sz, 3, false);
    CHECK(osqp_hip_test_lockstep_back(s, &c.t) == OSQP_FUNC_NOT_IMPLEMENTED && seen.calls == calls0 && c.untouched());
  }
  std::printf("n %d m %d: 3 calls answered, %d rejected, 3 declined\n", n, m, rejected);
  osqp_cleanup(s);
}
}  // namespace

int main() {
  one_handle(7, 9);
  one_handle(70, 37);
  one_handle(5, 0);
  std::printf(fails ? "%d checks FAILED\n" : "all checks passed\n", fails);
  return fails ? 1 : 0;
}
