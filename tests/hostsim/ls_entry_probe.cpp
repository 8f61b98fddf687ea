// tests/hostsim/ls_entry_probe.cpp -- TEST INFRASTRUCTURE ONLY.  Stand-alone program (own main) for the HOST side of osqp_hip_test_lockstep: every
// validation branch of Engine::test_lockstep, the lengths it stages and hands down, and its copies of the blocks, under the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -DHOSTSIM_LS_ENTRY_PROBE -o ls_entry_probe
//       tests/hostsim/ls_entry_probe.cpp tests/hostsim/backend_host.cpp osqp-python_amd/csrc/{engine,engine_setup,engine_api,api}.cpp && ./ls_entry_probe
// The simulator (built with HOSTSIM_LS_ENTRY_PROBE: it then reports resident vectors, which the lockstep routes ask for; their updates stay the no-ops they
// are) gets a be::lockstep_chunk that is never called and a be::test_lockstep of its own here, which records what it is handed, reads every staged array
// from its first to its last element and marks the block.  Every canvas is a heap block of exactly the length the call CLAIMS, so a copy one past it is a
// sanitizer report; every rejected call must leave all canvases as they were.  Prints what it checked and returns 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/osqp_hip.h"
#include "../../osqp-python_amd/csrc/backend.h"

namespace {
struct Seen { int calls = 0, n = 0, m = 0, count = 0, warm = 0, nops = 0, op0 = -1; bool q = false, l = false, u = false, Px = false, Ax = false, mat = false; double sum = 0; } seen;
}

namespace osqp_hip {
namespace be {
int lockstep_chunk(Dev &, const LockstepParams &, void *, double *) { return OSQP_FUNC_NOT_IMPLEMENTED; }
int test_lockstep(Dev &d, const LsProbe &t) {
  const LockstepParams &p = t.p;
  seen.calls++; seen.n = p.n; seen.m = p.m; seen.count = p.count; seen.warm = p.warm; seen.nops = t.nops; seen.op0 = t.ops[0];
  seen.q = p.q; seen.l = p.l; seen.u = p.u; seen.Px = p.Px; seen.Ax = p.Ax; seen.mat = p.mat_ws;
  double s = 0;
  auto rd = [&](const double *v, size_t cnt) { for (size_t k = 0; v && k < cnt; k++) s += v[k]; };      // (the staged copies are exactly this long)
  const size_t c = (size_t)p.count;
  rd(p.q, c * p.n); rd(p.l, c * p.m); rd(p.u, c * p.m); rd(p.x, c * p.n); rd(p.y, c * p.m); rd(p.rec, c * kBatchRec); rd(p.Px, c * d.nzP); rd(p.Ax, c * d.nzA);
  seen.sum = s;
  const size_t need = lockstep_ws_doubles(p.n, p.m);
  p.ws[0] += 1.0; p.ws[need - 1] += 2.0;
  if (p.mat_ws) p.mat_ws[lockstep_mat_ws_doubles(p.n, p.m, d.A.nnz, d.B.nnz) - 1] += 3.0;
  for (size_t k = 0; k < c * p.n; k++) p.x[k] = -p.x[k];
  p.rec[c * kBatchRec - 1] = 42.0;
  return OSQP_NO_ERROR;
}
}  // namespace be
}  // namespace osqp_hip

namespace {
int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

struct Csc { std::vector<OSQPInt> p, i; std::vector<OSQPFloat> x; OSQPCscMatrix m; };
void finish(Csc &c, int rows, int cols) { c.m = OSQPCscMatrix{rows, cols, c.p.data(), c.i.data(), c.x.data(), (OSQPInt)c.x.size(), -1}; }
// tridiagonal P, A = [I; a row pair per column]: no long row
OSQPSolver *make(int n, int m) {
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
  const OSQPInt rc = osqp_setup(&s, &P.m, q.data(), m ? &A.m : &A.m, l.data(), u.data(), m, n, &st);
  if (rc != 0) { std::printf("setup failed: %d\n", (int)rc); std::exit(2); }
  return s;
}
double *mk(long long c) { double *p = (double *)std::malloc(sizeof(double) * (size_t)(c > 0 ? c : 1)); for (long long k = 0; k < c; k++) p[k] = -7.0; return p; }
OSQPInt *mki(long long c) { OSQPInt *p = (OSQPInt *)std::malloc(sizeof(OSQPInt) * (size_t)(c > 0 ? c : 1)); for (long long k = 0; k < c; k++) p[k] = -7; return p; }
// every array of a call, each exactly as long as its length field says
struct Canvas {
  OSQPHipLockstepTest t;
  std::vector<double *> d; std::vector<long long> dl; std::vector<OSQPInt *> iv; std::vector<long long> il;
  OSQPInt ops[3] = {OSQP_HIP_LS_RHS, OSQP_HIP_LS_CGINIT, OSQP_HIP_LS_LOAD_N};
  double *D(long long c) { d.push_back(mk(c)); dl.push_back(c); return d.back(); }
  OSQPInt *I(long long c) { iv.push_back(mki(c)); il.push_back(c); return iv.back(); }
  Canvas(const OSQPHipLockstepTest &sz, int count, bool mat, bool handle) {
    std::memset(&t, 0, sizeof(t));
    const long long n = sz.n, m = sz.m, c = count;
    t.route = 0; t.mat = mat; t.count = count; t.warm = 1; t.nops = 3; t.ops = ops;
    t.q_len = c * n; t.l_len = t.u_len = t.y_len = c * m; t.x_len = c * n; t.rec_len = c * OSQP_HIP_BATCH_REC; t.ws_len = sz.ws_need;
    t.q = D(t.q_len); t.l = D(t.l_len); t.u = D(t.u_len); t.x = D(t.x_len); t.y = D(t.y_len); t.rec = D(t.rec_len); t.ws = D(t.ws_len);
    if (mat) { t.px_len = c * sz.nzP; t.ax_len = c * sz.nzA; t.mat_len = sz.mat_need; t.Px = D(t.px_len); t.Ax = D(t.ax_len); t.mat_ws = D(t.mat_len); }
    if (handle) {
      t.arp_len = m + 1; t.anz_len = sz.nnzA; t.brp_len = n + 1; t.bnz_len = sz.nnzB; t.n_len = n; t.m_len = m;
      t.A_rowptr = I(m + 1); t.A_col = I(sz.nnzA); t.B_rowptr = I(n + 1); t.B_col = I(sz.nnzB);
      t.A_val = D(sz.nnzA); t.B_val = D(sz.nnzB); t.D = D(n); t.Dinv = D(n); t.E = D(m); t.Einv = D(m);
    }
  }
  ~Canvas() { for (double *p : d) std::free(p); for (OSQPInt *p : iv) std::free(p); }
  bool untouched() const {
    for (size_t a = 0; a < d.size(); a++) for (long long k = 0; k < dl[a]; k++) if (d[a][k] != -7.0) return false;
    for (size_t a = 0; a < iv.size(); a++) for (long long k = 0; k < il[a]; k++) if (iv[a][k] != -7) return false;
    return true;
  }
};

void one_handle(int n, int m) {
  OSQPSolver *s = make(n, m);
  OSQPHipLockstepTest sz;
  std::memset(&sz, 0, sizeof(sz));
  CHECK(osqp_hip_test_lockstep(s, &sz) == OSQP_DATA_VALIDATION_ERROR);          // (the sizes come back from a rejected call)
  CHECK(sz.n == n && sz.m == m && sz.ws_need > 0 && sz.mat_need > 0 && sz.G >= 1 && sz.nnzB >= n);
  CHECK(osqp_hip_test_lockstep(s, nullptr) == OSQP_DATA_VALIDATION_ERROR);
  // ---- answered calls: what is handed down, what comes back
  for (int count : {1, 6, 64}) {
    Canvas c(sz, count, false, true);
    const int calls0 = seen.calls;
    const OSQPInt rc = osqp_hip_test_lockstep(s, &c.t);
    CHECK(rc == OSQP_NO_ERROR && seen.calls == calls0 + 1);
    if (rc != OSQP_NO_ERROR) std::printf("  (count %d answered %d)\n", count, (int)rc);
    CHECK(seen.n == n && seen.m == m && seen.count == count && seen.warm == 1 && seen.nops == 3 && seen.op0 == OSQP_HIP_LS_RHS && seen.q && seen.l && seen.u && !seen.Px && !seen.Ax && !seen.mat);
    const long long c64 = count;
    CHECK(seen.sum == -7.0 * (double)(c64 * (2 * n + 3 * m + OSQP_HIP_BATCH_REC)));
    CHECK(c.t.ws[0] == -6.0 && c.t.ws[sz.ws_need - 1] == -5.0 && c.t.ws[1] == -7.0);                      // the block came back, marked where the backend marked it
    CHECK(c.t.x[0] == 7.0 && c.t.x[c64 * n - 1] == 7.0 && c.t.rec[c64 * OSQP_HIP_BATCH_REC - 1] == 42.0 && c.t.rec[0] == -7.0 && (m == 0 || c.t.y[0] == -7.0));
    CHECK(c.t.A_rowptr[0] == 0 && c.t.A_rowptr[m] == sz.nnzA && c.t.B_rowptr[n] == sz.nnzB && c.t.D[n - 1] == 1.0 && c.t.c == 1.0);
    CHECK(c.t.q[0] == -7.0);
  }
  { // optional inputs absent
    Canvas c(sz, 2, false, false);
    c.t.q = nullptr; c.t.q_len = 0; c.t.l = nullptr; c.t.l_len = 0;
    CHECK(osqp_hip_test_lockstep(s, &c.t) == OSQP_NO_ERROR && !seen.q && !seen.l && seen.u);
  }
  // ---- rejections: one thing wrong at a time
  int rejected = 0;
  for (int what = 0; what < 60; what++) {
    Canvas c(sz, 3, false, true);
    OSQPHipLockstepTest &t = c.t;
    long long *lens[] = {&t.q_len, &t.l_len, &t.u_len, &t.x_len, &t.y_len, &t.rec_len, &t.ws_len, &t.arp_len, &t.anz_len, &t.brp_len, &t.bnz_len, &t.n_len, &t.m_len};
    OSQPInt bad_op = OSQP_HIP_LS_OP_COUNT, neg_op = -1, mat_op = OSQP_HIP_LS_NORMS;
    if (what < 26) { if (m == 0 && (lens[what / 2] == &t.l_len || lens[what / 2] == &t.u_len || lens[what / 2] == &t.y_len || lens[what / 2] == &t.m_len) && what % 2 == 0) continue; *lens[what / 2] += what % 2 ? 1 : -1; }
    else if (what == 26) t.route = 2;
    else if (what == 27) t.route = -1;
    else if (what == 28) t.mat = 2;
    else if (what == 29) t.count = 0;
    else if (what == 30) t.count = 65;
    else if (what == 31) t.nops = 0;
    else if (what == 32) t.nops = 65;
    else if (what == 33) t.ops = nullptr;
    else if (what == 34) { t.ops = &bad_op; t.nops = 1; }
    else if (what == 35) { t.ops = &neg_op; t.nops = 1; }
    else if (what == 36) { t.ops = &mat_op; t.nops = 1; }                    // an op of the matrices of a chunk without mat
    else if (what == 37) t.x = nullptr;
    else if (what == 38) t.rec = nullptr;
    else if (what == 39) t.ws = nullptr;
    else if (what == 40) t.q = nullptr;                                     // a length without its pointer
    else if (what == 41) { t.mat_ws = t.ws; }                               // a matrix block without mat
    else if (what == 42) { t.mat_len = sz.mat_need; }
    else if (what == 43) { if (sz.nnzA == 0) continue; t.A_col = nullptr; }   // half a group (an empty array may have any pointer)
    else if (what == 44) t.Dinv = nullptr;
    else if (what == 45) { t.pmap_len = sz.nzP + 1; }                         // a group's length without its pointers
    else if (what == 46) t.warm = 2;
    else if (what == 47) { t.px_len = 3 * sz.nzP + 3; t.Px = t.q; }             // per-problem values without mat
    else if (what == 48) { t.mat = 1; }                                     // mat without its block
    else if (what == 49) { if (m > 0) continue; static OSQPInt mop = OSQP_HIP_LS_LOAD_M; t.ops = &mop; t.nops = 1; }      // an m-side op on an m = 0 handle
    else continue;
    const int calls0 = seen.calls;
    const OSQPInt rc = osqp_hip_test_lockstep(s, &t);
    CHECK(rc == OSQP_DATA_VALIDATION_ERROR);
    if (rc != OSQP_DATA_VALIDATION_ERROR) std::printf("  (what = %d answered %d)\n", what, (int)rc);
    CHECK(seen.calls == calls0);
    c.t.ws = c.t.ws ? c.t.ws : nullptr;
    CHECK(c.untouched());
    rejected++;
  }
  { // the direct route declines a handle without long rows (the simulator sets no Woodbury correction up: that route's view lengths are checked on the GPU tier);
    // per-problem matrices need a backend that assembles on the device (the simulator does not)
    Canvas c(sz, 3, false, false);
    c.t.route = 1;
    const int calls0 = seen.calls;
    CHECK(osqp_hip_test_lockstep(s, &c.t) == OSQP_FUNC_NOT_IMPLEMENTED && seen.calls == calls0 && c.untouched());
    Canvas cm(sz, 3, true, false);
    CHECK(osqp_hip_test_lockstep(s, &cm.t) == OSQP_FUNC_NOT_IMPLEMENTED && seen.calls == calls0 && cm.untouched());
    for (long long *ln : {&cm.t.mat_len, &cm.t.px_len, &cm.t.ax_len}) {      // with mat the lengths are checked first
      Canvas c2(sz, 3, true, false);
      long long *l2 = ln == &cm.t.mat_len ? &c2.t.mat_len : (ln == &cm.t.px_len ? &c2.t.px_len : &c2.t.ax_len);
      *l2 -= 1;
      CHECK(osqp_hip_test_lockstep(s, &c2.t) == OSQP_DATA_VALIDATION_ERROR && c2.untouched());
      rejected++;
    }
  }
  std::printf("n %d m %d: 4 calls answered, %d rejected, 2 declined\n", n, m, rejected);
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
