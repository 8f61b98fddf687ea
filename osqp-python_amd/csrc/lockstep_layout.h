// lockstep_layout.h -- where everything sits in the work blocks of a lockstep chunk (lockstep_hip.hip): the pointer sets its kernels take and ONE carve per
// set, written over a cursor.  The drivers carve a device block with it, Engine::lockstep_mat_scaling finds D / E / c with it, lockstep_sc_offset counts
// with it, and tests/test_lockstep_layout.py checks it on the CPU against the size functions below (a counting cursor touches no memory).
// Plain C++: no HIP type enters here.
#pragma once
#include <cstddef>

namespace osqp_hip {

constexpr int kBatchRec = 12;     // doubles per problem in the result record of the batch kernels (OSQP_HIP_BATCH_REC in include/osqp_hip.h)
constexpr int kLsW = 64;          // chunk width: one wave's lanes
constexpr int kLsSlots = 32;      // partial-reduction slots of a chunk ([slot][workgroup][kLsW])
constexpr int kLsScal = 16, kLsInt = 12;      // rows of the per-problem fp64 / int32 state ([row][kLsW])
constexpr int kLsMatScalC = 11;   // row of the per-problem scalar state that holds c (lockstep_hip.hip SC_C; 1 / c follows)
// workgroups of the row passes (four waves each, a wave owns a strip of rows): from the row counts alone, so that the partition -- and with it every
// sum's order -- does not depend on what a chunk holds
inline int lockstep_grid(int n, int m) { const int r = n > m ? n : m, g = (r + 15) / 16; return g < 1 ? 1 : (g > 256 ? 256 : g); }
// columns of a block of the direct route's products with the long rows (a multiple of 64, at most 128 blocks): from n alone, like lockstep_grid
inline int lockstep_direct_colblock(int n) { const int t = (n + 63) / 64; return 64 * ((t + 127) / 128 > 0 ? (t + 127) / 128 : 1); }
inline int lockstep_direct_colblocks(int n) { const int cb = lockstep_direct_colblock(n); return (n + cb - 1) / cb; }

// ---- the pointer sets.  A block vector holds element (j, b) at j * kLsW + b; every range below starts at a multiple of kLsW doubles from its block's base.
struct LsWs {                                           // every route
  double *x, *xs, *r, *p, *Kp, *q, *Minv, *dx;        // n x W (x, xs, dx: n + r rows on the direct route, which has no Kp)
  double *z, *y, *t, *t2, *l, *u, *rho, *zt, *dy;     // m x W
  double *part, *parti, *sc, *rec;                    // [kLsSlots][G][W] partials, [tiles of m][W], [kLsScal][W] scalar state, [W][kBatchRec] records
  int *iw, *word;                                     // [kLsInt][W] integer state; the word block the host reads is its last row
  int G;
};
struct LsAdjWs { double *ax, *gdx, *rx, *ay, *gdy, *ry; int *code; };     // adjoint: x, dx, r_x (n), y, dy, r_y (m), the row codes (m ints)
struct LsPolWs { double *x, *y, *z, *l, *u; };                            // polish: the scaled ADMM x (n) and y, z, l, u (m)
struct LwVecs {                                                            // direct route
  double *S, *pg, *pg2, *h;             // [r][r][64] S, then S^-1;  [GC][r][64] partials of A_L v (two sets);  [r][64]
  int *fact;                            // [64] inversions of S per problem
};
struct LsMatVecs { double *Aval, *Bval, *D, *Dinv, *E, *Einv; };          // per-problem matrices: [nnz][W] values, n x W and m x W scalings
struct LwMatVecs { double *WT, *vval; };                                  // direct route with per-problem matrices: [n][r][W] dense rows, [nv][W] values of the view of A

// ---- the size functions (doubles; the closed forms include slack the carves do not use)
// a chunk's workspace: eight n- and nine m-block vectors, the partials, the per-problem state and records
inline size_t lockstep_ws_doubles(int n, int m) {
  return (size_t)kLsW * (8 * (size_t)n + 9 * (size_t)m + (size_t)kLsSlots * lockstep_grid(n, m) + (size_t)(m + 63) / 64 + 1 + kLsScal + kBatchRec + kLsInt) + 64;
}
// the matrix block of a chunk with per-problem matrices: both value arrays, D, Dinv, E, Einv
inline size_t lockstep_mat_ws_doubles(int n, int m, int nzA, int nzB) { return (size_t)kLsW * ((size_t)nzA + (size_t)nzB + 2 * (size_t)n + 2 * (size_t)m) + 64; }
// the polish work block: the scaled ADMM x (n) and y, z, l, u (m) of every problem of the chunk
inline size_t lockstep_polish_ws_doubles(int n, int m) { return (size_t)kLsW * ((size_t)n + 4 * (size_t)m) + 64; }
// the adjoint's work block: the forward's set, then x, dx, r_x (n), y, dy, r_y (m) and the row codes (m ints)
inline size_t lockstep_adjoint_ws_doubles(int n, int m) {
  return lockstep_ws_doubles(n, m) + (size_t)kLsW * (3 * (size_t)n + 3 * (size_t)m + ((size_t)m + 1) / 2) + 64;
}
// the direct route's workspace: x, x~, dx with n + r rows, four n- and nine m-block vectors, the partials and state of the lockstep route, then S
// (r x r per problem), two sets of column-block partials, h, the inversion counts
inline size_t lockstep_direct_ws_doubles(int n, int m, int r) {
  const size_t gc = (size_t)lockstep_direct_colblocks(n);
  return (size_t)kLsW * (3 * ((size_t)n + r) + 4 * (size_t)n + 9 * (size_t)m + (size_t)kLsSlots * lockstep_grid(n, m) + (size_t)(m + 63) / 64 + 1 + kLsScal + kBatchRec + kLsInt +
                         (size_t)r * r + 2 * gc * r + r + 1) + 64;
}
// its adjoint's: the direct forward's set, then the adjoint's own vectors
inline size_t lockstep_direct_adjoint_ws_doubles(int n, int m, int r) {
  return lockstep_direct_ws_doubles(n, m, r) + (size_t)kLsW * (3 * (size_t)n + 3 * (size_t)m + ((size_t)m + 1) / 2) + 64;
}

// the direct route's block with per-problem matrices: the matrix block, then the chunk's own dense rows (entry (column j, long row a) of problem b at
// ((j r + a) W + b), zero where A_L has no entry) and the values of the view of A (nv entries: the one-entry rows' and 1.0 per long row)
inline size_t lockstep_direct_mat_ws_doubles(int n, int m, int r, int nzA, int nzB, int nv) {
  return lockstep_mat_ws_doubles(n, m, nzA, nzB) + (size_t)kLsW * ((size_t)n * r + (size_t)nv) + 64;
}

// ---- the carves
// Consecutive ranges of doubles from `base`.  base == nullptr is the COUNTING cursor: take() hands out nullptr, touches nothing, and `off` is the answer.
// log (layout test): receives (offset, doubles) of every range taken.
struct LsCursor {
  double *base = nullptr;
  size_t off = 0;
  size_t *log = nullptr; int nlog = 0;
  double *take(size_t cnt) {
    if (log) { log[2 * nlog] = off; log[2 * nlog + 1] = cnt; nlog++; }
    double *p = base ? base + off : nullptr;
    off += cnt;
    return p;
  }
  int *take_ints(size_t ints) { return reinterpret_cast<int *>(take((ints + 1) / 2)); }
};
// The base set.  xrows: rows of x / x~ / dx (n; n + r on the direct route), kp: the PCG's Kp.  An m = 0 chunk still has one parti row (k_ls_init folds
// none, but the block keeps its place).  Returns where the scalar state starts.
inline size_t lockstep_carve_base(LsCursor &c, LsWs &w, int n, int m, int xrows, bool kp) {
  const size_t W = kLsW, nW = (size_t)n * W, mW = (size_t)m * W, xW = (size_t)xrows * W, tm = ((size_t)m + 63) / 64;
  w.G = lockstep_grid(n, m);
  w.x = c.take(xW); w.xs = c.take(xW); w.dx = c.take(xW);
  w.r = c.take(nW); w.p = c.take(nW); w.Kp = kp ? c.take(nW) : nullptr; w.q = c.take(nW); w.Minv = c.take(nW);
  w.z = c.take(mW); w.y = c.take(mW); w.t = c.take(mW); w.t2 = c.take(mW); w.l = c.take(mW); w.u = c.take(mW); w.rho = c.take(mW); w.zt = c.take(mW); w.dy = c.take(mW);
  w.part = c.take((size_t)kLsSlots * w.G * W); w.parti = c.take((tm > 0 ? tm : 1) * W);
  const size_t sc = c.off;
  w.sc = c.take((size_t)kLsScal * W); w.rec = c.take(W * kBatchRec);
  w.iw = c.take_ints((size_t)kLsInt * W); w.word = w.iw ? w.iw + (size_t)(kLsInt - 1) * W : nullptr;
  return sc;
}
inline void lockstep_carve_adjoint(LsCursor &c, LsAdjWs &a, int n, int m) {
  const size_t nW = (size_t)n * kLsW, mW = (size_t)m * kLsW;
  a.ax = c.take(nW); a.gdx = c.take(nW); a.rx = c.take(nW); a.ay = c.take(mW); a.gdy = c.take(mW); a.ry = c.take(mW); a.code = c.take_ints(mW);
}
inline void lockstep_carve_direct(LsCursor &c, LwVecs &d, int n, int r) {
  const size_t W = kLsW, gc = (size_t)lockstep_direct_colblocks(n);
  d.S = c.take((size_t)r * r * W); d.pg = c.take(gc * r * W); d.pg2 = c.take(gc * r * W); d.h = c.take((size_t)r * W); d.fact = c.take_ints(W);
}
inline void lockstep_carve_polish(LsCursor &c, LsPolWs &s, int n, int m) {
  const size_t nW = (size_t)n * kLsW, mW = (size_t)m * kLsW;
  s.x = c.take(nW); s.y = c.take(mW); s.z = c.take(mW); s.l = c.take(mW); s.u = c.take(mW);
}
inline void lockstep_carve_mat(LsCursor &c, LsMatVecs &t, int n, int m, int nzA, int nzB) {
  const size_t W = kLsW, nW = (size_t)n * W, mW = (size_t)m * W;
  t.Aval = c.take((size_t)nzA * W); t.Bval = c.take((size_t)nzB * W); t.D = c.take(nW); t.Dinv = c.take(nW); t.E = c.take(mW); t.Einv = c.take(mW);
}

// ---- the work blocks as the drivers carve them.  Each answers whether its carve FITS its size function: a driver asks before it creates an event or
// enqueues anything.  a != nullptr: the adjoint's vectors follow the forward's block (they start at the forward's size function).
inline bool lockstep_layout(LsCursor &c, int n, int m, LsWs &w, LsAdjWs *a) {
  lockstep_carve_base(c, w, n, m, n, true);
  if (c.off > lockstep_ws_doubles(n, m)) return false;
  if (!a) return true;
  c.off = lockstep_ws_doubles(n, m);
  lockstep_carve_adjoint(c, *a, n, m);
  return c.off <= lockstep_adjoint_ws_doubles(n, m);
}
inline bool lockstep_direct_layout(LsCursor &c, int n, int m, int r, LsWs &w, LwVecs &d, LsAdjWs *a) {
  lockstep_carve_base(c, w, n, m, n + r, false);
  lockstep_carve_direct(c, d, n, r);
  if (c.off > lockstep_direct_ws_doubles(n, m, r)) return false;
  if (!a) return true;
  c.off = lockstep_direct_ws_doubles(n, m, r);
  lockstep_carve_adjoint(c, *a, n, m);
  return c.off <= lockstep_direct_adjoint_ws_doubles(n, m, r);
}
inline bool lockstep_polish_layout(LsCursor &c, int n, int m, LsPolWs &s) { lockstep_carve_polish(c, s, n, m); return c.off <= lockstep_polish_ws_doubles(n, m); }
inline bool lockstep_mat_layout(LsCursor &c, int n, int m, int nzA, int nzB, LsMatVecs &t) {
  lockstep_carve_mat(c, t, n, m, nzA, nzB);
  return c.off <= lockstep_mat_ws_doubles(n, m, nzA, nzB);
}
// (the matrix block comes first and sits where lockstep_mat_layout puts it: ls_mat_block carves it from the same base)
inline bool lockstep_direct_mat_layout(LsCursor &c, int n, int m, int r, int nzA, int nzB, int nv, LsMatVecs &t, LwMatVecs &d) {
  lockstep_carve_mat(c, t, n, m, nzA, nzB);
  d.WT = c.take((size_t)n * r * kLsW); d.vval = c.take((size_t)nv * kLsW);
  return c.off <= lockstep_direct_mat_ws_doubles(n, m, r, nzA, nzB, nv);
}
// where the per-problem scalar state sits in a chunk's workspace: the counting carve's answer
inline size_t lockstep_sc_offset(int n, int m) { LsCursor c; LsWs w; return lockstep_carve_base(c, w, n, m, n, true); }

}  // namespace osqp_hip
