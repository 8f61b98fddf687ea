// lockstep_hip.hip -- the LOCKSTEP batch route (include/osqp_hip.h osqp_hip_batch_solve_lockstep; engine_api.cpp Engine::batch_solve_lockstep):
// a batch of QPs that share this handle's P, A, scaling and settings and differ in q / l / u (or, osqp_hip_batch_solve_lockstep_mat, have their own values of
// P and A on the handle's pattern and their own scaling: "matrices of a chunk"), at ANY size a handle can be set up for.  The two batch
// kernels of batch_hip.hip keep one problem in one workgroup's LDS; here the ADMM / PCG iteration of k_batch_admm's non-direct variants runs on BLOCK
// VECTORS instead: kLsW = 64 problems advance together, LANES ARE PROBLEMS.
//
//   layout      element (j, b) of a block vector sits at j * kLsW + b (problem-minor): every access of a wave is one contiguous 512-byte line.
//   products    Z = A X over the engine's scaled CSR of A, Y = B [X; T] over B = [P + sigma I | A'].  A wave owns a strip of rows and all 64 problems; a
//               row's column indices and values are wave-uniform (scalar loads / a broadcast), each stored entry is one 512-byte gather and 64 FMAs;
//               four entries are in flight per wave (indices, then gathers, then FMAs).  No atomics.
//   scalars     every dot product / max-norm is, per problem, a sum over rows: a lane accumulates over its wave's rows, the four waves of a workgroup
//               are combined in index order, the workgroup's partial goes to part[slot][workgroup][lane] and a one-workgroup fold kernel adds the
//               partials in index order.  alpha, beta, ||r||, the residual norms, rho ... live as [kLsW] device arrays.  The row partition and
//               the fold order depend on (n, m) alone -- never on the chunk's fill -- and no quantity of one problem enters another problem's
//               arithmetic: a problem's x, y and record are bit-identical whatever else is in the batch and wherever in it the problem sits.
//   freezing    a problem whose PCG has converged takes alpha = 0 and stores nothing; a problem whose ADMM has terminated stores nothing at all
//               (its record is written at that moment).  Lanes >= count are "terminated" from the start.
//   driving     per ADMM iteration the host enqueues the PCG iterations (six launches each) the previous one needed, plus one, without synchronising,
//               reads the word block, and goes on in groups of four up to cg_max_iter while the device word "some problem's PCG is still running"
//               is set; that word makes the launches past the last problem's convergence return at once (ls_pcg).  Termination, the infeasibility
//               tests, the statuses at max_iter and adaptive rho are decided per problem on the device (k_ls_decide: k_batch_admm's formulas, cited
//               there); the host reads one small word block per termination check.  The host side is written once -- "driving" in front of the chunk
//               functions: LsRun (stream, launches, words, events), LsPcgKernels (the kernels on the handle's or the chunk's own matrices), ls_pcg,
//               ls_recurrence (polish and both adjoints), LwRun (the direct route's argument views and launch groups) -- and each of the four chunk
//               functions is its own sequence over these.  Where the work blocks' vectors sit: lockstep_layout.h, one carve per pointer set.
// Transposes (LDS tiles, coalesced on both sides) move a chunk between the API's [nbatch][n] row-major arrays and the block vectors; they apply
// k_batch_admm's load / store scaling and, for a handle that works on a permuted copy, gather / scatter through the permutations.
// The BACKWARD pass of a chunk (osqp_hip_batch_adjoint_lockstep; lockstep_adjoint_chunk below): the adjoint system of every problem by the recurrence polish
// and the single-QP adjoint run, which is this file's iteration with alpha = 1 and a fixed rho -- see "adjoint derivatives of a chunk"; with matrices of
// the chunk's own (osqp_hip_batch_adjoint_lockstep_mat) the same pass behind the forward's assembly and equilibration, on the k_lsm_* instantiations.
// POLISH (settings.polishing): the chunk's SOLVED problems are polished by that same recurrence between the ADMM loop and the transposes out -- see
// "polish of a chunk".  With per-problem matrices it runs on the chunk's own matrix block.  The DIRECT route (Woodbury handles, "lockstep DIRECT") polishes by
// the same kernels with its own solve in place of the PCG: lockstep_direct_chunk.
#include "hip_common.h"

namespace osqp_hip {
namespace be {

namespace {

constexpr int W = kLsW;
constexpr int kLsPolMaxSteps = 30;               // Engine::polish's RecurrenceRule{false, 0.5, 30}

// partial slots (part[slot][workgroup][lane]); within a group the max-type slots come first
enum LsSlot {
  PS_BN = 0, PS_RN, PS_RZ, PS_PKP,
  PS_M0,                         // m side, max: pri_u ax_u z_u pri_s ax_s z_s dy_u dy_s adx_max -adx_min ; sum: pinf_lhs
  PS_N0 = PS_M0 + 11,            // n side, max: dua_u px_u aty_u dua_s px_s aty_s dx_u dx_s qn_s qn_u atdy_u atdy_s pdx_u pdx_s ; sum: xpx qx qdx
  PS_COUNT = PS_N0 + 17
};
static_assert(PS_COUNT <= kLsSlots, "lockstep_ws_doubles reserves kLsSlots partial slots");
enum LsScal { SC_RHOBAR = 0, SC_EQF, SC_EPSCG, SC_EPSPREV, SC_RZ, SC_RN, SC_TOL, SC_ALPHA, SC_BETA, SC_BEST /* adjoint: smallest error so far */, SC_NACT /* adjoint: active rows */,
              SC_C /* per-problem matrices: the problem's cost scale c, 1 / c, this pass's factor */, SC_CINV, SC_CT, SC_COUNT };
enum LsInt { IW_DONE = 0, IW_STATUS, IW_RHOUPD, IW_PCG, IW_RELRULE, IW_CGON, IW_RHOCH, IW_STEPS /* adjoint: recurrence steps */, IW_WORSE /* adjoint: steps in a row without progress */,
             IW_SIDE /* direct route: single_rho_rule's side at the previous adaptation point */, IW_POL /* polish: 1 attempted, 2 attempted and rejected */, IW_COUNT };
enum LsWord { WD_CGANY = 0, WD_LIVE, WD_RHOANY, WD_PCGSUM, WD_CGIT /* PCG iterations of the current ADMM iteration that some problem needed */,
              WD_POLACC /* polish: problems accepted */, WD_POLREJ /* rejected */, WD_COUNT };
static_assert(SC_C == kLsMatScalC, "Engine::lockstep_mat_scaling reads c from this row");
static_assert(SC_COUNT <= kLsScal && IW_COUNT + 1 == kLsInt, "lockstep_layout.h reserves kLsScal / kLsInt rows; the word block is the last int row");

// (LsWs and the other pointer sets: lockstep_layout.h, with their carves)
struct LsK { LockstepParams P; LsWs w; };

__device__ __forceinline__ int ls_lane() { return threadIdx.x & 63; }
__device__ __forceinline__ int ls_wave() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// the four waves' values of KM max-type and KS sum-type statistics, combined in wave order, to the workgroup's partials
template <int KM, int KS>
__device__ __forceinline__ void ls_put(double *part, int slot0, const double *vm, const double *vs, double *lds) {
  const int lane = ls_lane(), wv = ls_wave(), G = gridDim.x;
#pragma unroll
  for (int k = 0; k < KM; k++) lds[(k * 4 + wv) * 64 + lane] = vm[k];
#pragma unroll
  for (int k = 0; k < KS; k++) lds[((KM + k) * 4 + wv) * 64 + lane] = vs[k];
  __syncthreads();
  for (int k = wv; k < KM + KS; k += 4) {
    const double *s = lds + k * 256 + lane;
    double v;
    if (k < KM) { v = nanmax(s[0], s[64]); v = nanmax(v, s[128]); v = nanmax(v, s[192]); }
    else v = ((s[0] + s[64]) + s[128]) + s[192];
    part[((size_t)(slot0 + k) * G + blockIdx.x) * 64 + lane] = v;
  }
}
// sum / max of a slot's G partials in a fixed order: wave w takes g = w, w + 4, ..; the four results are combined in wave order.  One workgroup.
template <bool MAX>
__device__ __forceinline__ double ls_fold(const double *part, int G, int slot, double *lds) {
  const int lane = ls_lane(), wv = ls_wave();
  const double *s = part + (size_t)slot * G * 64 + lane;
  double a = MAX ? -INFINITY : 0.0;
  for (int g = wv; g < G; g += 4) { const double v = s[(size_t)g * 64]; a = MAX ? nanmax(a, v) : a + v; }
  lds[wv * 64 + lane] = a;
  __syncthreads();
  double v;
  if (MAX) { v = nanmax(lds[lane], lds[64 + lane]); v = nanmax(v, lds[128 + lane]); v = nanmax(v, lds[192 + lane]); }
  else v = ((lds[lane] + lds[64 + lane]) + lds[128 + lane]) + lds[192 + lane];
  __syncthreads();
  return v;
}

// ---------------------------------------------------------------------------------------------------------------- row passes
// Rows [r0, r1) of M belong to this wave (the partition depends on the row count and the grid alone).  F: begin(row); load(c, g) issues the gathers
// of one entry; fma(c, v, g, acc) adds it; row(row, acc) is the epilogue.  Everything about an entry but the gathered operands is wave-uniform.
// MAT (per-problem matrices, "matrices of a chunk" below): M.val is a block, entry k of problem b at k * 64 + b -- the value is one more 512-byte line per
// entry, loaded with the column indices ahead of the gathers, in place of a broadcast.
template <int NG, int NA, bool MAT = false, class F>
__device__ __forceinline__ void ls_rows(const DevCsr &M, F &f) {
  const int nw = gridDim.x * 4, rpw = (M.nrows + nw - 1) / nw;
  const int r0 = ((int)blockIdx.x * 4 + ls_wave()) * rpw, r1 = min(r0 + rpw, M.nrows);
  const int *__restrict__ rp = M.rowptr, *__restrict__ col = M.col;
  const double *__restrict__ val = MAT ? M.val + ls_lane() : M.val;
  for (int row = r0; row < r1; row++) {
    int k = __builtin_amdgcn_readfirstlane(rp[row]);
    const int k1 = __builtin_amdgcn_readfirstlane(rp[row + 1]);
    double acc[NA];
#pragma unroll
    for (int a = 0; a < NA; a++) acc[a] = 0.0;
    f.begin(row);
    for (; k + 4 <= k1; k += 4) {
      int c[4]; double v[4], g[4][NG];
#pragma unroll
      for (int u = 0; u < 4; u++) { c[u] = __builtin_amdgcn_readfirstlane(col[k + u]); v[u] = MAT ? val[(size_t)(k + u) * 64] : val[k + u]; }
#pragma unroll
      for (int u = 0; u < 4; u++) f.load(c[u], g[u]);
#pragma unroll
      for (int u = 0; u < 4; u++) f.fma(c[u], v[u], g[u], acc);
    }
    for (; k < k1; k++) {
      const int c = __builtin_amdgcn_readfirstlane(col[k]); const double v = MAT ? val[(size_t)k * 64] : val[k];
      double g[NG];
      f.load(c, g); f.fma(c, v, g, acc);
    }
    f.row(row, acc);
  }
}
#define IX(j) ((size_t)(j) * 64 + lane)
// a scaling D / Dinv / E / Einv: the handle's vector, or (MAT) the problem's own column of a block
template <bool MAT> __device__ __forceinline__ double ls_sv(const double *v, int j, int lane) { return MAT ? v[IX(j)] : v[j]; }
// a kernel body with and without per-problem matrices: NAME the shared route's kernel, k_lsm_NAME the other
#define LS_KERNEL_PAIR_OF(ARG, NAME) \
  __global__ __launch_bounds__(256) void k_ls_##NAME(ARG k) { ls_##NAME<false>(k); } \
  __global__ __launch_bounds__(256) void k_lsm_##NAME(ARG k) { ls_##NAME<true>(k); }
#define LS_KERNEL_PAIR(NAME) LS_KERNEL_PAIR_OF(LsK, NAME)

// Minv = 1 / diag(K_b) = 1 / (B_jj + sum_i rho_i,b A_ij^2), for the problems whose rho has just been set (one pass over the A' part of B, squared entries)
struct FMinv {
  const double *rho; double *Minv; const int *flag; int n, precond, lane, cur;
  __device__ __forceinline__ void begin(int row) { cur = row; }
  __device__ __forceinline__ void load(int c, double (&g)[1]) const { g[0] = c >= n ? rho[IX(c - n)] : 0.0; }
  __device__ __forceinline__ void fma(int c, double v, const double (&g)[1], double (&a)[2]) const { if (c >= n) a[0] += g[0] * v * v; else if (c == cur) a[1] = v; }
  __device__ __forceinline__ void row(int j, const double (&a)[2]) const { if (flag[lane]) Minv[IX(j)] = precond ? 1.0 / (a[1] + a[0]) : 1.0; }
};
template <bool MAT> __device__ __forceinline__ void ls_minv(const LsK &k) {
  if (!k.w.word[WD_RHOANY]) return;
  FMinv f{k.w.rho, k.w.Minv, k.w.iw + IW_RHOCH * W, k.P.n, k.P.precond, ls_lane(), 0};
  ls_rows<1, 2, MAT>(k.P.B, f);
}
LS_KERNEL_PAIR(minv)

// rhs = sigma x - q + A'(rho z - y);  r = rhs - K x~ with K x~ = B [x~; rho z~];  p = Minv r   (k_batch_admm: "rhs = ...", _osqp.py:649-650)
struct FRhs {
  const LsWs &w; double sigma; int n, lane, live;
  double bn = 0, rn = 0, rz = 0;
  __device__ __forceinline__ void begin(int) {}
  __device__ __forceinline__ void load(int c, double (&g)[2]) const {
    if (c < n) { g[0] = w.xs[IX(c)]; g[1] = 0.0; } else { g[0] = w.t[IX(c - n)]; g[1] = w.t2[IX(c - n)]; }
  }
  __device__ __forceinline__ void fma(int c, double v, const double (&g)[2], double (&a)[2]) const {
    if (c < n) a[1] += v * g[0]; else { a[0] += v * g[0]; a[1] += v * g[1]; }
  }
  __device__ __forceinline__ void row(int j, const double (&a)[2]) {
    const double rhs = sigma * w.x[IX(j)] - w.q[IX(j)] + a[0], rr = rhs - a[1], zz = w.Minv[IX(j)] * rr;
    if (live) { w.r[IX(j)] = rr; w.p[IX(j)] = zz; }
    rz += rr * zz; rn = nanmax(rn, fabs(rr)); bn = nanmax(bn, fabs(rhs));
  }
};
template <bool MAT> __device__ __forceinline__ void ls_rhs(const LsK &k) {
  __shared__ double lds[3 * 256];
  const int lane = ls_lane();
  FRhs f{k.w, k.P.sigma, k.P.n, lane, !k.w.iw[IW_DONE * W + lane]};
  ls_rows<2, 2, MAT>(k.P.B, f);
  const double vm[2] = {f.bn, f.rn}, vs[1] = {f.rz};
  ls_put<2, 1>(k.w.part, PS_BN, vm, vs, lds);
}
LS_KERNEL_PAIR(rhs)

// Kp = B [p; t],  <p, Kp>
struct FKp {
  const LsWs &w; int n, lane, on;
  double pkp = 0;
  __device__ __forceinline__ void begin(int) {}
  __device__ __forceinline__ void load(int c, double (&g)[1]) const { g[0] = c < n ? w.p[IX(c)] : w.t[IX(c - n)]; }
  __device__ __forceinline__ void fma(int, double v, const double (&g)[1], double (&a)[1]) const { a[0] += v * g[0]; }
  __device__ __forceinline__ void row(int j, const double (&a)[1]) { if (on) w.Kp[IX(j)] = a[0]; pkp += a[0] * w.p[IX(j)]; }
};
template <bool MAT> __device__ __forceinline__ void ls_kp(const LsK &k) {
  __shared__ double lds[256];
  if (!k.w.word[WD_CGANY]) return;
  const int lane = ls_lane();
  FKp f{k.w, k.P.n, lane, k.w.iw[IW_CGON * W + lane]};
  ls_rows<1, 1, MAT>(k.P.B, f);
  const double vs[1] = {f.pkp};
  ls_put<0, 1>(k.w.part, PS_PKP, vs, vs, lds);
}
LS_KERNEL_PAIR(kp)

// the n side of k_batch_admm's residuals(), with the second stage of both infeasibility tests (A' dy, P dx) from the same pass
template <bool MAT> struct FResN {
  const LsWs &w; const double *D, *Dinv; double sigma; int n, lane;
  ResRowsB rb = {};                                                           // (step_rules.h: named fields)
  double atdy_u = 0, atdy_s = 0, pdx_u = 0, pdx_s = 0;                        // second stages
  __device__ __forceinline__ void begin(int) {}
  __device__ __forceinline__ void load(int c, double (&g)[2]) const {
    if (c < n) { g[0] = w.x[IX(c)]; g[1] = w.dx[IX(c)]; } else { g[0] = w.y[IX(c - n)]; g[1] = w.dy[IX(c - n)]; }
  }
  __device__ __forceinline__ void fma(int c, double v, const double (&g)[2], double (&a)[4]) const {
    const double p0 = v * g[0], p1 = v * g[1]; const bool pn = c < n;       // (selects, not indexed accumulators: those would live in scratch)
    a[0] += pn ? p0 : 0.0; a[2] += pn ? p1 : 0.0; a[1] += pn ? 0.0 : p0; a[3] += pn ? 0.0 : p1;
  }
  __device__ __forceinline__ void row(int j, const double (&a)[4]) {
    const double dxj = w.dx[IX(j)], di = ls_sv<MAT>(Dinv, j, lane);
    res_row_b(rb, a[0], a[1], sigma, w.x[IX(j)], w.q[IX(j)], dxj, ls_sv<MAT>(D, j, lane), di);
    const double pdx = a[2] - sigma * dxj, atdy = a[3];
    atdy_u = nanmax(atdy_u, fabs(di * atdy)); atdy_s = nanmax(atdy_s, fabs(atdy)); pdx_u = nanmax(pdx_u, fabs(di * pdx)); pdx_s = nanmax(pdx_s, fabs(pdx));
  }
};
template <bool MAT> __device__ __forceinline__ void ls_resn(const LsK &k) {
  __shared__ double lds[17 * 256];
  FResN<MAT> f{k.w, k.P.D, k.P.Dinv, k.P.sigma, k.P.n, ls_lane()};
  ls_rows<2, 4, MAT>(k.P.B, f);
  const ResRowsB &b = f.rb;                                                   // (the slot order of PS_N0)
  const double vm[14] = {b.dua_u, b.px_u, b.aty_u, b.dua_s, b.px_s, b.aty_s, b.dxn_u, b.dxn_s, b.qn_s, b.qn_u, f.atdy_u, f.atdy_s, f.pdx_u, f.pdx_s}, vs[3] = {b.xpx, b.qx, b.qdx};
  ls_put<14, 3>(k.w.part, PS_N0, vm, vs, lds);
}
LS_KERNEL_PAIR(resn)

// z = z~ = A x at the start;  t = rho z - y,  t2 = rho z~  (what the next k_ls_rhs gathers)
struct FInitZ {
  const LsWs &w; int lane;
  __device__ __forceinline__ void begin(int) {}
  __device__ __forceinline__ void load(int c, double (&g)[1]) const { g[0] = w.x[IX(c)]; }
  __device__ __forceinline__ void fma(int, double v, const double (&g)[1], double (&a)[1]) const { a[0] += v * g[0]; }
  __device__ __forceinline__ void row(int i, const double (&a)[1]) const {
    const double rh = w.rho[IX(i)];
    w.z[IX(i)] = a[0]; w.zt[IX(i)] = a[0]; w.t[IX(i)] = rh * a[0] - w.y[IX(i)]; w.t2[IX(i)] = rh * a[0];
  }
};
template <bool MAT> __device__ __forceinline__ void ls_initz(const LsK &k) {
  FInitZ f{k.w, ls_lane()};
  ls_rows<1, 1, MAT>(k.P.A, f);
}
LS_KERNEL_PAIR(initz)

// t = rho .* (A p)
struct FT {
  const LsWs &w; int lane, on;
  __device__ __forceinline__ void begin(int) {}
  __device__ __forceinline__ void load(int c, double (&g)[1]) const { g[0] = w.p[IX(c)]; }
  __device__ __forceinline__ void fma(int, double v, const double (&g)[1], double (&a)[1]) const { a[0] += v * g[0]; }
  __device__ __forceinline__ void row(int i, const double (&a)[1]) const { if (on) w.t[IX(i)] = w.rho[IX(i)] * a[0]; }
};
template <bool MAT> __device__ __forceinline__ void ls_t(const LsK &k) {
  if (!k.w.word[WD_CGANY]) return;
  const int lane = ls_lane();
  FT f{k.w, lane, k.w.iw[IW_CGON * W + lane]};
  ls_rows<1, 1, MAT>(k.P.A, f);
}
LS_KERNEL_PAIR(t)

// z~ = A x~;  z, y update (_osqp.py:660-703);  and, elementwise,  x = alpha x~ + (1 - alpha) x,  dx
struct FUpd {
  const LsWs &w; double alpha; int lane, live;
  __device__ __forceinline__ void begin(int) {}
  __device__ __forceinline__ void load(int c, double (&g)[1]) const { g[0] = w.xs[IX(c)]; }
  __device__ __forceinline__ void fma(int, double v, const double (&g)[1], double (&a)[1]) const { a[0] += v * g[0]; }
  __device__ __forceinline__ void row(int i, const double (&acc)[1]) const {
    if (!live) return;
    const double a = acc[0], rh = w.rho[IX(i)];
    const StepRow s = step_row(alpha, a, rh, w.z[IX(i)], w.y[IX(i)], w.l[IX(i)], w.u[IX(i)]);
    w.y[IX(i)] = s.y; w.dy[IX(i)] = s.dy; w.z[IX(i)] = s.z; w.zt[IX(i)] = a;
    w.t[IX(i)] = rh * s.z - s.y; w.t2[IX(i)] = rh * a;
  }
};
template <bool MAT> __device__ __forceinline__ void ls_upd(const LsK &k) {
  const int lane = ls_lane(), live = !k.w.iw[IW_DONE * W + lane];
  if (k.P.m > 0) { FUpd f{k.w, k.P.alpha, lane, live}; ls_rows<1, 1, MAT>(k.P.A, f); }
  if (!live) return;
  const size_t tot = (size_t)k.P.n * 64;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += (size_t)gridDim.x * 256) {
    const StepCol c = step_col(k.P.alpha, k.w.xs[e], k.w.x[e]);
    k.w.dx[e] = c.dx; k.w.x[e] = c.x;
  }
}
LS_KERNEL_PAIR(upd)

// the m side of residuals(), with A dx of the dual infeasibility test (largest value over the rows with a finite upper bound, largest negated value over
// those with a finite lower one: "no row violates" is two comparisons of these with the threshold, which only the fold knows)
template <bool MAT> struct FResM {
  const LsWs &w; const double *E, *Einv; int lane, unsc;
  ResRowsA ra = {};                                                           // (step_rules.h: named fields)
  double adx_hi = -INFINITY, adx_lo = -INFINITY;                              // second stage
  __device__ __forceinline__ void begin(int) {}
  __device__ __forceinline__ void load(int c, double (&g)[2]) const { g[0] = w.x[IX(c)]; g[1] = w.dx[IX(c)]; }
  __device__ __forceinline__ void fma(int, double v, const double (&g)[2], double (&a)[2]) const { a[0] += v * g[0]; a[1] += v * g[1]; }
  __device__ __forceinline__ void row(int i, const double (&a)[2]) {
    const double ei = ls_sv<MAT>(Einv, i, lane), li = w.l[IX(i)], ui = w.u[IX(i)];
    res_row_a(ra, a[0], w.z[IX(i)], w.dy[IX(i)], li, ui, ls_sv<MAT>(E, i, lane), ei);
    const double adx = unsc ? ei * a[1] : a[1];
    if (upper_is_finite(ui)) adx_hi = nanmax(adx_hi, adx);
    if (lower_is_finite(li)) adx_lo = nanmax(adx_lo, -adx);
  }
};
template <bool MAT> __device__ __forceinline__ void ls_resm(const LsK &k) {
  __shared__ double lds[11 * 256];
  FResM<MAT> f{k.w, k.P.E, k.P.Einv, ls_lane(), k.P.unscaled};
  ls_rows<2, 2, MAT>(k.P.A, f);
  const ResRowsA &a = f.ra;                                                   // (the slot order of PS_M0)
  const double vm[10] = {a.pri_u, a.ax_u, a.z_u, a.pri_s, a.ax_s, a.z_s, a.dy_u, a.dy_s, f.adx_hi, f.adx_lo}, vs[1] = {a.pinf_lhs};
  ls_put<10, 1>(k.w.part, PS_M0, vm, vs, lds);
}
LS_KERNEL_PAIR(resm)

// ---------------------------------------------------------------------------------------------------------------- elementwise kernels
// rho by constraint class and the problem's rho_bar (_osqp.py:520-522), for the problems whose rho has just been set; t, t2 follow
__global__ __launch_bounds__(256) void k_ls_setrho(LsK k) {
  if (!k.w.word[WD_RHOANY]) return;
  const int lane = ls_lane();
  if (!k.w.iw[IW_RHOCH * W + lane]) return;
  const double rb = k.w.sc[SC_RHOBAR * W + lane], eqf = k.w.sc[SC_EQF * W + lane];
  const size_t tot = (size_t)k.P.m * 64;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += (size_t)gridDim.x * 256) {
    const double rh = row_rho(row_class(k.w.l[e], k.w.u[e], k.P.rho_is_vec), rb, eqf * rb);
    k.w.rho[e] = rh; k.w.t[e] = rh * k.w.z[e] - k.w.y[e]; k.w.t2[e] = rh * k.w.zt[e];
  }
}

// x~ += alpha p;  r -= alpha Kp;  <r, Minv r>, ||r||_inf.   Wave w of workgroup g takes rows (4 g + w), + 4 G, ..: fixed by the grid
__global__ __launch_bounds__(256) void k_ls_cgupd(LsK k) {
  __shared__ double lds[2 * 256];
  if (!k.w.word[WD_CGANY]) return;
  const int lane = ls_lane(), on = k.w.iw[IW_CGON * W + lane];
  const double al = k.w.sc[SC_ALPHA * W + lane];
  double rz = 0, rn = 0;
  for (int j = (int)blockIdx.x * 4 + ls_wave(); j < k.P.n; j += (int)gridDim.x * 4) {
    if (on) {
      k.w.xs[IX(j)] += al * k.w.p[IX(j)];
      const double rr = k.w.r[IX(j)] - al * k.w.Kp[IX(j)], zz = k.w.Minv[IX(j)] * rr;
      k.w.r[IX(j)] = rr;
      rz += rr * zz; rn = nanmax(rn, fabs(rr));
    }
  }
  const double vm[1] = {rn}, vs[1] = {rz};
  ls_put<1, 1>(k.w.part, PS_RN, vm, vs, lds);
}
// p = Minv r + beta p  (for the problems whose PCG goes on)
__global__ __launch_bounds__(256) void k_ls_cgp(LsK k) {
  if (!k.w.word[WD_CGANY]) return;
  const int lane = ls_lane();
  if (!k.w.iw[IW_CGON * W + lane]) return;
  const double be = k.w.sc[SC_BETA * W + lane];
  const size_t tot = (size_t)k.P.n * 64;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += (size_t)gridDim.x * 256) k.w.p[e] = k.w.Minv[e] * k.w.r[e] + be * k.w.p[e];
}

// settings.check_dualgap: per problem the support function of the scaled box at y, sum_i support_finite(l_i, u_i, y_i) (step_rules.h; what backend_hip.hip
// reduces for R_SUPP), for the dual objective of the next decision (term_rules.h term_dual_obj).  Rows by wave like k_ls_cgupd: wave w of workgroup g
// takes rows (4 g + w), + 4 G, .. -- fixed by the grid --, a lane adds its own problem's terms in row order, ls_put combines the four waves.  The partials
// go to PS_PKP: written by k_ls_kp and read by k_ls_cgalpha inside a PCG solve only, and this kernel runs between an iteration's k_ls_upd and the
// decision (the direct route and polish's accept test: no PCG is running either).  l, u, y carry all m rows on the direct route too.  Launched only with
// the setting, in front of a decision that tests termination; it stores to PS_PKP alone.
constexpr int PS_SUPP = PS_PKP;
__global__ __launch_bounds__(256) void k_ls_supp(LsK k) {
  __shared__ double lds[256];
  const int lane = ls_lane();
  double sp = 0.0;
  for (int i = (int)blockIdx.x * 4 + ls_wave(); i < k.P.m; i += (int)gridDim.x * 4) sp += support_finite(k.w.l[IX(i)], k.w.u[IX(i)], k.w.y[IX(i)]);
  const double vs[1] = {sp};
  ls_put<0, 1>(k.w.part, PS_SUPP, vs, vs, lds);
}

// ---------------------------------------------------------------------------------------------------------------- folds (one workgroup each)
__device__ __forceinline__ void ls_any(int *word, int flag) {
  const unsigned long long bal = __ballot(flag);
  if (threadIdx.x == 0) *word = bal != 0ull;
}
// PCG start: <r, Minv r>, ||r||, ||rhs||;  the stopping threshold of k_batch_admm's PCG variants
__global__ __launch_bounds__(256) void k_ls_cginit(LsK k) {
  __shared__ double lds[256];
  const int lane = ls_lane(), G = k.w.G;
  const double bn = ls_fold<true>(k.w.part, G, PS_BN, lds), rn = ls_fold<true>(k.w.part, G, PS_RN, lds), rz = ls_fold<false>(k.w.part, G, PS_RZ, lds);
  if (threadIdx.x >= 64) return;
  const double eps_cg = k.w.sc[SC_EPSCG * W + lane];
  const double tol = k.P.pcg_rel > 0.0 ? fmax(k.P.pcg_rel * bn, 1e-15)                       // the recurrence's own threshold (be::set_pcg_tol as Engine::run_recurrence calls it)
                                      : (k.w.iw[IW_RELRULE * W + lane] ? fmax(0.1 * bn, 1e-13) : fmax(1e-14 * bn, eps_cg));
  const int on = !k.w.iw[IW_DONE * W + lane] && k.P.cg_max > 0 && rn > tol;
  k.w.sc[SC_RZ * W + lane] = rz; k.w.sc[SC_RN * W + lane] = rn; k.w.sc[SC_TOL * W + lane] = tol;
  k.w.iw[IW_CGON * W + lane] = on;
  ls_any(k.w.word + WD_CGANY, on);
  if (threadIdx.x == 0) k.w.word[WD_CGIT] = 0;
}
__global__ __launch_bounds__(256) void k_ls_cgalpha(LsK k) {
  __shared__ double lds[256];
  if (!k.w.word[WD_CGANY]) return;
  const int lane = ls_lane();
  const double pkp = ls_fold<false>(k.w.part, k.w.G, PS_PKP, lds);
  if (threadIdx.x >= 64) return;
  k.w.sc[SC_ALPHA * W + lane] = k.w.iw[IW_CGON * W + lane] ? k.w.sc[SC_RZ * W + lane] / pkp : 0.0;
}
__global__ __launch_bounds__(256) void k_ls_cgbeta(LsK k) {
  __shared__ double lds[256];
  if (!k.w.word[WD_CGANY]) return;
  const int lane = ls_lane(), G = k.w.G;
  const double rn2 = ls_fold<true>(k.w.part, G, PS_RN, lds), rz2 = ls_fold<false>(k.w.part, G, PS_RZ, lds);
  if (threadIdx.x >= 64) return;
  int on = k.w.iw[IW_CGON * W + lane];
  if (on) {
    k.w.sc[SC_BETA * W + lane] = rz2 / k.w.sc[SC_RZ * W + lane];
    k.w.sc[SC_RZ * W + lane] = rz2; k.w.sc[SC_RN * W + lane] = rn2;
    k.w.iw[IW_PCG * W + lane] += 1;
    on = rn2 > k.w.sc[SC_TOL * W + lane];
    k.w.iw[IW_CGON * W + lane] = on;
  }
  ls_any(k.w.word + WD_CGANY, on);
  if (threadIdx.x == 0) k.w.word[WD_CGIT] += 1;
}

// Every check_termination / adaptive_rho_interval iterations: the batch family's decisions (term_rules.h: batch_check, batch_rho_rule -- single_rho_rule on the direct route --, batch_tol_rule), per problem.
// mode 0: a boundary of the loop;  1: the residuals of the start (sets the first inner tolerance);  2: the time limit has passed.
template <bool MAT> __device__ __forceinline__ void ls_decide(const LsK &k, int iter, int at_check, int at_rho, int mode) {
  __shared__ double lds[256];
  const LockstepParams &P = k.P;
  const int lane = ls_lane(), G = k.w.G;
  // the slots as k_ls_resm / k_ls_resn put them (all 64 lanes of every wave fold: the barriers are uniform)
  auto mx = [&](int slot) { return ls_fold<true>(k.w.part, G, slot, lds); };
  auto sm = [&](int slot) { return ls_fold<false>(k.w.part, G, slot, lds); };
  constexpr int M0 = PS_M0, N0 = PS_N0;
  const ResRowsA ra = {mx(M0), mx(M0 + 1), mx(M0 + 2), mx(M0 + 3), mx(M0 + 4), mx(M0 + 5), mx(M0 + 6), mx(M0 + 7), sm(M0 + 10)};
  const double adx_hi = mx(M0 + 8), adx_lo = mx(M0 + 9);                                                                      // second stages: folded with the rest
  const ResRowsB rb = {mx(N0), mx(N0 + 1), mx(N0 + 2), mx(N0 + 3), mx(N0 + 4), mx(N0 + 5), mx(N0 + 6), mx(N0 + 7), mx(N0 + 8), mx(N0 + 9), sm(N0 + 14), sm(N0 + 15), sm(N0 + 16)};
  const double atdy_u = mx(N0 + 10), atdy_s = mx(N0 + 11), pdx_u = mx(N0 + 12), pdx_s = mx(N0 + 13);
  const bool gap_on = P.check_dualgap && at_check && mode != 1;                                                               // (uniform: so is the fold's barrier)
  const double supp = (gap_on && P.m > 0) ? sm(PS_SUPP) : 0.0;                                                                // (k_ls_supp, launched in front of this decision)
  if (threadIdx.x >= 64) return;
  int *iw = k.w.iw; double *sc = k.w.sc;
  const int done = iw[IW_DONE * W + lane];
  int rhoch = 0;
  if (!done) {
    TermRes R;
    res_store(R, ra, rb);
    double eps_prev, eps_cg;
    bool rel_rule;
    auto put_tol = [&]() { sc[SC_EPSPREV * W + lane] = eps_prev; sc[SC_EPSCG * W + lane] = eps_cg; iw[IW_RELRULE * W + lane] = rel_rule; };
    if (mode == 1) { batch_tol_init(P.cg_frac, R.dua_s, &eps_prev, &eps_cg, &rel_rule); put_tol(); }
    else {
      const TermSet tset = {P.eps_abs, P.eps_rel, P.eps_pinf, P.eps_dinf, MAT ? sc[SC_C * W + lane] : P.c, MAT ? sc[SC_CINV * W + lane] : P.cinv, P.m, P.unscaled, P.scaling};
      const double rho_bar = sc[SC_RHOBAR * W + lane];
      double obj, prim_res, dual_res, rho_new;
      term_info(tset, R, &obj, &prim_res, &dual_res);
      const double dual_obj = gap_on ? term_dual_obj(tset, R, supp) : 0.0, gap = gap_on ? obj - dual_obj : 0.0;               // (check_dualgap: the ADMM point's)
      int status = batch_check_gap(tset, R, prim_res, dual_res, iter, P.max_iter, at_check != 0,
                                   [&](double &au, double &as) { au = atdy_u; as = atdy_s; }, [&](double &pu, double &ps) { pu = pdx_u; ps = pdx_s; },
                                   [&](double thr) { return !(adx_hi > thr) && !(adx_lo > thr); }, &obj, gap_on, dual_obj, gap);
      if (status == kBatchGoOn && mode == 2) status = OSQP_TIME_LIMIT_REACHED;
      const bool single = P.rho_tol_single > 0.0;                                            // (the direct route: the rule of the handle's own solve)
      bool rho_big = single ? false : batch_rho_rule(rho_bar, P.rho_tol, R, &rho_new);       // (rho_new: also the record's rho estimate)
      if (single) {                                                                          // (its side is that of the last adaptation point the problem went on from)
        int side = iw[IW_SIDE * W + lane];
        if (at_rho && status == kBatchGoOn) { rho_big = single_rho_rule(rho_bar, P.rho_tol_single, P.rho_persist, R, &side, &rho_new); iw[IW_SIDE * W + lane] = side; }
        else rho_new = term_rho_estimate(rho_bar, R);
      }
      if (status != kBatchGoOn) {
        batch_record(k.w.rec + (size_t)lane * kBatchRec, status, iter, obj, prim_res, dual_res, rho_bar, iw[IW_RHOUPD * W + lane], iw[IW_PCG * W + lane], rho_new);
        if (gap_on) batch_record_gap(k.w.rec + (size_t)lane * kBatchRec, status, gap);
        iw[IW_DONE * W + lane] = 1; iw[IW_STATUS * W + lane] = status;
      } else {
        if (at_rho && rho_big) { sc[SC_RHOBAR * W + lane] = rho_new; iw[IW_RHOUPD * W + lane] += 1; rhoch = 1; }
        eps_prev = sc[SC_EPSPREV * W + lane]; eps_cg = sc[SC_EPSCG * W + lane]; rel_rule = iw[IW_RELRULE * W + lane] != 0;
        batch_tol_rule(P.cg_frac, R.dua_s, &eps_prev, &eps_cg, &rel_rule);
        put_tol();
      }
    }
  }
  iw[IW_RHOCH * W + lane] = rhoch;
  const unsigned long long live = __ballot(!iw[IW_DONE * W + lane]), chg = __ballot(rhoch);
  int pcg = iw[IW_PCG * W + lane];                      // (statistics only: the sum over the chunk's problems)
  for (int o = 32; o > 0; o >>= 1) pcg += __shfl_xor(pcg, o);
  if (threadIdx.x == 0) { k.w.word[WD_LIVE] = __popcll(live); k.w.word[WD_RHOANY] = chg != 0ull; k.w.word[WD_PCGSUM] = pcg; }
}
__global__ __launch_bounds__(256) void k_ls_decide(LsK k, int iter, int at_check, int at_rho, int mode) { ls_decide<false>(k, iter, at_check, at_rho, mode); }
__global__ __launch_bounds__(256) void k_lsm_decide(LsK k, int iter, int at_check, int at_rho, int mode) { ls_decide<true>(k, iter, at_check, at_rho, mode); }

// ---------------------------------------------------------------------------------------------------------------- transposes
// tile[b][jl] <- src[b][perm(j0 + jl)] for the chunk's problems (coalesced along j without a permutation), zero elsewhere
__device__ __forceinline__ void ls_tile_in(const double *src, int width, int j0, int count, const int *perm, double (*tile)[65]) {
  const int lane = ls_lane(), wv = ls_wave(), j = j0 + lane;
  const int sj = j < width ? (perm ? perm[j] : j) : 0;
  for (int b = wv; b < 64; b += 4) tile[b][lane] = (b < count && j < width) ? src[(size_t)b * width + sj] : 0.0;
  __syncthreads();
}
__device__ __forceinline__ void ls_tile_out(double *dst, int width, int j0, int count, const int *perm, double (*tile)[65]) {
  const int lane = ls_lane(), wv = ls_wave(), j = j0 + lane;
  __syncthreads();
  if (j < width) {
    const int sj = perm ? perm[j] : j;
    for (int b = wv; b < count; b += 4) dst[(size_t)b * width + sj] = tile[b][lane];
  }
  __syncthreads();
}

// q <- c D q,  x <- Dinv x (warm) or 0,  x~ = x,  dx = 0   (k_batch_admm "load the problem")
template <bool MAT> __device__ __forceinline__ void ls_load_n(const LsK &k) {
  __shared__ double tile[64][65];
  const LockstepParams &P = k.P;
  const int lane = ls_lane(), wv = ls_wave(), j0 = blockIdx.x * 64;
  const bool mine = lane < P.count;
  if (P.q) ls_tile_in(P.q, P.n, j0, P.count, P.pc, tile);
  for (int jl = wv; jl < 64 && j0 + jl < P.n; jl += 4) {
    const int j = j0 + jl;
    const double qv = P.q ? tile[lane][jl] : P.q0[j];
    k.w.q[IX(j)] = mine ? in_q(MAT ? k.w.sc[SC_C * W + lane] : P.c, ls_sv<MAT>(P.D, j, lane), qv) : 0.0;
  }
  __syncthreads();
  if (P.warm) ls_tile_in(P.x, P.n, j0, P.count, P.pc, tile);
  for (int jl = wv; jl < 64 && j0 + jl < P.n; jl += 4) {
    const int j = j0 + jl;
    const double xv = (P.warm && mine) ? in_x(tile[lane][jl], ls_sv<MAT>(P.Dinv, j, lane)) : 0.0;
    k.w.x[IX(j)] = xv; k.w.xs[IX(j)] = xv; k.w.dx[IX(j)] = 0.0;
  }
}
LS_KERNEL_PAIR(load_n)
// l, u <- E clamp(l, u),  y <- c Einv y (warm) or 0,  dy = 0;  the problem's number of inequality rows (decides its equality weight)
template <bool MAT> __device__ __forceinline__ void ls_load_m(const LsK &k) {
  __shared__ double tile[64][65];
  __shared__ double red[256];
  const LockstepParams &P = k.P;
  const int lane = ls_lane(), wv = ls_wave(), i0 = blockIdx.x * 64;
  const bool mine = lane < P.count;
  double lo[16], cnt = 0.0;
  if (P.l) ls_tile_in(P.l, P.m, i0, P.count, P.pr, tile);
#pragma unroll
  for (int s = 0; s < 16; s++) { const int il = wv + 4 * s, i = min(i0 + il, P.m - 1); lo[s] = P.l ? tile[lane][il] : P.l0[i]; }
  __syncthreads();
  if (P.u) ls_tile_in(P.u, P.m, i0, P.count, P.pr, tile);
#pragma unroll
  for (int s = 0; s < 16; s++) {
    const int il = wv + 4 * s, i = i0 + il;
    if (i < P.m) {
      const double uv = P.u ? tile[lane][il] : P.u0[i];
      const double li = mine ? in_l(ls_sv<MAT>(P.E, i, lane), lo[s]) : -OSQP_INFTY, ui = mine ? in_u(ls_sv<MAT>(P.E, i, lane), uv) : OSQP_INFTY;
      k.w.l[IX(i)] = li; k.w.u[IX(i)] = ui; k.w.dy[IX(i)] = 0.0;
      cnt += row_class(li, ui, P.rho_is_vec) == 0 ? 1.0 : 0.0;
    }
  }
  __syncthreads();
  if (P.warm) ls_tile_in(P.y, P.m, i0, P.count, P.pr, tile);
  for (int il = wv; il < 64 && i0 + il < P.m; il += 4) {
    const int i = i0 + il;
    k.w.y[IX(i)] = (P.warm && mine) ? in_y(tile[lane][il], ls_sv<MAT>(P.Einv, i, lane), MAT ? k.w.sc[SC_C * W + lane] : P.c) : 0.0;
  }
  red[wv * 64 + lane] = cnt;
  __syncthreads();
  if (wv == 0) k.w.parti[(size_t)blockIdx.x * 64 + lane] = ((red[lane] + red[64 + lane]) + red[128 + lane]) + red[192 + lane];
}
LS_KERNEL_PAIR(load_m)
// the chunk's per-problem state: rho_bar, the equality weight (engine.cpp classify_constraints), counters; lanes >= count are terminated
__global__ __launch_bounds__(256) void k_ls_init(LsK k, int tiles_m) {
  __shared__ double lds[256];
  const int lane = ls_lane();
  const double n_ineq = ls_fold<false>(k.w.parti, tiles_m, 0, lds);
  if (threadIdx.x >= 64) return;
  double *sc = k.w.sc; int *iw = k.w.iw;
  sc[SC_RHOBAR * W + lane] = k.P.rho0; sc[SC_EQF * W + lane] = eq_weight(n_ineq == 0.0, k.P.eq_factor);
  sc[SC_EPSCG * W + lane] = 0.0; sc[SC_EPSPREV * W + lane] = INFINITY;
  iw[IW_DONE * W + lane] = lane >= k.P.count; iw[IW_STATUS * W + lane] = OSQP_UNSOLVED; iw[IW_RHOUPD * W + lane] = 0; iw[IW_PCG * W + lane] = 0;
  iw[IW_RELRULE * W + lane] = 1; iw[IW_CGON * W + lane] = 0; iw[IW_RHOCH * W + lane] = 1; iw[IW_SIDE * W + lane] = 0;
  if (threadIdx.x == 0) { k.w.word[WD_CGANY] = 0; k.w.word[WD_LIVE] = k.P.count; k.w.word[WD_RHOANY] = 1; k.w.word[WD_PCGSUM] = 0; k.w.word[WD_CGIT] = 0; }
}

// x = D x, y = cinv E y (_osqp.py:1110-1112); certificates in place of x / y for infeasible problems; the records
template <bool MAT> __device__ __forceinline__ void ls_store_n(const LsK &k) {
  __shared__ double tile[64][65];
  const LockstepParams &P = k.P;
  const int lane = ls_lane(), wv = ls_wave(), j0 = blockIdx.x * 64, status = k.w.iw[IW_STATUS * W + lane];
  for (int jl = wv; jl < 64 && j0 + jl < P.n; jl += 4) {
    const int j = j0 + jl;
    tile[lane][jl] = batch_out_x(status, P.unscaled, P.scaling, ls_sv<MAT>(P.D, j, lane), k.w.x[IX(j)], k.w.dx[IX(j)]);
  }
  ls_tile_out(P.x, P.n, j0, P.count, P.pc, tile);
  if (blockIdx.x == 0) for (int e = threadIdx.x; e < P.count * kBatchRec; e += 256) P.rec[e] = k.w.rec[e];
}
LS_KERNEL_PAIR(store_n)
template <bool MAT> __device__ __forceinline__ void ls_store_m(const LsK &k) {
  __shared__ double tile[64][65];
  const LockstepParams &P = k.P;
  const int lane = ls_lane(), wv = ls_wave(), i0 = blockIdx.x * 64, status = k.w.iw[IW_STATUS * W + lane];
  for (int il = wv; il < 64 && i0 + il < P.m; il += 4) {
    const int i = i0 + il;
    tile[lane][il] = batch_out_y(status, P.unscaled, P.scaling, MAT ? k.w.sc[SC_CINV * W + lane] : P.cinv, ls_sv<MAT>(P.E, i, lane), k.w.y[IX(i)], k.w.dy[IX(i)]);
  }
  ls_tile_out(P.y, P.m, i0, P.count, P.pr, tile);
}
LS_KERNEL_PAIR(store_m)
// ---------------------------------------------------------------------------------------------------------------- adjoint derivatives of a chunk
// The backward pass (include/osqp_hip.h osqp_hip_batch_adjoint_lockstep): per problem the adjoint system  [P, A_a'; A_a, 0] [r_x; r_a] = -[dx; dy_a]  is the
// KKT system of  min 1/2 r'Pr + dx'r  s.t.  A_a r = -dy_a  and is solved by the recurrence of Engine::run_recurrence -- THIS route's ADMM iteration
// (k_ls_rhs, the PCG, k_ls_upd, k_ls_resm / k_ls_resn) with alpha = 1, rho_bar = 1 / delta_eff on the active rows (equalities at -E dy), the other rows
// free, q~ = c D dx, a zero start -- as adjoint_hip.hip does around the single-QP recurrence.  What is new here surrounds that iteration: the transposes
// in with the classification (step_rules.h adjoint_active: the text k_batch_adjoint and EAdjClass call), the progress rule per problem (term_rules.h
// recurrence_ends: Engine::run_recurrence's), the unscaling and the residual of the unregularised system, the transposes out and the gradients at the
// stored entries.  Extra block vectors: the unscaled x, dx, r_x (n) and y, dy, r_y (m) and the row codes (ints, packed like iw).
// The five kernels here that read matrix values or scalings (load_n, class, unscale, resm, resn) are bodies ls_adj_NAME<MAT> like the forward's: k_ls_adj_NAME
// on the handle's, k_lsm_adj_NAME on the chunk's own matrix block ("matrices of a chunk" below), D / Dinv / E / Einv per lane and c, 1 / c from the rows
// SC_C / SC_CINV of the scalar state.  The others read neither and serve both.
struct LsAK { LockstepAdjointParams P; LsWs w; LsAdjWs a; };
enum LsAdjSlot { AS_ACT = PS_BN /* sum: active rows (before the first k_ls_rhs) */, AS_RM = PS_M0 /* max, after the last step: */, AS_GM, AS_RN, AS_GN };

// x (kept), x~ = Dinv x into p (the classification's operand; k_ls_rhs overwrites it), q~ = c D dx, dx (kept), the zero start
template <bool MAT> __device__ __forceinline__ void ls_adj_load_n(const LsAK &k) {
  __shared__ double tile[64][65];
  const LockstepAdjointParams &P = k.P;
  const int lane = ls_lane(), wv = ls_wave(), j0 = blockIdx.x * 64;
  ls_tile_in(P.sx, P.n, j0, P.count, P.pc, tile);                              // (zero for lanes >= count)
  for (int jl = wv; jl < 64 && j0 + jl < P.n; jl += 4) {
    const int j = j0 + jl;
    const double xv = tile[lane][jl];
    k.a.ax[IX(j)] = xv; k.w.p[IX(j)] = in_x(xv, ls_sv<MAT>(P.Dinv, j, lane));
    k.w.x[IX(j)] = 0.0; k.w.xs[IX(j)] = 0.0; k.w.dx[IX(j)] = 0.0;
  }
  __syncthreads();
  ls_tile_in(P.gx, P.n, j0, P.count, P.pc, tile);
  for (int jl = wv; jl < 64 && j0 + jl < P.n; jl += 4) {
    const int j = j0 + jl;
    const double gv = tile[lane][jl];
    k.a.gdx[IX(j)] = gv; k.w.q[IX(j)] = in_q(MAT ? k.w.sc[SC_C * W + lane] : P.c, ls_sv<MAT>(P.D, j, lane), gv);
  }
}
LS_KERNEL_PAIR_OF(LsAK, adj_load_n)
// y, dy (kept) and the caller's bounds (clamped, unscaled: k_ls_adj_class turns them into the recurrence's)
__global__ __launch_bounds__(256) void k_ls_adj_load_m(LsAK k) {
  __shared__ double tile[64][65];
  const LockstepAdjointParams &P = k.P;
  const int lane = ls_lane(), wv = ls_wave(), i0 = blockIdx.x * 64;
  const bool mine = lane < P.count;
  ls_tile_in(P.sy, P.m, i0, P.count, P.pr, tile);
  for (int il = wv; il < 64 && i0 + il < P.m; il += 4) k.a.ay[IX(i0 + il)] = tile[lane][il];
  __syncthreads();
  if (P.gy) ls_tile_in(P.gy, P.m, i0, P.count, P.pr, tile);
  for (int il = wv; il < 64 && i0 + il < P.m; il += 4) k.a.gdy[IX(i0 + il)] = P.gy ? tile[lane][il] : 0.0;
  __syncthreads();
  if (P.l) ls_tile_in(P.l, P.m, i0, P.count, P.pr, tile);
  for (int il = wv; il < 64 && i0 + il < P.m; il += 4) {
    const int i = i0 + il;
    k.w.l[IX(i)] = mine ? clamp_lower(P.l ? tile[lane][il] : P.l0[i]) : -OSQP_INFTY;
  }
  __syncthreads();
  if (P.u) ls_tile_in(P.u, P.m, i0, P.count, P.pr, tile);
  for (int il = wv; il < 64 && i0 + il < P.m; il += 4) {
    const int i = i0 + il;
    k.w.u[IX(i)] = mine ? clamp_upper(P.u ? tile[lane][il] : P.u0[i]) : OSQP_INFTY;
  }
}
// z = Einv (A x~) in the caller's units, the row's code, the recurrence's bounds (active: l = u = z = -E dy; the others free) and zero start
template <bool MAT> struct FAdjClass {
  const LsWs &w; const LsAdjWs &a; const double *E, *Einv; int has_dy, lane;
  double cnt = 0;
  __device__ __forceinline__ void begin(int) {}
  __device__ __forceinline__ void load(int c, double (&g)[1]) const { g[0] = w.p[IX(c)]; }
  __device__ __forceinline__ void fma(int, double v, const double (&g)[1], double (&acc)[1]) const { acc[0] += v * g[0]; }
  __device__ __forceinline__ void row(int i, const double (&acc)[1]) {
    const double zi = ls_sv<MAT>(Einv, i, lane) * acc[0];
    const RowActive act = adjoint_active(zi, w.l[IX(i)], w.u[IX(i)], a.ay[IX(i)]);
    const int kc = act.low ? 1 : (act.upp ? 2 : 0);
    const double b = (kc && has_dy) ? -(ls_sv<MAT>(E, i, lane) * a.gdy[IX(i)]) : 0.0;
    a.code[IX(i)] = kc;
    w.l[IX(i)] = kc ? b : -OSQP_INFTY; w.u[IX(i)] = kc ? b : OSQP_INFTY;
    w.z[IX(i)] = b; w.zt[IX(i)] = 0.0; w.y[IX(i)] = 0.0; w.dy[IX(i)] = 0.0;
    cnt += kc ? 1.0 : 0.0;
  }
};
template <bool MAT> __device__ __forceinline__ void ls_adj_class(const LsAK &k) {
  __shared__ double lds[256];
  FAdjClass<MAT> f{k.w, k.a, k.P.E, k.P.Einv, k.P.gy != nullptr, ls_lane()};
  ls_rows<1, 1, MAT>(k.P.A, f);
  const double vs[1] = {f.cnt};
  ls_put<0, 1>(k.w.part, AS_ACT, vs, vs, lds);
}
LS_KERNEL_PAIR_OF(LsAK, adj_class)
// the chunk's per-problem state: rho_bar = 1 / delta_eff with equality factor 1; a problem with more active rows than variables (status 2) and the
// lanes >= count are finished before the first step
__global__ __launch_bounds__(256) void k_ls_adj_init(LsAK k) {
  __shared__ double lds[256];
  const int lane = ls_lane();
  const double nact = k.P.m > 0 ? ls_fold<false>(k.w.part, k.w.G, AS_ACT, lds) : 0.0;
  if (threadIdx.x >= 64) return;
  double *sc = k.w.sc; int *iw = k.w.iw;
  const bool mine = lane < k.P.count, singular = nact > (double)k.P.n;
  sc[SC_RHOBAR * W + lane] = k.P.rho0; sc[SC_EQF * W + lane] = k.P.eq_factor; sc[SC_EPSCG * W + lane] = 0.0; sc[SC_EPSPREV * W + lane] = INFINITY;
  sc[SC_BEST * W + lane] = INFINITY; sc[SC_NACT * W + lane] = nact;
  iw[IW_DONE * W + lane] = !mine || singular; iw[IW_STATUS * W + lane] = (mine && singular) ? 2 : 0; iw[IW_RHOUPD * W + lane] = 0; iw[IW_PCG * W + lane] = 0;
  iw[IW_RELRULE * W + lane] = 0; iw[IW_CGON * W + lane] = 0; iw[IW_RHOCH * W + lane] = 1; iw[IW_STEPS * W + lane] = 0; iw[IW_WORSE * W + lane] = 0;
  const unsigned long long live = __ballot(mine && !singular);
  if (threadIdx.x == 0) { k.w.word[WD_CGANY] = 0; k.w.word[WD_LIVE] = __popcll(live); k.w.word[WD_RHOANY] = 1; k.w.word[WD_PCGSUM] = 0; k.w.word[WD_CGIT] = 0; }
}
// after every step: the progress rule per problem (term_rules.h recurrence_ends on the slots k_ls_resm / k_ls_resn have put); a problem that ends is frozen
__global__ __launch_bounds__(256) void k_ls_adj_decide(LsAK k) {
  __shared__ double lds[256];
  const int lane = ls_lane(), G = k.w.G;
  const bool has_m = k.P.m > 0;                                                 // (uniform: so are the folds' barriers)
  const double pri_s = has_m ? ls_fold<true>(k.w.part, G, PS_M0 + 3, lds) : 0.0, z_s = has_m ? ls_fold<true>(k.w.part, G, PS_M0 + 5, lds) : 0.0;
  const double dua_s = ls_fold<true>(k.w.part, G, PS_N0 + 3, lds), qn_s = ls_fold<true>(k.w.part, G, PS_N0 + 8, lds);
  if (threadIdx.x >= 64) return;
  double *sc = k.w.sc; int *iw = k.w.iw;
  if (!iw[IW_DONE * W + lane]) {
    const int steps = iw[IW_STEPS * W + lane] + 1;
    double best = sc[SC_BEST * W + lane]; int worse = iw[IW_WORSE * W + lane];
    const bool end = recurrence_ends(recurrence_err_rhs(pri_s, dua_s, qn_s, z_s), k.P.gain, steps, k.P.min_steps, k.P.max_steps, &best, &worse);
    iw[IW_STEPS * W + lane] = steps; sc[SC_BEST * W + lane] = best; iw[IW_WORSE * W + lane] = worse;
    if (end) iw[IW_DONE * W + lane] = 1;
  }
  iw[IW_RHOCH * W + lane] = 0;
  const unsigned long long live = __ballot(!iw[IW_DONE * W + lane]);
  int pcg = iw[IW_PCG * W + lane];                      // (statistics only)
  for (int o = 32; o > 0; o >>= 1) pcg += __shfl_xor(pcg, o);
  if (threadIdx.x == 0) { k.w.word[WD_LIVE] = __popcll(live); k.w.word[WD_RHOANY] = 0; k.w.word[WD_PCGSUM] = pcg; }
}
// r_x = D x,  r_y = cinv E y on the active rows and exactly 0 elsewhere (y itself too: the residual's A' multiplies it)
// (MAT: element e of a block is row e >> 6 of lane e & 63 -- this thread's lane, the stride being a multiple of 64 -- so the problem's own D, E sit at e)
template <bool MAT> __device__ __forceinline__ void ls_adj_unscale(const LsAK &k) {
  const size_t nt = (size_t)k.P.n * 64, mt = (size_t)k.P.m * 64, stride = (size_t)gridDim.x * 256;
  const double cinv = MAT ? k.w.sc[SC_CINV * W + ls_lane()] : k.P.cinv;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < nt; e += stride) k.a.rx[e] = k.P.D[MAT ? e : e >> 6] * k.w.x[e];
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < mt; e += stride) {
    const double ys = k.a.code[e] ? k.w.y[e] : 0.0;
    k.w.y[e] = ys; k.a.ry[e] = cinv * k.P.E[MAT ? e : e >> 6] * ys;
  }
}
LS_KERNEL_PAIR_OF(LsAK, adj_unscale)
// rows n .. n + active of g - K_a r:  -dy_i - (A r_x)_i  on the active rows (adjoint_hip.hip EAdjResM)
template <bool MAT> struct FAdjResM {
  const LsWs &w; const LsAdjWs &a; const double *Einv; int lane;
  double rm = 0, gm = 0;
  __device__ __forceinline__ void begin(int) {}
  __device__ __forceinline__ void load(int c, double (&g)[1]) const { g[0] = w.x[IX(c)]; }
  __device__ __forceinline__ void fma(int, double v, const double (&g)[1], double (&acc)[1]) const { acc[0] += v * g[0]; }
  __device__ __forceinline__ void row(int i, const double (&acc)[1]) {
    if (!a.code[IX(i)]) return;
    const double dyi = a.gdy[IX(i)];
    rm = nanmax(rm, fabs(dyi + ls_sv<MAT>(Einv, i, lane) * acc[0])); gm = nanmax(gm, fabs(dyi));
  }
};
template <bool MAT> __device__ __forceinline__ void ls_adj_resm(const LsAK &k) {
  __shared__ double lds[2 * 256];
  FAdjResM<MAT> f{k.w, k.a, k.P.Einv, ls_lane()};
  ls_rows<1, 1, MAT>(k.P.A, f);
  const double vm[2] = {f.rm, f.gm};
  ls_put<2, 0>(k.w.part, AS_RM, vm, vm, lds);
}
LS_KERNEL_PAIR_OF(LsAK, adj_resm)
// rows 0 .. n:  -dx_j - (P r_x + A_a' r_a)_j;  row j of B [x~; y~] is  c D_j (P r_x + A' r_y)_j + sigma x~_j  (adjoint_hip.hip EAdjResN)
template <bool MAT> struct FAdjResN {
  const LsWs &w; const LsAdjWs &a; const double *Dinv; double sigma, cinv; int n, lane;
  double rn = 0, gn = 0;
  __device__ __forceinline__ void begin(int) {}
  __device__ __forceinline__ void load(int c, double (&g)[1]) const { g[0] = c < n ? w.x[IX(c)] : w.y[IX(c - n)]; }
  __device__ __forceinline__ void fma(int c, double v, const double (&g)[1], double (&acc)[2]) const {
    const double p = v * g[0]; const bool pn = c < n;                          // (selects, not indexed accumulators)
    acc[0] += pn ? p : 0.0; acc[1] += pn ? 0.0 : p;
  }
  __device__ __forceinline__ void row(int j, const double (&acc)[2]) {
    const double kr = cinv * ls_sv<MAT>(Dinv, j, lane) * ((acc[0] - sigma * w.x[IX(j)]) + acc[1]), dxj = a.gdx[IX(j)];
    rn = nanmax(rn, fabs(dxj + kr)); gn = nanmax(gn, fabs(dxj));
  }
};
// (sigma sits on B's diagonal after the equilibration on both routes: the term is the same with per-problem matrices)
template <bool MAT> __device__ __forceinline__ void ls_adj_resn(const LsAK &k) {
  __shared__ double lds[2 * 256];
  const int lane = ls_lane();
  FAdjResN<MAT> f{k.w, k.a, k.P.Dinv, k.P.sigma, MAT ? k.w.sc[SC_CINV * W + lane] : k.P.cinv, k.P.n, lane};
  ls_rows<1, 2, MAT>(k.P.B, f);
  const double vm[2] = {f.rn, f.gn};
  ls_put<2, 0>(k.w.part, AS_RN, vm, vm, lds);
}
LS_KERNEL_PAIR_OF(LsAK, adj_resn)
// the record: {status, active rows, residual max |g - K_a r| / max |g|, recurrence steps}
__global__ __launch_bounds__(256) void k_ls_adj_final(LsAK k) {
  __shared__ double lds[256];
  const int lane = ls_lane(), G = k.w.G;
  const bool has_m = k.P.m > 0;
  const double rm = has_m ? ls_fold<true>(k.w.part, G, AS_RM, lds) : 0.0, gm = has_m ? ls_fold<true>(k.w.part, G, AS_GM, lds) : 0.0;
  const double rn = ls_fold<true>(k.w.part, G, AS_RN, lds), gn = ls_fold<true>(k.w.part, G, AS_GN, lds);
  if (threadIdx.x >= 64 || lane >= k.P.count || !k.P.arec) return;
  const bool singular = k.w.iw[IW_STATUS * W + lane] == 2;
  const double r = nanmax(rm, rn), g = nanmax(gm, gn);
  const double resid = singular ? INFINITY : (g > 0.0 ? r / g : (r > 0.0 ? INFINITY : 0.0));
  double *rc = k.P.arec + (size_t)lane * kAdjointRec;
  rc[0] = singular ? 2.0 : (resid < kAdjointTol ? 0.0 : 3.0); rc[1] = k.w.sc[SC_NACT * W + lane]; rc[2] = resid; rc[3] = k.w.iw[IW_STEPS * W + lane];
}
// dq = r_x;  dl = -r_y on the lower-active rows, du = -r_y on the upper-active ones, 0 elsewhere
__global__ __launch_bounds__(256) void k_ls_adj_out_n(LsAK k) {
  __shared__ double tile[64][65];
  const int lane = ls_lane(), wv = ls_wave(), j0 = blockIdx.x * 64;
  for (int jl = wv; jl < 64 && j0 + jl < k.P.n; jl += 4) tile[lane][jl] = k.a.rx[IX(j0 + jl)];
  ls_tile_out(k.P.dq, k.P.n, j0, k.P.count, k.P.pc, tile);
}
__global__ __launch_bounds__(256) void k_ls_adj_out_m(LsAK k) {
  __shared__ double tile[64][65];
  const int lane = ls_lane(), wv = ls_wave(), i0 = blockIdx.x * 64;
  for (int side = 1; side <= 2; side++) {
    double *dst = side == 1 ? k.P.dl : k.P.du;
    if (!dst) continue;                                                         // (uniform)
    for (int il = wv; il < 64 && i0 + il < k.P.m; il += 4) {
      const size_t e = IX(i0 + il);
      tile[lane][il] = k.a.code[e] == side ? -k.a.ry[e] : 0.0;
    }
    ls_tile_out(dst, k.P.m, i0, k.P.count, k.P.pr, tile);
  }
}
// dP_ij = (r_x,i x_j + r_x,j x_i) / 2 (SYM) and dA_ij = y_i r_x,j + r_y,i x_j at the stored entries, [count][nnz] row-major in the CALLER's CSC order.  A workgroup
// takes 64 of the caller's entries, a wave 16 of them: the entry's position in the engine's arrays (through the value map of a reordered handle) and its
// (i, j) are wave-uniform, each operand is one 512-byte line, four entries are in flight; the tile goes out coalesced along the entries.  One writer each.
template <bool SYM>
__global__ __launch_bounds__(256) void k_ls_adj_grad(LsAK k) {
  __shared__ double tile[64][65];
  const LockstepAdjointParams &P = k.P;
  const int nz = SYM ? P.nzP : P.nzA, lane = ls_lane(), wv = ls_wave(), e0 = blockIdx.x * 64;
  const int *__restrict__ ri = SYM ? P.Pi : P.Ai, *__restrict__ cj = SYM ? P.Pj : P.Aj, *__restrict__ map = SYM ? P.Pmap : P.Amap;
  const double *ra = SYM ? k.a.rx : k.a.ay, *ca = SYM ? k.a.ax : k.a.rx, *rb = SYM ? k.a.ax : k.a.ry, *cb = SYM ? k.a.rx : k.a.ax;
  double *out = SYM ? P.dP : P.dA;
  for (int s = wv * 16; s < wv * 16 + 16; s += 4) {
    int i[4], j[4]; double g[4][4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int e = min(e0 + s + u, nz - 1), pos = __builtin_amdgcn_readfirstlane(map ? map[e] : e);
      i[u] = __builtin_amdgcn_readfirstlane(ri[pos]); j[u] = __builtin_amdgcn_readfirstlane(cj[pos]);
    }
#pragma unroll
    for (int u = 0; u < 4; u++) { g[u][0] = ra[IX(i[u])]; g[u][1] = ca[IX(j[u])]; g[u][2] = rb[IX(i[u])]; g[u][3] = cb[IX(j[u])]; }
#pragma unroll
    for (int u = 0; u < 4; u++) tile[lane][s + u] = SYM ? 0.5 * (g[u][0] * g[u][1] + g[u][3] * g[u][2]) : g[u][0] * g[u][1] + g[u][2] * g[u][3];
  }
  __syncthreads();
  const int e = e0 + lane;
  if (e < nz) for (int b = wv; b < P.count; b += 4) out[(size_t)b * nz + e] = tile[b][lane];
}
// ---------------------------------------------------------------------------------------------------------------- polish of a chunk
// settings.polishing on this route (include/osqp_hip.h osqp_hip_batch_solve_lockstep, POLISH): every problem of the chunk that ended OSQP_SOLVED is polished
// between the ADMM loop and the transposes out, with the semantics of Engine::polish (engine.cpp; _osqp.py:1710-1828).  The reduced KKT system on the
// guessed active set is solved by the recurrence of Engine::run_recurrence, which is THIS route's iteration (k_ls_rhs, the PCG, k_ls_upd, k_ls_resm /
// k_ls_resn) with alpha = 1, rho_bar = 1 / delta_eff on the active rows, the others free, from the ADMM point -- as in "adjoint derivatives of a chunk".
// What is new surrounds it: which problems take part and their state (k_ls_pol_begin), the save and the classification (k_ls_pol_class: step_rules.h
// polish_active), polish's progress measure per problem (k_ls_pol_decide: term_rules.h recurrence_err_polish / recurrence_ends), z = A x and the
// normal-cone projection against the problem's own bounds (k_ls_pol_cone), the accept test against the record (k_ls_pol_accept: term_info,
// polish_accept) and, for a rejected problem, the ADMM x, y, z back (k_ls_pol_end).  A problem that does not take part is "terminated" all the way: no
// kernel stores to its lane.  The saved vectors live in a work block of their own (backend.h lockstep_polish_ws_doubles).
// With per-problem matrices ("matrices of a chunk" below) the recurrence runs on kLsOwnMat and the two kernels here that read matrix values or the cost
// scale are bodies ls_pol_NAME<MAT> like the forward's: k_lsm_pol_cone walks the chunk's own A, k_lsm_pol_accept takes c, 1 / c per lane.  The others
// read neither and serve both: k_ls_pol_class classifies on the scaled z, l, u, y -- with a per-lane E and c each problem's own scaled space, which is
// what Engine::polish does on a handle set up with that problem alone.
struct LsPK { LockstepParams P; LsWs w; LsPolWs s; };

// per problem: takes part iff SOLVED; IW_DONE becomes "not in the recurrence"; rho_bar = 1 / delta_eff with equality factor 1, flagged for k_ls_setrho / k_ls_minv
__global__ __launch_bounds__(256) void k_ls_pol_begin(LsPK k) {
  if (threadIdx.x >= 64) return;
  const int lane = ls_lane();
  double *sc = k.w.sc; int *iw = k.w.iw;
  const int pol = iw[IW_STATUS * W + lane] == OSQP_SOLVED;      // (lanes >= count: OSQP_UNSOLVED)
  if (pol) { sc[SC_RHOBAR * W + lane] = k.P.pol_rho; sc[SC_EQF * W + lane] = 1.0; sc[SC_BEST * W + lane] = INFINITY; }      // (the record has the ADMM's rho_bar already)
  iw[IW_POL * W + lane] = pol; iw[IW_DONE * W + lane] = !pol; iw[IW_RHOCH * W + lane] = pol; iw[IW_CGON * W + lane] = 0;
  iw[IW_PCG * W + lane] = 0; iw[IW_STEPS * W + lane] = 0; iw[IW_WORSE * W + lane] = 0;      // (IW_PCG: the record has the ADMM's count; from here on polish's, for the statistics)
  const unsigned long long live = __ballot(pol);
  if (threadIdx.x == 0) { k.w.word[WD_CGANY] = 0; k.w.word[WD_LIVE] = __popcll(live); k.w.word[WD_RHOANY] = live != 0ull; k.w.word[WD_CGIT] = 0; k.w.word[WD_POLACC] = 0; k.w.word[WD_POLREJ] = 0; }
}
// the ADMM point saved; per row the active side (equality rows, scaled l == u, always on the lower one) and the recurrence's bounds: active rows l = u = z =
// the bound, the others free with y = 0.  x, x~ and z~ = A x~ stay: k_ls_setrho, which follows, forms t and t2 from the new z, y.
__global__ __launch_bounds__(256) void k_ls_pol_class(LsPK k) {
  if (!k.w.iw[IW_POL * W + ls_lane()]) return;
  const size_t nt = (size_t)k.P.n * 64, mt = (size_t)k.P.m * 64, stride = (size_t)gridDim.x * 256;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < nt; e += stride) k.s.x[e] = k.w.x[e];
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < mt; e += stride) {
    const double z = k.w.z[e], y = k.w.y[e], l = k.w.l[e], u = k.w.u[e];
    k.s.z[e] = z; k.s.y[e] = y; k.s.l[e] = l; k.s.u[e] = u;
    const RowActive act = polish_active(z, l, u, y);
    const bool low = act.low || l == u, on = low || act.upp;
    const double b = low ? l : u;
    k.w.l[e] = on ? b : -OSQP_INFTY; k.w.u[e] = on ? b : OSQP_INFTY; k.w.z[e] = on ? b : z; k.w.y[e] = on ? y : 0.0;
  }
}
// after every step: polish's measure of the reduced system's residuals and the progress rule per problem; a problem that ends is frozen
__global__ __launch_bounds__(256) void k_ls_pol_decide(LsPK k) {
  __shared__ double lds[256];
  const int lane = ls_lane(), G = k.w.G;
  const bool has_m = k.P.m > 0;                                                 // (uniform: so are the folds' barriers)
  auto mx = [&](int slot) { return ls_fold<true>(k.w.part, G, slot, lds); };
  const double pri_s = has_m ? mx(PS_M0 + 3) : 0.0, ax_s = has_m ? mx(PS_M0 + 4) : 0.0, z_s = has_m ? mx(PS_M0 + 5) : 0.0;
  const double dua_s = mx(PS_N0 + 3), px_s = mx(PS_N0 + 4), aty_s = mx(PS_N0 + 5), qn_s = mx(PS_N0 + 8);
  if (threadIdx.x >= 64) return;
  double *sc = k.w.sc; int *iw = k.w.iw;
  if (!iw[IW_DONE * W + lane]) {
    const int steps = iw[IW_STEPS * W + lane] + 1;
    double best = sc[SC_BEST * W + lane]; int worse = iw[IW_WORSE * W + lane];
    const bool end = recurrence_ends(recurrence_err_polish(pri_s, ax_s, z_s, dua_s, aty_s, px_s, qn_s), 0.5, steps, k.P.pol_min_steps, kLsPolMaxSteps, &best, &worse);
    iw[IW_STEPS * W + lane] = steps; sc[SC_BEST * W + lane] = best; iw[IW_WORSE * W + lane] = worse;
    if (end) iw[IW_DONE * W + lane] = 1;
  }
  iw[IW_RHOCH * W + lane] = 0;
  const unsigned long long live = __ballot(!iw[IW_DONE * W + lane]);
  int pcg = iw[IW_PCG * W + lane];                      // (statistics only)
  for (int o = 32; o > 0; o >>= 1) pcg += __shfl_xor(pcg, o);
  if (threadIdx.x == 0) { k.w.word[WD_LIVE] = __popcll(live); k.w.word[WD_RHOANY] = 0; k.w.word[WD_PCGSUM] = pcg; }
}
// the polished point against the problem's own bounds: l, u back, z = A x, then the normal-cone projection of (z, y)  (_osqp.py:1773-1780)
struct FPolCone {
  const LsWs &w; const LsPolWs &s; int lane, pol;
  __device__ __forceinline__ void begin(int) {}
  __device__ __forceinline__ void load(int c, double (&g)[1]) const { g[0] = w.x[IX(c)]; }
  __device__ __forceinline__ void fma(int, double v, const double (&g)[1], double (&a)[1]) const { a[0] += v * g[0]; }
  __device__ __forceinline__ void row(int i, const double (&a)[1]) const {
    if (!pol) return;
    const double l = s.l[IX(i)], u = s.u[IX(i)];
    const ConeRow c = normal_cone(a[0] + w.y[IX(i)], l, u);
    w.l[IX(i)] = l; w.u[IX(i)] = u; w.z[IX(i)] = c.z; w.y[IX(i)] = c.y;
  }
};
template <bool MAT> __device__ __forceinline__ void ls_pol_cone(const LsPK &k) {
  const int lane = ls_lane();
  FPolCone f{k.w, k.s, lane, k.w.iw[IW_POL * W + lane]};
  ls_rows<1, 1, MAT>(k.P.A, f);
}
LS_KERNEL_PAIR_OF(LsPK, pol_cone)
// the info fields of the polished point (term_rules.h term_info on the slots k_ls_resm / k_ls_resn have put) against the record's: kept or rejected.
// MAT: the problem's own cost scale, as ls_decide<MAT> takes it -- rows SC_C / SC_CINV of the scalar state, which ls_mat_prepare wrote and nothing since:
// k_ls_init, the decisions and the PCG's folds write rows below SC_BEST, k_ls_pol_begin SC_RHOBAR, SC_EQF and SC_BEST, k_ls_pol_decide SC_BEST.
template <bool MAT> __device__ __forceinline__ void ls_pol_accept(const LsPK &k) {
  __shared__ double lds[256];
  const LockstepParams &P = k.P;
  const int lane = ls_lane(), G = k.w.G;
  const bool has_m = P.m > 0;
  TermRes R = {};
  R.pri_u = has_m ? ls_fold<true>(k.w.part, G, PS_M0, lds) : 0.0; R.pri_s = has_m ? ls_fold<true>(k.w.part, G, PS_M0 + 3, lds) : 0.0;
  R.dua_u = ls_fold<true>(k.w.part, G, PS_N0, lds); R.dua_s = ls_fold<true>(k.w.part, G, PS_N0 + 3, lds);
  R.xpx = ls_fold<false>(k.w.part, G, PS_N0 + 14, lds); R.qx = ls_fold<false>(k.w.part, G, PS_N0 + 15, lds);
  const bool gap_on = P.check_dualgap != 0;                                       // (uniform; k_ls_supp has run on the polished y and the problem's own bounds)
  const double supp = (gap_on && has_m) ? ls_fold<false>(k.w.part, G, PS_SUPP, lds) : 0.0;
  if (threadIdx.x >= 64) return;
  int *iw = k.w.iw;
  const int pol = iw[IW_POL * W + lane];
  bool ok = false;
  if (pol) {
    const TermSet tset = {P.eps_abs, P.eps_rel, P.eps_pinf, P.eps_dinf, MAT ? k.w.sc[SC_C * W + lane] : P.c, MAT ? k.w.sc[SC_CINV * W + lane] : P.cinv, P.m, P.unscaled, P.scaling};
    double obj, prim_res, dual_res;
    term_info(tset, R, &obj, &prim_res, &dual_res);
    double *rc = k.w.rec + (size_t)lane * kBatchRec;
    ok = polish_accept(prim_res, dual_res, rc[3], rc[4]);
    if (ok) {
      rc[2] = obj; rc[3] = prim_res; rc[4] = dual_res; rc[8] = 1.0;
      if (gap_on) { const double dual_obj = term_dual_obj(tset, R, supp); batch_record_gap(rc, OSQP_SOLVED, obj - dual_obj); }      // (a rejected problem keeps its ADMM gap)
    } else { rc[8] = -1.0; iw[IW_POL * W + lane] = 2; }
  }
  const unsigned long long acc = __ballot(pol && ok), rej = __ballot(pol && !ok);
  if (threadIdx.x == 0) { k.w.word[WD_POLACC] = __popcll(acc); k.w.word[WD_POLREJ] = __popcll(rej); }
}
LS_KERNEL_PAIR_OF(LsPK, pol_accept)
// the record's polish seconds for every problem that was attempted; a rejected problem's ADMM x, y, z back
__global__ __launch_bounds__(256) void k_ls_pol_end(LsPK k, double secs) {
  const int lane = ls_lane(), pol = k.w.iw[IW_POL * W + lane];
  if (!pol) return;
  if (blockIdx.x == 0 && threadIdx.x < 64) k.w.rec[(size_t)lane * kBatchRec + 9] = secs;
  if (pol != 2) return;
  const size_t nt = (size_t)k.P.n * 64, mt = (size_t)k.P.m * 64, stride = (size_t)gridDim.x * 256;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < nt; e += stride) k.w.x[e] = k.s.x[e];
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < mt; e += stride) { k.w.y[e] = k.s.y[e]; k.w.z[e] = k.s.z[e]; }
}
// ---------------------------------------------------------------------------------------------------------------- lockstep DIRECT (Woodbury handles)
// The route of osqp_hip_batch_solve_lockstep_direct (lockstep_direct_chunk below): a handle whose A is r <= kWbMaxRows dense rows A_L next to rows with one
// entry, P diagonal -- K0 = P + sigma I + A_S' rho_S A_S is DIAGONAL (D0), K_b = D0_b + A_L' rho_L,b A_L, and the Woodbury formula is the solve:
//     S_b = diag(1 / rho_L,b) + A_L D0_b^-1 A_L'  (r x r, SPD),   K_b^-1 v = u - D0_b^-1 A_L' S_b^-1 A_L u ,  u = D0_b^-1 v .
// No PCG.  The iteration keeps this file's kernels: k_ls_rhs leaves r_0 = rhs - K x~ (x~ of the previous iteration: the solve is one step of refinement
// on it) and p = Minv r_0 with Minv = 1 / D0 (k_lw_d0), then  g = A_L p  (k_lw_prod: column blocks, [GC][r][64] partials),  h = S^-1 g  (k_lw_h: the
// partials folded in block order, rows of h spread over workgroups and waves),  x~ += p - Minv A_L' h  (k_lw_x), k_ls_upd.
// The dense rows in the row passes over A: ls_rows gives a wave a strip of ROWS, so a row with thousands of entries is one wave's serial walk.  The passes
// (k_ls_initz, k_ls_upd, k_ls_resm) therefore run on a VIEW of A (LockstepDirectView::Av) in which long row a is the single entry 1.0 at column n + a,
// and the block vectors x, x~, dx carry r more rows: (A_L x)_a, (A_L x~)_a, (A_L dx)_a.  x~'s rows follow k_wbz's identity  A_L x~ += h ./ rho_L  (A_L of
// the update is g - (S - diag(1 / rho_L)) h = h ./ rho_L), x's and dx's follow by linearity from k_ls_upd's own elementwise loop (run over n + r rows); at
// the start and in front of every residual pass the rows of x and x~ are recomputed from the products (k_lw_prod twice, k_lw_setl), so the carried
// values never drift from what the residuals are about.  B = [P + sigma I | A'] has r + 2 entries per row: k_ls_rhs / k_ls_resn read it as it is.
// S_b is formed (k_lw_s) and inverted in place (k_lw_inv: one workgroup per problem, S_b in LDS, Gauss-Jordan without pivoting) at the start and for exactly
// the problems whose rho_bar k_ls_decide has changed.  A pivot that is not positive and finite makes that problem's inverse NaN: its x~ and residuals
// are NaN from the next iteration on and k_ls_decide ends it with OSQP_NON_CVX (term_rules.h: non-finite residuals); no other lane reads it.
// PER-PROBLEM MATRICES on this route (osqp_hip_batch_solve_lockstep_direct_mat; lockstep_direct_chunk with mat_ws): the chunk's own matrix block ("matrices
// of a chunk" below) and, behind it, the dense rows per lane -- WT of problem b: entry (column j, long row a) at ((j r + a) 64 + b) -- and the view's
// values per lane ([nv][64]).  The four kernels here that read matrix values (d0, s, prod, x) are bodies lw_NAME<MAT>: k_lw_NAME on the handle's arrays,
// k_lwm_NAME on the chunk's, where a value of WT is one 512-byte line per wave in place of a wave-uniform scalar load; inv, h, setl read none.
struct LwWs : LwVecs {                  // (S, pg, pg2, h, fact: lockstep_layout.h)
  const double *WT; const int *rows; const unsigned char *islong;
  int r, GC, cb;                        // long rows; column blocks and their width
};
struct LwK { LockstepParams P; LsWs w; LwWs d; };

// a kernel body on the handle's dense rows and on the chunk's own ("per-problem matrices" below): k_lw_NAME the shared route's kernel, k_lwm_NAME the other
#define LW_KERNEL_PAIR(NAME) \
  __global__ __launch_bounds__(256) void k_lw_##NAME(LwK k) { lw_##NAME<false>(k); } \
  __global__ __launch_bounds__(256) void k_lwm_##NAME(LwK k) { lw_##NAME<true>(k); }

// Minv = 1 / D0,  D0 = B_jj + sum over the ONE-ENTRY rows i of column j of rho_i,b A_ij^2  (k_ls_minv's diagonal without the long rows' squares)
struct FD0 {
  const double *rho; double *Minv; const int *flag; const unsigned char *islong; int n, lane, cur;
  __device__ __forceinline__ void begin(int row) { cur = row; }
  __device__ __forceinline__ void load(int c, double (&g)[1]) const { g[0] = (c >= n && !islong[c - n]) ? rho[IX(c - n)] : 0.0; }
  __device__ __forceinline__ void fma(int c, double v, const double (&g)[1], double (&a)[2]) const { if (c >= n) a[0] += g[0] * v * v; else if (c == cur) a[1] = v; }
  __device__ __forceinline__ void row(int j, const double (&a)[2]) const { if (flag[lane]) Minv[IX(j)] = 1.0 / (a[1] + a[0]); }
};
template <bool MAT> __device__ __forceinline__ void lw_d0(const LwK &k) {
  if (!k.w.word[WD_RHOANY]) return;
  FD0 f{k.w.rho, k.w.Minv, k.w.iw + IW_RHOCH * W, k.d.islong, k.P.n, ls_lane(), 0};
  ls_rows<1, 2, MAT>(k.P.B, f);
}
LW_KERNEL_PAIR(d0)
// S[a][c] = (a == c) / rho_a + sum_j A_L[a, j] Minv_j A_L[c, j] for the problems whose rho has just been set.  Workgroup (a, eight columns c): wave w takes
// the columns j = w, w + 4, .. of A_L (WT: column j of A_L contiguous), the four waves are combined in wave order.
// MAT: a value of WT is one 512-byte line per (j, a) and wave; the ten lines of a column (row a's, Minv's, the eight of c0 ..) are requested together, and
// no column is skipped: whether A_L[a, j] is zero is no longer wave-uniform, and the terms the shared form skips are exact zeros.
template <bool MAT> __device__ __forceinline__ void lw_s(const LwK &k) {
  __shared__ double lds[8 * 256];
  if (!k.w.word[WD_RHOANY]) return;
  const int lane = ls_lane(), wv = ls_wave(), r = k.d.r, n = k.P.n, cch = (r + 7) / 8;
  const int a = (int)blockIdx.x / cch, c0 = ((int)blockIdx.x % cch) * 8;
  const double *__restrict__ WT = k.d.WT;
  double acc[8];
#pragma unroll
  for (int u = 0; u < 8; u++) acc[u] = 0.0;
  if constexpr (MAT) {
    for (int j = wv; j < n; j += 4) {
      const double *__restrict__ wt = WT + (size_t)j * r * 64 + lane;
      double wc[8];
      const double va = wt[(size_t)a * 64], mi = k.w.Minv[IX(j)];
#pragma unroll
      for (int u = 0; u < 8; u++) wc[u] = wt[(size_t)min(c0 + u, r - 1) * 64];
      const double t = va * mi;
#pragma unroll
      for (int u = 0; u < 8; u++) acc[u] += t * (c0 + u < r ? wc[u] : 0.0);
    }
  } else {
    for (int j = wv; j < n; j += 4) {
      const double *__restrict__ wt = WT + (size_t)j * r;
      const double va = wt[a];                            // (wave-uniform)
      if (va == 0.0) continue;
      const double t = va * k.w.Minv[IX(j)];
#pragma unroll
      for (int u = 0; u < 8; u++) acc[u] += t * (c0 + u < r ? wt[c0 + u] : 0.0);
    }
  }
#pragma unroll
  for (int u = 0; u < 8; u++) lds[(u * 4 + wv) * 64 + lane] = acc[u];
  __syncthreads();
  for (int u = wv; u < 8; u += 4) {
    const int c = c0 + u;
    if (c >= r) continue;
    const double *s = lds + u * 256 + lane;
    double v = ((s[0] + s[64]) + s[128]) + s[192];
    if (c == a) v += 1.0 / k.w.rho[IX(k.d.rows[a])];
    if (k.w.iw[IW_RHOCH * W + lane]) k.d.S[((size_t)a * r + c) * 64 + lane] = v;
  }
}
LW_KERNEL_PAIR(s)
// S_b <- S_b^-1 in place: workgroup b holds S_b (r x r) and the pivot column in LDS, 8 (r^2 + r) bytes <= 129 KB at r = 128
__global__ __launch_bounds__(256) void k_lw_inv(LwK k) {
  extern __shared__ double lw_lds[];
  if (!k.w.word[WD_RHOANY]) return;
  const int b = blockIdx.x, r = k.d.r, t = threadIdx.x, rr = r * r;
  if (!k.w.iw[IW_RHOCH * W + b] || k.w.iw[IW_DONE * W + b]) return;      // (uniform over the workgroup)
  double *M = lw_lds, *col = lw_lds + rr;
  for (int e = t; e < rr; e += 256) M[e] = k.d.S[(size_t)e * 64 + b];
  __syncthreads();
  for (int kk = 0; kk < r; kk++) {
    const double p = M[kk * r + kk], ip = (p > 0.0 && p < INFINITY) ? 1.0 / p : NAN;
    __syncthreads();
    for (int j = t; j < r; j += 256) {
      if (j != kk) col[j] = M[j * r + kk];
      M[kk * r + j] = j == kk ? ip : M[kk * r + j] * ip;
    }
    __syncthreads();
    for (int e = t; e < rr; e += 256) {
      const int i = e / r, j = e - i * r;
      if (i != kk) M[e] = (j == kk ? 0.0 : M[e]) - col[i] * M[kk * r + j];
    }
    __syncthreads();
  }
  for (int e = t; e < rr; e += 256) k.d.S[(size_t)e * 64 + b] = M[e];
  if (t == 0) k.d.fact[b] += 1;
}
// out[block][a] = sum over the block's columns j of A_L[a, j] v_j: workgroup = a block of cb columns, wave w takes the rows 8 w .. 8 w + 7, + 32, ..
// MAT: a value is a 512-byte line of the chunk's own WT and no longer a scalar load, so the rows are spread further -- workgroup (column block, eight
// rows), a wave takes two of them (grid: GC x ceil(r / 8), from (n, r) alone) -- and eight columns are in flight: sixteen lines of WT and eight of v are
// requested before the first FMA.  A row's sum keeps the order of the block's columns: the partials are the shared form's, term for term.
template <bool MAT> __device__ __forceinline__ void lw_prod(const LwK &k, const double *v, double *out) {
  const int lane = ls_lane(), wv = ls_wave(), r = k.d.r;
  const double *__restrict__ WT = k.d.WT;
  if constexpr (MAT) {
    const int rg = (r + 7) / 8, g = (int)blockIdx.x / rg, a = ((int)blockIdx.x % rg) * 8 + 2 * wv;
    if (a >= r) return;
    const int j0 = g * k.d.cb, j1 = min(j0 + k.d.cb, k.P.n);
    const bool two = a + 1 < r;                          // (a wave whose second row is past r reads its first row twice and stores once)
    const size_t st = (size_t)r * 64;
    const double *__restrict__ w0 = WT + ((size_t)j0 * r + a) * 64 + lane, *__restrict__ w1 = w0 + (two ? 64 : 0), *__restrict__ vj = v + IX(j0);
    double s0 = 0.0, s1 = 0.0;
    int j = j0;
    for (; j + 8 <= j1; j += 8, w0 += 8 * st, w1 += 8 * st, vj += 8 * 64) {
      double e0[8], e1[8], vv[8];
#pragma unroll
      for (int u = 0; u < 8; u++) { e0[u] = w0[u * st]; e1[u] = w1[u * st]; vv[u] = vj[u * 64]; }
#pragma unroll
      for (int u = 0; u < 8; u++) { s0 += e0[u] * vv[u]; s1 += e1[u] * vv[u]; }
    }
    for (; j < j1; j++, w0 += st, w1 += st, vj += 64) { const double vv = vj[0]; s0 += w0[0] * vv; s1 += w1[0] * vv; }
    out[((size_t)g * r + a) * 64 + lane] = s0;
    if (two) out[((size_t)g * r + a + 1) * 64 + lane] = s1;
  } else {
    const int j0 = (int)blockIdx.x * k.d.cb, j1 = min(j0 + k.d.cb, k.P.n);
    for (int a0 = wv * 8; a0 < r; a0 += 32) {
      double acc[8];
#pragma unroll
      for (int u = 0; u < 8; u++) acc[u] = 0.0;
      for (int j = j0; j < j1; j++) {
        const double vj = v[IX(j)];
        const double *__restrict__ wt = WT + (size_t)j * r + a0;
#pragma unroll
        for (int u = 0; u < 8; u++) acc[u] += (a0 + u < r ? wt[u] : 0.0) * vj;
      }
#pragma unroll
      for (int u = 0; u < 8; u++) if (a0 + u < r) out[((size_t)blockIdx.x * r + a0 + u) * 64 + lane] = acc[u];
    }
  }
}
__global__ __launch_bounds__(256) void k_lw_prod(LwK k, const double *v, double *out) { lw_prod<false>(k, v, out); }
__global__ __launch_bounds__(256) void k_lwm_prod(LwK k, const double *v, double *out) { lw_prod<true>(k, v, out); }
// lw_prod for TWO operands in one pass over WT: out = A_L v and out2 = A_L v2, same grid, same partition, same loops.  Every value of WT is loaded once and
// multiplies both operands; each accumulator receives its terms in lw_prod's order, so both partial sets are those of two lw_prod launches bit for bit.
// MAT: 24 lines in flight per wave and group of eight columns become 32 (sixteen of WT, eight of each operand).  Used by polish's recurrence on the direct
// route (LwRun::long_rows2), where x and x~ are refreshed after every step and WT -- n r 512 bytes per chunk with per-problem matrices -- is the traffic.
template <bool MAT> __device__ __forceinline__ void lw_prod2(const LwK &k, const double *v, const double *v2, double *out, double *out2) {
  const int lane = ls_lane(), wv = ls_wave(), r = k.d.r;
  const double *__restrict__ WT = k.d.WT;
  if constexpr (MAT) {
    const int rg = (r + 7) / 8, g = (int)blockIdx.x / rg, a = ((int)blockIdx.x % rg) * 8 + 2 * wv;
    if (a >= r) return;
    const int j0 = g * k.d.cb, j1 = min(j0 + k.d.cb, k.P.n);
    const bool two = a + 1 < r;
    const size_t st = (size_t)r * 64;
    const double *__restrict__ w0 = WT + ((size_t)j0 * r + a) * 64 + lane, *__restrict__ w1 = w0 + (two ? 64 : 0);
    const double *__restrict__ vj = v + IX(j0), *__restrict__ uj = v2 + IX(j0);
    double s0 = 0.0, s1 = 0.0, t0 = 0.0, t1 = 0.0;
    int j = j0;
    for (; j + 8 <= j1; j += 8, w0 += 8 * st, w1 += 8 * st, vj += 8 * 64, uj += 8 * 64) {
      double e0[8], e1[8], vv[8], uu[8];
#pragma unroll
      for (int u = 0; u < 8; u++) { e0[u] = w0[u * st]; e1[u] = w1[u * st]; vv[u] = vj[u * 64]; uu[u] = uj[u * 64]; }
#pragma unroll
      for (int u = 0; u < 8; u++) { s0 += e0[u] * vv[u]; s1 += e1[u] * vv[u]; t0 += e0[u] * uu[u]; t1 += e1[u] * uu[u]; }
    }
    for (; j < j1; j++, w0 += st, w1 += st, vj += 64, uj += 64) {
      const double e0 = w0[0], e1 = w1[0], vv = vj[0], uu = uj[0];
      s0 += e0 * vv; s1 += e1 * vv; t0 += e0 * uu; t1 += e1 * uu;
    }
    const size_t o = ((size_t)g * r + a) * 64 + lane;
    out[o] = s0; out2[o] = t0;
    if (two) { out[o + 64] = s1; out2[o + 64] = t1; }
  } else {
    const int j0 = (int)blockIdx.x * k.d.cb, j1 = min(j0 + k.d.cb, k.P.n);
    for (int a0 = wv * 8; a0 < r; a0 += 32) {
      double acc[8], acc2[8];
#pragma unroll
      for (int u = 0; u < 8; u++) { acc[u] = 0.0; acc2[u] = 0.0; }
      for (int j = j0; j < j1; j++) {
        const double vj = v[IX(j)], uj = v2[IX(j)];
        const double *__restrict__ wt = WT + (size_t)j * r + a0;
#pragma unroll
        for (int u = 0; u < 8; u++) { const double e = a0 + u < r ? wt[u] : 0.0; acc[u] += e * vj; acc2[u] += e * uj; }
      }
#pragma unroll
      for (int u = 0; u < 8; u++) if (a0 + u < r) { const size_t o = ((size_t)blockIdx.x * r + a0 + u) * 64 + lane; out[o] = acc[u]; out2[o] = acc2[u]; }
    }
  }
}
__global__ __launch_bounds__(256) void k_lw_prod2(LwK k, const double *v, const double *v2, double *out, double *out2) { lw_prod2<false>(k, v, v2, out, out2); }
__global__ __launch_bounds__(256) void k_lwm_prod2(LwK k, const double *v, const double *v2, double *out, double *out2) { lw_prod2<true>(k, v, v2, out, out2); }
// the sum of GC partials `st` doubles apart, in block order, eight loads in flight (the additions keep their order)
__device__ __forceinline__ double lw_fold(const double *s, int GC, size_t st) {
  double a = 0.0;
  int g = 0;
  for (; g + 8 <= GC; g += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) v[u] = s[(size_t)(g + u) * st];
#pragma unroll
    for (int u = 0; u < 8; u++) a += v[u];
  }
  for (; g < GC; g++) a += s[(size_t)g * st];
  return a;
}
// the rows n .. n + r - 1 of x and x~ from the products (the fold of k_lw_prod's two partial sets in block order); at the start those of dx are zero
__global__ __launch_bounds__(256) void k_lw_setl(LwK k, int start) {
  const int lane = ls_lane(), wv = ls_wave(), r = k.d.r, GC = k.d.GC;
  const int live = !k.w.iw[IW_DONE * W + lane];
  for (int a = wv; a < r; a += 4) {
    const double sx = lw_fold(k.d.pg + (size_t)a * 64 + lane, GC, (size_t)r * 64), ss = lw_fold(k.d.pg2 + (size_t)a * 64 + lane, GC, (size_t)r * 64);
    if (live || start) { k.w.x[IX(k.P.n + a)] = sx; k.w.xs[IX(k.P.n + a)] = ss; }
    if (start) k.w.dx[IX(k.P.n + a)] = 0.0;
  }
}
// g = the fold of the partials in block order (every workgroup, into LDS);  h_a = sum_c S^-1[a][c] g_c for the workgroup's 16 rows a, a wave per row;
// (A_L x~)_a += h_a / rho_a
__global__ __launch_bounds__(256) void k_lw_h(LwK k) {
  extern __shared__ double lw_lds[];
  const int lane = ls_lane(), wv = ls_wave(), r = k.d.r, GC = k.d.GC;
  for (int c = wv; c < r; c += 4) {
    lw_lds[c * 64 + lane] = lw_fold(k.d.pg + (size_t)c * 64 + lane, GC, (size_t)r * 64);
  }
  __syncthreads();
  const int live = !k.w.iw[IW_DONE * W + lane], a1 = min(r, (int)blockIdx.x * 16 + 16);
  for (int a = (int)blockIdx.x * 16 + wv; a < a1; a += 4) {
    const double *Sa = k.d.S + (size_t)a * r * 64 + lane;
    double h = 0.0;
    for (int c = 0; c < r; c++) h += Sa[(size_t)c * 64] * lw_lds[c * 64 + lane];
    if (live) { k.d.h[a * 64 + lane] = h; k.w.xs[IX(k.P.n + a)] += h / k.w.rho[IX(k.d.rows[a])]; }
  }
}
// x~_j += p_j - Minv_j sum_a A_L[a, j] h_a  (h in LDS; wave w of workgroup g takes the columns 4 g + w, + 4 G, ..)
// MAT: column j's r values are r consecutive lines of the chunk's own WT, requested eight at a time (with p and Minv in the first group); the sum keeps
// the order of the rows.
template <bool MAT> __device__ __forceinline__ void lw_x(const LwK &k) {
  extern __shared__ double lw_lds[];
  const int lane = ls_lane(), r = k.d.r;
  for (int e = threadIdx.x; e < r * 64; e += 256) lw_lds[e] = k.d.h[e];
  __syncthreads();
  if (k.w.iw[IW_DONE * W + lane]) return;
  const double *__restrict__ WT = k.d.WT;
  for (int j = (int)blockIdx.x * 4 + ls_wave(); j < k.P.n; j += (int)gridDim.x * 4) {
    double s = 0.0;
    if constexpr (MAT) {
      const double *__restrict__ wt = WT + (size_t)j * r * 64 + lane;
      const double pj = k.w.p[IX(j)], mi = k.w.Minv[IX(j)], xj = k.w.xs[IX(j)];
      int a = 0;
      for (; a + 8 <= r; a += 8) {
        double e[8];
#pragma unroll
        for (int u = 0; u < 8; u++) e[u] = wt[(size_t)(a + u) * 64];
#pragma unroll
        for (int u = 0; u < 8; u++) s += e[u] * lw_lds[(a + u) * 64 + lane];
      }
      if (a < r) {
        double e[8];
#pragma unroll
        for (int u = 0; u < 8; u++) e[u] = wt[(size_t)min(a + u, r - 1) * 64];
#pragma unroll
        for (int u = 0; u < 8; u++) if (a + u < r) s += e[u] * lw_lds[(a + u) * 64 + lane];
      }
      k.w.xs[IX(j)] = xj + (pj - mi * s);
    } else {
      const double *__restrict__ wt = WT + (size_t)j * r;
      for (int a = 0; a < r; a++) s += wt[a] * lw_lds[a * 64 + lane];
      k.w.xs[IX(j)] += k.w.p[IX(j)] - k.w.Minv[IX(j)] * s;
    }
  }
}
LW_KERNEL_PAIR(x)
// the view's values: a copy of A's at the one-entry rows, 1.0 at a long row's single entry
__global__ __launch_bounds__(256) void k_lw_vals(int nv, const int *src, const double *Aval, double *out) {
  for (int e = blockIdx.x * 256 + threadIdx.x; e < nv; e += gridDim.x * 256) out[e] = src[e] >= 0 ? Aval[src[e]] : 1.0;
}
// ... and per lane (MAT): entry e of problem b at e * 64 + b, from the chunk's scaled values of A; a wave per entry, its source position wave-uniform
__global__ __launch_bounds__(256) void k_lwm_vals(int nv, const int *src, const double *Aval, double *out) {
  const int lane = ls_lane();
  for (int e = (int)blockIdx.x * 4 + ls_wave(); e < nv; e += (int)gridDim.x * 4) {
    const int sp = __builtin_amdgcn_readfirstlane(src[e]);
    out[IX(e)] = sp >= 0 ? Aval[IX(sp)] : 1.0;
  }
}
// the chunk's own WT: entry (column j, long row a) of problem b at ((j r + a) 64 + b), from the chunk's scaled values of A through the position map
// (pos[j r + a]: where the entry sits in A.val, -1: A_L has none there -- zero).  A wave per entry.
__global__ __launch_bounds__(256) void k_lwm_wt(int cnt, const int *pos, const double *Aval, double *out) {
  const int lane = ls_lane();
  for (int e = (int)blockIdx.x * 4 + ls_wave(); e < cnt; e += (int)gridDim.x * 4) {
    const int sp = __builtin_amdgcn_readfirstlane(pos[e]);
    out[IX(e)] = sp >= 0 ? Aval[IX(sp)] : 0.0;
  }
}
// ---- the backward pass of the direct route (lockstep_direct_adjoint_chunk below).  "adjoint derivatives of a chunk" with the PCG replaced by the solve
// above: rho never changes in the recurrence (alpha = 1, rho_bar = 1 / delta_eff on the active rows, rho_min on the others), so S_b is formed and
// inverted ONCE per problem.  The kernels are those two sections'; what they do not cover is the two below.  With per-problem matrices
// (osqp_hip_batch_adjoint_lockstep_direct_mat) the same pass behind the forward's preparation, on the k_lsm_adj_* twins and the k_lwm_* forms.
// the rows n .. n + r - 1 of `dst` from ONE set of k_lw_prod's partials (pg), folded in block order, for every lane: a wave per row
__global__ __launch_bounds__(256) void k_lwa_setl(LwK k, double *dst) {
  const int lane = ls_lane(), r = k.d.r;
  for (int a = (int)blockIdx.x * 4 + ls_wave(); a < r; a += (int)gridDim.x * 4)
    dst[IX(k.P.n + a)] = lw_fold(k.d.pg + (size_t)a * 64 + lane, k.d.GC, (size_t)r * 64);
}
// the zero start over n + r rows: x = x~ = dx = 0 (k_ls_adj_load_n has the first n rows only, and x~ has held the classification's operand since)
__global__ __launch_bounds__(256) void k_lwa_zero(LwK k) {
  const size_t tot = (size_t)(k.P.n + k.d.r) * 64;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += (size_t)gridDim.x * 256) { k.w.x[e] = 0.0; k.w.xs[e] = 0.0; k.w.dx[e] = 0.0; }
}
// ---------------------------------------------------------------------------------------------------------------- matrices of a chunk
// PER-PROBLEM MATRICES (include/osqp_hip.h osqp_hip_batch_solve_lockstep_mat; LockstepParams::mat_ws): every problem of the chunk has its own values of P
// and A on the handle's sparsity pattern.  The matrix block keeps them problem-minor like every block vector -- entry k of problem b at k * 64 + b -- next to the
// problem's own D, Dinv (n x 64), E, Einv (m x 64); c, 1 / c are rows SC_C / SC_CINV of the scalar state.  In front of the transposes in:
//   assembly       the chunk's rows of Px / Ax go through 64 x 64 LDS tiles (coalesced along the entries on the way in, along the problems on the way out)
//                  to the engine's positions (Dev::AmA / AmB / Pm1 / Pm2; a reordered handle's value maps first).  B's diagonal is zeroed before (k_lsm_begin)
//                  and receives sigma after the equilibration; one writer per (entry, lane): a handle with a repeated (j, j) entry is declined by the engine.
//                  Lanes >= count receive the handle's raw values (and its q): nothing non-finite is manufactured in a dead lane.
//   equilibration  the Ruiz iteration of the single-QP setup (backend_hip.hip ruiz(): _osqp.py:389-497) per lane, with the operand orders of k_ruiz_scale_A /
//                  k_ruiz_scale_B / k_ruiz_cost: dt, et from the row maxima of B, A (k_lsm_norms); A <- et A dt, E *= et, B <- dt [P | A'] [dt | et], q *= dt,
//                  D *= dt and, from the same pass, the column norms of the scaled P and max |q| through ls_put (k_lsm_scale); ct, c *= ct from ls_fold
//                  (k_lsm_cost); P *= ct, q *= ct (k_lsm_cost_apply).  Then Dinv, Einv, 1 / c and sigma on B's diagonal (k_lsm_finish).  Four launches per
//                  iteration.  The scratch lives in block vectors that are dead before k_ls_load_*: dt in r, et in t, the problem's q in q.
// The strips of rows are ls_rows' (from the row counts and the grid alone), so c's sum has a fixed order that depends on (n, m) only.
struct LsMat : LsMatVecs {              // (Aval, Bval, D, Dinv, E, Einv: lockstep_layout.h)
  const double *Praw, *Araw;
  const int *Pm1, *Pm2, *AmA, *AmB, *Bdiag;
  int nzP, nzA;
};
struct LsMK { LockstepParams P; LsWs w; LsMat t; };
__device__ __forceinline__ double ls_limit_scaling(double v) { return v < 1e-4 ? 1.0 : (v > 1e4 ? 1e4 : v); }     // _osqp.py:363-387
// this wave's strip of `nrows` rows (ls_rows' partition)
__device__ __forceinline__ void ls_strip(int nrows, int &r0, int &r1) {
  const int nw = gridDim.x * 4, rpw = (nrows + nw - 1) / nw;
  r0 = ((int)blockIdx.x * 4 + ls_wave()) * rpw; r1 = min(r0 + rpw, nrows);
}
// the problem's raw q (the handle's for lanes >= count) in the engine's numbering, D = E = c = 1, B's diagonal zero.  Grid: the tiles of n.
__global__ __launch_bounds__(256) void k_lsm_begin(LsMK k) {
  __shared__ double tile[64][65];
  const LockstepParams &P = k.P;
  const int lane = ls_lane(), wv = ls_wave(), j0 = blockIdx.x * 64;
  const bool mine = lane < P.count;
  if (P.q) ls_tile_in(P.q, P.n, j0, P.count, P.pc, tile);
  for (int jl = wv; jl < 64 && j0 + jl < P.n; jl += 4) {
    const int j = j0 + jl;
    k.w.q[IX(j)] = (P.q && mine) ? tile[lane][jl] : P.q0[j];
    k.t.D[IX(j)] = 1.0; k.t.Bval[IX(k.t.Bdiag[j])] = 0.0;
  }
  const size_t mt = (size_t)P.m * 64;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < mt; e += (size_t)gridDim.x * 256) k.t.E[e] = 1.0;
  if (blockIdx.x == 0 && threadIdx.x < 64) k.w.sc[SC_C * W + lane] = 1.0;
}
// 64 of the caller's entries per workgroup, 16 per wave: the tile comes in coalesced along the entries; an entry's engine positions are wave-uniform and its
// 64 values leave as one line each.  SYM: P's upper triangle (both mirrored positions of B), else A (A and its copy in B).
template <bool SYM>
__global__ __launch_bounds__(256) void k_lsm_asm(LsMK k) {
  __shared__ double tile[64][65];
  const LockstepParams &P = k.P;
  const int nz = SYM ? k.t.nzP : k.t.nzA, lane = ls_lane(), wv = ls_wave(), e0 = blockIdx.x * 64;
  const double *src = SYM ? P.Px : P.Ax, *raw = SYM ? k.t.Praw : k.t.Araw;
  const int *__restrict__ map = SYM ? P.pvmap : P.avmap;
  const bool own = src != nullptr && lane < P.count;
  if (src) ls_tile_in(src, nz, e0, P.count, nullptr, tile);
  for (int el = wv * 16; el < wv * 16 + 16 && e0 + el < nz; el++) {
    const int e = e0 + el, pos = __builtin_amdgcn_readfirstlane(map ? map[e] : e);
    const double v = own ? tile[lane][el] : raw[pos];
    if (SYM) {
      const int p1 = __builtin_amdgcn_readfirstlane(k.t.Pm1[pos]), p2 = __builtin_amdgcn_readfirstlane(k.t.Pm2[pos]);
      k.t.Bval[IX(p1)] = v;
      if (p2 >= 0 && p2 != p1) k.t.Bval[IX(p2)] = v;
    } else {
      k.t.Aval[IX(__builtin_amdgcn_readfirstlane(k.t.AmA[pos]))] = v; k.t.Bval[IX(__builtin_amdgcn_readfirstlane(k.t.AmB[pos]))] = v;
    }
  }
}
// dt_j = 1 / sqrt(limit(max |row j of B|)) (KKT column j = row j of [P | A']),  et_i = 1 / sqrt(limit(max |row i of A|))
__global__ __launch_bounds__(256) void k_lsm_norms(LsMK k) {
  const int lane = ls_lane();
  int r0, r1;
  ls_strip(k.P.n, r0, r1);
  for (int j = r0; j < r1; j++) {
    const int k0 = __builtin_amdgcn_readfirstlane(k.P.B.rowptr[j]), k1 = __builtin_amdgcn_readfirstlane(k.P.B.rowptr[j + 1]);
    double mx = 0.0;
#pragma unroll 4
    for (int e = k0; e < k1; e++) mx = fmax(mx, fabs(k.t.Bval[IX(e)]));
    k.w.r[IX(j)] = 1.0 / sqrt(ls_limit_scaling(mx));
  }
  ls_strip(k.P.m, r0, r1);
  for (int i = r0; i < r1; i++) {
    const int k0 = __builtin_amdgcn_readfirstlane(k.P.A.rowptr[i]), k1 = __builtin_amdgcn_readfirstlane(k.P.A.rowptr[i + 1]);
    double mx = 0.0;
#pragma unroll 4
    for (int e = k0; e < k1; e++) mx = fmax(mx, fabs(k.t.Aval[IX(e)]));
    k.w.t[IX(i)] = 1.0 / sqrt(ls_limit_scaling(mx));
  }
}
// A <- diag(et) A diag(dt), E *= et;  B <- [diag(dt) P diag(dt) | diag(dt) A' diag(et)], q *= dt, D *= dt;  per problem the sum of the scaled P's column
// norms and max |q| to the partials (slots PS_BN: max |q|, PS_BN + 1: the sum)
__global__ __launch_bounds__(256) void k_lsm_scale(LsMK k) {
  __shared__ double lds[2 * 256];
  const int lane = ls_lane(), n = k.P.n;
  const double *dt = k.w.r, *et = k.w.t;
  int r0, r1;
  ls_strip(k.P.m, r0, r1);
  for (int i = r0; i < r1; i++) {
    const int k0 = __builtin_amdgcn_readfirstlane(k.P.A.rowptr[i]), k1 = __builtin_amdgcn_readfirstlane(k.P.A.rowptr[i + 1]);
    const double ei = et[IX(i)];
    for (int e = k0; e < k1; e++) { const int c = __builtin_amdgcn_readfirstlane(k.P.A.col[e]); k.t.Aval[IX(e)] *= ei * dt[IX(c)]; }
    k.t.E[IX(i)] *= ei;
  }
  double sum = 0.0, nq = 0.0;
  ls_strip(n, r0, r1);
  for (int j = r0; j < r1; j++) {
    const int k0 = __builtin_amdgcn_readfirstlane(k.P.B.rowptr[j]), k1 = __builtin_amdgcn_readfirstlane(k.P.B.rowptr[j + 1]);
    const double dj = dt[IX(j)];
    double mx = 0.0;
    for (int e = k0; e < k1; e++) {
      const int c = __builtin_amdgcn_readfirstlane(k.P.B.col[e]);
      const double v = k.t.Bval[IX(e)] * (c < n ? dt[IX(c)] * dj : et[IX(c - n)] * dj);      // (same factor, same order of operands, as the entry's copy in A)
      k.t.Bval[IX(e)] = v;
      if (c < n) mx = fmax(mx, fabs(v));
    }
    const double qj = k.w.q[IX(j)] * dj;
    k.w.q[IX(j)] = qj; k.t.D[IX(j)] *= dj;
    sum += mx; nq = fmax(nq, fabs(qj));
  }
  const double vm[1] = {nq}, vs[1] = {sum};
  ls_put<1, 1>(k.w.part, PS_BN, vm, vs, lds);
}
// cost normalisation per problem: ct = 1 / limit(max(limit(||q||_inf), mean_j ||P_:j||_inf)),  c *= ct   (_osqp.py:443-448).  One workgroup.
__global__ __launch_bounds__(256) void k_lsm_cost(LsMK k) {
  __shared__ double lds[256];
  const int lane = ls_lane(), G = k.w.G;
  const double nq = ls_fold<true>(k.w.part, G, PS_BN, lds), sum = ls_fold<false>(k.w.part, G, PS_BN + 1, lds);
  if (threadIdx.x >= 64) return;
  const double mean = sum / (double)(k.P.n > 0 ? k.P.n : 1);
  const double ct = 1.0 / ls_limit_scaling(fmax(ls_limit_scaling(nq), mean));
  k.w.sc[SC_CT * W + lane] = ct; k.w.sc[SC_C * W + lane] *= ct;
}
// P <- ct P (the P part comes first in a row of B = [P | A']),  q <- ct q
__global__ __launch_bounds__(256) void k_lsm_cost_apply(LsMK k) {
  const int lane = ls_lane(), n = k.P.n;
  const double ct = k.w.sc[SC_CT * W + lane];
  int r0, r1;
  ls_strip(n, r0, r1);
  for (int j = r0; j < r1; j++) {
    const int k0 = __builtin_amdgcn_readfirstlane(k.P.B.rowptr[j]), k1 = __builtin_amdgcn_readfirstlane(k.P.B.rowptr[j + 1]);
    for (int e = k0; e < k1 && __builtin_amdgcn_readfirstlane(k.P.B.col[e]) < n; e++) k.t.Bval[IX(e)] *= ct;
    k.w.q[IX(j)] *= ct;
  }
}
// Dinv, Einv, 1 / c;  sigma on B's diagonal
__global__ __launch_bounds__(256) void k_lsm_finish(LsMK k) {
  const int lane = ls_lane();
  for (int j = (int)blockIdx.x * 4 + ls_wave(); j < k.P.n; j += (int)gridDim.x * 4) { k.t.Dinv[IX(j)] = 1.0 / k.t.D[IX(j)]; k.t.Bval[IX(k.t.Bdiag[j])] += k.P.sigma; }
  for (int i = (int)blockIdx.x * 4 + ls_wave(); i < k.P.m; i += (int)gridDim.x * 4) k.t.Einv[IX(i)] = 1.0 / k.t.E[IX(i)];
  if (blockIdx.x == 0 && threadIdx.x < 64) k.w.sc[SC_CINV * W + lane] = 1.0 / k.w.sc[SC_C * W + lane];
}
#undef IX

// ---------------------------------------------------------------------------------------------------------------- driving
// The pieces the four chunk functions below are made of, each written once.
inline double ls_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline hipStream_t ls_stream(Dev &d, void *stream) {
  HIP_CHECK(hipSetDevice(d.device));
  return stream ? static_cast<hipStream_t>(stream) : st(d);
}
// What a chunk function holds while it runs: the stream, the launch count, the host's copy of the word block, its events.  The events are destroyed on
// every way out (HIP_CHECK throws); the ones a chunk does not use are never created.
struct LsRun {
  struct Ev {
    hipEvent_t e = nullptr;
    ~Ev() { if (e) (void)hipEventDestroy(e); }
    void record(hipStream_t s) { if (!e) HIP_CHECK(hipEventCreate(&e)); HIP_CHECK(hipEventRecord(e, s)); }
  };
  hipStream_t s;
  const int *dword;                      // the chunk's word block on the device
  int words[WD_COUNT];
  long launches = 0;
  double t_sync;                         // the host's clock when it last waited for the stream: the time the GPU's work is known to have taken
  Ev e0, e1, em, ep0, ep1;               // the chunk; end of the matrix block's preparation; polish
  LsRun(hipStream_t stream, const int *word, int count) : s(stream), dword(word), words{0, count, 0, 0, 0, 0, 0}, t_sync(ls_now()) {}
  template <class K, class A, class... X> void gol(K kern, int grid, size_t lds, const A &a, X... x) { hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, a, x...); launches++; }
  template <class K, class A, class... X> void go(K kern, int grid, const A &a, X... x) { gol(kern, grid, 0, a, x...); }
  void fetch() { HIP_CHECK(hipMemcpyAsync(words, dword, sizeof(words), hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s)); t_sync = ls_now(); }
  static float ms(const Ev &a, const Ev &b) { float v = 0.f; HIP_CHECK(hipEventElapsedTime(&v, a.e, b.e)); return v; }
  // the end of a chunk: the last read of the words (with dfact: the direct route's inversion counts, summed into *nfact), the chunk's GPU ms
  float finish(const int *dfact = nullptr, long *nfact = nullptr) {
    int fact[W];
    e1.record(s);
    if (dfact) HIP_CHECK(hipMemcpyAsync(fact, dfact, sizeof(fact), hipMemcpyDeviceToHost, s));
    fetch();
    const float v = ms(e0, e1);
    HIP_CHECK(hipGetLastError());
    if (dfact) { *nfact = 0; for (int b = 0; b < W; b++) *nfact += fact[b]; }
    return v;
  }
};

// The kernels of the PCG route that come in two instantiations: on the handle's matrices, on the chunk's own ("matrices of a chunk")
using LsKern = void (*)(LsK);
struct LsPcgKernels {
  LsKern load_n, load_m, minv, initz, rhs, t, kp, upd, resm, resn;
  void (*decide)(LsK, int, int, int, int);
  LsKern store_n, store_m;
};
constexpr LsPcgKernels kLsShared = {k_ls_load_n, k_ls_load_m, k_ls_minv, k_ls_initz, k_ls_rhs, k_ls_t, k_ls_kp, k_ls_upd, k_ls_resm, k_ls_resn, k_ls_decide, k_ls_store_n, k_ls_store_m};
constexpr LsPcgKernels kLsOwnMat = {k_lsm_load_n, k_lsm_load_m, k_lsm_minv, k_lsm_initz, k_lsm_rhs, k_lsm_t, k_lsm_kp, k_lsm_upd, k_lsm_resm, k_lsm_resn, k_lsm_decide, k_lsm_store_n, k_lsm_store_m};

// ONE LAUNCH of a forward kernel of the PCG route, by its public name (include/osqp_hip.h OSQPHipLockstepOp): the kernel, its arguments and ITS GRID are
// stated here once, for every driver below and for the diagnostic entry (test_lockstep), which therefore launches what a solve launches.  The grids: G
// workgroups for the row passes and the elementwise kernels (k.w.G: lockstep_grid), the 64-wide tiles of n / m for the transposes, one workgroup for the
// folds and the state.  (decide is launched where it is used; the adjoint's and polish's kernels: ls_adj_go / ls_pol_go; the direct route's own: LwRun::go / lwa_go.)
inline int ls_tiles(int cnt) { return (cnt + 63) / 64; }
void ls_go(LsRun &R, const LsPcgKernels &K, int op, const LsK &k) {
  const int G = k.w.G, tn = ls_tiles(k.P.n), tm = ls_tiles(k.P.m);
  switch (op) {
    case OSQP_HIP_LS_LOAD_N: R.go(K.load_n, tn, k); break;
    case OSQP_HIP_LS_LOAD_M: R.go(K.load_m, tm, k); break;
    case OSQP_HIP_LS_INIT: R.go(k_ls_init, 1, k, k.P.m > 0 ? tm : 0); break;
    case OSQP_HIP_LS_STORE_N: R.go(K.store_n, tn, k); break;
    case OSQP_HIP_LS_STORE_M: R.go(K.store_m, tm, k); break;
    case OSQP_HIP_LS_MINV: R.go(K.minv, G, k); break;
    case OSQP_HIP_LS_INITZ: R.go(K.initz, G, k); break;
    case OSQP_HIP_LS_RHS: R.go(K.rhs, G, k); break;
    case OSQP_HIP_LS_T: R.go(K.t, G, k); break;
    case OSQP_HIP_LS_KP: R.go(K.kp, G, k); break;
    case OSQP_HIP_LS_UPD: R.go(K.upd, G, k); break;
    case OSQP_HIP_LS_RESM: R.go(K.resm, G, k); break;
    case OSQP_HIP_LS_RESN: R.go(K.resn, G, k); break;
    case OSQP_HIP_LS_SETRHO: R.go(k_ls_setrho, G, k); break;
    case OSQP_HIP_LS_CGUPD: R.go(k_ls_cgupd, G, k); break;
    case OSQP_HIP_LS_CGP: R.go(k_ls_cgp, G, k); break;
    case OSQP_HIP_LS_CGINIT: R.go(k_ls_cginit, 1, k); break;
    case OSQP_HIP_LS_CGALPHA: R.go(k_ls_cgalpha, 1, k); break;
    case OSQP_HIP_LS_CGBETA: R.go(k_ls_cgbeta, 1, k); break;
    case OSQP_HIP_LS_SUPP: R.go(k_ls_supp, G, k); break;
    default: throw std::logic_error("ls_go: not a forward kernel of the PCG route");
  }
}
// the same for the matrices of a chunk: 64 stored entries per workgroup for the assembly
void ls_mat_go(LsRun &R, int op, const LsMK &km) {
  const int G = km.w.G;
  switch (op) {
    case OSQP_HIP_LS_BEGIN: R.go(k_lsm_begin, ls_tiles(km.P.n), km); break;
    case OSQP_HIP_LS_ASM_A: R.go(k_lsm_asm<false>, ls_tiles(km.t.nzA), km); break;
    case OSQP_HIP_LS_ASM_P: R.go(k_lsm_asm<true>, ls_tiles(km.t.nzP), km); break;
    case OSQP_HIP_LS_NORMS: R.go(k_lsm_norms, G, km); break;
    case OSQP_HIP_LS_SCALE: R.go(k_lsm_scale, G, km); break;
    case OSQP_HIP_LS_COST: R.go(k_lsm_cost, 1, km); break;
    case OSQP_HIP_LS_COST_APPLY: R.go(k_lsm_cost_apply, G, km); break;
    case OSQP_HIP_LS_FINISH: R.go(k_lsm_finish, G, km); break;
    default: throw std::logic_error("ls_mat_go: not a kernel of the matrices of a chunk");
  }
}

// One PCG solve for every problem of the chunk: as many iterations as the previous solve needed (+ 1: est) are enqueued without synchronising; then the
// host reads the words and goes on in groups of four while some problem's PCG is still running, up to cg_max.  The estimate decides how many launches
// return at once, never how far a problem's PCG runs.
void ls_pcg(LsRun &R, const LsPcgKernels &K, const LsK &k, int &est) {
  const int cg_max = k.P.cg_max;
  ls_go(R, K, OSQP_HIP_LS_RHS, k);
  ls_go(R, K, OSQP_HIP_LS_CGINIT, k);
  for (int it = 0, grp = est; it < cg_max; grp = 4) {
    for (const int end = std::min(it + grp, cg_max); it < end; it++) {
      if (k.P.m > 0) ls_go(R, K, OSQP_HIP_LS_T, k);
      ls_go(R, K, OSQP_HIP_LS_KP, k); ls_go(R, K, OSQP_HIP_LS_CGALPHA, k); ls_go(R, K, OSQP_HIP_LS_CGUPD, k); ls_go(R, K, OSQP_HIP_LS_CGBETA, k); ls_go(R, K, OSQP_HIP_LS_CGP, k);
    }
    R.fetch();
    if (!R.words[WD_CGANY]) break;
  }
  est = std::max(2, R.words[WD_CGIT] + 1);
}

// The recurrence of polish and of the adjoints: while a problem is live and below the step cap -- step() (the solve and k_ls_upd), the residuals (K: the
// handle's matrices or the chunk's own; km: what K.resm reads A through), decide(), a read of the words.  Returns the steps taken.
template <class Step, class Decide>
int ls_recurrence(LsRun &R, const LsPcgKernels &K, const LsK &km, const LsK &kn, int max_steps, Step step, Decide decide) {
  int steps = 0;
  while (R.words[WD_LIVE] > 0 && steps < max_steps) {
    steps++;
    step();
    if (km.P.m > 0) ls_go(R, K, OSQP_HIP_LS_RESM, km);
    ls_go(R, K, OSQP_HIP_LS_RESN, kn);
    decide();
    R.fetch();
  }
  return steps;
}

// The matrices of a chunk ("matrices of a chunk" above), for the forward and the backward pass alike.  ls_mat_block: the carve of the matrix block -- asked
// "does it fit" before any event or launch -- and P's matrices and scalings pointed at it.  ls_mat_prepare: the assembly and the equilibration, in front of
// the chunk's transposes in; R.em marks their end, mat_stat[1] is their launch count.  The scratch (dt in r, et in t, the problem's q in q) and the rows
// SC_C / SC_CINV / SC_CT belong to the work block of the chunk that calls.
int ls_mat_block(const Dev &d, LockstepParams &P, LsMat &mt) {
  LsCursor cm{P.mat_ws};
  if (!d.Praw || !d.Araw) return OSQP_FUNC_NOT_IMPLEMENTED;
  if (!lockstep_mat_layout(cm, P.n, P.m, P.A.nnz, P.B.nnz, mt)) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  mt.Praw = d.Praw; mt.Araw = d.Araw; mt.Pm1 = d.Pm1; mt.Pm2 = d.Pm2; mt.AmA = d.AmA; mt.AmB = d.AmB; mt.Bdiag = d.Bdiag; mt.nzP = d.nzP; mt.nzA = d.nzA;
  P.A.val = mt.Aval; P.B.val = mt.Bval; P.D = mt.D; P.Dinv = mt.Dinv; P.E = mt.E; P.Einv = mt.Einv;
  return OSQP_NO_ERROR;
}
void ls_mat_prepare(LsRun &R, const LsMK &km) {
  const long launches0 = R.launches;
  ls_mat_go(R, OSQP_HIP_LS_BEGIN, km);
  if (km.t.nzA > 0) ls_mat_go(R, OSQP_HIP_LS_ASM_A, km);
  if (km.t.nzP > 0) ls_mat_go(R, OSQP_HIP_LS_ASM_P, km);
  for (int it = 0; it < km.P.mat_iters; it++) { ls_mat_go(R, OSQP_HIP_LS_NORMS, km); ls_mat_go(R, OSQP_HIP_LS_SCALE, km); ls_mat_go(R, OSQP_HIP_LS_COST, km); ls_mat_go(R, OSQP_HIP_LS_COST_APPLY, km); }
  ls_mat_go(R, OSQP_HIP_LS_FINISH, km);
  R.em.record(R.s);
  if (km.P.mat_stat) km.P.mat_stat[1] = (double)(R.launches - launches0);
}

// ONE LAUNCH of a kernel of the backward pass, by its public name (include/osqp_hip.h OSQPHipLockstepBackOp): the kernel -- on the handle's matrices or, mat, its
// twin on the chunk's own --, its arguments and ITS GRID are stated here once, for both backward passes and for the diagnostic entry (test_lockstep_back).
// The grids: the 64-wide tiles of n / m for the transposes, G for the row passes and the elementwise kernel, one workgroup for the folds and the state, 64
// stored entries per workgroup for the gradients.  ka: the argument view the caller's route gives the op (LwAdjViews on the direct route).
void ls_adj_go(LsRun &R, bool mat, int op, const LsAK &ka) {
  const LockstepAdjointParams &p = ka.P;
  const int G = ka.w.G, tn = ls_tiles(p.n), tm = ls_tiles(p.m);
  switch (op) {
    case OSQP_HIP_LSB_ADJ_LOAD_N: R.go(mat ? k_lsm_adj_load_n : k_ls_adj_load_n, tn, ka); break;
    case OSQP_HIP_LSB_ADJ_LOAD_M: R.go(k_ls_adj_load_m, tm, ka); break;
    case OSQP_HIP_LSB_ADJ_CLASS: R.go(mat ? k_lsm_adj_class : k_ls_adj_class, G, ka); break;
    case OSQP_HIP_LSB_ADJ_INIT: R.go(k_ls_adj_init, 1, ka); break;
    case OSQP_HIP_LSB_ADJ_DECIDE: R.go(k_ls_adj_decide, 1, ka); break;
    case OSQP_HIP_LSB_ADJ_UNSCALE: R.go(mat ? k_lsm_adj_unscale : k_ls_adj_unscale, G, ka); break;
    case OSQP_HIP_LSB_ADJ_RESM: R.go(mat ? k_lsm_adj_resm : k_ls_adj_resm, G, ka); break;
    case OSQP_HIP_LSB_ADJ_RESN: R.go(mat ? k_lsm_adj_resn : k_ls_adj_resn, G, ka); break;
    case OSQP_HIP_LSB_ADJ_FINAL: R.go(k_ls_adj_final, 1, ka); break;
    case OSQP_HIP_LSB_ADJ_OUT_N: R.go(k_ls_adj_out_n, tn, ka); break;
    case OSQP_HIP_LSB_ADJ_OUT_M: R.go(k_ls_adj_out_m, tm, ka); break;
    case OSQP_HIP_LSB_ADJ_GRAD_P: R.go(k_ls_adj_grad<true>, (p.nzP + 63) / 64, ka); break;
    case OSQP_HIP_LSB_ADJ_GRAD_A: R.go(k_ls_adj_grad<false>, (p.nzA + 63) / 64, ka); break;
    default: throw std::logic_error("ls_adj_go: not a kernel of the backward pass");
  }
}
// the same for polish: one workgroup for the state, the decisions and the accept test, G for the elementwise kernels and the row pass
void ls_pol_go(LsRun &R, bool mat, int op, const LsPK &kq, double secs = 0.0) {
  const int G = kq.w.G;
  switch (op) {
    case OSQP_HIP_LSB_POL_BEGIN: R.go(k_ls_pol_begin, 1, kq); break;
    case OSQP_HIP_LSB_POL_CLASS: R.go(k_ls_pol_class, G, kq); break;
    case OSQP_HIP_LSB_POL_DECIDE: R.go(k_ls_pol_decide, 1, kq); break;
    case OSQP_HIP_LSB_POL_CONE: R.go(mat ? k_lsm_pol_cone : k_ls_pol_cone, G, kq); break;
    case OSQP_HIP_LSB_POL_ACCEPT: R.go(mat ? k_lsm_pol_accept : k_ls_pol_accept, 1, kq); break;
    case OSQP_HIP_LSB_POL_END: R.go(k_ls_pol_end, G, kq, secs); break;
    default: throw std::logic_error("ls_pol_go: not a kernel of polish");
  }
}

// The adjoint's launches after the recurrence that both backward passes share: the outputs the caller asked for
void ls_adjoint_outputs(LsRun &R, bool mat, const LsAK &ka) {
  const LockstepAdjointParams &p = ka.P;
  if (p.dq) ls_adj_go(R, mat, OSQP_HIP_LSB_ADJ_OUT_N, ka);
  if (p.m > 0 && (p.dl || p.du)) ls_adj_go(R, mat, OSQP_HIP_LSB_ADJ_OUT_M, ka);
  if (p.dP && p.nzP > 0) ls_adj_go(R, mat, OSQP_HIP_LSB_ADJ_GRAD_P, ka);
  if (p.dA && p.nzA > 0) ls_adj_go(R, mat, OSQP_HIP_LSB_ADJ_GRAD_A, ka);
}

// The direct route's kernel arguments and launch groups.  k: what k_lw_* take.  Of this file's other kernels kb sees the handle as it is, kv reads A
// through the view, ku does too and runs k_ls_upd's elementwise loop over n + r rows.
struct LwRun {
  LwK k;
  LsK kb, kv, ku;
  int G, r, GC;
  size_t lds_inv, lds_h;
  bool mat;                              // per-problem matrices: p's A / B / scalings, v.Av.val and v.WT are the chunk's own blocks, the kernels the MAT forms
  LwRun(const LockstepParams &p, const LockstepDirectView &v, const LsWs &w, const LwVecs &d, bool own = false) : k{p, w, {}}, kb{p, w}, mat(own) {
    const int cb = lockstep_direct_colblock(p.n);
    G = w.G; r = v.r; GC = lockstep_direct_colblocks(p.n);
    static_cast<LwVecs &>(k.d) = d;
    k.d.WT = v.WT; k.d.rows = v.rows; k.d.islong = v.islong; k.d.r = r; k.d.GC = GC; k.d.cb = cb;
    kv = kb; kv.P.A = v.Av;
    ku = kv; ku.P.n = p.n + r;            // (k_ls_upd reads no scaling: nothing launched with ku indexes D .. Einv)
    lds_inv = sizeof(double) * ((size_t)r * r + r); lds_h = sizeof(double) * (size_t)r * 64;
    if (lds_inv > 64 * 1024) HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_lw_inv), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_inv));
  }
  const LsPcgKernels &K() const { return mat ? kLsOwnMat : kLsShared; }
  // the chunk's own dense rows and view values (per-problem matrices): what k_lwm_wt / k_lwm_vals fill, from the matrix block's scaled A
  const double *Aval = nullptr; const int *wtpos = nullptr, *vsrc = nullptr; double *WTown = nullptr, *vval = nullptr; int nv = 0;
  void own(const double *aval, const LockstepDirectView &v, const LwMatVecs &xm) { Aval = aval; wtpos = v.wtpos; vsrc = v.vsrc; WTown = xm.WT; vval = xm.vval; nv = v.Av.nnz; }
  // ONE LAUNCH of the direct route, by its public name (include/osqp_hip.h OSQPHipLockstepOp): kernel, arguments, grid and dynamic LDS stated here once, for
  // the launch groups below, the chunk functions and the diagnostic entry (test_lockstep).  The PCG route's kernels this route reuses go through ls_go with
  // the argument view that belongs to them: initz and resm read A through the view (kv), upd runs over n + r rows (ku), the others see the handle (kb).
  // The grids: G for d0 and x, a workgroup per (row a, eight columns) of S, a workgroup per problem for the inversion (S_b and a column in dynamic LDS,
  // raised above 64 KB in the constructor), the column blocks for the products -- times the groups of eight rows with per-problem matrices --, one
  // workgroup for setl, sixteen rows of h per workgroup, a wave per entry (at most 1024 workgroups) for the chunk's own WT and view values.
  const LsK &arg(int op) const { return (op == OSQP_HIP_LS_INITZ || op == OSQP_HIP_LS_RESM) ? kv : (op == OSQP_HIP_LS_UPD ? ku : kb); }
  void prod_to(LsRun &R, const double *v, double *out) const { if (mat) R.go(k_lwm_prod, GC * ((r + 7) / 8), k, v, out); else R.go(k_lw_prod, GC, k, v, out); }
  void go(LsRun &R, int op) const {
    switch (op) {
      case OSQP_HIP_LS_D0: R.go(mat ? k_lwm_d0 : k_lw_d0, G, k); break;
      case OSQP_HIP_LS_S: R.go(mat ? k_lwm_s : k_lw_s, r * ((r + 7) / 8), k); break;
      case OSQP_HIP_LS_INV: R.gol(k_lw_inv, W, lds_inv, k); break;
      case OSQP_HIP_LS_PROD_X: prod_to(R, k.w.x, k.d.pg); break;
      case OSQP_HIP_LS_PROD_XS: prod_to(R, k.w.xs, k.d.pg2); break;
      case OSQP_HIP_LS_PROD_P: prod_to(R, k.w.p, k.d.pg); break;
      case OSQP_HIP_LS_PROD2:
        if (mat) R.go(k_lwm_prod2, GC * ((r + 7) / 8), k, (const double *)k.w.x, (const double *)k.w.xs, k.d.pg, k.d.pg2);
        else R.go(k_lw_prod2, GC, k, (const double *)k.w.x, (const double *)k.w.xs, k.d.pg, k.d.pg2);
        break;
      case OSQP_HIP_LS_SETL0: R.go(k_lw_setl, 1, k, 0); break;
      case OSQP_HIP_LS_SETL1: R.go(k_lw_setl, 1, k, 1); break;
      case OSQP_HIP_LS_H: R.gol(k_lw_h, (r + 15) / 16, lds_h, k); break;
      case OSQP_HIP_LS_X: R.gol(mat ? k_lwm_x : k_lw_x, G, lds_h, k); break;
      case OSQP_HIP_LS_WT: { const int nwt = k.P.n * r; R.go(k_lwm_wt, std::min(1024, (nwt + 3) / 4), nwt, wtpos, Aval, WTown); break; }
      case OSQP_HIP_LS_VALS: R.go(k_lwm_vals, std::min(1024, (nv + 3) / 4), nv, vsrc, Aval, vval); break;
      default: ls_go(R, K(), op, arg(op));
    }
  }
  // x -> pg for another operand (the adjoint's and polish's own vectors)
  void prod(LsRun &R, const double *v, double *out) const { prod_to(R, v, out); }
  // ONE LAUNCH of the two kernels the direct backward pass and the direct polish add (OSQPHipLockstepBackOp LWA_*): a wave per long row for k_lwa_setl -- into
  // x or into x~ --, G for the zero start over n + r rows
  void lwa_go(LsRun &R, int op) const {
    switch (op) {
      case OSQP_HIP_LSB_LWA_SETL_X: R.go(k_lwa_setl, (r + 3) / 4, k, k.w.x); break;
      case OSQP_HIP_LSB_LWA_SETL_XS: R.go(k_lwa_setl, (r + 3) / 4, k, k.w.xs); break;
      case OSQP_HIP_LSB_LWA_ZERO: R.go(k_lwa_zero, G, k); break;
      default: throw std::logic_error("LwRun::lwa_go: not a kernel of the direct backward pass");
    }
  }
  // rho from rho_bar, D0, S and its inverse (for the problems whose rho has just been set)
  void factor(LsRun &R) const { go(R, OSQP_HIP_LS_SETRHO); go(R, OSQP_HIP_LS_D0); go(R, OSQP_HIP_LS_S); go(R, OSQP_HIP_LS_INV); }
  // x~ by the Woodbury formula, then the ADMM update
  void solve(LsRun &R) const { go(R, OSQP_HIP_LS_RHS); go(R, OSQP_HIP_LS_PROD_P); go(R, OSQP_HIP_LS_H); go(R, OSQP_HIP_LS_X); go(R, OSQP_HIP_LS_UPD); }
  // the rows n .. n + r - 1 of x and x~ from the products
  void long_rows(LsRun &R, int start) const { go(R, OSQP_HIP_LS_PROD_X); go(R, OSQP_HIP_LS_PROD_XS); go(R, start ? OSQP_HIP_LS_SETL1 : OSQP_HIP_LS_SETL0); }
  // the same rows with both products from one pass over WT (k_lw_prod2: the same partials bit for bit); polish's recurrence
  void long_rows2(LsRun &R) const { go(R, OSQP_HIP_LS_PROD2); go(R, OSQP_HIP_LS_SETL0); }
  // the chunk's own dense rows and view values from the matrix block's scaled A (per-problem matrices; after ls_mat_prepare)
  void own_rows(LsRun &R) const { go(R, OSQP_HIP_LS_WT); go(R, OSQP_HIP_LS_VALS); }
};
// The direct backward pass's argument views, stated once for the driver and the diagnostic entry: kl makes k_ls_adj_load_n put x~ = Dinv x where
// k_ls_adj_class, through the view (kc), will gather it -- the first n rows of the block vector x~ -- by exchanging the roles of p and x~ (the zeros then go
// to p, which k_ls_rhs overwrites); k_ls_adj_resm reads A through the view too.  With per-problem matrices kc's A is the view on the chunk's per-lane values
// ([nv][64]); E, Einv, D, Dinv are the block's in all three (ka.P after ls_mat_block).
struct LwAdjViews {
  LsAK ka, kl, kc;
  LwAdjViews(const LsAK &a, const DevCsr &Av) : ka(a), kl(a), kc(a) { kl.w.p = a.w.xs; kl.w.xs = a.w.p; kc.P.A = Av; kc.w.p = a.w.xs; }
  const LsAK &arg(int op) const { return op == OSQP_HIP_LSB_ADJ_LOAD_N ? kl : ((op == OSQP_HIP_LSB_ADJ_CLASS || op == OSQP_HIP_LSB_ADJ_RESM) ? kc : ka); }
};

}  // namespace

// One chunk of at most kLsW problems, from the transposes in to the transposes out, on `stream` (nullptr: the solver's); returns when the chunk's
// results are in p.x / p.y / p.rec.  The time limit is tested against the host's clock in every iteration.
// stat: {ADMM iterations of the slowest problem, PCG iterations summed, kernel launches, GPU ms}.
int lockstep_chunk(Dev &d, const LockstepParams &p, void *stream, double *stat) {
  const hipStream_t s = ls_stream(d, stream);
  const int n = p.n, m = p.m;
  const bool mat = p.mat_ws != nullptr, pol = p.polish && p.pol_ws;
  LsK k{p, {}};
  LsMat mt{};
  LsPK kq{p, {}, {}};
  LsCursor c{p.ws}, cp{p.pol_ws};
  if (!lockstep_layout(c, n, m, k.w, nullptr)) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  // per-problem matrices ("matrices of a chunk" above): the chunk's kernels read the matrix block in place of the handle's arrays
  if (mat) if (const int err = ls_mat_block(d, k.P, mt)) return err;
  if (pol && !lockstep_polish_layout(cp, n, m, kq.s)) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  const LsWs &w = k.w;
  const LsPcgKernels &K = mat ? kLsOwnMat : kLsShared;
  LsRun R(s, w.word, p.count);
  R.e0.record(s);
  if (mat) ls_mat_prepare(R, LsMK{k.P, w, mt});
  const double t_begin = ls_now();
  auto late_now = [&]() { return p.time_limit > 0 && ls_now() - t_begin > p.time_limit; };
  auto residuals = [&]() { if (m > 0) ls_go(R, K, OSQP_HIP_LS_RESM, k); ls_go(R, K, OSQP_HIP_LS_RESN, k); };
  auto new_rho = [&]() { if (m > 0) ls_go(R, K, OSQP_HIP_LS_SETRHO, k); ls_go(R, K, OSQP_HIP_LS_MINV, k); };
  const bool gap_check = p.check_dualgap && m > 0;       // settings.check_dualgap: k_ls_supp in front of every decision that tests termination (m = 0: no support term)

  ls_go(R, K, OSQP_HIP_LS_LOAD_N, k);
  if (m > 0) ls_go(R, K, OSQP_HIP_LS_LOAD_M, k);
  ls_go(R, K, OSQP_HIP_LS_INIT, k);
  new_rho();
  if (m > 0) ls_go(R, K, OSQP_HIP_LS_INITZ, k);
  residuals();
  R.go(K.decide, 1, k, 0, 0, 0, 1);
  int iter = 0, cg_est = 4;
  while (R.words[WD_LIVE] > 0 && iter < p.max_iter) {
    iter++;
    ls_pcg(R, K, k, cg_est);
    ls_go(R, K, OSQP_HIP_LS_UPD, k);
    const int at_check = (p.check > 0 && iter % p.check == 0) || iter >= p.max_iter;
    const int at_rho = p.rho_interval > 0 && iter % p.rho_interval == 0;
    const bool late = late_now();
    if (!at_check && !at_rho && !late) continue;
    residuals();
    if (gap_check && (at_check || late)) ls_go(R, K, OSQP_HIP_LS_SUPP, k);
    R.go(K.decide, 1, k, iter, late ? 1 : at_check, at_rho, late ? 2 : 0);
    if (at_rho && !late) new_rho();
    if (at_check || late) R.fetch();
  }
  // polish ("polish of a chunk" above).  A chunk whose time limit has passed does not polish.
  const bool polished = pol && !late_now();
  int pcg_admm = 0, pol_steps = 0, pol_pcg = 0, pol_att = 0;
  long pol_launches = 0;
  if (polished) {
    const long launches0 = R.launches;
    const double t_pol = ls_now();
    kq.P = k.P; kq.w = w;                              // (k.P: with a matrix block, A.val, B.val, D .. Einv point at it)
    LsK kp = k;                                        // what the ADMM's kernels take in the recurrence: alpha = 1, the recurrence's PCG rule
    kp.P.alpha = 1.0; kp.P.cg_max = p.pol_cg_max; kp.P.pcg_rel = p.pol_pcg_rel;
    R.ep0.record(s);
    ls_pol_go(R, mat, OSQP_HIP_LSB_POL_BEGIN, kq);
    R.fetch();                                         // (WD_PCGSUM: still the ADMM's)
    pcg_admm = R.words[WD_PCGSUM]; pol_att = R.words[WD_LIVE];
    if (pol_att > 0) {
      ls_pol_go(R, mat, OSQP_HIP_LSB_POL_CLASS, kq);
      if (m > 0) ls_go(R, K, OSQP_HIP_LS_SETRHO, kp);
      ls_go(R, K, OSQP_HIP_LS_MINV, kp);
      int cg_pol = 4;
      pol_steps = ls_recurrence(R, K, kp, kp, kLsPolMaxSteps, [&]() { ls_pcg(R, K, kp, cg_pol); ls_go(R, K, OSQP_HIP_LS_UPD, kp); }, [&]() { ls_pol_go(R, mat, OSQP_HIP_LSB_POL_DECIDE, kq); });
      pol_pcg = R.words[WD_PCGSUM];
      if (m > 0) { ls_pol_go(R, mat, OSQP_HIP_LSB_POL_CONE, kq); ls_go(R, K, OSQP_HIP_LS_RESM, kp); }
      ls_go(R, K, OSQP_HIP_LS_RESN, kp);
      if (gap_check) ls_go(R, K, OSQP_HIP_LS_SUPP, kp);  // (the polished y against the bounds k_ls_pol_cone has put back: an accepted problem's column 11)
      ls_pol_go(R, mat, OSQP_HIP_LSB_POL_ACCEPT, kq);
      R.fetch();
      ls_pol_go(R, mat, OSQP_HIP_LSB_POL_END, kq, ls_now() - t_pol);
    }
    R.ep1.record(s);
    pol_launches = R.launches - launches0;
  }
  ls_go(R, K, OSQP_HIP_LS_STORE_N, k);
  if (m > 0) ls_go(R, K, OSQP_HIP_LS_STORE_M, k);
  const float ms = R.finish(), pms = polished ? LsRun::ms(R.ep0, R.ep1) : 0.f;
  if (mat && p.mat_stat) p.mat_stat[0] = LsRun::ms(R.e0, R.em);
  // (the chunk's statistics are the ADMM part's; polish's go to their own block)
  if (stat) { stat[0] = iter; stat[1] = polished ? pcg_admm : R.words[WD_PCGSUM]; stat[2] = (double)(R.launches - pol_launches); stat[3] = ms - pms; }
  if (polished && p.pol_stat) {
    double *ps = p.pol_stat;
    ps[0] = pol_att; ps[1] = R.words[WD_POLACC]; ps[2] = R.words[WD_POLREJ]; ps[3] = pol_steps; ps[4] = pol_pcg; ps[5] = (double)pol_launches; ps[6] = pms;
  }
  return OSQP_NO_ERROR;
}

// Diagnostic (backend.h LsProbe; include/osqp_hip.h osqp_hip_test_lockstep, which has validated everything and uploaded the blocks): the carve of
// lockstep_chunk, then the listed ops -- one launch each through ls_go / ls_mat_go, the drivers' own launch text -- on the solver's stream.  No host loop,
// no event, no read of the words.
int test_lockstep(Dev &d, const LsProbe &t) {
  const hipStream_t s = ls_stream(d, nullptr);
  const int n = t.p.n, m = t.p.m;
  const bool mat = t.p.mat_ws != nullptr;
  LockstepDirectParams p = t.p;
  LsWs w;
  LsMat mt{};
  LsCursor c{p.ws};
  if (!t.direct) {
    if (!lockstep_layout(c, n, m, w, nullptr)) return OSQP_WORKSPACE_NOT_INIT_ERROR;
    if (mat) if (const int err = ls_mat_block(d, p, mt)) return err;
    const LsK k{p, w};
    const LsPcgKernels &K = mat ? kLsOwnMat : kLsShared;
    const LsMK km{p, w, mt};
    LsRun R(s, w.word, p.count);
    for (int i = 0; i < t.nops; i++) {
      if (t.ops[i] >= OSQP_HIP_LS_BEGIN && t.ops[i] <= OSQP_HIP_LS_FINISH) ls_mat_go(R, t.ops[i], km);
      else ls_go(R, K, t.ops[i], k);
    }
  } else {                                               // the direct route: lockstep_direct_chunk's carve and LwRun
    const int r = p.v.r;
    LwVecs x;
    LwMatVecs xm{};
    if (!lockstep_direct_layout(c, n, m, r, w, x, nullptr)) return OSQP_WORKSPACE_NOT_INIT_ERROR;
    if (mat) {
      if (!p.v.wtpos || !p.v.vsrc) return OSQP_FUNC_NOT_IMPLEMENTED;
      if (const int err = ls_mat_block(d, p, mt)) return err;
      LsCursor cm{p.mat_ws};
      LsMatVecs again;
      if (!lockstep_direct_mat_layout(cm, n, m, r, p.A.nnz, p.B.nnz, p.v.Av.nnz, again, xm)) return OSQP_WORKSPACE_NOT_INIT_ERROR;
      p.v.WT = xm.WT; p.v.Av.val = xm.vval;
    }
    LwRun D(p, p.v, w, x, mat);
    if (mat) D.own(mt.Aval, p.v, xm);
    const LsMK km{p, w, mt};
    LsRun R(s, w.word, p.count);
    for (int i = 0; i < t.nops; i++) {
      if (t.ops[i] >= OSQP_HIP_LS_BEGIN && t.ops[i] <= OSQP_HIP_LS_FINISH) ls_mat_go(R, t.ops[i], km);
      else D.go(R, t.ops[i]);
    }
  }
  HIP_CHECK(hipStreamSynchronize(s));
  HIP_CHECK(hipGetLastError());
  return OSQP_NO_ERROR;
}

// Diagnostic (backend.h LsBackProbe; include/osqp_hip.h osqp_hip_test_lockstep_back, which has validated everything and uploaded the blocks): the carve of
// the backward pass (lockstep_adjoint_chunk / lockstep_direct_adjoint_chunk) or of a polishing chunk (lockstep_chunk / lockstep_direct_chunk), then the
// listed ops -- one launch each through ls_adj_go / ls_pol_go / LwRun::lwa_go with the drivers' argument views -- on the solver's stream.  No host loop.
int test_lockstep_back(Dev &d, LsBackProbe &t) {
  const hipStream_t s = ls_stream(d, nullptr);
  const LockstepParams &base = t.polish ? static_cast<const LockstepParams &>(t.p) : static_cast<const LockstepParams &>(t.a);
  const int n = base.n, m = base.m;
  const bool mat = base.mat_ws != nullptr, direct = t.direct;
  t.pol_max_steps = kLsPolMaxSteps;
  LockstepDirectView v = t.polish ? t.p.v : t.a.v;
  const int r = v.r;
  if (direct && (r < 1 || r > kWbMaxRows || m < 1)) return OSQP_FUNC_NOT_IMPLEMENTED;
  LsAK ka{t.a, {}, {}};
  LockstepDirectParams p = t.p;
  LockstepParams &P = t.polish ? static_cast<LockstepParams &>(p) : static_cast<LockstepParams &>(ka.P);      // (what ls_mat_block points at the matrix block)
  LsWs w;
  LwVecs x;
  LsMat mt{};
  LwMatVecs xm{};
  LsPolWs pws{};
  LsCursor c{base.ws}, cp{p.pol_ws};
  if (!(direct ? lockstep_direct_layout(c, n, m, r, w, x, t.polish ? nullptr : &ka.a) : lockstep_layout(c, n, m, w, t.polish ? nullptr : &ka.a))) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (mat) {
    if (direct && (!v.wtpos || !v.vsrc)) return OSQP_FUNC_NOT_IMPLEMENTED;
    if (const int err = ls_mat_block(d, P, mt)) return err;
    if (direct) {
      LsCursor cm{P.mat_ws};
      LsMatVecs again;
      if (!lockstep_direct_mat_layout(cm, n, m, r, P.A.nnz, P.B.nnz, v.Av.nnz, again, xm)) return OSQP_WORKSPACE_NOT_INIT_ERROR;
      v.WT = xm.WT; v.Av.val = xm.vval;
    }
  }
  if (t.polish && !lockstep_polish_layout(cp, n, m, pws)) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  ka.w = w;
  p.v = v;
  LsRun R(s, w.word, base.count);
  auto lwa = [](int op) { return op >= OSQP_HIP_LSB_LWA_SETL_X && op <= OSQP_HIP_LSB_LWA_ZERO; };
  if (!direct) {
    const LsPK kq{p, w, pws};
    for (int i = 0; i < t.nops; i++) {
      if (t.polish) ls_pol_go(R, mat, t.ops[i], kq, t.secs); else ls_adj_go(R, mat, t.ops[i], ka);
    }
  } else if (t.polish) {                                 // lockstep_direct_chunk's polish: kq from the solve's own parameters (A through the view), the k_lwa launch from the alpha = 1 set
    const LwRun D(p, p.v, w, x, mat);
    const LsPK kq{D.kv.P, w, pws};
    LockstepDirectParams pp = p;
    pp.alpha = 1.0;
    const LwRun Dp(pp, pp.v, w, x, mat);
    for (int i = 0; i < t.nops; i++) {
      if (lwa(t.ops[i])) Dp.lwa_go(R, t.ops[i]); else ls_pol_go(R, mat, t.ops[i], kq, t.secs);
    }
  } else {
    const LwRun D(ka.P, v, w, x, mat);
    const LwAdjViews V(ka, v.Av);
    for (int i = 0; i < t.nops; i++) {
      if (lwa(t.ops[i])) D.lwa_go(R, t.ops[i]); else ls_adj_go(R, mat, t.ops[i], V.arg(t.ops[i]));
    }
  }
  HIP_CHECK(hipStreamSynchronize(s));
  HIP_CHECK(hipGetLastError());
  return OSQP_NO_ERROR;
}

// The backward pass of one chunk, from the transposes in to the transposes out, on `stream` (nullptr: the solver's); returns when the chunk's results are
// there.  The work block is the forward's set followed by the adjoint's own vectors; after every step of the recurrence the host reads the word block
// and ends the chunk when no problem is live.  stat: {recurrence steps of the slowest problem, PCG iterations summed, kernel launches, GPU ms}.
// PER-PROBLEM MATRICES (p.mat_ws != nullptr; include/osqp_hip.h osqp_hip_batch_adjoint_lockstep_mat): problem b's adjoint system is solved on its own P_b, A_b
// under its own D_b, E_b, c_b -- the forward's preparation (ls_mat_prepare) runs in front of the transposes in, with the handle's q for every problem (the
// adjoint does not depend on c in exact arithmetic; the shared adjoint runs on the handle's c too), and from then on the kernels are kLsOwnMat's and the
// k_lsm_adj_* twins.  The preparation's scratch is dead before it is written again: q by k_ls_adj_load_n, t by k_ls_setrho (k_ls_rhs where m = 0 never
// gathers it), r by the first k_ls_rhs.  c, 1 / c and ct are rows SC_C / SC_CINV / SC_CT of the scalar state of THIS work block (the adjoint's, not the
// forward's); no kernel of the backward pass writes them -- k_ls_adj_init sets the rows below SC_C it needs, the PCG's folds SC_RZ .. SC_BETA.
int lockstep_adjoint_chunk(Dev &d, const LockstepAdjointParams &p, void *stream, double *stat) {
  const hipStream_t s = ls_stream(d, stream);
  const int n = p.n, m = p.m;
  const bool mat = p.mat_ws != nullptr;
  LsAK ka{p, {}, {}};
  LsMat mt{};
  LsCursor c{p.ws};
  if (!lockstep_layout(c, n, m, ka.w, &ka.a)) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (mat) if (const int err = ls_mat_block(d, ka.P, mt)) return err;
  const LsK k{ka.P, ka.w};                              // what the forward's kernels take: the base of the parameters, the same block vectors
  const LsPcgKernels &K = mat ? kLsOwnMat : kLsShared;
  LsRun R(s, k.w.word, p.count);
  R.e0.record(s);
  if (mat) ls_mat_prepare(R, LsMK{k.P, k.w, mt});

  ls_adj_go(R, mat, OSQP_HIP_LSB_ADJ_LOAD_N, ka);
  if (m > 0) { ls_adj_go(R, mat, OSQP_HIP_LSB_ADJ_LOAD_M, ka); ls_adj_go(R, mat, OSQP_HIP_LSB_ADJ_CLASS, ka); }
  ls_adj_go(R, mat, OSQP_HIP_LSB_ADJ_INIT, ka);
  if (m > 0) ls_go(R, K, OSQP_HIP_LS_SETRHO, k);
  ls_go(R, K, OSQP_HIP_LS_MINV, k);
  R.fetch();
  int cg_est = 4;
  const int step = ls_recurrence(R, K, k, k, p.max_steps, [&]() { ls_pcg(R, K, k, cg_est); ls_go(R, K, OSQP_HIP_LS_UPD, k); }, [&]() { ls_adj_go(R, mat, OSQP_HIP_LSB_ADJ_DECIDE, ka); });
  ls_adj_go(R, mat, OSQP_HIP_LSB_ADJ_UNSCALE, ka);
  if (m > 0) ls_adj_go(R, mat, OSQP_HIP_LSB_ADJ_RESM, ka);
  ls_adj_go(R, mat, OSQP_HIP_LSB_ADJ_RESN, ka);
  ls_adj_go(R, mat, OSQP_HIP_LSB_ADJ_FINAL, ka);
  ls_adjoint_outputs(R, mat, ka);
  const int pcg_sum = R.words[WD_PCGSUM];
  const float ms = R.finish();
  if (mat && p.mat_stat) p.mat_stat[0] = LsRun::ms(R.e0, R.em);
  if (stat) { stat[0] = step; stat[1] = pcg_sum; stat[2] = (double)R.launches; stat[3] = ms; }
  return OSQP_NO_ERROR;
}

// One chunk of the DIRECT route ("lockstep DIRECT" above), from the transposes in to the transposes out, on `stream` (nullptr: the solver's).  A fixed
// launch sequence without an inner convergence test: five launches per ADMM iteration (LwRun::solve), enqueued back to back; at a termination check the
// host reads the word block once.  The time limit is tested against the host's clock as of the last such read (in between the host runs ahead of the
// GPU): a chunk past its limit ends at the iteration after the check that saw it, with OSQP_TIME_LIMIT_REACHED for the problems still running.
// stat: {ADMM iterations of the slowest problem, inversions of S summed over the problems, kernel launches, GPU ms} -- the ADMM part's; with p.polish the
// chunk's SOLVED problems are polished in front of the transposes out and polish's figures go to p.pol_stat (as lockstep_chunk's; the PCG count is 0).
// PER-PROBLEM MATRICES (p.mat_ws != nullptr; include/osqp_hip.h osqp_hip_batch_solve_lockstep_direct_mat): problem b runs on its own P_b, A_b under its own
// D_b, E_b, c_b.  In front of the transposes in: ls_mat_prepare (the PCG route's assembly and equilibration, unchanged), then the chunk's own WT and view
// values from the block's scaled A (k_lwm_wt, k_lwm_vals); R.em marks the end of all three.  From then on the row passes are kLsOwnMat's and the four
// kernels that read matrix values are the k_lwm_* forms; D0_b, S_b and S_b^-1 follow from them per lane.  The handle's own arrays are only read.
int lockstep_direct_chunk(Dev &d, const LockstepDirectParams &p0, void *stream, double *stat) {
  const hipStream_t s = ls_stream(d, stream);
  const int n = p0.n, m = p0.m, r = p0.v.r;
  const bool mat = p0.mat_ws != nullptr;
  if (r < 1 || r > kWbMaxRows || m < 1) return OSQP_FUNC_NOT_IMPLEMENTED;
  LsWs w;
  LwVecs x;
  LsCursor c{p0.ws};
  if (!lockstep_direct_layout(c, n, m, r, w, x, nullptr)) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  LockstepDirectParams p = p0;
  LsMat mt{};
  LwMatVecs xm{};
  if (mat) {
    if (!p.v.wtpos || !p.v.vsrc) return OSQP_FUNC_NOT_IMPLEMENTED;
    if (const int err = ls_mat_block(d, p, mt)) return err;
    LsCursor cm{p.mat_ws};
    LsMatVecs again;
    if (!lockstep_direct_mat_layout(cm, n, m, r, p.A.nnz, p.B.nnz, p.v.Av.nnz, again, xm)) return OSQP_WORKSPACE_NOT_INIT_ERROR;
    p.v.WT = xm.WT; p.v.Av.val = xm.vval;
  }
  LsPolWs pws{};
  LsCursor cp{p.pol_ws};
  if (p.polish && p.pol_ws && !lockstep_polish_layout(cp, n, m, pws)) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  LwRun D(p, p.v, w, x, mat);
  if (mat) D.own(mt.Aval, p.v, xm);
  const LsK &kb = D.kb, &kv = D.kv;
  const LsPcgKernels &K = D.K();
  LsRun R(s, w.word, p.count);
  R.e0.record(s);
  if (mat) {
    ls_mat_prepare(R, LsMK{p, w, mt});
    D.own_rows(R);
    R.em.record(s);
    if (p.mat_stat) p.mat_stat[1] += 2;
  }
  const double t_begin = R.t_sync;
  auto residuals = [&]() { D.go(R, OSQP_HIP_LS_RESM); D.go(R, OSQP_HIP_LS_RESN); };

  HIP_CHECK(hipMemsetAsync(x.fact, 0, sizeof(int) * W, s));
  D.go(R, OSQP_HIP_LS_LOAD_N);
  D.go(R, OSQP_HIP_LS_LOAD_M);
  D.go(R, OSQP_HIP_LS_INIT);
  D.factor(R);
  D.long_rows(R, 1);
  D.go(R, OSQP_HIP_LS_INITZ);
  residuals();
  R.go(K.decide, 1, kb, 0, 0, 0, 1);
  int iter = 0;
  while (R.words[WD_LIVE] > 0 && iter < p.max_iter) {
    iter++;
    D.solve(R);
    const int at_check = (p.check > 0 && iter % p.check == 0) || iter >= p.max_iter;
    const int at_rho = p.rho_interval > 0 && iter % p.rho_interval == 0;
    const bool late = p.time_limit > 0 && R.t_sync - t_begin > p.time_limit;    // (as of the last check: the host enqueues ahead of the GPU in between)
    if (!at_check && !at_rho && !late) continue;
    D.long_rows(R, 0);
    residuals();
    if (p.check_dualgap && (at_check || late)) D.go(R, OSQP_HIP_LS_SUPP);        // (settings.check_dualgap: l, u, y carry all m rows, the dense ones included)
    R.go(K.decide, 1, kb, iter, late ? 1 : at_check, at_rho, late ? 2 : 0);
    if (at_rho && !late) D.factor(R);
    if (at_check || late) R.fetch();
  }
  // polish ("polish of a chunk" above, with the direct adjoint's step in place of the PCG).  A chunk whose time limit has passed -- by the host's clock
  // now, not as of the last check -- does not polish.  The recurrence's rho is fixed: rho_bar = 1 / delta_eff on the guessed-active rows, rho_min on
  // the others (k_ls_pol_class frees them, so k_ls_setrho classes them loose -- the inactive dense rows too), alpha = 1; S_b is formed and inverted once
  // per attempted problem (Dp.factor) and never at a step.  A step is LwRun::solve and the refresh of the dense rows of x and x~; the cone projection
  // and the accept test's row pass read A through the view, so no wave walks a dense row.  k_ls_pol_end restores the first n rows of a rejected
  // problem's x: nothing behind it reads the rows >= n (k_ls_store_n runs over n rows, k_ls_store_m over y and dy).
  const bool polished = p.polish && p.pol_ws && !(p.time_limit > 0 && ls_now() - t_begin > p.time_limit);
  int pol_steps = 0, pol_att = 0;
  long pol_launches = 0;
  if (polished) {
    const LsPK kq{kv.P, w, pws};                         // (kv.P: with a matrix block its A is the view on the chunk's own values, B.val, D .. Einv the block's)
    const long launches0 = R.launches;
    const double t_pol = ls_now();
    LockstepDirectParams pp = p;
    pp.alpha = 1.0;
    const LwRun Dp(pp, pp.v, w, x, mat);
    R.ep0.record(s);
    ls_pol_go(R, mat, OSQP_HIP_LSB_POL_BEGIN, kq);
    R.fetch();
    pol_att = R.words[WD_LIVE];
    if (pol_att > 0) {
      ls_pol_go(R, mat, OSQP_HIP_LSB_POL_CLASS, kq);
      Dp.factor(R);
      pol_steps = ls_recurrence(R, K, Dp.kv, Dp.kb, kLsPolMaxSteps,
                                [&]() { Dp.solve(R); if (p.pol_prod2) Dp.long_rows2(R); else Dp.long_rows(R, 0); }, [&]() { ls_pol_go(R, mat, OSQP_HIP_LSB_POL_DECIDE, kq); });
      Dp.prod(R, w.x, x.pg);
      Dp.lwa_go(R, OSQP_HIP_LSB_LWA_SETL_X);
      ls_pol_go(R, mat, OSQP_HIP_LSB_POL_CONE, kq);
      Dp.go(R, OSQP_HIP_LS_RESM);
      Dp.go(R, OSQP_HIP_LS_RESN);
      if (p.check_dualgap) Dp.go(R, OSQP_HIP_LS_SUPP);
      ls_pol_go(R, mat, OSQP_HIP_LSB_POL_ACCEPT, kq);
      R.fetch();
      ls_pol_go(R, mat, OSQP_HIP_LSB_POL_END, kq, ls_now() - t_pol);
    }
    R.ep1.record(s);
    pol_launches = R.launches - launches0;
  }
  D.go(R, OSQP_HIP_LS_STORE_N);
  D.go(R, OSQP_HIP_LS_STORE_M);
  long nfact = 0;
  const float ms = R.finish(x.fact, &nfact), pms = polished ? LsRun::ms(R.ep0, R.ep1) : 0.f;
  if (mat && p.mat_stat) p.mat_stat[0] = LsRun::ms(R.e0, R.em);
  // (the chunk's statistics are the ADMM part's: k_lw_inv has counted one inversion for every problem polish attempted; polish's go to their own block)
  if (stat) { stat[0] = iter; stat[1] = (double)(nfact - pol_att); stat[2] = (double)(R.launches - pol_launches); stat[3] = ms - pms; }
  if (polished && p.pol_stat) {
    double *ps = p.pol_stat;
    ps[0] = pol_att; ps[1] = R.words[WD_POLACC]; ps[2] = R.words[WD_POLREJ]; ps[3] = pol_steps; ps[4] = 0.0; ps[5] = (double)pol_launches; ps[6] = pms;
  }
  return OSQP_NO_ERROR;
}

// The backward pass of one chunk on the DIRECT route, from the transposes in to the transposes out, on `stream` (nullptr: the solver's); returns when the
// chunk's results are there.  The sequence is lockstep_adjoint_chunk's with LwRun's solve in place of the PCG; the work block is the direct forward's
// set followed by the adjoint's own vectors.  The classification's operand x~ = Dinv x sits in the block vector x~ (n + r rows; its last r
// from the products), so that k_ls_adj_class reads A through the view like every other row pass here; x, x~ and dx are zeroed over n + r rows afterwards.
// rho is set, and S formed and inverted, once; a step is eleven launches and one read of the word block.  A pivot of S_b that is not positive and finite
// leaves NaN iterates in that lane alone: its residual is not below the threshold and it ends with status 3.
// stat: {recurrence steps of the slowest problem, inversions of S summed over the problems, kernel launches, GPU ms}.
// PER-PROBLEM MATRICES (p.mat_ws != nullptr; include/osqp_hip.h osqp_hip_batch_adjoint_lockstep_direct_mat): problem b's adjoint system is solved on its own
// P_b, A_b under its own D_b, E_b, c_b, by the Woodbury formula per lane.  The block is the direct forward's (the matrix block, then the chunk's own WT and
// view values); in front of the transposes in it is prepared as lockstep_direct_chunk prepares it -- ls_mat_prepare with the handle's q for every problem (as
// lockstep_adjoint_chunk: the adjoint does not depend on c in exact arithmetic), then k_lwm_wt and k_lwm_vals on the block's scaled A; R.em marks the end of
// all three.  From then on the row passes are kLsOwnMat's and the k_lsm_adj_* twins, the dense rows' kernels the k_lwm_* forms; a step
// stays eleven launches.  The shared path launches what it launched before.
// The preparation's scratch is dead before it is written again.  Its users are the k_lsm_* kernels of ls_mat_prepare alone: k_lwm_wt / k_lwm_vals read the
// block's Aval and write the block's WT / vval, nothing of the work block.  Then, in launch order:
//   q           written by k_lsm_adj_load_n (q~ = c D dx, all n rows, every lane) -- the first launch after the preparation; nothing reads q before.
//   et in t     the launches up to D.factor -- adj_load_n / adj_load_m, k_lwm_prod + k_lwa_setl (read x~, write pg and rows n .. n + r - 1 of x~),
//               k_lsm_adj_class (reads x~, l, u, ay, gdy; writes code, l, u, z, zt, y, dy), k_ls_adj_init (scalar rows, iw), k_lwa_zero (x, x~, dx over
//               n + r rows: none of them is r, t or q) -- neither read nor write t.  k_ls_setrho, D.factor's first launch, writes t = rho z - y and t2 over all
//               m rows for every lane (k_ls_adj_init flags them all; m >= 1 here), and the first reader of t is the first k_lsm_rhs, after it.
//   dt in r     D.factor's other launches (k_lwm_d0: Minv; k_lwm_s: S; k_lw_inv: S, fact) do not touch r; the first k_lsm_rhs writes r for every live lane
//               before k_lwm_prod .. k_lwm_x, which read p and Minv, not r.  A lane that is not live (>= count, or status 2) keeps dt in r: no kernel
//               reads r but k_ls_rhs' successors in the PCG, which this route does not have.
//   SC_C, SC_CINV, SC_CT   rows of THIS work block's scalar state (the direct adjoint's, not the forward's).  After the preparation they are only read
//               (adj_load_n, adj_unscale, adj_resn): k_ls_adj_init writes SC_RHOBAR, SC_EQF, SC_EPSCG, SC_EPSPREV, SC_BEST, SC_NACT and k_ls_adj_decide SC_BEST,
//               all below SC_C; there are no PCG folds here.
// The block vectors x, x~, dx have n + r rows here; the preparation never uses them.
int lockstep_direct_adjoint_chunk(Dev &d, const LockstepDirectAdjointParams &p, void *stream, double *stat) {
  const hipStream_t s = ls_stream(d, stream);
  const int n = p.n, m = p.m, r = p.v.r;
  const bool mat = p.mat_ws != nullptr;
  if (r < 1 || r > kWbMaxRows || m < 1) return OSQP_FUNC_NOT_IMPLEMENTED;
  LsAK ka{p, {}, {}};
  LwVecs x;
  LsCursor c{p.ws};
  if (!lockstep_direct_layout(c, n, m, r, ka.w, x, &ka.a)) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  LockstepDirectView v = p.v;
  LsMat mt{};
  LwMatVecs xm{};
  if (mat) {
    if (!v.wtpos || !v.vsrc) return OSQP_FUNC_NOT_IMPLEMENTED;
    if (const int err = ls_mat_block(d, ka.P, mt)) return err;
    LsCursor cm{p.mat_ws};
    LsMatVecs again;
    if (!lockstep_direct_mat_layout(cm, n, m, r, p.A.nnz, p.B.nnz, v.Av.nnz, again, xm)) return OSQP_WORKSPACE_NOT_INIT_ERROR;
    v.WT = xm.WT; v.Av.val = xm.vval;
  }
  const LsWs &w = ka.w;
  LwRun D(ka.P, v, w, x, mat);
  if (mat) D.own(mt.Aval, v, xm);
  const LsPcgKernels &K = D.K();
  const LwAdjViews V(ka, v.Av);                         // (which op takes which view: LwAdjViews)
  LsRun R(s, w.word, p.count);
  R.e0.record(s);
  if (mat) {
    ls_mat_prepare(R, LsMK{ka.P, w, mt});
    D.own_rows(R);
    R.em.record(s);
    if (p.mat_stat) p.mat_stat[1] += 2;
  }
  auto long_rows_of = [&](double *vec, int setl) { D.prod(R, vec, x.pg); D.lwa_go(R, setl); };
  auto adj = [&](int op) { ls_adj_go(R, mat, op, V.arg(op)); };

  HIP_CHECK(hipMemsetAsync(x.fact, 0, sizeof(int) * W, s));
  adj(OSQP_HIP_LSB_ADJ_LOAD_N);
  adj(OSQP_HIP_LSB_ADJ_LOAD_M);
  long_rows_of(w.xs, OSQP_HIP_LSB_LWA_SETL_XS);
  adj(OSQP_HIP_LSB_ADJ_CLASS);
  adj(OSQP_HIP_LSB_ADJ_INIT);
  D.lwa_go(R, OSQP_HIP_LSB_LWA_ZERO);
  D.factor(R);
  R.fetch();
  const int step = ls_recurrence(R, K, D.kv, D.kb, p.max_steps, [&]() { D.solve(R); D.long_rows(R, 0); }, [&]() { adj(OSQP_HIP_LSB_ADJ_DECIDE); });
  adj(OSQP_HIP_LSB_ADJ_UNSCALE);
  long_rows_of(w.x, OSQP_HIP_LSB_LWA_SETL_X);
  adj(OSQP_HIP_LSB_ADJ_RESM);
  adj(OSQP_HIP_LSB_ADJ_RESN);
  adj(OSQP_HIP_LSB_ADJ_FINAL);
  ls_adjoint_outputs(R, mat, ka);
  long nfact = 0;
  const float ms = R.finish(x.fact, &nfact);
  if (mat && p.mat_stat) p.mat_stat[0] = LsRun::ms(R.e0, R.em);
  if (stat) { stat[0] = step; stat[1] = (double)nfact; stat[2] = (double)R.launches; stat[3] = ms; }
  return OSQP_NO_ERROR;
}

// the values of the view of A (LockstepDirectView::Av) from A's current ones, on `stream` (nullptr: the solver's)
int lockstep_direct_values(Dev &d, int nv, const int *src, double *out, void *stream) {
  HIP_CHECK(hipSetDevice(d.device));
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : st(d);
  hipLaunchKernelGGL(k_lw_vals, dim3(std::max(1, std::min(256, (nv + 255) / 256))), dim3(256), 0, s, nv, src, (const double *)d.A.val, out);
  HIP_CHECK(hipGetLastError());
  return OSQP_NO_ERROR;
}

}  // namespace be
}  // namespace osqp_hip
