// adjoint_hip.hip -- the device side of the adjoint derivatives of ONE large QP on the PCG path (engine_api.cpp Engine::adjoint_compute_pcg;
// include/osqp_hip.h osqp_adjoint_derivative_compute).  The adjoint system
//     [ P    A_a' ] [ r_x ]     [ dx   ]
//     [ A_a  0    ] [ r_a ] = - [ dy_a ]
// is the KKT system of  min 1/2 r'Pr + dx'r  s.t.  A_a r = -dy_a:  polish's matrix with another right-hand side, solved by the recurrence polish
// runs (engine.cpp Engine::run_recurrence) on the scaled problem with  q~ = c D dx,  b~ = -E dy.  The kernels here do what surrounds that solve:
//   k_adj_prep / k_adj_classify   the active set by the rule of the batch adjoint (caller's units, on the stored solution, z = A x), the recurrence's
//                                 linear term, bounds, constraint classes and zero start, the active-row count;
//   k_adj_unscale                 r_x = D r~_x,  r_y = E y~ / c on the active rows (0 elsewhere),  dl / du;
//   k_adj_res_m / k_adj_res_n     max |g - K_a r| and max |g| of the UNREGULARISED system in the caller's units (the batch record's definition);
//   k_adj_grad                    dP and dA at the stored entries, one thread per entry and pass.
// All vectors are in the engine's numbering (a reordered handle permutes on the host, engine_api.cpp).  Reductions go through the per-workgroup
// partials of Dev::part in a fixed order (no atomics): two calls on the same state give the same bits.
#include "hip_common.h"

namespace osqp_hip {
namespace be {

namespace {

// partial slots (relative to SL_RES0: the residual kernels' scratch, rewritten by every be::residuals)
enum AdjSlot { AS_ACT = 0, AS_RM, AS_GM, AS_RN, AS_GN };

__global__ __launch_bounds__(kBlock) void k_adj_prep(Dev d, AdjointPcg a) {
  const int stride = gridDim.x * kBlock;
  for (int j = blockIdx.x * kBlock + threadIdx.x; j < d.n; j += stride) {
    d.w[j] = d.Dinv[j] * a.x[j];                       // x~ of the stored solution (the SpMV of the classification runs on the scaled A)
    d.q[j] = a.c * d.D[j] * a.dx[j];                   // as k_scale_q
    d.x[j] = 0.0; d.xs[j] = 0.0; d.dx[j] = 0.0;        // zero start
  }
}

struct EAdjClass : NoPrefetch {
  const double *y, *dy, *lraw, *uraw, *E, *Einv;
  double *l, *u, *z, *yit; int *ctype, *code; int rho_is_vec;
  double cnt = 0;
  __device__ __forceinline__ void operator()(int i, const double (&s)[1]) {
    const double zi = Einv[i] * s[0], yi = y[i], li = lraw[i], ui = uraw[i];
    const RowActive act = adjoint_active(zi, li, ui, yi);
    const int k = act.low ? 1 : (act.upp ? 2 : 0);
    const double b = (k && dy) ? -(E[i] * dy[i]) : 0.0;
    code[i] = k;
    l[i] = k ? b : -OSQP_INFTY; u[i] = k ? b : OSQP_INFTY;      // active rows: equalities at b~; the others: free
    z[i] = b; yit[i] = 0.0;
    ctype[i] = rho_is_vec ? (k ? 1 : -1) : 0;                    // (what classify_constraints gives polish's bounds)
    cnt += k ? 1.0 : 0.0;
  }
};
__global__ __launch_bounds__(kBlock) void k_adj_classify(Dev d, AdjointPcg a) {
  __shared__ StreamLdsW<1, double> lds;
  GVec g{d.w};
  EAdjClass e{{}, a.y, a.dy, d.lraw, d.uraw, d.E, d.Einv, d.l, d.u, d.z, d.y, d.ctype, a.code, a.rho_is_vec};
  process_rows<1>(d.A, g, e, lds);
  __syncthreads();
  put_partial(d.part, SL_RES0 + AS_ACT, block_sum(e.cnt, lds.red));
}
__global__ __launch_bounds__(kBlock) void k_adj_count(Dev d, AdjointPcg a) {
  __shared__ double sred[2 * kWaves];
  const double v = partial_sum(d.part + (SL_RES0 + AS_ACT) * kGrid, sred);
  if (threadIdx.x == 0) a.rec[0] = v;
}

__global__ __launch_bounds__(kBlock) void k_adj_unscale(Dev d, AdjointPcg a) {
  const int stride = gridDim.x * kBlock;
  for (int j = blockIdx.x * kBlock + threadIdx.x; j < d.n; j += stride) a.rx[j] = d.D[j] * d.x[j];
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < d.m; i += stride) {
    const int k = a.code[i];
    const double ys = k ? d.y[i] : 0.0, ry = a.cinv * d.E[i] * ys;     // as store_solution unscales y
    d.y[i] = ys;                                                        // (the residual kernel multiplies A' by it)
    a.ry[i] = ry;
    a.dl[i] = k == 1 ? -ry : 0.0; a.du[i] = k == 2 ? -ry : 0.0;
  }
}

// rows n .. n + active of g - K_a r:  -dy_i - (A r_x)_i  on the active rows
struct EAdjResM : NoPrefetch {
  const double *dy, *Einv; const int *code;
  double rm = 0, gm = 0;
  __device__ __forceinline__ void operator()(int i, const double (&s)[1]) {
    if (!code[i]) return;
    const double dyi = dy ? dy[i] : 0.0;
    rm = nanmax(rm, fabs(dyi + Einv[i] * s[0])); gm = nanmax(gm, fabs(dyi));
  }
};
__global__ __launch_bounds__(kBlock) void k_adj_res_m(Dev d, AdjointPcg a) {
  __shared__ StreamLdsW<1, double> lds;
  GVec g{d.x};
  EAdjResM e{{}, a.dy, d.Einv, a.code};
  process_rows<1>(d.A, g, e, lds);
  __syncthreads();
  double *red = lds.red;
  put_partial(d.part, SL_RES0 + AS_RM, block_max(e.rm, red)); put_partial(d.part, SL_RES0 + AS_GM, block_max(e.gm, red));
}
// rows 0 .. n:  -dx_j - (P r_x + A_a' r_a)_j.   B = [c D P D + sigma I | (E A D)']: row j of B [x~; y~] is  c D_j (P r_x + A' r_y)_j + sigma x~_j
struct GAdjTwo {
  const double *pn, *pm; int n;
  __device__ __forceinline__ void operator()(int c, double v, double (&pr)[2]) const {
    if (c < n) { pr[0] = v * pn[c]; pr[1] = 0.0; } else { pr[0] = 0.0; pr[1] = v * pm[c - n]; }
  }
};
struct EAdjResN : NoPrefetch {
  const double *xs, *dx, *Dinv; double sigma, cinv;
  double rn = 0, gn = 0;
  __device__ __forceinline__ void operator()(int j, const double (&s)[2]) {
    const double kr = cinv * Dinv[j] * ((s[0] - sigma * xs[j]) + s[1]), dxj = dx[j];
    rn = nanmax(rn, fabs(dxj + kr)); gn = nanmax(gn, fabs(dxj));
  }
};
__global__ __launch_bounds__(kBlock) void k_adj_res_n(Dev d, AdjointPcg a) {
  __shared__ StreamLds<2> lds;
  GAdjTwo g{d.x, d.y, d.n};
  EAdjResN e{{}, d.x, a.dx, d.Dinv, d.sigma, a.cinv};
  process_rows<2>(d.B, g, e, lds);
  __syncthreads();
  double *red = lds.red;
  put_partial(d.part, SL_RES0 + AS_RN, block_max(e.rn, red)); put_partial(d.part, SL_RES0 + AS_GN, block_max(e.gn, red));
}
__global__ __launch_bounds__(kBlock) void k_adj_res_final(Dev d, AdjointPcg a) {
  __shared__ double sred[2 * kWaves];
  const double rm = d.m > 0 ? partial_max(d.part + (SL_RES0 + AS_RM) * kGrid, sred) : 0.0;
  const double gm = d.m > 0 ? partial_max(d.part + (SL_RES0 + AS_GM) * kGrid, sred) : 0.0;
  const double rn = partial_max(d.part + (SL_RES0 + AS_RN) * kGrid, sred);
  const double gn = partial_max(d.part + (SL_RES0 + AS_GN) * kGrid, sred);
  if (threadIdx.x == 0) { a.rec[1] = nanmax(rm, rn); a.rec[2] = nanmax(gm, gn); }
}

// Gradients at the stored entries: per entry two 4-byte indices (coalesced streams), four gathers and ONE 8-byte store by the one thread that owns
// the entry.  The entries come in CSC order: the column-side gathers (x_j, r_x,j) hit the same line across a wave, the row-side ones stay inside a
// column's rows.  kU entries per thread and pass: every index load of a pass is issued before the first gather waits, every gather before the
// first store.
constexpr int kAdjU = 4;
template <bool SYM>
__device__ __forceinline__ void adj_entries(int nz, const int *__restrict__ ri, const int *__restrict__ cj, const double *__restrict__ rowa,
                                            const double *__restrict__ cola, const double *__restrict__ rowb, const double *__restrict__ colb,
                                            double *__restrict__ out) {
  const int stride = gridDim.x * kBlock;
  for (int k0 = blockIdx.x * kBlock + threadIdx.x; k0 < nz; k0 += kAdjU * stride) {
    int i[kAdjU], j[kAdjU];
    double ra[kAdjU], ca[kAdjU], rb[kAdjU], cb[kAdjU];
#pragma unroll
    for (int u = 0; u < kAdjU; u++) { const int k = min(k0 + u * stride, nz - 1); i[u] = ri[k]; j[u] = cj[k]; }
#pragma unroll
    for (int u = 0; u < kAdjU; u++) { ra[u] = rowa[i[u]]; ca[u] = cola[j[u]]; rb[u] = rowb[i[u]]; cb[u] = colb[j[u]]; }
#pragma unroll
    for (int u = 0; u < kAdjU; u++) {
      const int k = k0 + u * stride;
      if (k < nz) out[k] = SYM ? 0.5 * (ra[u] * ca[u] + cb[u] * rb[u]) : ra[u] * ca[u] + rb[u] * cb[u];
    }
  }
}
__global__ __launch_bounds__(kBlock) void k_adj_grad(Dev d, AdjointPcg a) {
  adj_entries<true>(d.nzP, d.Pi, d.Pj, a.rx, a.x, a.x, a.rx, a.dP);        // dP_ij = (r_i x_j + r_j x_i) / 2
  adj_entries<false>(d.nzA, d.Ai, d.Aj, a.y, a.rx, a.ry, a.x, a.dA);       // dA_ij = y_i r_x,j + r_y,i x_j
}

}  // namespace

void adjoint_load(Dev &d, const AdjointPcg &a) {
  HIP_CHECK(hipSetDevice(d.device));
  LAUNCH(k_adj_prep, d, d, a);
  if (d.m > 0) { LAUNCH(k_adj_classify, d, d, a); hipLaunchKernelGGL(k_adj_count, dim3(1), dim3(kBlock), 0, st(d), d, a); }
  else HIP_CHECK(hipMemsetAsync(a.rec, 0, sizeof(double), st(d)));
}

void adjoint_residual(Dev &d, const AdjointPcg &a) {
  HIP_CHECK(hipSetDevice(d.device));
  LAUNCH(k_adj_unscale, d, d, a);
  if (d.m > 0) LAUNCH(k_adj_res_m, d, d, a);
  LAUNCH(k_adj_res_n, d, d, a);
  hipLaunchKernelGGL(k_adj_res_final, dim3(1), dim3(kBlock), 0, st(d), d, a);
}

void adjoint_gradients(Dev &d, const AdjointPcg &a) {
  HIP_CHECK(hipSetDevice(d.device));
  if (d.nzP + d.nzA > 0) LAUNCH(k_adj_grad, d, d, a);
}

}  // namespace be
}  // namespace osqp_hip
