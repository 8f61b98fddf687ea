// batch_hip.hip -- batched OSQP for many small QPs that share (P, A) and differ in q, l, u  (BASELINE configs[4]:
// 4096 MPC QPs, n = 120, m = 240; semantics = the reference's update-style batching, one solver re-used through
// update(q, l, u) + solve(), /root/reference/src/osqp/nn/torch.py:128-164).
//
// MI355X mapping: ONE WORKGROUP PER PROBLEM, one kernel launch for the whole batch.  All iterates and PCG vectors of a
// problem live in LDS (10 n + 8 m doubles = 25 KB at n=120, m=240 -> 6 workgroups per CU); the shared scaled matrices
// A (CSR) and B = [P + sigma I | A'] (CSR) are the base solver's device arrays (28 KB: L1/L2 resident for every
// workgroup).  The complete ADMM solve -- rhs, reduced-KKT PCG (Jacobi), x/z/y update, residuals, termination test,
// infeasibility tests, adaptive rho -- runs inside the kernel with __syncthreads() as the only synchronisation and
// wave64 __shfl_down + LDS reductions for every dot product / norm.  No host round trip, no global-memory iterates.
// The arithmetic is the same as the large-problem engine (backend_hip.hip / engine.cpp); formulas cite
// /root/reference/src/osqppurepy/_osqp.py.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>
#include <type_traits>

#include "../../include/osqp_hip.h"
#include "backend.h"
#include "step_rules.h"

namespace osqp_hip {
namespace be {

namespace {

// Wave64 reductions with DPP moves (VALU rate; HIP's __shfl_* compile to ds_bpermute_b32 -- an LDS round trip per 32-bit half
// and step; see backend_hip.hip wave_sum).  Zero fill = identity of the sums and of the maxima of magnitudes.  Result in LANE 63.
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ double bdpp(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wsum63(double v) {
  v += bdpp<0xb1>(v); v += bdpp<0x4e>(v); v += bdpp<0x114>(v); v += bdpp<0x118>(v); v += bdpp<0x142, 0xa>(v); v += bdpp<0x143, 0xc>(v);
  return v;
}
__device__ __forceinline__ double wmax63(double v) {
  v = nanmax(v, bdpp<0xb1>(v)); v = nanmax(v, bdpp<0x4e>(v)); v = nanmax(v, bdpp<0x114>(v)); v = nanmax(v, bdpp<0x118>(v));
  v = nanmax(v, bdpp<0x142, 0xa>(v)); v = nanmax(v, bdpp<0x143, 0xc>(v));
  return v;
}

// Block reductions; all threads get the result.  NW = waves per workgroup.  With ONE wave per problem (NW = 1) a
// reduction is six DPP steps and a v_readlane broadcast: no LDS, no barrier.
template <int NW>
struct Red {
  double *s;   // >= 16 doubles of LDS (NW > 1 only)
  __device__ __forceinline__ double sum(double v) const {
    v = wsum63(v);
    if constexpr (NW == 1) return readlane_f64(v, 63);
    else {
      if ((threadIdx.x & 63) == 63) s[threadIdx.x >> 6] = v;
      __syncthreads();
      double t = 0.0;
#pragma unroll
      for (int w = 0; w < NW; w++) t += s[w];
      __syncthreads();
      return t;
    }
  }
  __device__ __forceinline__ double max(double v) const {
    v = wmax63(v);
    if constexpr (NW == 1) return readlane_f64(v, 63);
    else {
      if ((threadIdx.x & 63) == 63) s[threadIdx.x >> 6] = v;
      __syncthreads();
      double t = 0.0;
#pragma unroll
      for (int w = 0; w < NW; w++) t = nanmax(t, s[w]);
      __syncthreads();
      return t;
    }
  }
  // K maxima and S sums behind ONE pair of barriers (K + S <= 4: the 16 doubles of s): the same wave reductions and the same order over the waves as
  // max() / sum() -- identical results; the residuals' 22 block reductions cost 44 barriers one at a time, 14 in groups of four
  template <int K, int S>
  __device__ __forceinline__ void max_sum_n(double (&mx)[K > 0 ? K : 1], double (&sm)[S > 0 ? S : 1]) const {
    static_assert(NW * (K + S) <= 16, "scratch");
    double *scr = s;
    if constexpr (NW == 1) {
#pragma unroll
      for (int k = 0; k < K; k++) mx[k] = max(mx[k]);
#pragma unroll
      for (int k = 0; k < S; k++) sm[k] = sum(sm[k]);
    } else {
      const int w = threadIdx.x >> 6; const bool last = (threadIdx.x & 63) == 63;
#pragma unroll
      for (int k = 0; k < K; k++) { const double v = wmax63(mx[k]); if (last) scr[w * (K + S) + k] = v; }
#pragma unroll
      for (int k = 0; k < S; k++) { const double v = wsum63(sm[k]); if (last) scr[w * (K + S) + K + k] = v; }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < K; k++) { double t = 0.0; for (int q = 0; q < NW; q++) t = nanmax(t, scr[q * (K + S) + k]); mx[k] = t; }
#pragma unroll
      for (int k = 0; k < S; k++) { double t = 0.0; for (int q = 0; q < NW; q++) t += scr[q * (K + S) + K + k]; sm[k] = t; }
      __syncthreads();
    }
  }
  __device__ __forceinline__ void sum_max(double &a, double &b) const {   // a: sum, b: max
    if constexpr (NW == 1) { a = sum(a); b = max(b); }
    else {
      a = wsum63(a); b = wmax63(b);
      if ((threadIdx.x & 63) == 63) { s[threadIdx.x >> 6] = a; s[8 + (threadIdx.x >> 6)] = b; }
      __syncthreads();
      a = 0.0; b = 0.0;
#pragma unroll
      for (int w = 0; w < NW; w++) { a += s[w]; b = nanmax(b, s[8 + w]); }
      __syncthreads();
    }
  }
};

}  // namespace


namespace {

// sum of prod[a .. z) in entry order; the loads of a batch of eight are independent (one LDS latency per batch, not per entry)
__device__ __forceinline__ double row_sum(const double *prod, int a, int z) {
  double acc = 0.0;
  int k = a;
  for (; k + 8 <= z; k += 8) {
    double v[8];
#pragma unroll
    for (int b = 0; b < 8; b++) v[b] = prod[k + b];
#pragma unroll
    for (int b = 0; b < 8; b++) acc += v[b];
  }
  if (k < z) {
    double v[8];
#pragma unroll
    for (int b = 0; b < 8; b++) v[b] = k + b < z ? prod[k + b] : 0.0;
#pragma unroll
    for (int b = 0; b < 8; b++) acc += v[b];
  }
  return acc;
}

// hi + lo += a * v in double-double: the product exactly (FMA), the sum by TwoSum.  Contraction is switched off for this body:
// a fused a * v + hi would break the error terms.
__device__ __forceinline__ void dd_acc(double a, double v, double &hi, double &lo) {
#pragma clang fp contract(off)
  const double pr = a * v;
  const double pe = __builtin_fma(a, v, -pr);
  const double sm_ = hi + pr, bv = sm_ - hi;
  lo += ((hi - (sm_ - bv)) + (pr - bv)) + pe;
  hi = sm_;
}

// kBB = threads per problem: 64 (one wave: barriers are free, reductions are pure shuffles; small problems) or 256.
// EA / EB > 0: every lane keeps EA entries of A and EB entries of B (value + column) in registers for the whole solve
// (entry k belongs to lane k % kBB); an SpMV is then  prod[k] = val * v[col]  for the lane's own entries (LDS only),
// a barrier, and one lane per row summing its segment of prod -- no matrix traffic inside the ADMM / PCG loops and a
// balanced first phase (the MPC rows have 1..13 entries).  EA = EB = 0: generic row loops reading the matrices from
// global memory (L1/L2), for patterns with more than 8 * kBB entries per matrix.
//
// DIRECT: the linear system of every ADMM iteration is solved exactly, as the reference's direct path does
// (_osqp.py:286-311), instead of by PCG.  K = P + sigma I + A' diag(rho) A is assembled in LDS under the bandwidth-reducing
// permutation prepared by the engine (column-major lower band, padded: band_ldl.h), Cholesky-factorised in
// place at every rho change, and each solve is two substitutions that keep the live window of the right-hand side in
// REGISTERS: element e of the vector lives in lane e % 64 from the step that loads it until its own pivot step (bw < 64),
// a pivot is broadcast with v_readlane, every other lane applies its one update -- no LDS traffic on the dependency chain
// except the (prefetchable) column of L.
// POLISH (direct variants): a separate instantiation that ends with the polish step, so that the plain kernel's register allocation
// is not touched by code most launches never run.
// SPEC (256 threads, n <= kBatchSpecN, no polish): the direct solve in its SPECTRAL form (engine.hpp BatchSpectral).  K(rho)^-1 = V diag(1 / (1 + (rho -
// rho_ref) lambda)) V' with V, lambda shared by the whole batch: the workgroup keeps K^-1 in REGISTERS (thread t: row t / 2, the 64 columns of half t % 2),
// rebuilds it from V at a rho update (V streamed through LDS in chunks of columns; ~20 us, no factorisation) and solves with one dense product
// (64 FMAs per thread against broadcast LDS reads + one lane exchange): the 240-pivot substitution chain of the banded form (9 of an iteration's 14 us)
// becomes ~0.5 us, and no band lives in LDS.
// SPW: workgroups per CU the spectral instantiation is compiled for.  1: K^-1 and everything else in registers (370 of the 512 a lone workgroup may
// use) -- 5.0 us per ADMM iteration, the form for batches that fit the chip in two rounds (latency: 256 QPs 1.0 ms, 512 QPs 1.5 ms).  2: the 256
// registers of two resident workgroups, ~150 of the kernel's values in scratch -- 8 us per iteration, but twice the problems in flight: 4096 QPs
// 8.4 ms against 10.1 (and 10.6 for the banded form).  batch_solve picks by batch size.
// GAP (settings.check_dualgap): like POLISH a separate instantiation of every variant, for the same reason -- with the duality-gap test as a run-time
// branch the instantiations at 256 registers spill 12 - 56 bytes more and the others take 4 - 7 registers more; the GAP = false kernels are the kernels
// without the setting, to the bit.
template <int kBB, int EA, int EB, bool DIRECT, bool POLISH = false, bool N128 = false, bool SPEC = false, int SPW = 1, bool GAP = false>
__global__ __launch_bounds__(kBB, (DIRECT && kBB == 256 && EA <= 8) ? (SPEC ? SPW : 2) : 1) void k_batch_admm(BatchParams P) {
  static_assert(!SPEC || (DIRECT && !POLISH && kBB == 256), "the spectral form: 256 threads, direct, no polish");
#ifdef OSQP_HIP_KTRACE
  // diagnostic build: 100 MHz clock ticks spent in the phases; reported in rec[5..7] INSTEAD of rho / rho_updates / pcg_iters
  unsigned long long tk_all = wall_clock64(), tk_fact = 0, tk_solve = 0, tk0 = 0, tk1 = 0, tk_rhs = 0, tk_upd = 0, tk_fwd = 0, tk_res = 0;
#define BT_BEGIN() (tk0 = wall_clock64())
#define BT_END(acc) (acc += wall_clock64() - tk0)
#define BT2_BEGIN() (tk1 = wall_clock64())
#define BT2_END(acc) (acc += wall_clock64() - tk1)
#else
#define BT_BEGIN() ((void)0)
#define BT_END(acc) ((void)0)
#define BT2_BEGIN() ((void)0)
#define BT2_END(acc) ((void)0)
#endif
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int n = P.n, m = P.m, tid = threadIdx.x;
  if ((int)blockIdx.x >= P.nbatch) return;
  const int b = P.order ? P.order[blockIdx.x] : (int)blockIdx.x;      // (workgroups are dispatched in index order: expected-longest problems first)
  if (!SPEC && P.only_marked && P.rec[(size_t)b * kBatchRec] != kBatchUnsolved) return;      // (second launch behind the spectral one: only what that one left)
  // per-problem matrices (BatchParams::mat_on): this workgroup's copy of the parameter block points at ITS problem's scaled values, equilibration and
  // products -- everything below reads them through the same names as the shared case (block-uniform: scalar registers)
  if (P.mat_on) {
    P.A.val = P.Aval_b + (size_t)b * P.A.nnz; P.B.val = P.Bval_b + (size_t)b * P.B.nnz;
    P.D = P.D_b + (size_t)b * P.n; P.Dinv = P.Dinv_b + (size_t)b * P.n; P.E = P.E_b + (size_t)b * P.m; P.Einv = P.Einv_b + (size_t)b * P.m;
    P.c = P.c_b[b]; P.cinv = 1.0 / P.c; P.kp_val = P.kp_val_b + (size_t)b * P.nprod;
  }
  // ---- LDS carve ----
  double *x = sm, *xs = x + n, *r = xs + n, *zv = r + n, *p = zv + n, *Kp = p + n, *q = Kp + n, *Minv = q + n, *dx = Minv + n, *tn = dx + n;
  double *z = tn + n, *y = z + m, *t = y + m, *l = t + m, *u = l + m, *rho = u + m, *zt = rho + m, *dy = zt + m;
  Red<kBB / 64> red{dy + m};
  double *prod = dy + m + 16;                       // max(nnzA, nnzB) products (register path only)
  const DevCsr &A = P.A, &B = P.B;
  [[maybe_unused]] const int bw = P.bw, W = band_stride(bw), n8 = band_cols(n);      // DIRECT: the band (band_ldl.h)
  // register path: the row pointers of A and B and the direct variant's permutation live in LDS too (they are read in every
  // SpMV / solve of every iteration: an L2 round trip each time otherwise)
  const int prod_len = ((A.nnz > B.nnz ? A.nnz : B.nnz) + 1) & ~1;
  int *rpA = reinterpret_cast<int *>(prod + prod_len), *rpB = rpA + (m + 1), *perm_l = rpB + (n + 1);
  double *Lb = prod + prod_len + batch_index_doubles(n, m) + kBandFront;      // DIRECT: the band factor (band_ldl.h) behind everything else
  double *dinv = zv, *wbuf = r;                     // DIRECT: 1/D and the permuted right-hand side / solution reuse PCG vectors
  constexpr bool kReg = EA > 0;
  double aA[EA > 0 ? EA : 1], aB[EB > 0 ? EB : 1];
  int cA[EA > 0 ? EA : 1], cB[EB > 0 ? EB : 1];
  if constexpr (kReg) {
#pragma unroll
    for (int e = 0; e < EA; e++) { const int k = tid + e * kBB; const bool ok = k < A.nnz; aA[e] = ok ? A.val[k] : 0.0; cA[e] = ok ? A.col[k] : 0; }
#pragma unroll
    for (int e = 0; e < EB; e++) { const int k = tid + e * kBB; const bool ok = k < B.nnz; aB[e] = ok ? B.val[k] : 0.0; cB[e] = ok ? B.col[k] : 0; }
  }
  // out_i = f(i, (A v)_i)  for every row i of A
  auto applyA = [&](const double *v, auto &&f) {
    if constexpr (kReg) {
#pragma unroll
      for (int e = 0; e < EA; e++) { const int k = tid + e * kBB; if (k < A.nnz) prod[k] = aA[e] * v[cA[e]]; }
      __syncthreads();
      for (int i = tid; i < m; i += kBB) f(i, row_sum(prod, rpA[i], rpA[i + 1]));
      __syncthreads();
    } else {
      for (int i = tid; i < m; i += kBB) { double a = 0.0; for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; k++) a += A.val[k] * v[A.col[k]]; f(i, a); }
      __syncthreads();
    }
  };
  // f(j, (B [pn; pm])_j) for every row j of B; pn == nullptr drops the P + sigma I part, pm == nullptr the A' part
  auto applyB = [&](const double *pn, const double *pm, auto &&f) {
    if constexpr (kReg) {
#pragma unroll
      for (int e = 0; e < EB; e++) {
        const int k = tid + e * kBB;
        if (k < B.nnz) { const int c = cB[e]; prod[k] = c < n ? (pn ? aB[e] * pn[c] : 0.0) : (pm ? aB[e] * pm[c - n] : 0.0); }
      }
      __syncthreads();
      for (int j = tid; j < n; j += kBB) f(j, row_sum(prod, rpB[j], rpB[j + 1]));
      __syncthreads();
    } else {
      for (int j = tid; j < n; j += kBB) {
        double a = 0.0;
        for (int k = B.rowptr[j]; k < B.rowptr[j + 1]; k++) { const int c = B.col[k]; a += c < n ? (pn ? B.val[k] * pn[c] : 0.0) : (pm ? B.val[k] * pm[c - n] : 0.0); }
        f(j, a);
      }
      __syncthreads();
    }
  };
  if constexpr (kReg) {
    for (int i = tid; i <= m; i += kBB) rpA[i] = A.rowptr[i];
    for (int j = tid; j <= n; j += kBB) rpB[j] = B.rowptr[j];
    if constexpr (DIRECT) { for (int j = tid; j < n; j += kBB) perm_l[j] = P.perm[j]; }
  }
  // ---- load the problem ----
  // inputs arrive UNSCALED; the scaling of update_lin_cost / update_bounds / warm_start (_osqp.py:1328, :1357-1358, :1505-1506)
  // is applied here (step_rules.h in_q / in_l / in_u / in_x / in_y)
  for (int j = tid; j < n; j += kBB) {
    q[j] = in_q(P.c, P.D[j], P.q ? P.q[(size_t)b * n + j] : P.q0[j]);
    x[j] = P.warm ? in_x(P.x[(size_t)b * n + j], P.Dinv[j]) : 0.0; dx[j] = 0.0;
  }
  int n_ineq_local = 0;
  for (int i = tid; i < m; i += kBB) {
    const double li = in_l(P.E[i], P.l ? P.l[(size_t)b * m + i] : P.l0[i]), ui = in_u(P.E[i], P.u ? P.u[(size_t)b * m + i] : P.u0[i]);
    l[i] = li; u[i] = ui; y[i] = P.warm ? in_y(P.y[(size_t)b * m + i], P.Einv[i], P.c) : 0.0; dy[i] = 0.0;
    n_ineq_local += (row_class(li, ui, P.rho_is_vec) == 0);
  }
  __syncthreads();
  const double n_ineq = red.sum((double)n_ineq_local);
  const double eqf = eq_weight(n_ineq == 0.0, DIRECT ? P.eq_factor_direct : P.eq_factor);
  double rho_bar = P.rho0;
  // SPEC: K^-1 of this problem, and the LDS the form needs (in the band's place): the zero-padded right-hand side, 1 / (1 + delta lambda)
  // SPEC: K^-1 in the register layout of the f64 matrix instruction's result (v_mfma_f64_16x16x4: lane l, register r of a 16 x 16 tile = element
  // (l / 16 + 4 r, l % 16); tools/mfma_f64_layout.hip).  Wave w owns rows 32 w .. 32 w + 31: tiles kacc[tr * 8 + tc], tr = 0, 1 (16 rows each), tc = 0 .. 7.
  typedef double v4d __attribute__((ext_vector_type(4)));
  [[maybe_unused]] v4d kacc[SPEC ? 16 : 1];
  [[maybe_unused]] double *sp_rhs = Lb, *sp_dk = Lb + kBatchSpecN + 2;
  if constexpr (SPEC) {
    // V was built for ONE set of constraint classes: a problem whose own bounds give other classes (or another equality weight) is not ours
    double mism = (eqf != P.sp_eqf) ? 1.0 : 0.0;
    for (int i = tid; i < m; i += kBB) { if (row_class(l[i], u[i], P.rho_is_vec) != P.sp_ctype[i]) mism = 1.0; }
    mism = red.sum(mism);
    if (mism != 0.0) { if (tid == 0) P.rec[(size_t)b * kBatchRec] = kBatchUnsolved; return; }
  }
  // SPEC: K^-1 <- V diag(dk) V',  dk = 1 / (1 + (rb - rho_ref) lambda): V (column-major, kBatchSpecN rows per column) streamed through `prod` in chunks
  [[maybe_unused]] auto update_kinv = [&](double rb) {
    if constexpr (SPEC) {
      BT_BEGIN();
      if (P.sp_K0 && rb == P.sp_K0_rho) {                      // the batch's starting rho: the host has formed this K^-1 once for everybody, in this layout
#pragma unroll
        for (int t = 0; t < 16; t++) {
#pragma unroll
          for (int r = 0; r < 4; r++) kacc[t][r] = P.sp_K0[(size_t)(t * 4 + r) * kBB + tid];
        }
        __syncthreads();
        BT_END(tk_fact);
        return;
      }
      const double dl = rb - P.sp_rho_ref;
      if (tid < kBatchSpecN) sp_dk[tid] = 1.0 / (1.0 + dl * P.sp_lam[tid]);
#pragma unroll
      for (int t = 0; t < 16; t++) kacc[t] = v4d{0.0, 0.0, 0.0, 0.0};
      // K^-1 = (V diag(dk)) V' as a 128 x 128 x 128 product on the matrix cores: per step of four columns of V a wave issues 16 v_mfma_f64_16x16x4
      // (its two row tiles against the eight column tiles); both operands are "V(16 t + l % 16, k + l / 16)" -- ten LDS reads per step.
      const int lj = tid & 15, lk = (tid >> 4) & 3, wv = tid >> 6;
      constexpr int kCol = kBatchSpecN + 2;                     // a staged column: rows 0..63, one double of padding, rows 64..127
      constexpr int kChMax = 16;
      const int CH = min(prod_len / kCol, kChMax) & ~3;         // columns of V per chunk: a multiple of four (batch_solve requires >= 4)
      constexpr int kStage = kChMax * kBatchSpecN / kBB;
      double st[kStage];                                        // the chunk after this one, fetched while this one is consumed
      auto fetch = [&](int k0) {
        const int nk = min(CH, n - k0);
#pragma unroll
        for (int t = 0; t < kStage; t++) { const int e = tid + t * kBB; st[t] = (k0 < n && e < nk * kBatchSpecN) ? P.sp_V[(size_t)k0 * kBatchSpecN + e] : 0.0; }
      };
      const int ra0 = 32 * wv + lj, ra1 = ra0 + 16;
      const int oa0 = ra0 + (ra0 >= 64), oa1 = ra1 + (ra1 >= 64);
      fetch(0);
      for (int k0 = 0; k0 < n; k0 += CH) {
        const int nk = min(CH, n - k0), nk4 = (nk + 3) & ~3;    // (columns nk .. nk4 are staged as zeros)
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kStage; t++) { const int e = tid + t * kBB; if (e < nk4 * kBatchSpecN) { const int kk = e / kBatchSpecN, r_ = e % kBatchSpecN; prod[kk * kCol + r_ + (r_ >= 64)] = st[t]; } }
        __syncthreads();
        fetch(k0 + CH);
        for (int ks = 0; ks < nk4; ks += 4) {
          const double *vc = prod + (ks + lk) * kCol;
          const double dkv = sp_dk[min(k0 + ks + lk, kBatchSpecN - 1)];
          double bb[8];
#pragma unroll
          for (int tc = 0; tc < 8; tc++) bb[tc] = vc[16 * tc + lj + (tc >= 4)];
          const double a0 = vc[oa0] * dkv, a1 = vc[oa1] * dkv;
#pragma unroll
          for (int tc = 0; tc < 8; tc++) {
            kacc[tc] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, bb[tc], kacc[tc], 0, 0, 0);
            kacc[8 + tc] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, bb[tc], kacc[8 + tc], 0, 0, 0);
          }
        }
      }
      __syncthreads();
      BT_END(tk_fact);
    }
  };
  // DIRECT: assemble  K = (P + sigma I) + shift I + A' diag(rho) A  in the band and factorise it (shift = 0 for the ADMM system;
  // the polish step factorises P + delta I + A_act' (1/delta) A_act with shift = delta - sigma and rho = the active-row weights)
  [[maybe_unused]] auto factorize = [&](double shift) {
    BT_BEGIN();
    // ---- assemble K (lower band, permuted) ----
    band_clear<kBB>(Lb, n, bw);
    for (int k = tid; k < B.nnz; k += kBB) { const int s_ = P.bp_slot[k]; if (s_ >= 0) Lb[s_] = B.val[k]; }      // P + sigma I
    __syncthreads();
    if (shift != 0.0) { for (int c = tid; c < n; c += kBB) Lb[band_slot(bw, c, c)] += shift; __syncthreads(); }
    for (int e = tid; e < P.nents; e += kBB) {                                                              // + A' rho A
      double acc = 0.0;
      for (int q_ = P.ke_ptr[e]; q_ < P.ke_ptr[e + 1]; q_++) acc += rho[P.kp_row[q_]] * P.kp_val[q_];
      Lb[P.ke_slot[e]] += acc;
    }
    __syncthreads();
    band_factor<kBB, false>(Lb, n, bw, dinv, P.tri, P.ntri, 0.0);
    BT_END(tk_fact);
  };
  auto set_rho = [&](double rb) {
    // (step_rules.h row_rho, in this kernel's own text: with eqf * rb formed outside the equality branch, as the call needs it, three instantiations
    //  without scratch start to spill and the 64-thread PCG one drops from three waves per SIMD to two: profiles/step_rules_ab.txt)
    for (int i = tid; i < m; i += kBB) {
      const int ty = row_class(l[i], u[i], P.rho_is_vec);
      rho[i] = ty == -1 ? kRowRhoLoose : (ty == 1 ? eqf * rb : rb);                               // _osqp.py:520-522
    }
    __syncthreads();
    if constexpr (SPEC) update_kinv(rb);
    else if constexpr (DIRECT) factorize(0.0);
    else {
      for (int j = tid; j < n; j += kBB) {                   // Jacobi preconditioner = 1/diag(K)
        double sacc = 0.0, dg = 0.0;
        for (int k = B.rowptr[j]; k < B.rowptr[j + 1]; k++) { const int c = B.col[k]; const double a = B.val[k]; if (c == j) dg = a; if (c >= n) sacc += rho[c - n] * a * a; }
        Minv[j] = P.precond ? 1.0 / (dg + sacc) : 1.0;
      }
      __syncthreads();
    }
  };
  // DIRECT: out = K^-1 rhs  (both in the caller's variable order) by the band's substitutions (band_ldl.h); the diagnostic build times the forward pass
  [[maybe_unused]] auto stamp_fwd = [&](int after) { if (after) BT2_END(tk_fwd); else BT2_BEGIN(); };
  auto ksolve = [&](const double *rhs, double *out) {
    if constexpr (SPEC) {
      if (tid < kBatchSpecN) sp_rhs[tid + (tid >= 64)] = tid < n ? rhs[tid] : 0.0;
      __syncthreads();
      BT2_BEGIN();
      // out = K^-1 rhs in the tile layout: a lane multiplies its 64 elements by the right-hand side entries of ITS column (l % 16 of each of the eight
      // column tiles: eight LDS reads, one line per wave instruction), sums over the tiles per row, and the sixteen lanes of a DPP row -- the sixteen
      // columns of a tile -- are summed with row-local DPP moves.  Fixed order, no atomics.
      const int lj = tid & 15, lk = (tid >> 4) & 3, wv = tid >> 6;
      double bb[8];
#pragma unroll
      for (int tc = 0; tc < 8; tc++) bb[tc] = sp_rhs[16 * tc + lj + (tc >= 4)];
      double pv[8];                                             // pv[tr * 4 + r]: this lane's share of row 32 wv + 16 tr + lk + 4 r
#pragma unroll
      for (int tr = 0; tr < 2; tr++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
          double a = kacc[tr * 8][r] * bb[0];
#pragma unroll
          for (int tc = 1; tc < 8; tc++) a = fma(kacc[tr * 8 + tc][r], bb[tc], a);
          pv[tr * 4 + r] = a;
        }
      }
      // eight values per lane, each to be summed over the 16 lanes of its DPP row: two halving exchanges (lane ^ 1, lane ^ 2: a lane keeps the values
      // whose index has its own low bits and hands the others over -- 4 + 2 exchanges instead of 8 + 8), then two rotations by 4 and 8 lanes on the two
      // values left.  Lane lj < 4 ends with the complete sums of rows  16 i + lk + 4 lj,  i = 0, 1.
      const bool b0 = tid & 1, b1 = tid & 2;
      double w4[4], u2[2];
#pragma unroll
      for (int i = 0; i < 4; i++) { const double keep = b0 ? pv[2 * i + 1] : pv[2 * i], send = b0 ? pv[2 * i] : pv[2 * i + 1]; w4[i] = keep + bdpp<0xb1>(send); }
#pragma unroll
      for (int i = 0; i < 2; i++) { const double keep = b1 ? w4[2 * i + 1] : w4[2 * i], send = b1 ? w4[2 * i] : w4[2 * i + 1]; u2[i] = keep + bdpp<0x4e>(send); }
#pragma unroll
      for (int i = 0; i < 2; i++) { u2[i] += bdpp<0x124>(u2[i]); u2[i] += bdpp<0x128>(u2[i]); }      // row_ror:4, row_ror:8
      if (lj < 4) {
#pragma unroll
        for (int i = 0; i < 2; i++) { const int row = 32 * wv + 16 * i + lk + 4 * lj; if (row < n) out[row] = u2[i]; }
      }
      BT2_END(tk_fwd);
      __syncthreads();
      return;
    }
    const double *__restrict__ Lr = Lb;
    constexpr int NB = kBatchNB;
    // N128 (n <= 128, chosen by the host for the 256-thread kernels): a lane's (at most) two elements e = tid, tid + 64 stay in
    // registers from the right-hand side to the solution -- no store / refill of finished elements (an LDS round trip behind the
    // block's eight factor reads on the in-order LDS counter), no barrier between the passes, the D^-1 scaling in registers.
    // Same operations in the same order as the general form below: bit-identical results.  Two things the compiler has to be
    // told: not to unroll the block loop (it then keeps every block's LDS addresses and masks live: 80 spilled VGPRs), and not to
    // sink the next block's factor reads below the chain they are meant to overlap (without an LDS write in the loop nothing
    // stops it): 286 k QP/s without the pin, 327 k with it, 310 k for the general form.
    // (This form and its two fetch lambdas -- the text of band_ldl.h's band_fetch_fwd / band_fetch_bwd -- stay HERE: moved into the header, in any shape,
    //  the instantiations at the 256-register limit spill 12 - 28 bytes more and one that had no scratch starts to: profiles/band_ldl_ab.txt.  The
    //  lambdas read the band by the same padding invariants as the header's helpers -- the zero slot at Lr - 1, the kBatchNB zeros per column, the
    //  read slack: the two texts have to be kept in step.)
    if constexpr (N128) {
#define KSOLVE_PIN() do { asm volatile("" ::: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)
      BT2_BEGIN();
      if (tid < 64) {
        const int e0 = tid, e1 = tid + 64;
        double cur = e0 < n ? rhs[perm_l[e0]] : 0.0, nxt = e1 < n ? rhs[perm_l[e1]] : 0.0;
        const double di0 = e0 < n ? dinv[e0] : 0.0, di1 = e1 < n ? dinv[e1] : 0.0;
        double v0 = 0.0, v1 = 0.0;
        const int nblk = n8 / NB;
        {
          auto fetch = [&](int p0, double (&l)[NB]) {
            const int dl = (tid - p0) & 63;
            const bool act = dl < bw + NB && p0 < n8;
            const double *col = act ? Lr + p0 * W + dl : Lr - 1;
            const int stride = act ? W - 1 : 0;
#pragma unroll
            for (int q = 0; q < NB; q++) l[q] = col[q * stride];
          };
          auto block = [&](int p0, const double (&l)[NB]) {
#pragma unroll
            for (int q = 0; q < NB; q++) { const double vq = readlane_f64(cur, (p0 + q) & 63); cur -= l[q] * vq; }
            const bool piv = ((tid - p0) & 63) < NB, lo = p0 < 64;   // pivoted in this block: final (blocks never straddle element 64)
            v0 = (piv && lo) ? cur : v0; v1 = (piv && !lo) ? cur : v1;
            cur = piv ? nxt : cur;
          };
          double la[NB], lb[NB];
          fetch(0, la);
#pragma clang loop unroll(disable)
          for (int b = 0; b < nblk; b += 2) {
            fetch((b + 1) * NB, lb); KSOLVE_PIN();
            block(b * NB, la);
            if (b + 1 < nblk) { fetch((b + 2) * NB, la); KSOLVE_PIN(); block((b + 1) * NB, lb); }
          }
        }
        BT2_END(tk_fwd);
        v0 *= di0; v1 *= di1;                                     // g = D^-1 v
        {
          const bool two = e1 <= n8 - 1;                          // this lane holds an element of the upper half
          cur = two ? v1 : v0; nxt = two ? v0 : 0.0;
          double x0 = 0.0, x1 = 0.0;
          auto fetch = [&](int top, double (&l)[NB]) {
            const int dl = (top - tid) & 63, i = top - dl;
            const bool act = dl < bw + NB && i >= 0 && top >= 0;
            const double *row = act ? Lr + i * W + dl : Lr - 1;
            const int stride = act ? 1 : 0;
#pragma unroll
            for (int q = 0; q < NB; q++) l[q] = row[-q * stride];
          };
          auto block = [&](int top, const double (&l)[NB]) {
#pragma unroll
            for (int q = 0; q < NB; q++) { const double xq = readlane_f64(cur, (top - q) & 63); cur -= l[q] * xq; }
            const bool piv = ((top - tid) & 63) < NB, hi = top >= 64;
            x1 = (piv && hi) ? cur : x1; x0 = (piv && !hi) ? cur : x0;
            cur = piv ? nxt : cur;
          };
          double la[NB], lb[NB];
          fetch(n8 - 1, la);
#pragma clang loop unroll(disable)
          for (int b = nblk - 1; b >= 0; b -= 2) {
            fetch(b * NB - 1, lb); KSOLVE_PIN();
            block(b * NB + NB - 1, la);
            if (b >= 1) { fetch(b * NB - NB - 1, la); KSOLVE_PIN(); block(b * NB - 1, lb); }
          }
          if (e0 < n) out[perm_l[e0]] = x0;
          if (e1 < n) out[perm_l[e1]] = x1;
        }
      }
      __syncthreads();
      return;
#undef KSOLVE_PIN
    }
    band_solve<kBB>(Lb, n, bw, dinv, perm_l, wbuf, rhs, out, stamp_fwd);
  };
  set_rho(rho_bar);
  // y = A v   (thread per row of A)
  auto spmv_A = [&](const double *v, double *out, bool times_rho) {
    for (int i = tid; i < m; i += kBB) {
      double a = 0.0;
      for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; k++) a += A.val[k] * v[A.col[k]];
      out[i] = times_rho ? rho[i] * a : a;
    }
    __syncthreads();
  };
  // z = A x, zt = A xs (xs = x)   (_osqp.py:1509 / cold start)
  for (int j = tid; j < n; j += kBB) xs[j] = x[j];
  __syncthreads();
  spmv_A(x, z, false);
  for (int i = tid; i < m; i += kBB) { zt[i] = z[i]; if (P.zs && P.warm) z[i] = P.zs[(size_t)b * m + i]; }      // (a continued solve keeps its z iterate)
  __syncthreads();

  // residuals of the current (x, z, y): returns through references; all threads hold identical values
  TermRes R;
  const TermSet tset = {P.eps_abs, P.eps_rel, P.eps_pinf, P.eps_dinf, P.c, P.cinv, m, P.unscaled, P.scaling};
  // (step_rules.h res_row_a / res_row_b / res_store, in this kernel's own text -- the same expressions in the same order, to be kept in step: folded
  //  through the header's accumulators the instantiations at 256 registers spill 24 - 56 bytes more and three that had no scratch start to:
  //  profiles/step_rules_ab.txt.  The lockstep passes call the header; k_batch_wave keeps its own text as well, for another reason, given there.)
  auto residuals = [&]() {
    double a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0, a6 = 0, a7 = 0, a8 = 0, s1 = 0;
    for (int i = tid; i < m; i += kBB) {
      double ax = 0.0;
      for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; k++) ax += A.val[k] * x[A.col[k]];
      const double pr = ax - z[i], ei = P.Einv[i], dyi = dy[i];
      a1 = nanmax(a1, fabs(ei * pr)); a2 = nanmax(a2, fabs(ei * ax)); a3 = nanmax(a3, fabs(ei * z[i]));
      a4 = nanmax(a4, fabs(pr)); a5 = nanmax(a5, fabs(ax)); a6 = nanmax(a6, fabs(z[i]));
      a7 = nanmax(a7, fabs(P.E[i] * dyi)); a8 = nanmax(a8, fabs(dyi));
      s1 += u[i] * fmax(dyi, 0.0) + l[i] * fmin(dyi, 0.0);
    }
    { double g1[4] = {a1, a2, a3, a4}, g2[4] = {a5, a6, a7, a8}, g3[1] = {s1}, none[1] = {0.0};
      red.template max_sum_n<4, 0>(g1, none); red.template max_sum_n<4, 0>(g2, none); red.template max_sum_n<0, 1>(none, g3);
      R.pri_u = g1[0]; R.ax_u = g1[1]; R.z_u = g1[2]; R.pri_s = g1[3]; R.ax_s = g2[0]; R.z_s = g2[1]; R.dy_u = g2[2]; R.dy_s = g2[3]; R.pinf_lhs = g3[0]; }
    double b1 = 0, b2 = 0, b3 = 0, b4 = 0, b5 = 0, b6 = 0, b7 = 0, b8 = 0, b9 = 0, b10 = 0, t1 = 0, t2 = 0, t3 = 0;
    for (int j = tid; j < n; j += kBB) {
      double sp = 0.0, sa = 0.0;
      for (int k = B.rowptr[j]; k < B.rowptr[j + 1]; k++) { const int c = B.col[k]; if (c < n) sp += B.val[k] * x[c]; else sa += B.val[k] * y[c - n]; }
      const double px = sp - P.sigma * x[j], dr = px + q[j] + sa, di = P.Dinv[j];
      b1 = nanmax(b1, fabs(di * dr)); b2 = nanmax(b2, fabs(di * px)); b3 = nanmax(b3, fabs(di * sa));
      b4 = nanmax(b4, fabs(dr)); b5 = nanmax(b5, fabs(px)); b6 = nanmax(b6, fabs(sa));
      b7 = nanmax(b7, fabs(P.D[j] * dx[j])); b8 = nanmax(b8, fabs(dx[j])); b9 = nanmax(b9, fabs(q[j])); b10 = nanmax(b10, fabs(di * q[j]));
      t1 += x[j] * px; t2 += q[j] * x[j]; t3 += q[j] * dx[j];
    }
    { double g1[4] = {b1, b2, b3, b4}, g2[4] = {b5, b6, b7, b8}, g3[2] = {b9, b10}, sm[2] = {t1, t2}, g4[1] = {t3}, none[1] = {0.0};
      red.template max_sum_n<4, 0>(g1, none); red.template max_sum_n<4, 0>(g2, none); red.template max_sum_n<2, 2>(g3, sm); red.template max_sum_n<0, 1>(none, g4);
      R.dua_u = g1[0]; R.px_u = g1[1]; R.aty_u = g1[2]; R.dua_s = g1[3]; R.px_s = g2[0]; R.aty_s = g2[1]; R.dxn_u = g2[2]; R.dxn_s = g2[3]; R.qn_s = g3[0]; R.qn_u = g3[1];
      R.xpx = sm[0]; R.qx = sm[1]; R.qdx = g4[0]; }
  };

  int status = OSQP_UNSOLVED, iter = 0, rho_updates = 0;
  long pcg_total = 0;
  double obj = 0, prim_res = 0, dual_res = 0;
  residuals();
  double eps_cg, eps_prev;
  bool rel_rule;
  batch_tol_init(P.cg_frac, R.dua_s, &eps_prev, &eps_cg, &rel_rule);
  const bool unsc = P.unscaled != 0;
  // the second stages of the infeasibility tests (term_rules.h batch_check calls them when a first stage passed: uniform over the workgroup)
  auto pinf_stage2 = [&](double &mu, double &ms) {                                     // A' dy   (is_primal_infeasible :815-818)
    for (int j = tid; j < n; j += kBB) {
      double sa = 0.0;
      for (int k = B.rowptr[j]; k < B.rowptr[j + 1]; k++) { const int c = B.col[k]; if (c >= n) sa += B.val[k] * dy[c - n]; }
      mu = nanmax(mu, fabs(P.Dinv[j] * sa)); ms = nanmax(ms, fabs(sa));
    }
    mu = red.max(mu); ms = red.max(ms);
  };
  auto pdx_stage2 = [&](double &mu, double &ms) {                                      // P dx    (is_dual_infeasible :846-853)
    for (int j = tid; j < n; j += kBB) {
      double sp = 0.0;
      for (int k = B.rowptr[j]; k < B.rowptr[j + 1]; k++) { const int c = B.col[k]; if (c < n) sp += B.val[k] * dx[c]; }
      sp -= P.sigma * dx[j];
      mu = nanmax(mu, fabs(P.Dinv[j] * sp)); ms = nanmax(ms, fabs(sp));
    }
    mu = red.max(mu); ms = red.max(ms);
  };
  auto adx_stage2 = [&](double thr) {                                                  // A dx    (:855-872)
    double viol = 0;
    for (int i = tid; i < m; i += kBB) {
      double a = 0.0;
      for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; k++) a += A.val[k] * dx[A.col[k]];
      if (unsc) a *= P.Einv[i];
      if (adx_violates(a, l[i], u[i], thr)) viol += 1.0;
    }
    viol = red.sum(viol);
    return viol == 0.0;
  };
  // settings.check_dualgap: the support function of the scaled box at y, the dual objective and the gap of the point residuals() has just measured
  // (term_rules.h term_dual_obj; a pass of its own, compiled into the GAP instantiations only: residuals() is what it was).  Uniform over the workgroup.  Nothing
  // of it lives across an ADMM iteration: the record's gap is formed again behind the loop, from the same point by the same text -- the same bits.
  constexpr bool gap_on = GAP;                                                         // (batch_solve picks the instantiation by P.check_dualgap)
  auto duality_gap = [&](double obj_of_point, double *dual_obj) {
    double sp = 0.0;
    for (int i = tid; i < m; i += kBB) sp += support_finite(l[i], u[i], y[i]);
    *dual_obj = term_dual_obj(tset, R, red.sum(sp));
    return obj_of_point - *dual_obj;
  };

  while (true) {
    iter++;
    // ---- rhs = sigma x - q + A'(rho z - y);  r = rhs - K xs with K xs = B[xs; rho zt]   (_osqp.py:649-650) ----
    [[maybe_unused]] double rz_l = 0, rn_l = 0, bn_l = 0;
    BT2_BEGIN();
    for (int i = tid; i < m; i += kBB) t[i] = rho[i] * z[i] - y[i];
    __syncthreads();
    applyB(nullptr, t, [&](int j, double sA) { Kp[j] = P.sigma * x[j] - q[j] + sA; });          // Kp holds rhs for a moment
    BT2_END(tk_rhs);
    if constexpr (DIRECT) {
      BT_BEGIN();
      ksolve(Kp, xs);                                                                    // x~ = K^-1 rhs   (_osqp.py:307-311, reduced form)
      BT_END(tk_solve);
    } else {
      for (int i = tid; i < m; i += kBB) t[i] = rho[i] * zt[i];
      __syncthreads();
      applyB(xs, t, [&](int j, double sK) {
        const double rhs = Kp[j], rr = rhs - sK, zz = Minv[j] * rr;
        r[j] = rr; zv[j] = zz; p[j] = zz;
        rz_l += rr * zz; rn_l = nanmax(rn_l, fabs(rr)); bn_l = nanmax(bn_l, fabs(rhs));
      });
      double rz = rz_l, rn = rn_l;
      red.sum_max(rz, rn);
      const double bn = red.max(bn_l);
      const double tol = rel_rule ? fmax(0.1 * bn, 1e-13) : fmax(1e-14 * bn, eps_cg);
      // ---- PCG on K = P + sigma I + A' diag(rho) A ----
      for (int it = 0; it < P.cg_max && rn > tol; it++) {
        applyA(p, [&](int i, double a) { t[i] = rho[i] * a; });              // t = rho .* (A p)
        double pkp_l = 0.0;
        applyB(p, t, [&](int j, double a) { Kp[j] = a; pkp_l += a * p[j]; });
        const double pkp = red.sum(pkp_l);
        const double al = rz / pkp;
        double rz2 = 0.0, rn2 = 0.0;
        for (int j = tid; j < n; j += kBB) {
          xs[j] += al * p[j];
          const double rr = r[j] - al * Kp[j], zz = Minv[j] * rr;
          r[j] = rr; zv[j] = zz;
          rz2 += rr * zz; rn2 = nanmax(rn2, fabs(rr));
        }
        red.sum_max(rz2, rn2);
        const double be = rz2 / rz;
        rz = rz2; rn = rn2;
        for (int j = tid; j < n; j += kBB) p[j] = zv[j] + be * p[j];
        __syncthreads();
        pcg_total++;
      }
    }
    // ---- z~ = A xs; x, z, y update (_osqp.py:660-703) ----
    BT2_BEGIN();
    applyA(xs, [&](int i, double a) {
      const StepRow s = step_row(P.alpha, a, rho[i], z[i], y[i], l[i], u[i]);
      y[i] = s.y; dy[i] = s.dy; z[i] = s.z; zt[i] = a;
    });
    for (int j = tid; j < n; j += kBB) { const StepCol s = step_col(P.alpha, xs[j], x[j]); dx[j] = s.dx; x[j] = s.x; }
    __syncthreads();
    BT2_END(tk_upd);

    const bool at_check = (P.check > 0 && iter % P.check == 0) || iter >= P.max_iter;
    const bool at_rho = P.rho_interval > 0 && iter % P.rho_interval == 0;
    if (!at_check && !at_rho) continue;
    BT2_BEGIN();
    residuals();
    BT2_END(tk_res);
    term_info(tset, R, &obj, &prim_res, &dual_res);
    double dual_obj = 0.0, gap = 0.0;
    if (gap_on && at_check) gap = duality_gap(obj, &dual_obj);
    const int st = batch_check_gap(tset, R, prim_res, dual_res, iter, P.max_iter, at_check, pinf_stage2, pdx_stage2, adx_stage2, &obj, gap_on, dual_obj, gap);
    if (st != kBatchGoOn) { status = st; break; }
    double rho_new;
    if (at_rho && batch_rho_rule(rho_bar, P.rho_tol, R, &rho_new)) { rho_bar = rho_new; set_rho(rho_bar); rho_updates++; }
    batch_tol_rule(P.cg_frac, R.dua_s, &eps_prev, &eps_cg, &rel_rule);                 // inner tolerance: engine.cpp solve()
  }
  // ---- polish (_osqp.py:1710-1828), direct variants only: the reference's algorithm on the factor already in LDS ----
  // Active rows guessed from the scaled (z, y) (:1719-1720); the regularised reduced KKT system
  //     [P + delta I, A_act'; A_act, -delta I] [dx; dy] = [r1; r2]
  // is solved through its Schur complement  (P + delta I + A_act' A_act / delta) dx = r1 + A_act' r2 / delta,  dy = (A_act dx - r2) / delta,
  // ONE banded factorisation (factorize: weights 1/delta on active rows, 0 elsewhere, diagonal shift delta - sigma), and the
  // first solve plus polish_refine_iter refinement steps (:1692-1708) all have the same form: with (x, y) = 0 at the start,
  //     t = y - (b - A_act x) / delta,   rhs = -q - P x - A_act' t,   dx = K^-1 rhs,   x += dx,   y = t + A_act dx / delta.
  // Then z = A x, the normal-cone projection (:1773-1780) and the accept test on the residuals (:1786-1793).
  // rho estimate of the ADMM point (_osqp.py:1275, :880-908), before any polish
  const double rho_est = term_rho_estimate(rho_bar, R);
  // check_dualgap: the gap of the ADMM point the loop ended at (where obj carries a status convention instead, batch_record_gap writes NaN)
  double rec_gap = 0.0;
  if (gap_on) { double dobj; rec_gap = duality_gap(obj, &dobj); }
  int status_polish = 0;
  [[maybe_unused]] unsigned long long pol_ticks = 0;
  if constexpr (DIRECT && POLISH) {
    if (status == OSQP_SOLVED) {
      const unsigned long long tp0 = wall_clock64();
      const double idel = 1.0 / P.delta;
      // ADMM point kept in p (x), zt (z), dy (y): none of them is live in the direct variant after the loop
      for (int j = tid; j < n; j += kBB) { p[j] = x[j]; x[j] = 0.0; }
      for (int i = tid; i < m; i += kBB) {
        const double zi = z[i], yi = y[i];
        zt[i] = zi; dy[i] = yi;
        const RowActive act = polish_active(zi, l[i], u[i], yi);
        rho[i] = (act.low || act.upp) ? idel : 0.0;
        z[i] = act.low ? l[i] : u[i];                                              // b_i of an active row (unused otherwise)
        y[i] = 0.0;
      }
      __syncthreads();
      factorize(P.delta - P.sigma);
      // The Schur complement amplifies an error of A x - b by 1/delta: the constraint residual of the current x is accumulated in
      // double-double (exact products by FMA, compensated sums), the classic higher-precision residual of iterative refinement,
      // and y advances by the correction of the step (t + A dx / delta) -- its noise floor is eps |y|, not eps |A||x| / delta.
      for (int k = 0; k <= P.refine; k++) {
        for (int i = tid; i < m; i += kBB) {
          double tv = 0.0;
          if (rho[i] != 0.0) {
            double hi = -z[i], lo = 0.0;                                        // (A x)_i - b_i
            for (int e = A.rowptr[i]; e < A.rowptr[i + 1]; e++) {
              const double a = A.val[e], v = x[A.col[e]];
              dd_acc(a, v, hi, lo);
            }
            tv = y[i] + (hi + lo) * idel;                                       // y - r2 / delta,  r2 = b - A x
          }
          t[i] = tv;
        }
        __syncthreads();
        applyB(x, t, [&](int j, double s_) { Kp[j] = -q[j] + P.sigma * x[j] - s_; });       // (B carries P + sigma I)
        ksolve(Kp, Minv);
        for (int j = tid; j < n; j += kBB) x[j] += Minv[j];
        __syncthreads();
        applyA(Minv, [&](int i, double adx) { if (rho[i] != 0.0) y[i] = t[i] + adx * idel; });
      }
      applyA(x, [&](int i, double ax) { const ConeRow c = normal_cone(ax + y[i], l[i], u[i]); z[i] = c.z; y[i] = c.y; });
      const double pri0 = prim_res, dua0 = dual_res;
      residuals();
      double pobj, ppri, pdua;
      term_info(tset, R, &pobj, &ppri, &pdua);
      if (polish_accept(ppri, pdua, pri0, dua0)) {
        obj = pobj; prim_res = ppri; dual_res = pdua; status_polish = 1;
        if (gap_on) { double dobj; rec_gap = duality_gap(obj, &dobj); }              // (the record's gap is the polished point's; uniform: so are its barriers)
      } else {
        status_polish = -1;
        for (int j = tid; j < n; j += kBB) x[j] = p[j];
        for (int i = tid; i < m; i += kBB) { z[i] = zt[i]; y[i] = dy[i]; }
      }
      __syncthreads();
      pol_ticks = wall_clock64() - tp0;
    }
  }
  // ---- store: x = D x, y = cinv E y (_osqp.py:1110-1112); certificates in place of x / y for infeasible problems ----
  for (int j = tid; j < n; j += kBB) P.x[(size_t)b * n + j] = batch_out_x(status, P.unscaled, P.scaling, P.D[j], x[j], dx[j]);
  if (P.zs) for (int i = tid; i < m; i += kBB) P.zs[(size_t)b * m + i] = z[i];
  for (int i = tid; i < m; i += kBB) P.y[(size_t)b * m + i] = batch_out_y(status, P.unscaled, P.scaling, P.cinv, P.E[i], y[i], dy[i]);
  if (tid == 0) {
    double *rc = P.rec + (size_t)b * kBatchRec;
    batch_record(rc, status, iter, obj, prim_res, dual_res, rho_bar, rho_updates, (double)pcg_total, rho_est);
    rc[8] = status_polish; rc[9] = 1e-8 * (double)pol_ticks;      // (100 MHz wall clock -> seconds)
    if (gap_on) batch_record_gap(rc, status, rec_gap);
    if (P.iters_out) P.iters_out[b] = iter;
#ifdef OSQP_HIP_KTRACE
    rc[5] = (double)tk_fact; rc[6] = (double)tk_solve; rc[7] = (double)(wall_clock64() - tk_all);
    rc[3] = (double)tk_rhs; rc[4] = (double)tk_upd; rc[8] = (double)tk_fwd; rc[9] = (double)tk_res;
#endif
  }
}


// ---------------------------------------------------------------------------------------------------------------- one WAVE per problem, spectral form
// k_batch_admm gives a problem a whole workgroup -- and, in its spectral form, the whole register file of a CU for K^-1: ONE problem in flight per CU,
// 3.7 us per ADMM iteration of which the dense product is 0.6 (profiles/r06_batch_trace.txt).  Here a problem is ONE WAVE and a CU runs kBatchWaveW of
// them at once, with what they share kept once:
//   * V (the batch's common eigenvectors, engine.hpp BatchSpectral) in LDS, row-major with an odd row stride -- 116 KB at n = 120.  A solve is
//     x~ = V (d . (V' rhs)),  d_k = 1 / (1 + (rho - rho_ref) lambda_k):  two passes over V by the wave itself (lane k reads column k of row j for V' rhs --
//     consecutive words; lane i reads row i for V t -- stride 121 doubles: conflict-free), the vector entries broadcast with v_readlane from the lane
//     that owns them.  No K^-1 exists: a rho update is two divisions per lane (the workgroup kernel rebuilds K^-1 from V: ~20 us).
//   * the matrices' values once in LDS as well, in ELL steps with one lane per row (BatchParams::wv_*: groups of 64 rows, A's rows sorted by length so
//     that a step's rows are about equally long -- 26 KB for the MPC pattern); every wave keeps its lanes' column indices in registers (two per
//     register) and gathers through one staged vector of its own in LDS.  (Values in registers -- 112 more per lane -- was the first form: 185 of them
//     spilled at eight waves per CU.)
//   * every iterate in registers (n <= 128: two slots per lane, m <= 256: four); reductions are DPP moves + v_readlane.  No barrier after the prologue:
//     a wave takes the next position of the launch order from a device counter when its problem is done (longest-expected problems first, as before).
// Same arithmetic as k_batch_admm's direct path up to the order of the sums (FMA chains per row here, products summed in entry order there; the two-stage
// solve instead of K^-1 times rhs): iteration counts agree, iterates to ~1e-12 (tests/test_gpu_batch_wave.py).
#ifdef OSQP_HIP_KTRACE
#define WT_MARK(v) const unsigned long long v = wall_clock64()
#define WT_ADD(acc, d) (acc += (d))
#else
#define WT_MARK(v) ((void)0)
#define WT_ADD(acc, d) ((void)0)
#endif
template <int N8>
__global__ __launch_bounds__(64 * kBatchWaveW, 1) void k_batch_wave(BatchParams P) {
  static_assert(N8 % 8 == 0 && N8 <= kBatchSpecN, "rows / columns of V in LDS (n rounded up; zero beyond n): compile-time -- the dense products are straight-line code");
  constexpr int S = N8 + 1;                            // row stride: odd (conflict-free column walks)
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int n = P.n, m = P.m, tid = threadIdx.x, L = tid & 63, wv = tid >> 6;
  constexpr int n8 = N8;                               // (>= n: batch_solve picks the instantiation)
  double *Vl = sm;
  const int stg_len = ((n > m ? n : m) + 1) & ~1;
  const int ae0 = P.wv_aend[0], ae1 = P.wv_aend[1], ae2 = P.wv_aend[2], ae3 = P.wv_aend[3], te0 = P.wv_tend[0], te1 = P.wv_tend[1];
  double *eA = sm + (((size_t)n8 * S + 1) & ~(size_t)1), *eT = eA + (size_t)ae3 * 64;
  double *stage = eT + (size_t)te1 * 64 + (size_t)wv * stg_len;
  unsigned short *kA = reinterpret_cast<unsigned short *>(eT + (size_t)te1 * 64 + (size_t)kBatchWaveW * stg_len), *kT = kA + (size_t)ae3 * 64;
  for (int e = tid; e < n8 * S; e += 64 * kBatchWaveW) Vl[e] = 0.0;
  for (int e = tid; e < ae3 * 64; e += 64 * kBatchWaveW) { const int ix = P.wv_Aidx[e]; eA[e] = ix >= 0 ? P.A.val[ix] : 0.0; kA[e] = (unsigned short)P.wv_Acol[e]; }
  for (int e = tid; e < te1 * 64; e += 64 * kBatchWaveW) { const int ix = P.wv_Tidx[e]; eT[e] = ix >= 0 ? P.B.val[ix] : 0.0; kT[e] = (unsigned short)P.wv_Tcol[e]; }
  __syncthreads();
  for (int e = tid; e < n * kBatchSpecN; e += 64 * kBatchWaveW) { const int k = e / kBatchSpecN, j = e % kBatchSpecN; if (j < n) Vl[j * S + k] = P.sp_V[e]; }      // V(j, k)
  __syncthreads();                                       // (the last barrier of the kernel)
  const DevCsr &B = P.B;
  // ---- the matrices: ELL values and columns (16 bits) in LDS, one copy for the eight waves ----
  int rowm[4]; bool vm[4], vn[2];
#pragma unroll
  for (int s = 0; s < 4; s++) { rowm[s] = (s * 64 + L < 256) ? P.wv_row[s * 64 + L] : -1; vm[s] = rowm[s] >= 0; if (!vm[s]) rowm[s] = 0; }
#pragma unroll
  for (int s = 0; s < 2; s++) vn[s] = s * 64 + L < n;
  const int jn[2] = {min(L, n - 1), min(64 + L, n - 1)};          // (clamped: lanes without an element read a valid one and drop the result)
  const double lam0 = P.sp_lam[jn[0]], lam1 = P.sp_lam[jn[1]];
  auto wave_sync = [&]() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); };
  auto wsum = [&](double v) { return readlane_f64(wsum63(v), 63); };
  auto wmax = [&](double v) { return readlane_f64(wmax63(v), 63); };
  auto stage_n = [&](const double (&v)[2]) {
    wave_sync();
#pragma unroll
    for (int s = 0; s < 2; s++) if (vn[s]) stage[s * 64 + L] = v[s];
    wave_sync();
  };
  auto stage_m = [&](const double (&v)[4]) {
    wave_sync();
#pragma unroll
    for (int s = 0; s < 4; s++) if (vm[s]) stage[rowm[s]] = v[s];
    wave_sync();
  };
  // one group of 64 rows: steps [s0, s1) of an ELL array (values ev, 16-bit columns kv; a lane's entries beyond its row are padding: value 0, column 0)
  // against the vector staged in LDS.  A runtime loop per group with nothing but loads and one FMA chain in it (first form: one unrolled sequence over
  // all groups with the group picked by uniform branches per step -- the compiler turned that into a branch and two dependent LDS round trips per step,
  // 6 of an iteration's 12 us).
  auto ell_group = [&](const double *ev, const unsigned short *kv, int s0, int s1) {
    // (blocks of four steps: four column reads and four value reads, then the four gathers, then the FMAs -- two LDS round trips per block; written as a
    //  plain loop the compiler serialises column read -> gather -> FMA per step.  The steps of a last, partial block re-read the group's last step with
    //  the value replaced by zero.)
    double acc = 0.0;
    for (int b0 = s0; b0 < s1; b0 += 4) {
      int c[4]; double v[4], pv[4];
#pragma unroll
      for (int j = 0; j < 4; j++) { const bool on = b0 + j < s1; const int si = on ? b0 + j : s1 - 1; c[j] = kv[si * 64 + L]; v[j] = ev[si * 64 + L]; v[j] = on ? v[j] : 0.0; }
#pragma unroll
      for (int j = 0; j < 4; j++) pv[j] = stage[c[j]];
#pragma unroll
      for (int j = 0; j < 4; j++) acc = fma(v[j], pv[j], acc);
    }
    return acc;
  };
  // out[slot] = (A v)_row for the n-vector v staged in LDS
  auto mulA = [&](double (&out)[4]) { out[0] = ell_group(eA, kA, 0, ae0); out[1] = ell_group(eA, kA, ae0, ae1); out[2] = ell_group(eA, kA, ae1, ae2); out[3] = ell_group(eA, kA, ae2, ae3); };
  // out[slot] = (A' w)_j for the m-vector w staged in LDS (original row numbering)
  auto mulT = [&](double (&out)[2]) { out[0] = ell_group(eT, kT, 0, te0); out[1] = ell_group(eT, kT, te0, te1); };
  // out[slot] = ((P + sigma I) v)_j for the n-vector staged in LDS: B's entries with column < n, from memory (residuals and certificates only)
  auto mulP = [&](double (&out)[2]) {
#pragma unroll
    for (int s = 0; s < 2; s++) {
      double a = 0.0;
      if (vn[s]) { const int j = s * 64 + L; for (int k = B.rowptr[j]; k < B.rowptr[j + 1]; k++) { const int c = B.col[k]; if (c < n) a = fma(B.val[k], stage[c], a); } }
      out[s] = a;
    }
  };
  // The two dense products of a solve, x~ = V (d . (V' rhs)), fully unrolled, straight-line code (the size n8 of the LDS copy is a template parameter): every
  // LDS offset and every v_readlane lane index is then an immediate -- per step one or two reads, two v_readlane, two FMAs.  (First form: a runtime loop,
  // indices in registers: a v_add per read, an s_add + wait states per v_readlane -- 2 250 instructions per solve, 10 of an iteration's 23 us with eight
  // waves per CU.  Rows / columns n .. n8 of the LDS copy are zero.)
  // (Every block of eight steps sits behind a uniform branch on an OPAQUE copy of n8: the branch is never taken, but it keeps the compiler from treating a
  //  product as one straight line -- it then hoists all 240 reads and the v_readlanes in front of the FMAs and spills 500 - 1 000 registers, with or
  //  without scheduling barriers between hand-pipelined blocks: 12.5 ms per batch instead of 4.9.)
  // w = V' rhs: lane = column k (and k + 64), step = row j;  rhs_j from lane j % 64 of rhs[j / 64]
  auto vt_mul = [&](const double (&rhs)[2], double &o0, double &o1) {
    const double *vc = Vl + L;
    int n8r = N8;
    asm volatile("" : "+s"(n8r));
    double a0[2] = {0.0, 0.0}, a1[2] = {0.0, 0.0};
    double va[8], vb[8], na[8], nb[8];
    auto load = [&](int j0, double (&ua)[8], double (&ub)[8]) {
#pragma unroll
      for (int jj = 0; jj < 8; jj++) { ua[jj] = vc[(j0 + jj) * S]; ub[jj] = vc[(j0 + jj) * S + 64]; }
    };
    auto compute = [&](int j0, const double (&ua)[8], const double (&ub)[8]) {
#pragma unroll
      for (int jj = 0; jj < 8; jj++) { const double r = readlane_f64(rhs[j0 >> 6], (j0 & 63) + jj); a0[jj & 1] = fma(ua[jj], r, a0[jj & 1]); a1[jj & 1] = fma(ub[jj], r, a1[jj & 1]); }
    };
    load(0, va, vb);
#pragma unroll
    for (int j0 = 0; j0 < N8; j0 += 16) {
      if (j0 < n8r) { if (j0 + 8 < N8) load(j0 + 8, na, nb); compute(j0, va, vb); }            // (the block's reads are the NEXT block's: one LDS latency behind eight steps of FMAs)
      if (j0 + 8 < N8 && j0 + 8 < n8r) { if (j0 + 16 < N8) load(j0 + 16, va, vb); compute(j0 + 8, na, nb); }
    }
    o0 = a0[0] + a0[1]; o1 = a1[0] + a1[1];
  };
  // x = V t: lane = row i (and i + 64), step = column k
  auto v_mul = [&](double t0, double t1, double &o0, double &o1) {
    const double *vr0 = Vl + jn[0] * S, *vr1 = Vl + jn[1] * S;
    int n8r = N8;
    asm volatile("" : "+s"(n8r));
    double a0[2] = {0.0, 0.0}, a1[2] = {0.0, 0.0};
    double va[8], vb[8], na[8], nb[8];
    auto load = [&](int k0, double (&ua)[8], double (&ub)[8]) {
#pragma unroll
      for (int kk = 0; kk < 8; kk++) { ua[kk] = vr0[k0 + kk]; ub[kk] = vr1[k0 + kk]; }
    };
    auto compute = [&](int k0, const double (&ua)[8], const double (&ub)[8]) {
#pragma unroll
      for (int kk = 0; kk < 8; kk++) { const double r = readlane_f64(k0 < 64 ? t0 : t1, (k0 & 63) + kk); a0[kk & 1] = fma(ua[kk], r, a0[kk & 1]); a1[kk & 1] = fma(ub[kk], r, a1[kk & 1]); }
    };
    load(0, va, vb);
#pragma unroll
    for (int k0 = 0; k0 < N8; k0 += 16) {
      if (k0 < n8r) { if (k0 + 8 < N8) load(k0 + 8, na, nb); compute(k0, va, vb); }
      if (k0 + 8 < N8 && k0 + 8 < n8r) { if (k0 + 16 < N8) load(k0 + 16, va, vb); compute(k0 + 8, na, nb); }
    }
    o0 = a0[0] + a0[1]; o1 = a1[0] + a1[1];
  };
  auto ksolve = [&](const double (&rhs)[2], double dk0, double dk1, double (&out)[2]) {
    double w0, w1;
    vt_mul(rhs, w0, w1);
    v_mul(vn[0] ? dk0 * w0 : 0.0, vn[1] ? dk1 * w1 : 0.0, out[0], out[1]);
  };
  const bool unsc = P.unscaled != 0;
  const TermSet tset = {P.eps_abs, P.eps_rel, P.eps_pinf, P.eps_dinf, P.c, P.cinv, m, P.unscaled, P.scaling};
  bool first = true;

  while (true) {
    // ---- the next problem of the launch order ----
    // The first problem of a wave is position (wave index) x (workgroups) + (workgroup): the longest-expected problems land one per CU.  Later ones
    // come from the device counter.  (EVERY lane adds one -- the compiler folds that into a single atomic per wave -- and the counter runs in units of
    //  64.  The obvious form, lane 0 alone behind `if (L == 0)`, hangs: the loop is then compiled with a second version for the lanes that never run the
    //  atomic, whose position stays 0.)
    int pos;
    if (first) { pos = P.wv_first + __builtin_amdgcn_readfirstlane(wv) * (int)gridDim.x + (int)blockIdx.x; first = false; }
    else pos = P.wv_first + (int)gridDim.x * kBatchWaveW + (__builtin_amdgcn_readfirstlane(atomicAdd(P.wv_queue, 1)) >> 6);
    if (pos >= P.nbatch) break;
    const int b = P.order ? P.order[pos] : pos;
    double x[2], q[2], dx[2], xs[2], z[4], y[4], l[4], u[4], dy[4];
    int ty[4];
#pragma unroll
    for (int s = 0; s < 2; s++) {
      const int j = jn[s];
      q[s] = vn[s] ? in_q(P.c, P.D[j], P.q ? P.q[(size_t)b * n + j] : P.q0[j]) : 0.0;
      x[s] = (vn[s] && P.warm) ? in_x(P.x[(size_t)b * n + j], P.Dinv[j]) : 0.0; dx[s] = 0.0; xs[s] = 0.0;
    }
    double n_ineq_l = 0.0, mism = 0.0;
#pragma unroll
    for (int s = 0; s < 4; s++) {
      const int i = rowm[s];
      const double li = in_l(P.E[i], P.l ? P.l[(size_t)b * m + i] : P.l0[i]), ui = in_u(P.E[i], P.u ? P.u[(size_t)b * m + i] : P.u0[i]);
      l[s] = vm[s] ? li : 0.0; u[s] = vm[s] ? ui : 0.0;
      y[s] = (vm[s] && P.warm) ? in_y(P.y[(size_t)b * m + i], P.Einv[i], P.c) : 0.0; dy[s] = 0.0; z[s] = 0.0;
      const int t_ = row_class(li, ui, P.rho_is_vec);
      ty[s] = t_;
      if (vm[s]) { n_ineq_l += (t_ == 0); if (t_ != P.sp_ctype[i]) mism = 1.0; }
    }
    const double n_ineq = wsum(n_ineq_l);
    const double eqf = eq_weight(n_ineq == 0.0, P.eq_factor_direct);
    // V was built for ONE set of constraint classes: a problem whose own bounds give other classes (or another equality weight) is the banded kernel's
    mism = wsum(mism) + (eqf != P.sp_eqf ? 1.0 : 0.0);
    if (mism != 0.0) { if (L == 0) P.rec[(size_t)b * kBatchRec] = kBatchUnsolved; continue; }
    double rho_bar = P.rho0, rho_eq = 0.0, dk0 = 0.0, dk1 = 0.0;
    auto rho_of = [&](int s) { return row_rho(ty[s], rho_bar, rho_eq); };             // (three values: not kept per row)
    auto set_rho = [&](double rb) {
      rho_eq = eqf * rb;
      const double dl = rb - P.sp_rho_ref;
      dk0 = 1.0 / (1.0 + dl * lam0); dk1 = 1.0 / (1.0 + dl * lam1);
    };
    set_rho(rho_bar);
    // z = A x   (_osqp.py:1509 / cold start); a continued solve keeps its z iterate
    stage_n(x);
    mulA(z);
    if (P.zs && P.warm) {
#pragma unroll
      for (int s = 0; s < 4; s++) if (vm[s]) z[s] = P.zs[(size_t)b * m + rowm[s]];
    }
    TermRes R = {};
    // (step_rules.h res_row_a / res_row_b / res_store, in this kernel's own text -- the same expressions in the same order, to be kept in step: through
    //  the header the two products of the support term reach the compiler in the other order and the other one is contracted into the FMA, another
    //  rounding of pinf_lhs: profiles/step_rules_ab.txt)
    auto residuals = [&]() {
      double a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0, a6 = 0, a7 = 0, a8 = 0, s1 = 0;
      stage_n(x);
      double ax[4], sp[2], sa[2];
      mulA(ax); mulP(sp);
#pragma unroll
      for (int s = 0; s < 4; s++) if (vm[s]) {
        const int i = rowm[s];
        const double pr = ax[s] - z[s], ei = P.Einv[i], dyi = dy[s];
        a1 = nanmax(a1, fabs(ei * pr)); a2 = nanmax(a2, fabs(ei * ax[s])); a3 = nanmax(a3, fabs(ei * z[s]));
        a4 = nanmax(a4, fabs(pr)); a5 = nanmax(a5, fabs(ax[s])); a6 = nanmax(a6, fabs(z[s]));
        a7 = nanmax(a7, fabs(P.E[i] * dyi)); a8 = nanmax(a8, fabs(dyi));
        s1 += u[s] * fmax(dyi, 0.0) + l[s] * fmin(dyi, 0.0);
      }
      R.pri_u = wmax(a1); R.ax_u = wmax(a2); R.z_u = wmax(a3); R.pri_s = wmax(a4); R.ax_s = wmax(a5); R.z_s = wmax(a6); R.dy_u = wmax(a7); R.dy_s = wmax(a8); R.pinf_lhs = wsum(s1);
      stage_m(y);
      mulT(sa);
      double b1 = 0, b2 = 0, b3 = 0, b4 = 0, b5 = 0, b6 = 0, b7 = 0, b8 = 0, b9 = 0, b10 = 0, t1 = 0, t2 = 0, t3 = 0;
#pragma unroll
      for (int s = 0; s < 2; s++) if (vn[s]) {
        const int j = s * 64 + L;
        const double px = sp[s] - P.sigma * x[s], dr = px + q[s] + sa[s], di = P.Dinv[j];
        b1 = nanmax(b1, fabs(di * dr)); b2 = nanmax(b2, fabs(di * px)); b3 = nanmax(b3, fabs(di * sa[s]));
        b4 = nanmax(b4, fabs(dr)); b5 = nanmax(b5, fabs(px)); b6 = nanmax(b6, fabs(sa[s]));
        b7 = nanmax(b7, fabs(P.D[j] * dx[s])); b8 = nanmax(b8, fabs(dx[s])); b9 = nanmax(b9, fabs(q[s])); b10 = nanmax(b10, fabs(di * q[s]));
        t1 += x[s] * px; t2 += q[s] * x[s]; t3 += q[s] * dx[s];
      }
      R.dua_u = wmax(b1); R.px_u = wmax(b2); R.aty_u = wmax(b3); R.dua_s = wmax(b4); R.px_s = wmax(b5); R.aty_s = wmax(b6); R.dxn_u = wmax(b7); R.dxn_s = wmax(b8);
      R.qn_s = wmax(b9); R.qn_u = wmax(b10);
      R.xpx = wsum(t1); R.qx = wsum(t2); R.qdx = wsum(t3);
    };
    // the second stages of the infeasibility tests (term_rules.h batch_check calls them when a first stage passed: uniform over the wave)
    auto pinf_stage2 = [&](double &mu, double &ms) {                                     // A' dy   (is_primal_infeasible :815-818)
      double sa[2];
      stage_m(dy); mulT(sa);
#pragma unroll
      for (int s = 0; s < 2; s++) if (vn[s]) { mu = nanmax(mu, fabs(P.Dinv[s * 64 + L] * sa[s])); ms = nanmax(ms, fabs(sa[s])); }
      mu = wmax(mu); ms = wmax(ms);
    };
    auto pdx_stage2 = [&](double &mu, double &ms) {                                      // P dx    (is_dual_infeasible :846-853)
      double sp[2];
      stage_n(dx); mulP(sp);
#pragma unroll
      for (int s = 0; s < 2; s++) if (vn[s]) { const double v = sp[s] - P.sigma * dx[s]; mu = nanmax(mu, fabs(P.Dinv[s * 64 + L] * v)); ms = nanmax(ms, fabs(v)); }
      mu = wmax(mu); ms = wmax(ms);
    };
    auto adx_stage2 = [&](double thr) {                                                  // A dx    (:855-872; dx is staged)
      double adx[4], viol = 0;
      mulA(adx);
#pragma unroll
      for (int s = 0; s < 4; s++) if (vm[s]) {
        double a = adx[s];
        if (unsc) a *= P.Einv[rowm[s]];
        if (adx_violates(a, l[s], u[s], thr)) viol += 1.0;
      }
      viol = wsum(viol);
      return viol == 0.0;
    };
    int status = OSQP_UNSOLVED, iter = 0, rho_updates = 0;
    double obj = 0, prim_res = 0, dual_res = 0;
#ifdef OSQP_HIP_KTRACE
    unsigned long long tkT = 0, tkS = 0, tkA = 0, tkR = 0;
#endif
    WT_MARK(tk0);
    if (P.max_iter <= 0) residuals();
    while (true) {
      iter++;
      // ---- rhs = sigma x - q + A'(rho z - y);  x~ = K^-1 rhs   (_osqp.py:649-650, :307-311 in reduced form) ----
      double t[4], rhs[2], sA[2];
      WT_MARK(c0);
#pragma unroll
      for (int s = 0; s < 4; s++) t[s] = rho_of(s) * z[s] - y[s];
      stage_m(t);
      mulT(sA);
      WT_MARK(c1); WT_ADD(tkT, c1 - c0);
#pragma unroll
      for (int s = 0; s < 2; s++) rhs[s] = vn[s] ? P.sigma * x[s] - q[s] + sA[s] : 0.0;
      ksolve(rhs, dk0, dk1, xs);
      WT_MARK(c2); WT_ADD(tkS, c2 - c1);
      // ---- z~ = A x~; x, z, y update (_osqp.py:660-703) ----
      stage_n(xs);
      double zt[4];
      mulA(zt);
#pragma unroll
      for (int s = 0; s < 4; s++) {
        const StepRow r = step_row(P.alpha, zt[s], rho_of(s), z[s], y[s], l[s], u[s]);
        y[s] = r.y; dy[s] = r.dy; z[s] = r.z;
      }
#pragma unroll
      for (int s = 0; s < 2; s++) { const StepCol c = step_col(P.alpha, xs[s], x[s]); dx[s] = c.dx; x[s] = c.x; }
      WT_MARK(c3); WT_ADD(tkA, c3 - c2);
      const bool at_check = (P.check > 0 && iter % P.check == 0) || iter >= P.max_iter;
      const bool at_rho = P.rho_interval > 0 && iter % P.rho_interval == 0;
      if (!at_check && !at_rho) continue;
      WT_MARK(c4);
      residuals();
      WT_MARK(c5); WT_ADD(tkR, c5 - c4);
      term_info(tset, R, &obj, &prim_res, &dual_res);
      const int st = batch_check(tset, R, prim_res, dual_res, iter, P.max_iter, at_check, pinf_stage2, pdx_stage2, adx_stage2, &obj);
      if (st != kBatchGoOn) { status = st; break; }
      double rho_new;
      if (at_rho && batch_rho_rule(rho_bar, P.rho_tol, R, &rho_new)) { rho_bar = rho_new; set_rho(rho_bar); rho_updates++; }
    }
    const double rho_est = term_rho_estimate(rho_bar, R);
    // ---- store: x = D x, y = cinv E y (_osqp.py:1110-1112); certificates in place of x / y for infeasible problems ----
#pragma unroll
    for (int s = 0; s < 2; s++) if (vn[s]) { const int j = s * 64 + L; P.x[(size_t)b * n + j] = batch_out_x(status, P.unscaled, P.scaling, P.D[j], x[s], dx[s]); }
#pragma unroll
    for (int s = 0; s < 4; s++) if (vm[s]) {
      const int i = rowm[s];
      if (P.zs) P.zs[(size_t)b * m + i] = z[s];
      P.y[(size_t)b * m + i] = batch_out_y(status, P.unscaled, P.scaling, P.cinv, P.E[i], y[s], dy[s]);
    }
    if (L == 0) {
      double *rc = P.rec + (size_t)b * kBatchRec;
      batch_record(rc, status, iter, obj, prim_res, dual_res, rho_bar, rho_updates, 0.0, rho_est);
#ifdef OSQP_HIP_KTRACE
      rc[7] = (double)tkT; rc[8] = (double)tkS; rc[9] = (double)tkA; rc[11] = (double)tkR; rc[10] = (double)(wall_clock64() - tk0);      // 100 MHz ticks per phase (tools/batch_wave_probe.py)
#endif
      if (P.iters_out) P.iters_out[b] = iter;
    }
  }
}

}  // namespace

__global__ void k_batch_products(DevCsr A, int nprod, const int *a, const int *b, double *out) {
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < nprod; p += gridDim.x * blockDim.x) out[p] = A.val[a[p]] * A.val[b[p]];
}
// rank of problem b among all by descending iteration count (ties by index) = its place in the launch order
// (sixteen lanes -- one DPP row -- share a problem: each compares against every sixteenth count, the row's partial ranks are summed with DPP moves.
//  nbatch / 16 workgroups instead of nbatch / 256: with one thread per problem the 4096 x 4096 comparisons ran on 16 CUs and took 177 us per call,
//  3 % of a 4096-problem batch)
__global__ __launch_bounds__(256) void k_batch_order(int nbatch, const int *iters, int *order) {
  const int b = blockIdx.x * 16 + (threadIdx.x >> 4), jl = threadIdx.x & 15;
  const int mine = b < nbatch ? iters[b] : 0;
  int rank = 0;
  for (int j = jl; j < nbatch; j += 16) { const int v = iters[j]; rank += (v > mine) || (v == mine && j < b); }
  rank += __builtin_amdgcn_update_dpp(0, rank, 0xb1, 0xf, 0xf, false);       // lane ^ 1
  rank += __builtin_amdgcn_update_dpp(0, rank, 0x4e, 0xf, 0xf, false);       // lane ^ 2
  rank += __builtin_amdgcn_update_dpp(0, rank, 0x124, 0xf, 0xf, false);      // row_ror:4
  rank += __builtin_amdgcn_update_dpp(0, rank, 0x128, 0xf, 0xf, false);      // row_ror:8
  if (jl == 0 && b < nbatch) order[rank] = b;
}
void batch_order(Dev &d, int nbatch, const int *iters, int *order, void *stream) {
  if (hipSetDevice(d.device) != hipSuccess) throw DeviceError("osqp_hip: hipSetDevice failed");
  if (nbatch > 0) hipLaunchKernelGGL(k_batch_order, dim3((nbatch + 15) / 16), dim3(256), 0, static_cast<hipStream_t>(stream ? stream : d.stream), nbatch, iters, order);
}
void batch_products(Dev &d, int nprod, const int *a, const int *b, double *out) {
  if (hipSetDevice(d.device) != hipSuccess) throw DeviceError("osqp_hip: hipSetDevice failed");
  if (nprod > 0) hipLaunchKernelGGL(k_batch_products, dim3((nprod + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(d.stream), d.A, nprod, a, b, out);
}

// ---- per-problem matrices: assembly + equilibration of every problem's own (P_b, A_b), one workgroup per problem, everything in LDS.
// The same arithmetic, entry for entry, as the single-QP setup (backend_hip.hip k_asm_scatter, k_rowmax, k_ruiz_*: _osqp.py:389-497): an element of a
// per-element batch is scaled exactly as a solver set up with its matrices alone would scale it -- the reference's forward builds one solver per
// element (nn/torch.py:142-157).  Output: the scaled CSR values of A and B = [P + sigma I | A'], D, 1/D, E, 1/E, c and the banded variant's products.
__device__ __forceinline__ double batch_limit_scaling(double v) { return v < 1e-4 ? 1.0 : (v > 1e4 ? 1e4 : v); }     // _osqp.py:363-387
__global__ __launch_bounds__(256) void k_batch_prepare(BatchParams P, Dev d, const double *Px_b, const double *Ax_b, int iters) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int n = P.n, m = P.m, tid = threadIdx.x, b = blockIdx.x, nzA = P.A.nnz, nzB = P.B.nnz;
  if (b >= P.nbatch) return;
  double *Av = sm, *Bv = Av + ((nzA + 1) & ~1), *D = Bv + ((nzB + 1) & ~1), *E = D + n, *dt = E + m, *et = dt + n, *q = et + m, *np_ = q + n, *scr = np_ + n;
  Red<4> red{scr};
  const double *Ar = Ax_b ? Ax_b + (size_t)b * d.nzA : d.Araw, *Pr = Px_b ? Px_b + (size_t)b * d.nzP : d.Praw;
  for (int k = tid; k < nzB; k += 256) Bv[k] = 0.0;
  __syncthreads();
  for (int k = tid; k < d.nzA; k += 256) { const double v = Ar[k]; Av[d.AmA[k]] = v; Bv[d.AmB[k]] = v; }
  for (int k = tid; k < d.nzP; k += 256) {
    const int i = d.Pi[k], j = d.Pj[k]; const double v = Pr[k];
    if (i == j) atomicAdd(&Bv[d.Pm1[k]], v);            // (repeated (j, j) entries of a valid CSC sum up)
    else { Bv[d.Pm1[k]] = v; Bv[d.Pm2[k]] = v; }
  }
  for (int j = tid; j < n; j += 256) { D[j] = 1.0; q[j] = P.q ? P.q[(size_t)b * n + j] : P.q0[j]; }
  for (int i = tid; i < m; i += 256) E[i] = 1.0;
  double c = 1.0;
  __syncthreads();
  const int *Arp = P.A.rowptr, *Ac = P.A.col, *Brp = P.B.rowptr, *Bc = P.B.col;
  for (int it = 0; it < iters; it++) {
    for (int j = tid; j < n; j += 256) { double mx = 0.0; for (int k = Brp[j]; k < Brp[j + 1]; k++) mx = fmax(mx, fabs(Bv[k])); dt[j] = 1.0 / sqrt(batch_limit_scaling(mx)); }      // KKT column j = row j of [P | A']
    for (int i = tid; i < m; i += 256) { double mx = 0.0; for (int k = Arp[i]; k < Arp[i + 1]; k++) mx = fmax(mx, fabs(Av[k])); et[i] = 1.0 / sqrt(batch_limit_scaling(mx)); }
    __syncthreads();
    for (int i = tid; i < m; i += 256) { const double ei = et[i]; for (int k = Arp[i]; k < Arp[i + 1]; k++) Av[k] *= ei * dt[Ac[k]]; E[i] *= ei; }
    for (int j = tid; j < n; j += 256) {
      const double dj = dt[j];
      for (int k = Brp[j]; k < Brp[j + 1]; k++) { const int cc = Bc[k]; Bv[k] *= cc < n ? dt[cc] * dj : et[cc - n] * dj; }
      q[j] *= dj; D[j] *= dj;
    }
    __syncthreads();
    double sum = 0.0, nq = 0.0;
    for (int j = tid; j < n; j += 256) { double mx = 0.0; for (int k = Brp[j]; k < Brp[j + 1] && Bc[k] < n; k++) mx = fmax(mx, fabs(Bv[k])); sum += mx; nq = fmax(nq, fabs(q[j])); }
    red.sum_max(sum, nq);
    const double mean = sum / (double)(n > 0 ? n : 1);
    const double ct = 1.0 / batch_limit_scaling(fmax(batch_limit_scaling(nq), mean));
    c *= ct;
    for (int j = tid; j < n; j += 256) { for (int k = Brp[j]; k < Brp[j + 1] && Bc[k] < n; k++) Bv[k] *= ct; q[j] *= ct; }
    __syncthreads();
  }
  for (int j = tid; j < n; j += 256) { Bv[d.Bdiag[j]] += P.sigma; P.D_b[(size_t)b * n + j] = D[j]; P.Dinv_b[(size_t)b * n + j] = 1.0 / D[j]; }
  for (int i = tid; i < m; i += 256) { P.E_b[(size_t)b * m + i] = E[i]; P.Einv_b[(size_t)b * m + i] = 1.0 / E[i]; }
  if (tid == 0) P.c_b[b] = c;
  __syncthreads();
  for (int k = tid; k < nzA; k += 256) P.Aval_b[(size_t)b * nzA + k] = Av[k];
  for (int k = tid; k < nzB; k += 256) P.Bval_b[(size_t)b * nzB + k] = Bv[k];
  if (P.kp_val_b) for (int k = tid; k < P.nprod; k += 256) P.kp_val_b[(size_t)b * P.nprod + k] = Av[P.kp_a[k]] * Av[P.kp_b[k]];
}
int batch_prepare(Dev &d, const BatchParams &p, const double *Px_b, const double *Ax_b, int scaling_iters, void *stream) {
  if (hipSetDevice(d.device) != hipSuccess) return OSQP_ALGEBRA_LOAD_ERROR;
  const size_t lds = sizeof(double) * ((size_t)((p.A.nnz + 1) & ~1) + ((p.B.nnz + 1) & ~1) + 4 * (size_t)p.n + 2 * (size_t)p.m + 16);
  if (lds > 144 * 1024) return OSQP_FUNC_NOT_IMPLEMENTED;
  if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void *>(&k_batch_prepare), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) { (void)hipGetLastError(); return OSQP_FUNC_NOT_IMPLEMENTED; }
  hipLaunchKernelGGL(k_batch_prepare, dim3(p.nbatch), dim3(256), lds, static_cast<hipStream_t>(stream ? stream : d.stream), p, d, Px_b, Ax_b, scaling_iters);
  return OSQP_NO_ERROR;
}

// ---------------------------------------------------------------------------------------------------------------- adjoint derivatives
// Backward pass of a batch of solved QPs: given (x, y) of  min 1/2 x'Px + q'x, l <= Ax <= u  and incoming gradients dx = dL/dx, dy = dL/dy, the
// gradients of L with respect to q, l, u and the stored entries of P and A.  ONE WORKGROUP PER PROBLEM, everything in LDS, in the caller's UNSCALED
// units (the raw matrix values are assembled into the CSR layouts of A and B = [P | A'] exactly as k_batch_prepare does, without equilibration).
//   1. z = A x; active rows by polish's rule (k_batch_admm: low = z - l < -y, upp = u - z < y; an equality row is always active).
//   2. [P, A_a'; A_a, 0] [r_x; r_a] = -[dx; dy_a]  through the regularised system of polish: ONE banded factorisation of
//      S = P + delta I + A_a' A_a / delta  (the forward's permutation, band slots and product lists), then the first solve and `refine` refinement
//      steps against the UNREGULARISED residual, each of the form
//          t = r_a + (A_a r_x - g_a) / delta,   rhs = g_x - P r_x - A_a' t,   s = S^-1 rhs,   r_x += s,   r_a = t + A_a s / delta
//      with the constraint residual accumulated in double-double (it is amplified by 1 / delta, as in polish).
//   3. dq = r_x;  dl / du = -r_a on lower- / upper-active rows;  dP_ij = (r_i x_j + r_j x_i) / 2 and dA_ij = y_i r_x,j + r_y,i x_j on the stored
//      entries, in the caller's CSC order: one writer per entry, no atomics.
// Record per problem (kAdjointRec doubles): status, active rows, final relative residual max |g - K r| / max |g|, reserved.
//   status 0: residual < kAdjointTol;  1: a pivot of S was not positive (replaced by its magnitude or 1: the problem is not convex or the inputs are
//   not finite);  2: more active rows than variables (K is singular whatever the values);  3: the refinement stalled above kAdjointTol (a dependent
//   active set).  The outputs of such an element are the regularised solution.
namespace {
__global__ __launch_bounds__(256) void k_batch_adjoint(AdjointParams P) {
  constexpr int kBB = 256;
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int n = P.n, m = P.m, tid = threadIdx.x, b = blockIdx.x, nzA = P.A.nnz, nzB = P.B.nnz;
  if (b >= P.nbatch) return;
  double *Av = sm, *Bv = Av + ((nzA + 1) & ~1), *x = Bv + ((nzB + 1) & ~1), *rx = x + n, *gx = rx + n, *rhs = gx + n, *sol = rhs + n, *wbuf = sol + n, *dinv = wbuf + n;
  double *y = dinv + n, *w = y + m, *ra = w + m, *ga = ra + m, *t = ga + m, *sd = t + m;
  Red<kBB / 64> red{sd + m};
  const int bw = P.bw;
  double *Lb = sd + m + 16 + kBandFront;
  const int *Arp = P.A.rowptr, *Ac = P.A.col, *Brp = P.B.rowptr, *Bc = P.B.col;
  // ---- the problem's own unscaled matrices in the CSR layouts ----
  const double *Ar = P.Ax_b ? P.Ax_b + (size_t)b * P.nzA : P.Araw, *Pr = P.Px_b ? P.Px_b + (size_t)b * P.nzP : P.Praw;
  for (int k = tid; k < nzB; k += kBB) Bv[k] = 0.0;
  __syncthreads();
  for (int k = tid; k < P.nzA; k += kBB) { const double v = Ar[k]; Av[P.AmA[k]] = v; Bv[P.AmB[k]] = v; }
  for (int k = tid; k < P.nzP; k += kBB) {
    const int i = P.Pi[k], j = P.Pj[k]; const double v = Pr[k];
    if (i == j) atomicAdd(&Bv[P.Pm1[k]], v);            // (repeated (j, j) entries of a valid CSC sum up)
    else { Bv[P.Pm1[k]] = v; Bv[P.Pm2[k]] = v; }
  }
  double gmax_l = 0.0;
  for (int j = tid; j < n; j += kBB) { x[j] = P.x[(size_t)b * n + j]; const double g = -P.dx[(size_t)b * n + j]; gx[j] = g; rx[j] = 0.0; gmax_l = nanmax(gmax_l, fabs(g)); }
  for (int i = tid; i < m; i += kBB) y[i] = P.y[(size_t)b * m + i];
  __syncthreads();
  // ---- z = A x, the active set, the right-hand side of the active rows ----
  const double idel = 1.0 / P.delta;
  double nact_l = 0.0;
  for (int i = tid; i < m; i += kBB) {
    double z = 0.0;
    for (int k = Arp[i]; k < Arp[i + 1]; k++) z += Av[k] * x[Ac[k]];
    const double li = clamp_lower(P.l ? P.l[(size_t)b * m + i] : P.l0[i]), ui = clamp_upper(P.u ? P.u[(size_t)b * m + i] : P.u0[i]), yi = y[i];
    const RowActive ra_ = adjoint_active(z, li, ui, yi);
    const bool low = ra_.low, upp = ra_.upp, act = low || upp;
    const double g = act ? -(P.dy ? P.dy[(size_t)b * m + i] : 0.0) : 0.0;
    w[i] = act ? idel : 0.0; sd[i] = low ? -1.0 : (upp ? 1.0 : 0.0); ga[i] = g; ra[i] = 0.0;
    nact_l += act ? 1.0 : 0.0; gmax_l = nanmax(gmax_l, fabs(g));
  }
  __syncthreads();
  const double nact = red.sum(nact_l), gmax = red.max(gmax_l);
  // ---- S = P + delta I + A_a' A_a / delta in the band (lower, permuted: the forward's slots and product lists) and its factor (band_ldl.h) ----
  band_clear<kBB>(Lb, n, bw);
  for (int k = tid; k < nzB; k += kBB) { const int s_ = P.bp_slot[k]; if (s_ >= 0) Lb[s_] = Bv[k]; }
  __syncthreads();
  for (int c = tid; c < n; c += kBB) Lb[band_slot(bw, c, c)] += P.delta;
  __syncthreads();
  for (int e = tid; e < P.nents; e += kBB) {
    double acc = 0.0;
    for (int q_ = P.ke_ptr[e]; q_ < P.ke_ptr[e + 1]; q_++) acc += w[P.kp_row[q_]] * (Av[P.kp_a[q_]] * Av[P.kp_b[q_]]);
    Lb[P.ke_slot[e]] += acc;
  }
  __syncthreads();
  const bool bad = band_factor<kBB, true>(Lb, n, bw, dinv, P.tri, P.ntri, P.delta);
  auto ksolve = [&](const double *in, double *out) { band_solve<kBB>(Lb, n, bw, dinv, P.perm, wbuf, in, out, [](int) {}); };
  // ---- first solve + refinement steps ----
  for (int it = 0; it <= P.refine; it++) {
    for (int i = tid; i < m; i += kBB) {
      double tv = 0.0;
      if (w[i] != 0.0) {
        double hi = -ga[i], lo = 0.0;                                       // (A r_x)_i - g_a,i
        for (int e = Arp[i]; e < Arp[i + 1]; e++) dd_acc(Av[e], rx[Ac[e]], hi, lo);
        tv = ra[i] + (hi + lo) * idel;
      }
      t[i] = tv;
    }
    __syncthreads();
    for (int j = tid; j < n; j += kBB) {
      double a = 0.0;
      for (int k = Brp[j]; k < Brp[j + 1]; k++) { const int c = Bc[k]; a += Bv[k] * (c < n ? rx[c] : t[c - n]); }
      rhs[j] = gx[j] - a;
    }
    __syncthreads();
    ksolve(rhs, sol);
    for (int j = tid; j < n; j += kBB) rx[j] += sol[j];
    for (int i = tid; i < m; i += kBB) {
      if (w[i] != 0.0) {
        double a = 0.0;
        for (int e = Arp[i]; e < Arp[i + 1]; e++) a += Av[e] * sol[Ac[e]];
        ra[i] = t[i] + a * idel;
      }
    }
    __syncthreads();
  }
  // ---- residual of the unregularised system ----
  double rmax_l = 0.0;
  for (int j = tid; j < n; j += kBB) {
    double a = 0.0;
    for (int k = Brp[j]; k < Brp[j + 1]; k++) { const int c = Bc[k]; a += Bv[k] * (c < n ? rx[c] : ra[c - n]); }
    rmax_l = nanmax(rmax_l, fabs(gx[j] - a));
  }
  for (int i = tid; i < m; i += kBB) {
    if (w[i] != 0.0) {
      double a = 0.0;
      for (int e = Arp[i]; e < Arp[i + 1]; e++) a += Av[e] * rx[Ac[e]];
      rmax_l = nanmax(rmax_l, fabs(ga[i] - a));
    }
  }
  const double rmax = red.max(rmax_l);
  const double resid = gmax > 0.0 ? rmax / gmax : rmax;
  // ---- gradients ----
  if (P.dq) for (int j = tid; j < n; j += kBB) P.dq[(size_t)b * n + j] = rx[j];
  for (int i = tid; i < m; i += kBB) {
    const double v = -ra[i], s_ = sd[i];
    if (P.dl) P.dl[(size_t)b * m + i] = s_ < 0.0 ? v : 0.0;
    if (P.du) P.du[(size_t)b * m + i] = s_ > 0.0 ? v : 0.0;
  }
  if (P.dP) for (int k = tid; k < P.nzP; k += kBB) {
    const int i = P.Pi[k], j = P.Pj[k];
    P.dP[(size_t)b * P.nzP + k] = i == j ? rx[i] * x[i] : 0.5 * (rx[i] * x[j] + rx[j] * x[i]);
  }
  if (P.dA) for (int k = tid; k < P.nzA; k += kBB) {
    const int i = P.Ai[k], j = P.Aj[k];
    P.dA[(size_t)b * P.nzA + k] = y[i] * rx[j] + ra[i] * x[j];
  }
  if (tid == 0 && P.arec) {
    double *rc = P.arec + (size_t)b * kAdjointRec;
    rc[0] = bad ? 1.0 : (nact > (double)n ? 2.0 : (resid < kAdjointTol ? 0.0 : 3.0)); rc[1] = nact; rc[2] = resid; rc[3] = 0.0;
  }
}

}  // namespace

int batch_adjoint(Dev &d, const AdjointParams &p, void *stream) {
  if (hipSetDevice(d.device) != hipSuccess) return OSQP_ALGEBRA_LOAD_ERROR;
  const size_t lds = batch_adjoint_lds_bytes(p.n, p.m, p.A.nnz, p.B.nnz, p.bw);
  if (!lds || !p.perm) return OSQP_FUNC_NOT_IMPLEMENTED;
  if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void *>(&k_batch_adjoint), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) { (void)hipGetLastError(); return OSQP_FUNC_NOT_IMPLEMENTED; }
  hipStream_t st = static_cast<hipStream_t>(stream ? stream : d.stream);
  hipLaunchKernelGGL(k_batch_adjoint, dim3(p.nbatch), dim3(256), lds, st, p);
  const hipError_t e = stream ? hipGetLastError() : hipStreamSynchronize(st);
  if (e != hipSuccess) throw DeviceError(std::string("osqp_hip: adjoint kernel failed: ") + hipGetErrorString(e));
  return OSQP_NO_ERROR;
}

void batch_release(Dev &d) {
  if (d.bside) { (void)hipStreamDestroy(static_cast<hipStream_t>(d.bside)); d.bside = nullptr; }
  if (d.bev0) { (void)hipEventDestroy(static_cast<hipEvent_t>(d.bev0)); d.bev0 = nullptr; }
  if (d.bev1) { (void)hipEventDestroy(static_cast<hipEvent_t>(d.bev1)); d.bev1 = nullptr; }
}
namespace {
// run-time value -> compile-time constant: f(std::integral_constant<int, V>()) for the V of Vs equal to v (plan_batch picks v from the same list)
template <int... Vs, class F>
void with_const(int v, F &&f) { (void)((v == Vs && (f(std::integral_constant<int, Vs>()), true)) || ...); }
template <class F>
void with_bool(bool b, F &&f) { if (b) f(std::true_type()); else f(std::false_type()); }
using BatchKernel = void (*)(BatchParams);
bool reserve_lds(BatchKernel k, size_t lds) { return hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess; }
}  // namespace

// Carries out plan_batch(p): the spectral stage, if planned, then the follow-up.  A stage whose LDS the device refuses falls back: the wave form to the
// spectral workgroup form (its split positions to the wave kernel), the spectral workgroup form to the follow-up alone.  d.batch_wave_ran reports
// what was launched.
int batch_solve(Dev &d, const BatchParams &p, void *stream) {
  d.batch_wave_ran = -1;
  if (hipSetDevice(d.device) != hipSuccess) return OSQP_ALGEBRA_LOAD_ERROR;
  hipStream_t st = static_cast<hipStream_t>(stream ? stream : d.stream);
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, d.device);
  const BatchPlan pl = plan_batch(p, cus);
  const bool gap = p.check_dualgap != 0;                  // (settings.check_dualgap: the GAP instantiation of whichever variant is launched)
  bool spectral = false;
  // spectral workgroup kernel on the first q.nbatch positions of the launch order, on stream s; false: the device refused the LDS reservation
  auto spec_launch = [&](const BatchParams &q, int w, hipStream_t s) {
    bool ok = false;
    with_const<2, 4, 6, 8>(pl.spec_e, [&](auto E) {
      with_const<1, 2>(w, [&](auto W) { with_bool(gap, [&](auto GAP) {
        const BatchKernel k = &k_batch_admm<256, decltype(E)::value, decltype(E)::value, true, false, false, true, decltype(W)::value, decltype(GAP)::value>;
        ok = reserve_lds(k, pl.lds_spec);
        if (ok) hipLaunchKernelGGL(k, dim3(q.nbatch), dim3(256), pl.lds_spec, s, q); else (void)hipGetLastError();
      }); });
    });
    return ok;
  };
  if (pl.spec == BatchPlan::kSpecWave) {
    with_const<64, 120, 128>(pl.n8, [&](auto N8) {
      const BatchKernel k = &k_batch_wave<decltype(N8)::value>;
      if (!reserve_lds(k, pl.lds_w)) { (void)hipGetLastError(); return; }
      BatchParams pw = p;
      hipStream_t side = nullptr; hipEvent_t ev0 = nullptr, ev1 = nullptr;
      if (pl.split) {
        if (!d.bside) {
          hipStream_t s2; hipEvent_t a, b;
          if (hipStreamCreateWithFlags(&s2, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&a, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&b, hipEventDisableTiming) != hipSuccess)
            throw DeviceError("osqp_hip: cannot create the batch path's second stream");
          d.bside = s2; d.bev0 = a; d.bev1 = b;
        }
        side = static_cast<hipStream_t>(d.bside); ev0 = static_cast<hipEvent_t>(d.bev0); ev1 = static_cast<hipEvent_t>(d.bev1);
        BatchParams ph = p; ph.nbatch = pl.split; ph.wv_on = 0;
        if (hipEventRecord(ev0, st) != hipSuccess || hipStreamWaitEvent(side, ev0, 0) != hipSuccess) throw DeviceError("osqp_hip: batch stream fork failed");
        if (spec_launch(ph, pl.split_w, side)) pw.wv_first = pl.split;               // (refused: the wave kernel takes them as well)
        if (hipEventRecord(ev1, side) != hipSuccess) throw DeviceError("osqp_hip: batch stream join failed");
      }
      if (hipMemsetAsync(p.wv_queue, 0, sizeof(int), st) != hipSuccess) throw DeviceError("osqp_hip: batch queue reset failed");
      hipLaunchKernelGGL(k, dim3(pw.wv_first ? pl.wgs : pl.wgs_all), dim3(64 * kBatchWaveW), pl.lds_w, st, pw);
      if (pl.split && hipStreamWaitEvent(st, ev1, 0) != hipSuccess) throw DeviceError("osqp_hip: batch stream join failed");
      d.batch_wave_ran = pw.wv_first; spectral = true;
    });
  }
  if (pl.spec != BatchPlan::kNoSpec && !spectral) spectral = spec_launch(p, pl.spec_w, st);
  BatchParams pm = p;
  if (spectral) pm.only_marked = 1;
  auto launch = [&](BatchKernel k) {
    if (pl.direct && !reserve_lds(k, pl.lds)) throw DeviceError("osqp_hip: cannot reserve LDS for the direct batch kernel");
    hipLaunchKernelGGL(k, dim3(p.nbatch), dim3(pl.tb), pl.lds, st, pm);
  };
  with_bool(gap, [&](auto GAPT) {
    constexpr bool GAP = decltype(GAPT)::value;
    switch (pl.variant) {
      case 2:
        with_const<2, 4, 6, 8, 16>(pl.e, [&](auto E) { with_bool(pl.pol, [&](auto POL) { with_bool(pl.small, [&](auto SMALL) {
          launch(&k_batch_admm<256, decltype(E)::value, decltype(E)::value, true, decltype(POL)::value, decltype(SMALL)::value, false, 1, GAP>); }); }); });
        break;
      case 1:
        with_const<8, 16, 24>(pl.e, [&](auto E) { with_bool(pl.pol, [&](auto POL) { launch(&k_batch_admm<64, decltype(E)::value, decltype(E)::value, true, decltype(POL)::value, false, false, 1, GAP>); }); });
        break;
      case 3: with_const<8, 16, 24>(pl.e, [&](auto E) { launch(&k_batch_admm<64, decltype(E)::value, decltype(E)::value, false, false, false, false, 1, GAP>); }); break;
      case 4: with_const<2, 4, 8>(pl.e, [&](auto E) { launch(&k_batch_admm<256, decltype(E)::value, decltype(E)::value, false, false, false, false, 1, GAP>); }); break;
      case 5: launch(&k_batch_admm<256, 0, 0, false, false, false, false, 1, GAP>); break;
      default: break;
    }
  });
  if (pl.variant < 1 || pl.variant > 5) return OSQP_FUNC_NOT_IMPLEMENTED;
  hipError_t e = stream ? hipGetLastError() : hipStreamSynchronize(st);
  if (e != hipSuccess) throw DeviceError(std::string("osqp_hip: batch kernel failed: ") + hipGetErrorString(e));
  return OSQP_NO_ERROR;
}

// ---- diagnostic entry (backend.h test_band, include/osqp_hip.h osqp_hip_test_band): band_ldl.h's functions, unchanged, on a test's matrix ----
// One workgroup.  LDS: the band, then wbuf and dinv (band_cols(n) doubles each); right-hand sides and results stay in global memory.  The host has
// validated every field (Engine::test_band).
namespace {
template <int kBB, bool GUARD>
__global__ __launch_bounds__(kBB) void k_test_band(BandProbe P) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int n = P.n, bw = P.bw, tid = threadIdx.x, nimg = (int)band_doubles(n, bw), nband = n * (bw + 1);
  double *Lb = sm + kBandFront, *wbuf = sm + nimg, *dinv = wbuf + band_cols(n);
  band_clear<kBB>(Lb, n, bw);
  for (int s_ = tid; s_ < nband; s_ += kBB) {
    const int c = s_ / (bw + 1), k = s_ - c * (bw + 1);
    if (c + k < n) Lb[band_slot(bw, c, c + k)] = P.band[s_];
  }
  __syncthreads();
  const bool bad = band_factor<kBB, GUARD>(Lb, n, bw, dinv, P.tri, P.ntri, P.pivot_floor);
  for (int r = 0; r < P.nrhs; r++) band_solve<kBB>(Lb, n, bw, dinv, P.perm, wbuf, P.rhs + (size_t)r * n, P.x + (size_t)r * n, [](int) {});
  for (int s_ = tid; s_ < nimg; s_ += kBB) P.image[s_] = sm[s_];
  for (int c = tid; c < n; c += kBB) P.dinv[c] = dinv[c];
  if (tid == 0) *P.bad = bad ? 1 : 0;
}
}  // namespace

int test_band(Dev &d, const BandProbe &p) {
  if (hipSetDevice(d.device) != hipSuccess) return OSQP_ALGEBRA_LOAD_ERROR;
  const size_t lds = test_band_lds_bytes(p.n, p.bw);
  if (!lds) return OSQP_DATA_VALIDATION_ERROR;
  using Kernel = void (*)(BandProbe);
  const Kernel k = p.threads == 64 ? &k_test_band<64, false> : (p.guard ? &k_test_band<256, true> : &k_test_band<256, false>);
  if (lds > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) { (void)hipGetLastError(); return OSQP_FUNC_NOT_IMPLEMENTED; }
  hipStream_t st = static_cast<hipStream_t>(d.stream);
  hipLaunchKernelGGL(k, dim3(1), dim3(p.threads), lds, st, p);
  hipError_t e = hipGetLastError();                    // (a refused launch) ...
  if (e == hipSuccess) e = hipStreamSynchronize(st);   // ... or the kernel's own
  if (e != hipSuccess) throw DeviceError(std::string("osqp_hip: band probe kernel failed: ") + hipGetErrorString(e));
  return OSQP_NO_ERROR;
}

}  // namespace be
}  // namespace osqp_hip
