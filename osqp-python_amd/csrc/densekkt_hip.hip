// densekkt_hip.hip -- the DENSE KKT mode (backend.h DevDk; include/osqp_hip.h osqp_hip_dense_kkt).
//
// A single QP with n between a few hundred and a few thousand is too large for one workgroup (Engine::solve_small_direct) and too small for the PCG
// path to be anything but a string of launch latencies: k + 2 launches per ADMM iteration on banded matrices, 2 k + 4 on unstructured ones, each
// about as long as an empty launch, and the inner solves inexact.  Here the reduced KKT matrix of an ADMM iteration
//     K = P + sigma I + A' diag(rho) A          (_osqp.py:291-301 is the KKT matrix it is the Schur complement of)
// is held as its dense INVERSE (n x n fp64, full storage: 33.5 MB at n = 2 048 -- it stays in the Infinity Cache from one iteration to the next), and
// the linear solve of the iteration (:649-658 in reduced form) is one dense matrix-vector product:
//     kb_rhs      r_0 = sigma x - q + A' v - K x_g                 (the PCG's start residual at the extrapolated x_g, pcg_hip.hip)
//     dk_apply    u = K^-1 r_0,   x~ = x_g + u                     (k_dk_apply below: the hot path)
//     ka          z~ = A x~, the z / y / x update                  (:660-703)
// Factorisation (dk_factor; wherever rho or the matrices change: be::precond), all on the device by the engine's own dense kernels (dense_hip.hip):
//     W[i][j] = sqrt(rho_i) A_ij   (m x n, from the scaled CSR of A; a stored (i, j) that repeats adds up)
//     K = W' W                     (dense_gemm_sym: one triangle on the fp64 matrix cores, mirrored)
//     K += P + sigma I             (the columns below n of B = [P + sigma I | A']: both triangles are stored there)
//     K <- K^-1                    (dense_spd_inverse: block Gauss-Jordan without pivoting, in place)
//     probe                        max |K^-1 (K v) - v| <= kDkProbeTol max |v|,  K v = B [v; rho .* (A v)] by the handle's own sparse products
// Every launch of it has a fixed grid and a fixed summation order, and no atomic touches a double: the same data give the same bits.
#include "hip_common.h"

namespace osqp_hip {
namespace be {

namespace {

// W[i][:] += sqrt(rho_i) A[i][:]  on a zeroed W: one thread per row, its entries in stored order (a repeated (i, j) adds: tests/test_csc_duplicates.py)
__global__ __launch_bounds__(kBlock) void k_dk_fillW(Dev d) {
  const size_t n = (size_t)d.n;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < d.m; i += gridDim.x * kBlock) {
    const double sr = sqrt(d.rho[i]);
    double *row = d.dk.W + (size_t)i * n;
    for (int k = d.A.rowptr[i]; k < d.A.rowptr[i + 1]; k++) row[d.A.col[k]] += sr * d.A.val[k];
  }
}
// K[j][:] += (P + sigma I)[j][:]: one thread per row of B (ONE writer per dense entry), the terms of an entry in stored order; B holds both triangles of P
__global__ __launch_bounds__(kBlock) void k_dk_addP(Dev d) {
  const int n = d.n;
  for (int j = blockIdx.x * kBlock + threadIdx.x; j < n; j += gridDim.x * kBlock) {
    double *row = d.dk.Kinv + (size_t)j * n;
    for (int k = d.B.rowptr[j]; k < d.B.rowptr[j + 1]; k++) { const int c = d.B.col[k]; if (c < n) row[c] += d.B.val[k]; }
  }
}
// the probe's vectors (the recipe of woodbury_hip.hip's probe): v, rho .* (A v), comparison of K^-1 K v with v
__global__ __launch_bounds__(kBlock) void k_dk_probe_init(Dev d) {
  for (int j = blockIdx.x * kBlock + threadIdx.x; j < d.n; j += gridDim.x * kBlock) {
    const double v = 0.5 + (double)((((unsigned)j * 2654435761u) >> 8) & 0xffffu) / 65536.0;
    d.dk.pv[j] = v; d.dk.pv[(size_t)d.n + d.m + j] = v;
  }
}
__global__ __launch_bounds__(kBlock) void k_dk_probe_rho(Dev d) {
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < d.m; i += gridDim.x * kBlock) d.dk.pv[(size_t)d.n + i] *= d.rho[i];
}
__global__ __launch_bounds__(kBlock) void k_dk_maxdiff(const double *a, const double *b, int cnt, double *out) {      // one workgroup: out[0] = max |a - b|, out[1] = max |b|
  __shared__ double red[2 * kWaves];
  double e = 0.0, s = 0.0;
  for (int j = threadIdx.x; j < cnt; j += kBlock) { e = nanmax(e, fabs(a[j] - b[j])); s = nanmax(s, fabs(b[j])); }
  block_max2(e, s, red);
  if (threadIdx.x == 0) { out[0] = e; out[1] = s; }
}

// THE HOT PATH.  u = K^-1 r_0, x~ = x_g + u: one workgroup per TWO rows of K^-1 against one read of r_0 (half the requests for r_0, and two independent
// chains of fused multiply-adds per lane).  V2 (n even, r_0 16-byte aligned: both rows then start on a 16-byte boundary): 16-byte loads, four row
// pairs of them in flight per lane before the first is consumed; otherwise (odd n: every second row starts on an odd double) the same with 8-byte loads.
// Plain -- temporal -- loads: K^-1 is the one operand the Infinity Cache can keep from one ADMM iteration to the next (k_wbd_gemv of woodbury_hip.hip
// measured non-temporal loads slower for exactly this operand).  The lanes' partial sums are folded in a fixed order (DPP wave sums, the four
// waves in index order): the same r_0 gives the same bits.  direct != 0: also x~ and the PCG's flags -- written by workgroup 0 at its END and not read by
// this launch (a workgroup that starts late must not take the flag for the previous solve's).
template <bool V2>
__global__ __launch_bounds__(kBlock) void k_dk_apply(Dev d, int direct) {
  __shared__ double red[2 * kWaves];
  const int n = d.n, a0 = blockIdx.x * 2;
  if (a0 >= n) return;
  const bool two = a0 + 1 < n;
  const double *__restrict__ r = d.r;
  const double *__restrict__ r0 = d.dk.Kinv + (size_t)a0 * n;
  const double *__restrict__ r1 = d.dk.Kinv + (size_t)(two ? a0 + 1 : a0) * n;      // (the last row of an odd n: read twice, stored once)
  double s0 = 0.0, s1 = 0.0;
  if (V2) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    int k = threadIdx.x * 2;
    for (; k + 3 * 2 * kBlock < n; k += 4 * 2 * kBlock) {
      d2 u[4], p[4], q[4];
#pragma unroll
      for (int t = 0; t < 4; t++) { u[t] = *reinterpret_cast<const d2 *>(r + k + t * 2 * kBlock); p[t] = *reinterpret_cast<const d2 *>(r0 + k + t * 2 * kBlock); q[t] = *reinterpret_cast<const d2 *>(r1 + k + t * 2 * kBlock); }
#pragma unroll
      for (int t = 0; t < 4; t++) { s0 = fma(p[t].x, u[t].x, s0); s0 = fma(p[t].y, u[t].y, s0); s1 = fma(q[t].x, u[t].x, s1); s1 = fma(q[t].y, u[t].y, s1); }
    }
    for (; k < n; k += 2 * kBlock) {
      const d2 u = *reinterpret_cast<const d2 *>(r + k), p = *reinterpret_cast<const d2 *>(r0 + k), q = *reinterpret_cast<const d2 *>(r1 + k);
      s0 = fma(p.x, u.x, s0); s0 = fma(p.y, u.y, s0); s1 = fma(q.x, u.x, s1); s1 = fma(q.y, u.y, s1);
    }
  } else {
    int k = threadIdx.x;
    for (; k + 3 * kBlock < n; k += 4 * kBlock) {
      double u[4], p[4], q[4];
#pragma unroll
      for (int t = 0; t < 4; t++) { u[t] = r[k + t * kBlock]; p[t] = r0[k + t * kBlock]; q[t] = r1[k + t * kBlock]; }
#pragma unroll
      for (int t = 0; t < 4; t++) { s0 = fma(p[t], u[t], s0); s1 = fma(q[t], u[t], s1); }
    }
    for (; k < n; k += kBlock) { const double u = r[k]; s0 = fma(r0[k], u, s0); s1 = fma(r1[k], u, s1); }
  }
  block_sum2(s0, s1, red);
  if (threadIdx.x == 0) { d.uu[a0] = s0; if (direct) d.xs[a0] = d.xg[a0] + s0; }
  if (threadIdx.x == 64 && two) { d.uu[a0 + 1] = s1; if (direct) d.xs[a0 + 1] = d.xg[a0 + 1] + s1; }
  if (direct && blockIdx.x == 0 && threadIdx.x == 0) { d.flags[F_DONE] = 1; d.flags[F_ITERS] = 0; }
}

void launch_apply(Dev &d, int direct) {
  const dim3 grid((d.n + 1) / 2), block(kBlock);
  const bool v2 = (d.n & 1) == 0 && (reinterpret_cast<uintptr_t>(d.r) & 15) == 0 && (reinterpret_cast<uintptr_t>(d.dk.Kinv) & 15) == 0;
  if (v2) hipLaunchKernelGGL(k_dk_apply<true>, grid, block, 0, st(d), d, direct);
  else hipLaunchKernelGGL(k_dk_apply<false>, grid, block, 0, st(d), d, direct);
}

// max |K^-1 (K v) - v| and max |v| into pv's tail, with the CURRENT matrices, rho vector and inverse.  Overwrites d.r and d.uu.
void enqueue_probe(Dev &d) {
  DevDk &k = d.dk;
  double *out = k.pv + (size_t)d.n + d.m + d.n;
  LAUNCH(k_dk_probe_init, d, d);
  LAUNCH(k_test_spmv, d, d.A, k.pv, k.pv + d.n);
  LAUNCH(k_dk_probe_rho, d, d);
  LAUNCH(k_test_spmv, d, d.B, k.pv, d.r);
  launch_apply(d, 0);
  hipLaunchKernelGGL(k_dk_maxdiff, dim3(1), dim3(kBlock), 0, st(d), d.uu, k.pv + (size_t)d.n + d.m, d.n, out);
}
double fetch_probe(Dev &d) {
  double chk[2] = {1.0, 0.0};
  HIP_CHECK(hipMemcpyAsync(chk, d.dk.pv + (size_t)d.n + d.m + d.n, sizeof(chk), hipMemcpyDeviceToHost, st(d)));
  HIP_CHECK(hipStreamSynchronize(st(d)));
  return chk[1] > 0.0 ? chk[0] / chk[1] : (chk[0] == 0.0 ? 0.0 : INFINITY);      // (NaN stays NaN: refused)
}

}  // namespace

int dk_enable(Dev &d) {
  HIP_CHECK(hipSetDevice(d.device));
  (void)gj_aux(d);                                          // (the lookahead stream of the inverse: the handle's own, created here rather than inside a factorisation)
  DevDk k;
  const size_t n = (size_t)d.n, m = (size_t)d.m;
  const size_t cnt[4] = {n * n, m * n, dense_spd_inverse_work(d.n) + 1, n + m + n + 2};
  double **dst[4] = {&k.Kinv, &k.W, &k.work, &k.pv};
  for (int q = 0; q < 4; q++) {
    void *p = nullptr;
    if (hipMalloc(&p, sizeof(double) * cnt[q]) != hipSuccess) {
      (void)hipGetLastError();
      for (int b = 0; b < q; b++) (void)hipFree(*dst[b]);
      return OSQP_MEM_ALLOC_ERROR;
    }
    *dst[q] = static_cast<double *>(p);
    k.bytes += (double)(sizeof(double) * cnt[q]);
  }
  k.on = 1; k.state = 2;
  d.dk = k;
  return OSQP_NO_ERROR;
}

void dk_release(Dev &d) {
  if (!d.dk.on) return;
  (void)hipSetDevice(d.device);
  (void)hipStreamSynchronize(st(d));
  for (double *p : {d.dk.Kinv, d.dk.W, d.dk.work, d.dk.pv}) if (p) (void)hipFree(p);
  d.dk = DevDk();
}

void dk_factor(Dev &d, double *K_out) {
  DevDk &k = d.dk;
  if (!k.on) return;
  HIP_CHECK(hipSetDevice(d.device));
  HIP_CHECK(hipStreamSynchronize(st(d)));                   // (the wall clock below measures this factorisation alone)
  const double t0 = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
  const int n = d.n, m = d.m;
  HIP_CHECK(hipMemsetAsync(k.W, 0, sizeof(double) * (size_t)m * n, st(d)));
  hipLaunchKernelGGL(k_dk_fillW, dim3(std::min((m + kBlock - 1) / kBlock, kGrid)), dim3(kBlock), 0, st(d), d);
  dense_gemm_sym(st(d), n, m, 1.0, k.W, 1, n, k.W, n, 1, k.Kinv, n);      // K(i, j) = sum_a W[a][i] W[a][j]: one triangle on the matrix cores, mirrored
  hipLaunchKernelGGL(k_dk_addP, dim3(std::min((n + kBlock - 1) / kBlock, kGrid)), dim3(kBlock), 0, st(d), d);
  if (K_out) { HIP_CHECK(hipMemcpyAsync(K_out, k.Kinv, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost, st(d))); HIP_CHECK(hipStreamSynchronize(st(d))); }
  double *minpiv = k.work + dense_spd_inverse_work(n);
  dense_spd_inverse(st(d), k.Kinv, n, n, k.work, minpiv, gj_aux(d));
  enqueue_probe(d);
  double piv = 0.0;
  HIP_CHECK(hipMemcpyAsync(&piv, minpiv, sizeof(double), hipMemcpyDeviceToHost, st(d)));
  const double pr = fetch_probe(d);
  HIP_CHECK(hipGetLastError());
  k.minpiv = piv; k.probe = pr;
  k.state = (piv > 0.0 && std::isfinite(piv) && pr <= kDkProbeTol) ? 1 : 2;
  k.nfac += 1;
  k.fac_ms += 1e3 * (std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() - t0);
}

void dk_apply(Dev &d) { launch_apply(d, 1); }

// Diagnostic (backend.h DkProbe).  What the ops overwrite of a solve's state -- d.r, d.uu, d.xs, d.xg, the flags -- is saved first and put back last,
// also when one of them throws; what dk_factor writes besides is a function of the matrices and the rho vector.
int test_dense_kkt(Dev &d, DkProbe &p) {
  HIP_CHECK(hipSetDevice(d.device));
  const size_t n = d.n, m = d.m;
  struct Saved {
    Dev &d; hipStream_t s;
    struct V { double *ptr; double *bak; } v[4];
    int flags[F_COUNT]; bool have = false;
    Saved(Dev &d_, hipStream_t s_) : d(d_), s(s_), v{{d_.r, nullptr}, {d_.uu, nullptr}, {d_.xs, nullptr}, {d_.xg, nullptr}} {}
    void save() {
      for (auto &e : v) {
        HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&e.bak), (size_t)d.n * sizeof(double)));
        HIP_CHECK(hipMemcpyAsync(e.bak, e.ptr, (size_t)d.n * sizeof(double), hipMemcpyDeviceToDevice, s));
      }
      HIP_CHECK(hipMemcpyAsync(flags, d.flags, sizeof(flags), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      have = true;
    }
    ~Saved() {                                                // (no throw from here: a failed restore leaves the device error for the next call to report)
      if (have) {
        for (auto &e : v) if (e.bak) (void)hipMemcpyAsync(e.ptr, e.bak, (size_t)d.n * sizeof(double), hipMemcpyDeviceToDevice, s);
        (void)hipMemcpyAsync(d.flags, flags, sizeof(flags), hipMemcpyHostToDevice, s);
        (void)hipStreamSynchronize(s);
      }
      for (auto &e : v) if (e.bak) (void)hipFree(e.bak);
    }
  } saved(d, st(d));
  saved.save();
  if (p.op == 0) {
    const long long nfac = d.dk.nfac; const double ms = d.dk.fac_ms;
    dk_factor(d, p.K);
    d.dk.nfac = nfac; d.dk.fac_ms = ms;                       // (a diagnostic re-factorisation of what the handle already holds is not one of the handle's)
    if (m) HIP_CHECK(hipMemcpyAsync(p.rho, d.rho, m * sizeof(double), hipMemcpyDeviceToHost, st(d)));
  } else if (p.op == 1) {
    HIP_CHECK(hipMemcpyAsync(d.r, p.r, n * sizeof(double), hipMemcpyHostToDevice, st(d)));
    HIP_CHECK(hipMemcpyAsync(d.xg, p.xg, n * sizeof(double), hipMemcpyHostToDevice, st(d)));
    HIP_CHECK(hipMemsetAsync(d.flags + F_DONE, 0, sizeof(int), st(d)));
    dk_apply(d);
    int flags[F_COUNT];
    HIP_CHECK(hipMemcpyAsync(p.xs, d.xs, n * sizeof(double), hipMemcpyDeviceToHost, st(d)));
    HIP_CHECK(hipMemcpyAsync(p.u, d.uu, n * sizeof(double), hipMemcpyDeviceToHost, st(d)));
    HIP_CHECK(hipMemcpyAsync(flags, d.flags, sizeof(flags), hipMemcpyDeviceToHost, st(d)));
    HIP_CHECK(hipStreamSynchronize(st(d)));
    p.done = flags[F_DONE]; p.iters = flags[F_ITERS];
  } else {
    enqueue_probe(d);
    p.probe = fetch_probe(d);
  }
  HIP_CHECK(hipStreamSynchronize(st(d)));
  HIP_CHECK(hipGetLastError());
  if (p.op != 2) p.probe = d.dk.probe;
  p.state = d.dk.state; p.minpiv = d.dk.minpiv;
  return OSQP_NO_ERROR;
}

}  // namespace be
}  // namespace osqp_hip
