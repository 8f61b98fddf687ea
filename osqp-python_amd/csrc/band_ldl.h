// band_ldl.h -- the padded band of the small-QP batch path and the arithmetic on it: ONE text for the layout (host + device), the banded LDL'
// factorisation and the wave-0 substitutions in their general form.  k_batch_admm (its ADMM system and, with POLISH, the polish system) and
// k_batch_adjoint call the device part (HIP compilations only); be::batch_direct_lds_bytes, batch_adjoint_lds_bytes and
// Engine::prepare_batch_direct size and address the band with the host part (plain C++: compiles under g++ with the rest of backend.h), which also
// builds band_factor's pair list.  tests/test_gpu_band_kernels.py runs the device part on its own (k_test_band in batch_hip.hip) and pins the invariants.
// Assembling a matrix into the band stays with each kernel.  One more reader of the invariants below lives outside this file: the
// register-resident n <= 128 form of the substitutions in k_batch_admm (batch_hip.hip), whose two fetch lambdas carry the text of
// band_fetch_fwd / band_fetch_bwd -- a change to the padding has to be made there as well.
//
// Layout.  A symmetric positive definite matrix of order n and half bandwidth bw <= kBatchDirectMaxBw, lower triangle, column-major: entry (r, c),
// c <= r <= c + bw, is Lb[band_slot(bw, c, r)] = Lb[c W + (r - c)], W = band_stride(bw).  Lb = first + kBandFront; the band takes band_doubles(n, bw).
// Invariants the substitutions rely on (band_clear establishes them, band_factor keeps them):
//   * W = bw + kBatchNB: every column ends in kBatchNB zeros, so a block's strided reads of the factor that leave the band read zeros;
//   * kBandFront = kBatchNB zeros in front of column 0: Lb[-1] is the one slot every lane beyond a block's reach reads (stride 0), and the backward
//     pass's reads of a column's head step back into the previous column's padding;
//   * band_cols(n) columns -- n rounded up to a multiple of kBatchNB, the columns past n zero: the substitutions run in whole blocks;
//   * kBandSlack = 64 doubles behind the last column: the read-ahead of the last block stays inside the allocation;
//   * after band_factor the diagonal slots are zero too (unit-lower L^ read as 0 there) and 1 / D lives in a vector of its own.
#pragma once
#include <stddef.h>
#include <vector>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

namespace osqp_hip {

constexpr int kBatchNB = 8;                        // pivots per block of the substitutions = zeros of padding per column
constexpr int kBatchDirectMaxBw = 64 - kBatchNB;   // band limit: one wave holds the live window of a block
constexpr int kBandFront = kBatchNB, kBandSlack = 64;
constexpr int band_stride(int bw) { return bw + kBatchNB; }
constexpr int band_cols(int n) { return (n + kBatchNB - 1) / kBatchNB * kBatchNB; }
constexpr int band_slot(int bw, int c, int r) { return c * band_stride(bw) + (r - c); }
constexpr size_t band_doubles(int n, int bw) { return (size_t)kBandFront + (size_t)band_cols(n) * (size_t)band_stride(bw) + (size_t)kBandSlack; }
// the pairs (a | b << 8), 1 <= a <= b <= bw, of one elimination step's trailing update: band_factor's `tri` (Engine::prepare_batch_direct and the
// diagnostic entry osqp_hip_test_band upload this list)
inline std::vector<int> band_tri_pairs(int bw) {
  std::vector<int> tri;
  for (int a = 1; a <= bw; a++) for (int b = a; b <= bw; b++) tri.push_back(a | (b << 8));
  return tri;
}

#if defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------------------------- device part
// value of v in lane `lane` (wave-uniform index) broadcast to the whole wave: two v_readlane_b32
__device__ __forceinline__ double readlane_f64(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// Every function below takes the band as (Lb, n, bw), by value: Lb = column 0, kBandFront doubles behind the band's first.

// all zeros, padding included (kBB = threads of the workgroup, all of them call).  The caller then adds its matrix at band_slot()s.
template <int kBB>
__device__ __forceinline__ void band_clear(double *Lb, int n, int bw) {
  const int tid = threadIdx.x;
  for (int s_ = tid - kBandFront; s_ < (int)(band_doubles(n, bw) - kBandFront); s_ += kBB) Lb[s_] = 0.0;
  __syncthreads();
}

// Banded Cholesky in place, right-looking: column c, then the (bw x bw)/2 trailing update spread over the workgroup (tri: [ntri] (a | b << 8),
// 1 <= a <= b <= bw, the pairs of one elimination step), then
//   K = L L' = L^ D L^' with unit-lower L^ = L diag(1/L_jj), D = diag(L_jj^2): the substitutions carry no division or pivot scaling on their
//   dependency chain.  Lb <- L^ (strictly lower part, diagonal slots read as L^ = 0), dinv <- 1/D.
// GUARD: a pivot that is not positive (or not finite) is replaced by its magnitude if that lies in (pivot_floor, 1e300], else by 1, and the call returns
// true (block-uniform: every thread reads the same pivot).  Without GUARD the pivots are taken as they are and the result is false.
template <int kBB, bool GUARD>
__device__ __forceinline__ bool band_factor(double *Lb, int n, int bw, double *dinv, const int *tri, int ntri, [[maybe_unused]] double pivot_floor) {
  const int tid = threadIdx.x, W = band_stride(bw);
  bool bad = false;
  for (int c = 0; c < n; c++) {
    double pv = Lb[c * W];
    if constexpr (GUARD) { if (!(pv > 0.0) || pv > 1e300) { bad = true; pv = (fabs(pv) > pivot_floor && fabs(pv) <= 1e300) ? fabs(pv) : 1.0; } }
    const double di = 1.0 / sqrt(pv);
    const int kmax = min(bw, n - 1 - c);
    const bool mine = tid >= 1 && tid <= kmax;
    double v = 0.0;
    if (mine) v = Lb[c * W + tid] * di;
    __syncthreads();
    if (mine) Lb[c * W + tid] = v;
    if (tid == 0) dinv[c] = di;
    __syncthreads();
    for (int t_ = tid; t_ < ntri; t_ += kBB) {
      const int ab = tri[t_], a = ab & 255, b_ = ab >> 8;
      if (b_ <= kmax) Lb[(c + a) * W + (b_ - a)] -= Lb[c * W + b_] * Lb[c * W + a];
    }
    __syncthreads();
  }
  for (int s_ = tid; s_ < n * W; s_ += kBB) { const int c = s_ / W, k = s_ - c * W; if (k >= 1 && k <= bw) Lb[s_] *= dinv[c]; }
  __syncthreads();
  for (int c = tid; c < n; c += kBB) { const double di = dinv[c]; dinv[c] = di * di; Lb[c * W] = 0.0; }
  __syncthreads();
  return bad;
}

// out = K^-1 rhs  (both in the caller's variable order; perm: position in the band's order -> variable):
//   L^ v = P rhs ;  g = D^-1 v ;  L^' x = g ;  out = P' x.
// Substitutions on ONE wave, kBatchNB pivots per block.  Element e lives in lane e % 64 while it is within 64 of the
// pivots.  Per block a lane fetches its kBatchNB entries of L^ with plain strided LDS reads one block AHEAD (the padded
// band makes every out-of-band read a zero, lanes beyond the block's reach are masked once), then for each pivot:
// v_readlane broadcast + one FMA.  Lanes whose element has pivoted store it and continue with the element 64 further on,
// already waiting in a register.  ~8 instructions per pivot, no LDS access, branch or division on the dependency chain.
// What a pivot costs is the broadcast itself (tools/lane_bcast_bench.hip, one wave: v_readlane_b32 ~14 cycles whether or not it
// is on a dependency chain -> 43.5 cycles per pivot for the two halves + FMA; DPP row_newbcast 30.6 but only inside a row of 16;
// an LDS round trip 178 per 8 values): resolving a block of 8 through its inverted diagonal block (two rounds of 8 INDEPENDENT
// broadcasts instead of a chain of 8) was tried and is slower, 12.6 vs 9.0 us per solve -- twice the broadcasts, and they do
// not pipeline.
//
// The factor entries of one block for this lane.  Forward, pivots p0 .. p0 + NB - 1, the lane's element p0 + dl:
// L^[p0 + dl][p0 + q] = Lr[(p0 + q) W + dl - q].  Lanes beyond the block's reach read the zero in front of column 0 eight times (stride 0): no
// masking after the load.
__device__ __forceinline__ void band_fetch_fwd(const double *Lr, int bw, int W, int n8, int tid, int p0, double (&l)[kBatchNB]) {
  const int dl = (tid - p0) & 63;
  const bool act = dl < bw + kBatchNB && p0 < n8;
  const double *col = act ? Lr + p0 * W + dl : Lr - 1;
  const int stride = act ? W - 1 : 0;
#pragma unroll
  for (int q = 0; q < kBatchNB; q++) l[q] = col[q * stride];
}
// Backward, pivots top - q, the lane's element i = top - dl:  L^[top - q][i] = Lr[i W + dl - q]
__device__ __forceinline__ void band_fetch_bwd(const double *Lr, int bw, int W, int tid, int top, double (&l)[kBatchNB]) {
  const int dl = (top - tid) & 63, i = top - dl;
  const bool act = dl < bw + kBatchNB && i >= 0 && top >= 0;
  const double *row = act ? Lr + i * W + dl : Lr - 1;
  const int stride = act ? 1 : 0;
#pragma unroll
  for (int q = 0; q < kBatchNB; q++) l[q] = row[-q * stride];
}

// The general form, any n: the permuted vector in buf (n doubles of LDS), finished elements stored and the element 128 further on refilled from it.
// Every thread of the workgroup calls; wave 0 substitutes, the others wait at the barriers.  stamp(0) / stamp(1) are called in front of and behind
// the forward pass (diagnostic builds time it; empty otherwise).
template <int kBB, class Stamp>
__device__ __forceinline__ void band_solve(const double *Lb, int n, int bw, const double *dinv, const int *perm, double *wbuf, const double *rhs, double *out, Stamp &&stamp) {
  constexpr int NB = kBatchNB;
  const int tid = threadIdx.x, W = band_stride(bw), n8 = band_cols(n);
  const double *__restrict__ Lr = Lb;
  double *__restrict__ buf = wbuf;
  for (int k = tid; k < n; k += kBB) buf[k] = rhs[perm[k]];
  __syncthreads();
  const int nblk = n8 / NB;
  const bool w0 = tid < 64;
  stamp(0);
  // ---- forward, unit lower:  v_e = w_e - sum_{j in [e-bw, e)} L^[e][j] v_j ----
  if (w0) {
    double cur = tid < n ? buf[tid] : 0.0, nxt = 64 + tid < n ? buf[64 + tid] : 0.0;
    auto block = [&](int p0, const double (&l)[NB]) {
#pragma unroll
      for (int q = 0; q < NB; q++) { const double vq = readlane_f64(cur, (p0 + q) & 63); cur -= l[q] * vq; }
      const int dl = (tid - p0) & 63;
      if (dl < NB) {                                          // pivoted in this block: final
        const int e = p0 + dl;
        if (e < n) buf[e] = cur;
        cur = nxt; nxt = e + 128 < n ? buf[e + 128] : 0.0;   // (requesting this before the chain was tried: the compiler then drains the LDS counter in front of the chain, +17 %)
      }
    };
    double la[NB], lb[NB];                                    // two blocks in flight, roles alternate (no register rotation)
    band_fetch_fwd(Lr, bw, W, n8, tid, 0, la);
    for (int b = 0; b < nblk; b += 2) {
      band_fetch_fwd(Lr, bw, W, n8, tid, (b + 1) * NB, lb);
      block(b * NB, la);
      if (b + 1 < nblk) { band_fetch_fwd(Lr, bw, W, n8, tid, (b + 2) * NB, la); block((b + 1) * NB, lb); }
    }
  }
  __syncthreads();
  stamp(1);
  for (int k = tid; k < n; k += kBB) buf[k] *= dinv[k];                          // g = D^-1 v
  __syncthreads();
  // ---- backward, unit upper (L^'):  x_i = g_i - sum_{j in (i, i+bw]} L^[j][i] x_j ; blocks from the top ----
  if (w0) {
    auto elem = [&](int top) { return top - ((top - tid) & 63); };
    const int i0 = elem(n8 - 1);
    double cur = (i0 >= 0 && i0 < n) ? buf[i0] : 0.0, nxt = i0 - 64 >= 0 ? buf[i0 - 64] : 0.0;
    auto block = [&](int top, const double (&l)[NB]) {
#pragma unroll
      for (int q = 0; q < NB; q++) { const double xq = readlane_f64(cur, (top - q) & 63); cur -= l[q] * xq; }
      const int dl = (top - tid) & 63;
      if (dl < NB) {
        const int i = top - dl;
        if (i < n) buf[i] = cur;
        cur = nxt; nxt = i - 128 >= 0 ? buf[i - 128] : 0.0;
      }
    };
    double la[NB], lb[NB];
    band_fetch_bwd(Lr, bw, W, tid, n8 - 1, la);
    for (int b = nblk - 1; b >= 0; b -= 2) {
      band_fetch_bwd(Lr, bw, W, tid, b * NB - 1, lb);
      block(b * NB + NB - 1, la);
      if (b >= 1) { band_fetch_bwd(Lr, bw, W, tid, b * NB - NB - 1, la); block(b * NB - 1, lb); }
    }
  }
  __syncthreads();
  for (int k = tid; k < n; k += kBB) out[perm[k]] = buf[k];
  __syncthreads();
}

#endif  // __HIPCC__

}  // namespace osqp_hip
