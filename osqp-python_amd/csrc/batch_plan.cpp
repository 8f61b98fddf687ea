// batch_plan.cpp -- which kernels the batch path (batch_hip.hip) launches for a BatchParams, and the LDS they need.  Host arithmetic only: no HIP
// call, so the CPU test tier compiles it on its own (tests/hostsim/batch_plan_probe.cpp).
#include <algorithm>
#include <cstring>

#include "backend.h"

namespace osqp_hip {
namespace be {

namespace {
// LDS needed per problem (bytes); 0 if the problem does not fit one workgroup's LDS.  nnz > 0 adds the product buffer of
// the register-resident path.
size_t batch_lds_bytes_nnz(int n, int m, int nnz) {
  const size_t b = sizeof(double) * ((size_t)10 * n + (size_t)8 * m + 16 + (nnz > 0 ? (size_t)((nnz + 1) & ~1) + batch_index_doubles(n, m) : 0));
  return b <= 64 * 1024 ? b : 0;
}
// rows / columns of V in the wave kernel's LDS: compile-time, three instantiations (n <= 64: 33 KB; n <= 120: the MPC batch's 116 KB; n <= 128)
int batch_wave_n8(int n) { return n <= 64 ? 64 : (n <= 120 ? 120 : 128); }
}  // namespace

size_t batch_lds_bytes(int n, int m) { return batch_lds_bytes_nnz(n, m, 0); }
size_t batch_direct_lds_bytes(int n, int m, int nnz, int bw) {
  if (bw < 0 || bw > kBatchDirectMaxBw) return 0;
  const size_t b = sizeof(double) * ((size_t)10 * n + (size_t)8 * m + 16 + (size_t)((nnz + 1) & ~1) + batch_index_doubles(n, m) + band_doubles(n, bw));
  return b <= 144 * 1024 ? b : 0;         // (above the default 64 KB dynamic-LDS limit: batch_solve raises it; gfx950 has 160 KB per CU)
}
size_t batch_wave_lds_bytes(int n, int m, int steps) {
  if (n < 1 || n > kBatchSpecN || m < 1 || m > 256) return 0;
  const size_t n8 = (size_t)batch_wave_n8(n), S = n8 + 1, stg = (size_t)((n > m ? n : m) + 1) & ~(size_t)1;
  const size_t b = sizeof(double) * (((n8 * S + 1) & ~(size_t)1) + (size_t)steps * 64 + (size_t)kBatchWaveW * stg) + sizeof(unsigned short) * (size_t)steps * 64;
  // (V t reads row min(64 + lane, n - 1) and V' rhs reads 64 words past a row's start: both stay inside V + staging)
  return b <= 160 * 1024 ? b : 0;
}
bool batch_direct_selected(const BatchParams &p) { const int v = plan_batch(p, 0).variant; return v == 1 || v == 2; }

}  // namespace be

namespace {
// the smallest of the compiled entries per lane (`buckets`, ascending) that holds e -- the last one if none does (the checks in front rule that out)
template <size_t K>
int bucket(int e, const int (&buckets)[K]) {
  for (int b : buckets) if (e <= b) return b;
  return buckets[K - 1];
}
}  // namespace

BatchPlan plan_batch(const BatchParams &p, int cus) {
  BatchPlan pl;
  const int mx = p.A.nnz > p.B.nnz ? p.A.nnz : p.B.nnz;
  const size_t lds_reg = be::batch_lds_bytes_nnz(p.n, p.m, mx), lds_gen = be::batch_lds_bytes(p.n, p.m), lds_dir = be::batch_direct_lds_bytes(p.n, p.m, mx, p.bw);
  const int e64 = (mx + 63) / 64, e256 = (mx + 255) / 256;
  const bool can64 = lds_reg && e64 <= 24 && p.n <= 1024 && p.m <= 2048, can256 = lds_reg && e256 <= 8;
  // (the direct variant with four waves also comes with 16 entries per lane: up to 4096 stored entries per matrix, one problem per CU)
  const bool can_dir = can64 && lds_dir && p.perm, can_dir256 = lds_reg && e256 <= 16 && lds_dir && p.perm;
  // default: the direct solve with four waves per problem (MPC batch: 14.2 ms; one wave 18.6 ms; PCG, one wave: 37 ms).  OSQPHipPolicy::batch_variant
  // forces one (debugging / A-B runs): the others are then off, and a forced variant that does not fit falls back to the generic one
  const int force = (p.variant >= 1 && p.variant <= 5) ? p.variant : 0;
  auto allowed = [&](int v, bool can) { return (force ? force == v : true) && can; };
  if (allowed(2, can_dir256)) { pl.variant = 2; pl.tb = 256; pl.e = bucket(e256, {2, 4, 6, 8, 16}); }
  else if (allowed(1, can_dir)) { pl.variant = 1; pl.tb = 64; pl.e = bucket(e64, {8, 16, 24}); }
  else if (allowed(3, can64)) { pl.variant = 3; pl.tb = 64; pl.e = bucket(e64, {8, 16, 24}); }
  else if (allowed(4, can256)) { pl.variant = 4; pl.tb = 256; pl.e = bucket(e256, {2, 4, 8}); }
  else if (lds_gen) { pl.variant = 5; pl.tb = 256; pl.e = 0; }
  pl.direct = pl.variant == 1 || pl.variant == 2;
  pl.pol = pl.direct && p.polish;
  pl.small = pl.variant == 2 && p.n <= 128;        // (256-thread kernels: n <= 128 takes the instantiation whose substitutions keep every element in registers, ksolve)
  pl.lds = pl.direct ? lds_dir : (pl.variant == 5 ? lds_gen : lds_reg);

  // The spectral form of the direct solve where the engine has prepared it (BatchParams::sp_V): every problem whose constraint classes are the
  // reference's is solved by it; the others are marked and left to the banded kernel launched right behind (only_marked).
  const int prod_len = (mx + 1) & ~1;
  if (pl.variant != 2 || !p.sp_V || p.mat_on || p.polish || p.n > kBatchSpecN || e256 > 8 || prod_len < 4 * (kBatchSpecN + 2) || p.only_marked) return pl;
  pl.spec_e = bucket(e256, {2, 4, 6, 8});
  pl.lds_spec = lds_reg + sizeof(double) * (kBatchNB + 2 * kBatchSpecN + 4);
  // One workgroup per CU (everything in registers) at every batch size: since K^-1 lives in the matrix instruction's result registers the two-per-CU
  // form (256 registers, scratch) no longer wins on large batches either -- 4096 QPs 5.9 ms against 6.2 ms.  BatchParams::wide_rounds = r selects it for
  // batches of more than r rounds of one workgroup per CU (A/B runs).
  pl.spec_w = p.nbatch > p.wide_rounds * cus ? 2 : 1;
  pl.spec = BatchPlan::kSpecWorkgroup;
  // ... one WAVE per problem where the engine has prepared that form (wv_on): eight problems in flight per CU.  A problem on one wave takes ~12 us per ADMM
  // iteration against 3.7 for a workgroup, and a batch ends with its slowest problem: with a launch order (longest-expected first) the first wv_split
  // positions -- the outliers, 38 of the MPC batch's 4096 problems take 200 .. 375 iterations against a mean of 95 -- go to the workgroup kernel on a second
  // stream, one CU each, while the wave kernel runs on the other CUs.  (No room for the wave form's LDS: the workgroup form.)
  pl.lds_w = p.wv_on ? be::batch_wave_lds_bytes(p.n, p.m, p.wv_aend[3] + p.wv_tend[1]) : 0;
  if (!pl.lds_w) return pl;
  pl.spec = BatchPlan::kSpecWave;
  pl.n8 = be::batch_wave_n8(p.n);
  pl.split = (p.order && p.wv_split > 0 && p.wv_cus > 0 && p.nbatch >= 8 * p.wv_split && cus > 2 * p.wv_cus) ? p.wv_split : 0;
  pl.split_w = pl.split > p.wide_rounds * cus ? 2 : 1;
  pl.wgs_all = std::max(1, std::min(cus, p.nbatch));      // (fewer problems than CUs: one wave per workgroup gets one)
  pl.wgs = pl.split ? std::max(1, std::min(cus - p.wv_cus, p.nbatch - pl.split)) : pl.wgs_all;
  return pl;
}

}  // namespace osqp_hip
