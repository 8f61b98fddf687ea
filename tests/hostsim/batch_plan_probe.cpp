// TEST INFRASTRUCTURE: osqp-python_amd/csrc/batch_plan.cpp (which kernels the batch path launches) behind a C ABI, so that the CPU tier can check its
// rules (tests/test_batch_plan.py).  Never part of the product.
#include "../../osqp-python_amd/csrc/backend.h"

using namespace osqp_hip;

extern "C" {
// A batch of nbatch problems (n, m; max(nnz(A), nnz(B)) = nnz, band bw) with the spectral form prepared (spectral), the wave form attached (wave,
// 32 ELL steps) and a launch order (order).  out: spec, split, variant, e, spec_e, spec_w, split_w, n8, wgs, wgs_all.
void bpp_plan(int n, int m, int nnz, int bw, int nbatch, int spectral, int wave, int order, int wv_split, int wv_cus, int wide_rounds, int cus, int *out) {
  static const int dummy[1] = {0};
  static const double ddummy[1] = {0.0};
  BatchParams p{};
  p.n = n; p.m = m; p.nbatch = nbatch; p.A.nnz = nnz; p.B.nnz = nnz; p.bw = bw; p.perm = bw >= 0 ? dummy : nullptr;
  p.sp_V = spectral ? ddummy : nullptr; p.wv_on = wave; p.wv_aend[3] = 16; p.wv_tend[1] = 16;
  p.order = order ? dummy : nullptr; p.wv_split = wv_split; p.wv_cus = wv_cus; p.wide_rounds = wide_rounds;
  const BatchPlan pl = plan_batch(p, cus);
  const int v[] = {pl.spec, pl.split, pl.variant, pl.e, pl.spec_e, pl.spec_w, pl.split_w, pl.n8, pl.wgs, pl.wgs_all};
  for (int k = 0; k < 10; k++) out[k] = v[k];
}
}
