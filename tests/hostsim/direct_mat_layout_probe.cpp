// direct_mat_layout_probe.cpp -- TEST INFRASTRUCTURE (tests/test_lockstep_direct_mat_layout.py): the block of a direct lockstep chunk with per-problem
// matrices as lockstep_direct_chunk carves it (osqp-python_amd/csrc/lockstep_layout.h lockstep_direct_mat_layout), behind a C interface.  Plain C++.
#include "../../osqp-python_amd/csrc/lockstep_layout.h"

using namespace osqp_hip;

extern "C" {
constexpr int kProbeRanges = 16;
// base: nullptr for the counting cursor.  ranges: (offset, doubles) of every range in carve order;  info: end of the carve, fits (0 / 1), the offsets of
// the dense rows and of the view values from the pointer set (counting cursor: 0).  Returns the number of ranges.
int dm_carve(double *base, int n, int m, int r, int nzA, int nzB, int nv, size_t *ranges, size_t *info) {
  LsCursor c; c.base = base; c.log = ranges;
  LsMatVecs t; LwMatVecs d;
  const bool fits = lockstep_direct_mat_layout(c, n, m, r, nzA, nzB, nv, t, d);
  info[0] = c.off; info[1] = fits ? 1 : 0;
  info[2] = base ? (size_t)(d.WT - base) : 0; info[3] = base ? (size_t)(d.vval - base) : 0;
  return c.nlog;
}
size_t dm_size(int n, int m, int r, int nzA, int nzB, int nv) { return lockstep_direct_mat_ws_doubles(n, m, r, nzA, nzB, nv); }
// the matrix block alone, as ls_mat_block carves it from the same base: the direct carve must begin with exactly these ranges
int dm_carve_mat(int n, int m, int nzA, int nzB, size_t *ranges, size_t *info) {
  LsCursor c; c.log = ranges;
  LsMatVecs t;
  const bool fits = lockstep_mat_layout(c, n, m, nzA, nzB, t);
  info[0] = c.off; info[1] = fits ? 1 : 0;
  return c.nlog;
}
size_t dm_size_mat(int n, int m, int nzA, int nzB) { return lockstep_mat_ws_doubles(n, m, nzA, nzB); }
int dm_const(int which) { const int v[] = {kLsW, kProbeRanges}; return v[which]; }
}

// Stand-alone form (-DDIRECT_MAT_PROBE_MAIN: g++ -fsanitize=address,undefined of this file alone): the carve over a heap block of exactly the size
// function's doubles, every range written at both ends.
#ifdef DIRECT_MAT_PROBE_MAIN
#include <cstdio>
int main() {
  const int ns[] = {1, 63, 64, 65, 604, 2127}, ms[] = {1, 64, 65, 605}, rs[] = {1, 5, 21, 128};
  long carves = 0;
  for (int n : ns) for (int m : ms) for (int r : rs) {
    const int nzA = 3 * m + n, nzB = 3 * m + 2 * n, nv = m;
    size_t got[2 * kProbeRanges], info[4];
    const size_t size = dm_size(n, m, r, nzA, nzB, nv);
    double *block = new double[size];
    const int k = dm_carve(block, n, m, r, nzA, nzB, nv, got, info);
    if (!info[1] || info[0] > size) { std::printf("n %d m %d r %d: end %zu > size %zu\n", n, m, r, info[0], size); return 1; }
    for (int q = 0; q < k; q++) if (got[2 * q + 1]) { block[got[2 * q]] = 1.0; block[got[2 * q] + got[2 * q + 1] - 1] = 2.0; }
    delete[] block;
    carves++;
  }
  std::printf("direct mat layout probe: %ld carves, no finding\n", carves);
  return 0;
}
#endif
