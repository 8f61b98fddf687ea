// backend.h -- device-op interface between the host ADMM driver (engine.cpp) and the compute backend.
//
// Two implementations exist:
//   backend_hip.hip   hand-written gfx950 kernels; the ONLY backend linked into libosqp_hip.so (the product)
//   backend_host.cpp  plain loops with identical semantics; built ONLY by tests/ into tests/_build/ so that the
//                     driver logic (termination, adaptive rho, PCG budget, updates) can be exercised on machines
//                     without a GPU.  It is never shipped, never loaded by the package, and is not a fallback.
//
// Every ADMM quantity lives in SCALED space (Appendix A of SURVEY.md); formulas cite
// /root/reference/src/osqppurepy/_osqp.py ("_osqp.py:LINE").
//
// Matrices on the device (fp64 values, int32 indices):
//   A : m x n      CSR of the scaled constraint matrix
//   B : n x (n+m)  CSR of [ P + sigma I | A' ]  (P full symmetric; column n+i is constraint i)
// so that the reduced KKT operator of the PCG  K = P + sigma I + A' diag(rho) A  is applied as
//   t = rho .* (A p)   (kernel K1, m rows)      Kp = B [p; t]   (kernel K2, n rows).
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>

#include "lockstep_layout.h"     // the lockstep routes' work blocks: kLsW, kBatchRec, the pointer sets, one carve per set, the size functions
#include "band_ldl.h"            // the padded band of the batch path's direct solve: kBatchNB, kBatchDirectMaxBw, the layout

namespace osqp_hip {

// A failed HIP runtime call.  Thrown by the backend, caught at the C-API boundary (api.cpp) and reported as an
// osqp_error_type value -- the library never calls abort() and never falls back to a CPU path.
struct DeviceError : std::runtime_error { using std::runtime_error::runtime_error; };
struct NotPositiveDefinite : DeviceError { using DeviceError::DeviceError; };      // be::precond: the Woodbury system at this rho vector has no positive definite factorisation (the device itself is fine)

#ifndef OSQP_HIP_KBLOCK
#define OSQP_HIP_KBLOCK 256
#define OSQP_HIP_KGRID 1024
#endif
constexpr int kBlock = OSQP_HIP_KBLOCK;   // threads per workgroup (wave64s)
constexpr int kGrid = OSQP_HIP_KGRID;     // workgroups per launch = number of partial-reduction slots
constexpr int kChunk = 8 * kBlock;        // nnz staged through LDS per row-block (8 per thread, all loads in flight at once)
constexpr int kLongRow = 128;      // rows with more nnz get a workgroup of their own (block-wide reduction)
constexpr int kMaxRowsPerBlock = 1024;
constexpr int kPartSlots = 40;     // rows of Dev::part (each kGrid doubles)
constexpr int kMaxCg = 1024;       // hard cap on the PCG budget (size of the alpha/gamma history)
constexpr int kWinCap = 1472;      // input-vector window of a row block staged in LDS (elements; 23 KB as 16-byte pairs: 4 workgroups per CU)
// One-launch PCG iteration ("F1" form, DevF1 below)
constexpr int kF1Win = 512;        // widest window of a row block of A the F1 form takes (two elements per lane)
constexpr int kF1MaxD = 4;         // most replicas of the partial A' t vector
constexpr int kF1PChunk = 256;     // most (P + sigma I) entries of a block's own rows (one per lane)
constexpr int kF1MaxOwn = 512;     // most own columns of a block
constexpr int kF1MaxRows = 512;    // most rows of a block
constexpr int kF1Chunk = 1024;     // most entries of a row block of A
constexpr int kF1StreamBytes = kF1Chunk * 12;   // a block's slice of DevF1::stream: 8-byte values + 4-byte packed index words

struct DevCsr {
  int nrows = 0, ncols = 0, nnz = 0, nblk = 0;
  int *rowptr = nullptr, *col = nullptr;
  int *blkdesc = nullptr;        // nblk x {first row, end row, first nnz, end nnz}: one 16-byte load per row block.  A LONG row
                                 // (one row, more than kLongRow entries: reduced by the whole workgroup) carries -(1 + base) as its
                                 // end row: base = its first entry in runinfo
  int *runinfo = nullptr;        // per kChunk-entry slice of a long row: first column if the slice's columns are consecutive
                                 // (dense data blocks: the kernels then skip the index loads, 4 of 12 bytes per entry), else -1
  double *val = nullptr;
  // Windowed row blocks (banded matrices): the columns a block touches lie in at most two short ranges -- [w.x, w.x + w.y) of the
  // columns below `split` and [split + w.z, split + w.z + w.w) of those from `split` on (B = [P | A']: split = n; A: split = ncols) --
  // with w.y + w.w <= kWinCap.  The kernels then stage that window of the input vector(s) in LDS with coalesced loads and gather
  // from LDS through 16-bit LOCAL indices (10 instead of 12 bytes per entry, and no dependent global gather).
  int *blkwin = nullptr;         // nblk x {w.x, w.y, w.z, w.w}; w.y < 0: not windowed (global gather through col)
  unsigned short *lcol = nullptr;// [nnz] position inside the block's window (first range, then second); unused for other blocks
  int split = 0;
  int nwin = 0;                  // number of windowed blocks (statistics)
  int single = 0;                // 1: at most kGrid row blocks, each with at most kBlock rows (a workgroup's first pass covers all its rows)
};

// One launch per PCG iteration ("F1" form).  K = P + sigma I + A' diag(rho) A is applied from A ALONE: the
// workgroup that owns row block g of A forms  t = rho .* (A u)  for its rows and, in the same launch, the products  A_g' t_g  of those
// rows summed per column of the block's window (a second, column-ordered pass over the block's entries held in registers: the
// entries' 16-bit local row and their position in column order are stored next to the local column).  That partial slice goes to
// one of D "replica" n-vectors (block g -> replica g mod D; the windows of blocks g and g + D never overlap, and a block also zero-
// fills the gap up to the next window of its replica, so every replica is rewritten completely by every launch); whoever needs
// (A' t)_j next -- every workgroup whose window holds column j -- sums the D replicas in index order (deterministic, no atomics).
// The (P + sigma I) part is applied by the block to its OWN columns [cs0, cs1) from a compact CSR of P + sigma I.  One launch then
// performs a whole Chronopoulos-Gear iteration: scalars from the previous launch's partials, vector update on the window (each
// workgroup recomputes u_{k+1} on the columns it gathers -- nothing is exchanged inside a launch), SpMV, partials for the next.
struct DevF1 {
  int on = 0;                    // plan valid (Engine::prepare_f1); 0: the two-kernel form
  int D = 0;                     // replicas
  int *blk = nullptr;            // nblk(A) x 16 words, one scalar load per block:
                                 //   {first row, end row, first entry, end entry}  (the block's descriptor in A)
                                 //   {cov0, cov1, cs0, cs1}: replica coverage [cov0, cov1) (zero outside the window: zeroed by upload_f1, never stored by a kernel), own columns [cs0, cs1)
                                 //   {offset of the block's column pointers in cptr, first and end entry of its own rows in the P arrays, far columns (mix)}
                                 //   {g0, gl, a0, wl}: gather window [g0, g0 + gl) (columns of the block's rows of A -- plus those of its own
                                 //   rows of P if that widens it by at most a quarter), scatter window [a0, a0 + wl) (columns of its rows of A)
  // The matrix stream of a block, in the layout the kernel's LDS buffer has (pcg_hip.hip F1Stream): block b owns the kF1StreamBytes bytes at
  // stream + b * kF1StreamBytes = { double val[kF1Chunk]; unsigned ent[kF1Chunk]; } -- the block's values of A (copied from A.val by be::f1_refresh)
  // and one packed word per entry: column relative to g0 (9 bits) | local row << 9 (9 bits) | position of the entry in the block's
  // column-major order << 18 (11 bits).  Fixed stride: the address depends on the block index alone, so a workgroup requests its first block's
  // stream at the very head of a launch -- before any record has arrived -- and the NEXT block's stream while the current one is in its LDS
  // phases, both as LDS-direct loads (global_load_lds_dwordx4: no VGPR destination).
  unsigned char *stream = nullptr;
  unsigned short *cptr = nullptr;// per block: window length + 1 column pointers (block-local, column-major entry positions)
  int *prp = nullptr, *pcol = nullptr, *psrc = nullptr;   // compact CSR of P + sigma I (n rows): row pointers, columns, position of each entry in B.val
  double *pval = nullptr;        // values, refreshed from B.val by be::f1_refresh (after assembly / equilibration / matrix updates)
  int pnnz = 0;
  // the n-vectors of the iteration in ONE arena, stride ns doubles: Minv, x~, p, r (parity 0 = Dev::r, 1), s (0 = Dev::s, 1),
  // rep (parity 0: D vectors, parity 1: D vectors; their sum is K u_k: a block adds (P + sigma I) u_k of its own columns to its slice), and a third
  // set of D vectors: KA leaves the slices of rhs = sigma x - q + A' v in the parity-1 set and those of K x_g in the third (pcg_hip.hip f1_ka_body).
  // Dev::Minv / xs / p / r / s point into it.  r_k, s_{k-1} and rep_k (what launch F_k writes) live in parity k & 1.
  double *va = nullptr; size_t ns = 0;
  // The same allocation continues with every other array the F body's load phase reads: rho (Dev::rho points here), pval, pcol, prp, a copy of
  // A.rowptr and cptr, at the byte offsets below.  The F body reads all of them through ONE buffer resource over the arena (base va, vbytes records)
  // at 32-bit offsets: no 64-bit pointer per array to fetch, hold or re-fetch (pcg_hip.hip F1Arena).  upload_f1 refuses an arena of 2 GiB or more.
  unsigned vbytes = 0, o_rho = 0, o_pval = 0, o_pcol = 0, o_prp = 0, o_rowptr = 0, o_cptr = 0, nsb = 0;     // (nsb = 8 ns: the stride in bytes)
  // Per-block mixing (mix = 1): a row block of A whose columns do not fit one window keeps a window of at most kF1Win - kF1MaxFar columns and
  // treats the remaining columns -- at most kF1MaxFar distinct ones -- as FAR columns.  They occupy the LAST kF1MaxFar slots of the block's gather
  // list (the same 4 + D vector loads at column fcol[.] instead of g0 + e; which lanes serve them does not depend on the block's record) and
  // nfc more segments of its column-ordered pass.  A far column's sum goes to the block's SPILL SLOT for it instead of a replica: spill is
  // ordered by (column, block), so whoever reconstructs column c adds its slots in index order to the replicas' sum -- written by launch F_k,
  // read by F_{k+1}, three sets like the replicas (parity 0, parity 1 / r_0's slices, rhs's slices).  No atomics, fixed order: results do not
  // depend on scheduling, and every workgroup that recomputes a column obtains the same bits.  blk word 11 = the block's number of far columns.
  int mix = 0;
  int wt = 0;                    // the launches' results are written through the XCD's L2 (pcg_hip.hip gst_): set while the working set fits the Infinity Cache
  int *fcol = nullptr, *fq = nullptr;   // fixed stride kF1MaxFar per block: far columns (ascending) as pairs {column, spk[column]}, and the spill slot of each
  int *sp_ptr = nullptr;         // [n + 1] spill slots by column (host-side order; kept for inspection)
  int *spk = nullptr;            // [n] one packed word per column: first slot << 6 | count  (the plan refuses columns with more than 63 slots)
  double *spill = nullptr; size_t nsp = 0;      // 3 x (nsp + 2): the sets are padded (a reader takes its first two slots unconditionally)
};
constexpr int kF1MaxFar = 128;     // most far columns of a row block

// One launch per PCG iteration for ANY sparsity pattern ("K form", pcg_hip.hip k_slotk).  The reduced operator of the PCG,
//     K = P + sigma I + A' diag(rho) A            (/root/reference/src/osqppurepy/_osqp.py:291-301 is the KKT matrix it is the Schur complement of)
// is held EXPLICITLY as a CSR matrix (n x n, full symmetric pattern = pattern(P) + union over the rows i of A of cols(i) x cols(i)), so that one
// PCG iteration is ONE sparse product instead of two dependent ones (t = rho .* (A u), then B [u; t]: two launches, each paying the launch boundary).
// Symbolic part, once at setup (Engine::prepare_kf): every K entry owns a list of TERMS -- a copy of an entry of B.val (the P + sigma I part,
// row < 0) or a product  rho_i A_ia A_ib  (row i, positions a, b in A.val); numeric part, k_kf_values: one streaming pass over the term lists
// wherever rho or the matrix values change (be::precond), i.e. a rho update costs one more small kernel, not a re-assembly.  Chosen at setup when
// neither the one-launch form on A alone (DevF1: banded A, 0.72 x the bytes) nor a Woodbury mode applies and the fill stays moderate
// (sum_i nnz(row i)^2 <= kKfMaxFill nnz(A): configs[1] with unstructured columns: 41 entries per row, 49 MB; lasso / portfolio rows are dense: never).
// The Chronopoulos-Gear recurrences fit the launch boundary as in the F1 form (pcg_hip.hip): launch F_k folds the previous launch's partials (gamma,
// delta, ||r||), rebuilds  u_k[c] = Minv (r_{k-1} - alpha (w_{k-1} + beta s_{k-2}))[c]  at EVERY column c it gathers from the column's 32-byte
// RECORD {Minv, r_{k-1}, w_{k-1}, s_{k-2}} (one aligned 32-byte gather per entry instead of four scattered ones; same instruction sequence as the
// owner's update: all copies are bit-identical), updates its own rows' x~, p, r, s, applies K and leaves the next record + partials.  Records are
// double-buffered by the parity of k.
constexpr int kKfMaxFill = 8;
struct DevKf {
  int on = 0;
  DevCsr K;
  int *tptr = nullptr;           // [nnz(K) + 1] term ranges
  int *trow = nullptr, *ta = nullptr, *tb = nullptr;   // per term: constraint row (< 0: copy of B.val[ta]), positions of A_ia, A_ib in A.val
  int nterm = 0;
  double *rec = nullptr;         // [2][n][4] records {Minv, r, w, s}: launch F_k reads parity (k + 1) & 1, writes parity k & 1 (KB writes parity 1)
};

// Woodbury correction of the Jacobi preconditioner for a FEW dense rows of A (portfolio: k + 1 rows with thousands of entries next to
// n one-entry rows).  With L = the long rows (more than kLongRow entries; at most kWbMaxRows of them),
//     K = K0 + A_L' diag(rho_L) A_L ,   M = D0 + A_L' diag(rho_L) A_L ,   D0 = diag(K0) = diag(P) + sigma + sum_{i not in L} rho_i A_ij^2
//     M^-1 r = y - D0^-1 A_L' S^-1 A_L y ,   y = D0^-1 r ,   S = diag(1 / rho_L) + A_L D0^-1 A_L'          (r_L x r_L, dense, SPD)
// Jacobi alone sees nothing of the rank-r_L block, which carries the large eigenvalues (portfolio: 18.6 PCG iterations per ADMM
// iteration); M is exact whenever K0 is diagonal.  Per application: one pass over the long rows (g = A_L y), an r_L x r_L product
// (h = S^-1 g, S^-1 formed on the host at every rho update: r_L^3 / 3 flops), one pass over their transpose.  Three-kernel PCG form.
constexpr int kWbMaxRows = 128;
// MANY dense rows (lasso: 10 000 sample rows of 5 000 entries next to two-entry rows): the same correction with S formed, factorised
// and inverted on the device -- W = A_L D0^-1/2 as a dense r x ct block (ct = columns the long rows touch), S = W W' + diag(1 / rho_L)
// by one fp64 GEMM and S^-1 by a block Gauss-Jordan inverse, both this engine's own kernels on the matrix cores (dense_hip.hip; no
// vendor library), h = S^-1 g by a dense matrix-vector kernel (r^2 x 8 bytes per application).  Whether M = K (the direct mode) is
// decided NUMERICALLY after every factorisation: M^-1 (K v) must reproduce a probe vector v to DevWb::exact_tol.
constexpr int kWbLargeMax = 16384;
inline size_t wb_inverse_work(int n) { return (size_t)n * 64 * 3 + 2 * 64 * 64 + 8; }      // dense_hip.hip dense_spd_inverse: column panel, row panel, R, two pivot blocks
// The direct mode in TWO launches per ADMM iteration (wbdirect_hip.hip): P diagonal, every short row of A has exactly one entry, n <= kWbxMaxN.
// A workgroup owns kWbxCols consecutive columns and keeps its dense r x kWbxCols tile of A_L in LDS; the two global reductions of the
// iteration (g = A_L D0^-1 r_0, z~_L = A_L x~) travel as per-workgroup partials, summed in index order by every consumer.
constexpr int kWbxCols = 64;
constexpr int kWbxMaxN = 16384;           // at most 256 workgroups: every consumer folds all partials (G x kWbMaxRows doubles)
struct DevWbx {
  int on = 0, G = 0, nsc = 0;
  int slots = 0;                          // run the two launches as device-scheduled slots (device-driven boundaries; OSQPHipPolicy::device_driven = 2) instead of captured strings of 2 N + 1 launches
  double *tile2 = nullptr;                // [G][kWbMaxRows][kWbxCols] S^-1 A_L by column block (wbx_factor, after every inversion of S)
  double *tile = nullptr;                 // [G][kWbMaxRows][kWbxCols] A_L by column block, zero where A_L has no entry (rows >= r unused)
  double *partG = nullptr, *partZ = nullptr;   // [G][kWbMaxRows] partial sums of the two reductions
  double *ls0 = nullptr, *ls1 = nullptr;  // [3 r] {z, y, z~} of the long rows: read by X from ls0, written by X (workgroup 0) to ls1, handed over by Y
  // ONE launch per ADMM iteration (one = 1; wbdirect_hip.hip k_wbz; round 6).  The second global reduction of the two-launch form is not needed:
  //   z~_L = A_L x~ = A_L x_g + A_L D0^-1 r_0 - (A_L D0^-1 A_L') S^-1 g = A_L x_g + g - (S - diag(1 / rho_L)) h = A_L x_g + h ./ rho_L ,   h = S^-1 g,
  // and A_L x_g is carried along by linearity (Dev::ztg) -- so a launch folds the previous launch's partials of g, forms h with S^-1 held in registers
  // (sinvp: rows padded to kWbMaxRows, loaded at the head of the launch), updates the long rows, its own columns and one-entry rows, builds the next
  // right-hand side and leaves the next partials of g.  The partials alternate between partG and partZ, the long rows' state {z, y, z~, A x_g}
  // between lz0 and lz1, by the parity of the launch (no workgroup reads what its own launch writes).
  int one = 0;
  double *sinvp = nullptr;                // [kWbMaxRows][kWbMaxRows] S^-1, zero-padded (wbx_factor)
  double *lz0 = nullptr, *lz1 = nullptr;  // [4 kWbMaxRows] {z, y, z~, A x_g} of the long rows
  int *sc_ptr = nullptr, *sc_row = nullptr, *sc_src = nullptr;   // per column: its one-entry rows (CSR over columns) and where their values sit in A.val
  double *sc_val = nullptr;
  double *bjj = nullptr;                  // [n] P_jj + sigma (the diagonal of B), refreshed with the tiles
};
struct DevWb {
  int on = 0, r = 0;
  int large = 0;                 // r > kWbMaxRows: device-side dense factorisation; WT unused, W / colmap / ct in use
  int ct = 0;                    // columns with an entry in a long row
  int probe = 0;                 // decide `exact` by the probe after every factorisation (large mode)
  double exact_tol = 1e-6;       // ... the direct mode is on while  max |M^-1 K v - v| <= exact_tol max |v|  (OSQPHipPolicy::woodbury_direct_tol)
  int log = 0;                   // print the checks and the timing of every factorisation (OSQPHipPolicy::woodbury_log)
  int *colmap = nullptr;         // [n] column -> position among the ct touched ones (-1: untouched)
  double *W = nullptr;           // [r][ct] rows of A_L scaled by D0^-1/2 (zero where A_L has no entry)
  double *pv = nullptr;          // [n + m + n] probe vector v, rho .* (A v), v again (the reference M^-1 K v is compared with)
  int *info = nullptr;           // [2] status words of the factorisation / inversion
  int *dbg = nullptr;            // [1] test hook: upcoming device-side inversions to report as failed (OSQPHipPolicy::debug_fail_refactor)
  int exact = 0;                 // K0 is diagonal (P diagonal, every short row of A has one entry): M = K, and M^-1 r_0 IS the solve -- no PCG iteration
                                 // (Engine::run_chunk: KB, the three kernels of M^-1, k_wb_direct, KA); cleared when S^-1 fails its accuracy check
  DevWbx x;                      // exact mode in two launches per ADMM iteration (x.on)
  DevCsr AL, ALT;                // the long rows (r x n) and their transpose (n x r); values gathered from A.val through al_src / alt_src
  int *al_src = nullptr, *alt_src = nullptr;
  unsigned char *islong = nullptr;   // [m]
  int *rows = nullptr;           // [r] row indices in A
  double *WT = nullptr;          // [n][r] dense transpose of the long rows (column j of A_L contiguous): S is formed from it
  double *S = nullptr, *Sinv = nullptr;   // [r][r]
  // large form: the last few inverses, by the rho_bar they were computed for (woodbury_hip.hip wb_factor_large).  A handle that is solved again and
  // again -- parametric re-solves, the steps of a benchmark, which all restart from the setting's rho -- walks the same rho values each time:
  // the r^3 factorisation is then replaced by a look-up + the numerical probe (M^-1 K v = v against the CURRENT matrices and rho vector), which a
  // stale entry cannot pass.  Sinv points at one of the buffers; 8 r^2 bytes each (lasso: 0.8 GB of the 288).
  static constexpr int kCache = 4;
  double rho_key = 0.0;          // rho_bar of the last be::set_rho
  double *cache_buf[kCache] = {nullptr, nullptr, nullptr, nullptr}; double cache_rho[kCache] = {0, 0, 0, 0}; int cache_used = 0, cache_next = 0;
  int cache_hits = 0, cache_on = 1;
  double *g = nullptr, *h = nullptr;      // [r]  (dual form: [max(r, cd)])
  double *Dinv0 = nullptr;       // [n]  1 / D0
  // COLUMN-SPACE ("dual") form of the device-factorised correction (large only; Engine::prepare_wb takes it when it is the smaller system).  The columns
  // the long rows touch split into DENSE columns (two or more long-row entries: cd of them) and SINGLETON columns (exactly one: the lasso's -y_i of
  // the rows  y = A_d x - b).  Eliminating the singletons of every row a (Sherman-Morrison on its block  diag(D0_j) + rho_a s_a s_a') leaves, on the
  // dense columns C,
  //     T = D0_C + A_d' diag(w) A_d ,   w_a = rho_a / (1 + rho_a sigma_a) ,   sigma_a = sum_{j singleton of a} A_aj^2 / D0_j        (cd x cd, SPD)
  // and  M^-1 r  is:  beta_a = sum_{j singleton of a} A_aj r_j / D0_j ;  x_C = T^-1 (r_C - A_d' (w .* beta)) ;  t_a = (beta_a + A_d[a] x_C) / (1 + rho_a sigma_a) ;
  // x_j = (r_j - rho_a A_aj t_a) / D0_j on a singleton column of row a,  x_j = r_j / D0_j on the columns no long row touches.  Exactly the same M as the
  // row-space form (S = 1 / rho_L + A_L D0^-1 A_L', r x r) -- with cd x cd instead of r x r to form, factorise, invert and stream per application:
  // lasso 5k x 10k: cd = 5 000 against r = 10 000 -- an eighth of the factorisation's flops, a quarter of the inverse's bytes.
  // In this form: ct = cd, colmap = index among the dense columns, W [r][cd] = sqrt(w_a) A_d, S = T, Sinv = T^-1 (cd x cd).
  double *gjwork = nullptr;      // [wb_inverse_work(order) + 1] panels of the block Gauss-Jordan inverse, the smallest pivot behind them
  int dual = 0, cd = 0;
  int *kind = nullptr;           // [n] 0: no long row touches the column, 1: dense, 2: singleton
  int *dcol = nullptr;           // [cd] the dense columns, ascending
  int *srow = nullptr, *ssrc = nullptr; double *sval = nullptr;      // [n] singleton column -> index a of its long row, position of its entry in A.val, the entry (wb_refresh)
  int *sg_ptr = nullptr, *sg_col = nullptr;                          // per long row: its singleton columns (CSR over the r rows; sums run in list order)
  double *wv = nullptr, *den = nullptr, *beta = nullptr, *wbeta = nullptr, *rt = nullptr;      // [r] w_a, 1 + rho_a sigma_a, beta_a, w_a beta_a, rho_a t_a
  double *uz = nullptr;          // [n] x_C scattered to its columns, ZERO everywhere else (only dense positions are ever written): the vector the row pass gathers
  // FUSED ADMM iteration of the column-space direct mode (fused = 1; woodbury_hip.hip wbf_iteration): the dense block of A is streamed TWICE per ADMM
  // iteration instead of four times (KB's A' v, the g pass, the t pass, KA's A x~).  With c = v - t0 (v = rho z - y, t0 = rho A x_g):
  //   r_0 = sigma x - q - (P + sigma I) x_g + A' c,   so   g_C = [sigma x - q - (P + sigma I) x_g]_C + A_C' (c - w .* beta on the dense rows):
  // ONE transposed pass with the combined vector cc does KB's and the g pass's work; and since x~ = x_g + u,  z~ = A x_g + A u  on a dense row a is
  // ztg_a + (A_d[a] u_C + beta_a - rho_a t_a sigma_a): the t pass already holds A_d[a] u_C, so it also performs KA's z / y update of the dense rows.
  int fused = 0;
  DevCsr Bd, Bn, As;             // views of B / A (same arrays, other block lists): row blocks of B holding a dense column / a column that is not dense; row blocks of A holding a short row
  double *cc = nullptr;          // [m] v - t0 (- w_a beta_a on dense row a)
  int *lidx = nullptr;           // [m] constraint row -> its index among the dense rows (rows[lidx[i]] = i; 0 on short rows)
  double *sig = nullptr;         // [r] sigma_a
  // ... with the dense block held DENSE (dense = 1: cd even, the block at least half full): Ad [r][cd] row-major = A_d, zeros where A has no entry
  // (filled by wb_refresh).  The two passes over the block are then plain dense kernels -- 8 bytes per entry, 16-byte loads, no index stream, no row
  // slices: k_wbf_gd (column sums by row blocks into gp, fixed order) + k_wbf_gr (their sum + the short rows' and P's part from the small lists bq_*)
  // in place of k_wbf_g, and k_wbf_td (two rows per workgroup against ud) in place of k_wbf_t.
  int dense = 0, grb = 0;        // grb: row blocks of the column-sum pass
  int thin = 0;                  // every row of B of a column that is not dense and every short row of A has <= 64 entries: k_wbf_rb / k_wbf_s2 (one thread per row)
  double *Ad = nullptr, *ud = nullptr, *ccd = nullptr, *gp = nullptr;     // ud [cd] = x_C compact (k_wbd_gemv), ccd [r] = cc on the dense rows, gp [grb][cd] partial column sums
  int *bq_ptr = nullptr, *bq_idx = nullptr, *bq_col = nullptr;            // per dense column: its entries of B outside the dense rows (position in B.val, column of B)
};

// DENSE KKT mode (densekkt_hip.hip; include/osqp_hip.h osqp_hip_dense_kkt): a single QP with n between a few hundred and a
// few thousand holds  K^-1 = (P + sigma I + A' diag(rho) A)^-1  as a dense n x n matrix (n = 2 048: 33.5 MB, resident in the Infinity Cache), formed and
// inverted by the dense kernels of dense_hip.hip wherever rho or the matrices change (be::precond -> dk_factor).  An ADMM iteration is then three launches
// with an EXACT linear solve:  kb_rhs;  dk_apply (u = K^-1 r_0, x~ = x_g + u);  ka  -- whatever n is, against k + 2 launches of an inexact PCG.
// Whether the inverse is good enough is decided numerically after every factorisation, by the probe of the Woodbury direct mode:
// max |K^-1 (K v) - v| <= kDkProbeTol max |v|  with K v from the handle's own sparse products.
constexpr int kDkMaxN = 1000;                 // OSQP_HIP_DENSE_KKT_MAX_N: what the sweep of DESIGN.md section 6 supports (above it a rho update's factorisation costs more than the iterations save)
constexpr long long kDkMaxW = 1LL << 25;      // entries of the m x n work matrix (256 MB)
constexpr double kDkProbeTol = 1e-6;          // OSQPHipPolicy::woodbury_direct_tol's default, with the same meaning
struct DevDk {
  int on = 0;                    // the mode is enabled for this handle (buffers allocated)
  int state = 0;                 // 0 off; 1 K^-1 accepted by the probe: the solves run direct; 2 refused for the current rho: the handle's ordinary PCG path
  int suspend = 0;               // inside Engine::run_recurrence (rho = 1 / delta: no unpivoted inverse of that K): precond leaves the mode alone, chunks take the PCG path
  double *Kinv = nullptr;        // [n][n] full storage; the address is fixed for the life of the mode (captured launches hold it)
  double *W = nullptr;           // [m][n] sqrt(rho_i) A_ij
  double *work = nullptr;        // [dense_spd_inverse_work(n) + 1] panels of the inverse, the smallest pivot behind them
  double *pv = nullptr;          // [n + m + n + 2] probe vector v, rho .* (A v), v again, the two results of the comparison
  // host-side bookkeeping of the factorisations (dk_factor)
  double probe = 0.0, minpiv = 0.0, fac_ms = 0.0;
  long long nfac = 0;
  double bytes = 0.0;
};
inline bool dk_direct(const DevDk &k) { return k.on && k.state == 1 && !k.suspend; }

// indices into Dev::res (results of the residual kernels, reduced on the device)
enum ResId {
  R_PRI_U = 0, R_AX_U, R_Z_U, R_PRI_S, R_AX_S, R_Z_S, R_DY_U, R_DY_S, R_PINF_LHS, R_SUPP,   // m-side
  R_DUA_U, R_PX_U, R_ATY_U, R_DUA_S, R_PX_S, R_ATY_S, R_DX_U, R_DX_S, R_XPX, R_QX, R_QDX,    // n-side
  R_QN_S, R_QN_U,                                                                            // ||q||_inf, ||Dinv q||_inf (scaled q)
  R_ATDY_U, R_ATDY_S, R_PDX_U, R_PDX_S, R_ADX_VIOL,                                          // infeasibility 2nd stage
  R_COUNT
};
// indices into the int32 status block
// F_STAT_STAG: solves that ran into the iteration limit having reduced the residual by less than 10x (a STAGNATING inner solver, as
// opposed to one that converges steadily but needs more iterations than it was given)
enum FlagId { F_DONE = 0, F_ITERS, F_STAT_SUM, F_STAT_MAX, F_STAT_UNCONV, F_STAT_SUMSQ, F_STAT_N, F_STAT_STAG, F_COUNT };
// indices into the fp64 scalar block
enum ScalId { S_TOL_REL = 0, S_TOL_ABS, S_TOL_NOW, S_RN0 /* ||r_0||_inf of the current PCG */, S_RN0H /* the same by parity of the ADMM iteration (slot form): [2] */, S_HIST = 8 /* gamma[kMaxCg+1], alpha[kMaxCg+1], beta[kMaxCg+1] */ };

struct Ctl;       // policy.h: the state block of the chunk-boundary rules (device-driven solves keep one in device memory)
struct Dev {
  int n = 0, m = 0, device = 0;
  Ctl *ctl = nullptr;            // device copy of the driver's state block (nullptr: boundaries are processed by the host)
  double sigma = 0, alpha = 0;
  double rho_eq_factor = 1e3;    // rho_i = rho_eq_factor * rho_bar on equality rows (_osqp.py:27 uses 1e3; see engine.cpp)
  DevCsr A, B;
  int *Bdiag = nullptr;          // position of the diagonal entry of row j inside B.val
  // device-side assembly (setup, update_data_mat): the caller's UNSCALED values in their CSC order and where each goes
  double *Praw = nullptr, *Araw = nullptr;
  int nzP = 0, nzA = 0;
  int *Pi = nullptr, *Pj = nullptr, *Pm1 = nullptr, *Pm2 = nullptr;   // row, column, position in B.val, position of the mirrored entry (-1: diagonal)
  int *Ai = nullptr, *Aj = nullptr, *AmA = nullptr, *AmB = nullptr;   // row, column, position in A.val, position in B.val
  double *cs = nullptr;          // [2] device scalars of the equilibration: cost scale c, this pass's factor
  // problem data (scaled) and scaling
  double *q = nullptr, *l = nullptr, *u = nullptr, *D = nullptr, *Dinv = nullptr, *E = nullptr, *Einv = nullptr;
  double *rho = nullptr, *rho_inv = nullptr;
  int *ctype = nullptr;          // -1 loose, 0 inequality, 1 equality (_osqp.py:516-518)
  // vector updates on the device: the caller's UNSCALED q, l, u stay resident; scaling (_osqp.py:1328, :1357-1358)
  // and the constraint classification (:505-518) are kernels
  double *qraw = nullptr, *lraw = nullptr, *uraw = nullptr;
  int *cnt = nullptr;            // [2] device counters: {inequality rows found by the classification, rows with l > u}
  int eq_from_cnt = 0;           // 1: k_set_rho derives the equality weight from cnt[0] (device classification), 0: rho_eq_factor
  double rho_eq_mixed = 10.0;    // equality weight when inequality rows exist (engine.cpp classify_constraints)
  // ADMM iterates
  double *x = nullptr, *z = nullptr, *y = nullptr, *dx = nullptr, *dy = nullptr;
  double *xs = nullptr;          // x~ : PCG solution, kept as warm start for the next ADMM iteration
  // PCG start of the NEXT ADMM iteration: x~ extrapolated along the last step, xg = x~ + theta (x~ - x~_prev) (KA writes it, KB gathers it
  // and resets xs to it); ztg = A xg by linearity = z~ + theta (z~ - z~_prev), so that t0 = rho .* ztg keeps K xg = B [xg; t0] exact.
  double *xg = nullptr, *xsp = nullptr, *ztg = nullptr;
  int wt = 0;                    // two-kernel form: results written through the XCD's L2 (pcg_hip.hip stw) -- set while matrices + vectors fit the Infinity Cache
  double theta = 0.9;            // extrapolation weight (OSQP_HIP_EXTRAP; 0 = start from the previous x~)
  double *zt = nullptr;          // z~ = A x~
  double *t0 = nullptr;          // rho .* z~  (so K x~ = B [x~; t0] needs no extra SpMV)
  double *v = nullptr;           // rho .* z - y
  // PCG (Chronopoulos-Gear single-reduction form)
  double *r = nullptr, *uu = nullptr, *p = nullptr, *s = nullptr, *w = nullptr, *t = nullptr, *Minv = nullptr;
  double *uu2 = nullptr, *ms = nullptr;  // fused PCG: u_k lives in (k&1 ? uu2 : uu); ms (2n) = interleaved pairs {u_k[j], (Minv .* s_k)[j]}
  int fused = 0;                 // 1: two kernels per PCG iteration (vector update k-1 fused into the SpMV-A kernel of iteration k)
  // what the last be::batch_solve launched (OSQPHipStats::batch_wave_split): -1 no wave-per-problem kernel; >= 0 the wave kernel, with this many
  // positions of the launch order on the workgroup kernel beside it.  (In the padding in front of f1: the layout kernels receive by value stays.)
  int batch_wave_ran = -1;
  DevF1 f1;                      // one launch per PCG iteration (slot form only; f1.on)
  DevKf kf;                      // one launch per PCG iteration on the explicit reduced matrix (slot form only; kf.on; never together with f1.on)
  DevWb wb;                      // Woodbury-corrected preconditioner for a few dense rows (three-kernel PCG form; wb.on)
  // reductions
  double *part = nullptr;        // [kPartSlots][kGrid] partial results, slots see backend implementation
  double *res = nullptr;         // [R_COUNT]
  double *scal = nullptr;        // [S_HIST + 2*(kMaxCg+1)]
  int *flags = nullptr;          // [F_COUNT]
  int *slot = nullptr;           // [16] the two phase records of the slot kernels (backend_hip.hip "slot kernels"); nullptr: not used
  void *stream = nullptr;        // hipStream_t (product) / unused (host simulator)
  void *bside = nullptr, *bev0 = nullptr, *bev1 = nullptr;      // batch path: second stream + fork / join events (batch_hip.hip, created on first use)
  void *impl = nullptr;          // backend private (events, graphs, pinned staging)
  DevDk dk;                      // dense KKT mode (dk.on; never together with wb.on).  Last: every other field keeps its offset
};

// Batched small-QP solve (batch_hip.hip): nbatch problems sharing the solver's scaled A / B, one workgroup each (kBatchRec: lockstep_layout.h).
// The settings snapshot every batch route runs with (Engine::fill_batch_settings): base of BatchParams and LockstepParams
struct BatchSettings {
  double c = 1, cinv = 1, sigma = 0, alpha = 0, rho0 = 0, eq_factor = 0, eps_abs = 0, eps_rel = 0, eps_pinf = 0, eps_dinf = 0, cg_frac = 0, rho_tol = 0;
  int max_iter = 0, check = 0, rho_interval = 0, cg_max = 0, unscaled = 0, scaling = 0, precond = 0, rho_is_vec = 0, warm = 0;
  int check_dualgap = 0;        // settings.check_dualgap: the forward routes test the duality gap per problem (term_rules.h batch_check_gap) and write it to
                                // the record's column 11; the adjoint entries fill this struct too and never read it
};
struct BatchParams : BatchSettings {
  int n, m, nbatch;
  DevCsr A, B;
  const double *D, *Dinv, *E, *Einv;
  const double *q, *l, *u;      // UNSCALED, [nbatch][n] / [nbatch][m]; nullptr = the shared vector q0 / l0 / u0 for every problem
  const double *q0, *l0, *u0;   // UNSCALED shared vectors [n] / [m]
  double *x, *y;                // in: UNSCALED warm start (if warm), out: UNSCALED solution  [nbatch][n] / [nbatch][m]
  double *rec;                  // [nbatch][kBatchRec]: status, iter, obj, prim_res, dual_res, rho, rho_updates, pcg_iters, status_polish, polish seconds,
                                // rho_estimate (_osqp.py:1275, at the ADMM point), duality_gap (with check_dualgap; else 0)
  int *iters_out = nullptr;     // optional [nbatch]: ADMM iterations of every problem (device; feeds the next call's launch order)
  const int *order = nullptr;   // optional [nbatch]: workgroup w solves problem order[w] (longest-expected first: the batch ends with its slowest
                                // problems otherwise; Engine::batch_solve keeps the order of the previous call's iteration counts)
  double *zs = nullptr;         // optional, SCALED z iterates [nbatch][m]: read as the start when warm (a continued solve keeps its z, _osqp.py:1197-1204),
                                // written at the end (single-QP path: the handle's own d.z)
  int variant = 0;              // 0: automatic choice of the kernel variant; 1-5 force one (OSQPHipPolicy::batch_variant)
  int polish = 0, refine = 0;   // direct variants: polish a SOLVED problem in the kernel (reduced KKT on the active set + refine refinement steps)
  double delta = 1e-6;          // polish regularisation (_osqp.py:1740-1754)
  // Direct linear solve (banded Cholesky of K = P + sigma I + A' diag(rho) A under a bandwidth-reducing symmetric
  // permutation, factor held in LDS): bw < 0 selects the PCG path.  Built by Engine::prepare_batch_direct().
  int bw = -1;                  // half bandwidth of the permuted K (<= kBatchDirectMaxBw)
  double eq_factor_direct = 1e3; // equality-row weight of the direct variant: the reference's 1e3 (_osqp.py:27) -- the value 10 of
                                 // the PCG variants exists only to keep K well conditioned for CG (engine.cpp classify_constraints)
  int nents = 0, ntri = 0;
  const int *perm = nullptr;    // [n] position in the permuted order -> variable
  const int *bp_slot = nullptr; // [nnz(B)] band slot (band_ldl.h band_slot) of each (P + sigma I) entry of B in the permuted lower triangle, else -1
  const int *ke_slot = nullptr, *ke_ptr = nullptr;   // band slots that receive A' rho A terms, and their product ranges
  const int *kp_row = nullptr;  // per product: constraint row i (-> rho_i)
  const double *kp_val = nullptr;                    // per product: A_ia * A_ib (scaled values; refreshed before every batch call)
  const int *tri = nullptr;     // [ntri] (a | b << 8), 1 <= a <= b <= bw: the trailing-update pairs of one elimination step
  // Spectral form of the direct solve (engine.hpp BatchSpectral; n <= kBatchSpecN): V [kBatchSpecN x kBatchSpecN, column-major, zero-padded], lambda [kBatchSpecN],
  // the constraint classes and the equality weight they were built for.  nullptr: not available.  A problem whose own bounds give other classes is
  // left to the banded kernel: the spectral launch marks its record (kBatchUnsolved in rec[0]), a second launch with only_marked solves the marked ones.
  const double *sp_V = nullptr, *sp_lam = nullptr; const int *sp_ctype = nullptr;
  double sp_rho_ref = 0.0, sp_eqf = 0.0;
  // K^-1 for rho_bar = sp_K0_rho (the batch's starting rho: the same for every problem), built on the host with the kernel's own operation order and laid
  // out as the threads hold it -- [64 columns][256 threads]: a problem LOADS its first K^-1 (coalesced, L2-resident) instead of rebuilding it from V
  const double *sp_K0 = nullptr; double sp_K0_rho = 0.0;
  int only_marked = 0;
  // PER-PROBLEM MATRICES (the reference's forward with a P_val / A_val per batch element, /root/reference/src/osqp/nn/torch.py:128-157, 184-217: one
  // solver object per element, each set up -- and therefore SCALED -- with its own matrices).  mat_on != 0: problem b reads its own scaled values
  // Aval_b + b nnz(A), Bval_b + b nnz(B), its own equilibration D_b / Dinv_b (+ b n), E_b / Einv_b (+ b m), c_b[b] and, in the banded direct variant,
  // its own products kp_val_b + b nprod -- all written by be::batch_prepare (k_batch_prepare: assembly + Ruiz equilibration of _osqp.py:389-497 per
  // problem, one workgroup each, in LDS) right before the solve launch.  The spectral form (shared V) does not apply.
  int mat_on = 0, nprod = 0;
  double *Aval_b = nullptr, *Bval_b = nullptr, *D_b = nullptr, *Dinv_b = nullptr, *E_b = nullptr, *Einv_b = nullptr, *c_b = nullptr, *kp_val_b = nullptr;
  const int *kp_a = nullptr, *kp_b = nullptr;   // per product: positions of A_ia, A_ib in A.val (the products are formed per problem)
  // ONE WAVE PER PROBLEM, spectral form (batch_hip.hip k_batch_wave; built by Engine::prepare_batch_wave).  A workgroup of kBatchWaveW waves keeps V and
  // the shared matrices' values in LDS once for all of them; a wave keeps its problem's iterates in registers, rows spread over the lanes: row r of A' (and
  // of every n-vector) belongs to lane r % 64, slot r / 64; the rows of A are sorted by length (descending) first and the sorted position decides
  // lane and slot (wv_row: position -> row, -1 = none), so that the rows one ELL step treats together have similar lengths.  ELL steps of a group of 64 rows:
  // [wv_aend[g - 1], wv_aend[g]); entry (step s, lane l): value A.val[wv_Aidx[s 64 + l]] (index -1: padding, value 0), column wv_Acol[s 64 + l].
  // A' the same over B's entries with column >= n (wv_Tcol = the constraint ROW, original numbering).
  int wv_on = 0;
  int wv_aend[4] = {0, 0, 0, 0}, wv_tend[2] = {0, 0};
  const int *wv_Aidx = nullptr, *wv_Acol = nullptr, *wv_Tidx = nullptr, *wv_Tcol = nullptr, *wv_row = nullptr;
  int wv_first = 0;              // positions [0, wv_first) of the launch order are not the wave kernel's (be::batch_solve sends them to the workgroup kernel)
  int wv_split = 0;              // how many of the first positions the engine wants treated that way (0: none; needs a launch order)
  int wv_cus = 0;                // ... and on how many CUs (the wave kernel's grid leaves them free; wv_split > wv_cus: several problems per CU, one after the other)
  int wide_rounds = 1 << 20;     // the spectral workgroup kernel takes its two-per-CU form for more than wide_rounds rounds of one workgroup per CU (A/B runs)
  int *wv_queue = nullptr;       // device counter: the next position of the launch order not yet taken by a wave (zeroed before the launch)
};
constexpr int kBatchWaveW = 8;          // waves (= problems in flight) per workgroup of the wave-per-problem kernel; one workgroup per CU
constexpr int kBatchWaveSA = 128, kBatchWaveST = 128;   // most ELL steps of A / A' (what decides is the LDS they take: be::batch_wave_lds_bytes)
constexpr int kBatchSpecN = 128;        // the spectral form keeps K^-1 in registers: row i = thread / 2, 64 columns per thread
constexpr double kBatchUnsolved = -1000.0;

// Doubles of LDS taken by the index arrays of the batch kernel's register path: row pointers of A (m + 1) and B (n + 1), permutation (n).
constexpr int batch_index_doubles(int n, int m) { return (m + 2 * n + 2 + 1) / 2; }

// What be::batch_solve launches for a BatchParams (batch_plan.cpp, host arithmetic only): an optional spectral stage for the problems whose
// constraint classes are the reference's, then the follow-up kernel for the rest (only the problems the spectral stage marked, if it ran).
struct BatchPlan {
  enum Spec { kNoSpec, kSpecWorkgroup, kSpecWave };
  int spec = kNoSpec;
  // spectral workgroup kernel k_batch_admm<256, spec_e, spec_e, true, false, false, true, W>: W = spec_w for a launch of the whole batch,
  // split_w for one of the first `split` positions of the launch order
  int spec_e = 0, spec_w = 1, split_w = 1;
  size_t lds_spec = 0;
  // wave kernel k_batch_wave<n8>: the first `split` positions go to the workgroup kernel on a second stream; grid wgs, or wgs_all without the split
  int n8 = 0, split = 0, wgs = 0, wgs_all = 0;
  size_t lds_w = 0;
  // follow-up k_batch_admm<tb, e, e, direct, pol, small>; variant as OSQPHipPolicy::batch_variant (1 direct, 2 direct256, 3 w64, 4 w256, 5 generic),
  // 0: no variant fits
  int variant = 0, tb = 0, e = 0;
  bool direct = false, pol = false, small = false;
  size_t lds = 0;
};
BatchPlan plan_batch(const BatchParams &p, int cus);        // cus: compute units of the device

// Adjoint derivatives of a batch of solved QPs (batch_hip.hip k_batch_adjoint; include/osqp_hip.h osqp_hip_batch_adjoint): one workgroup per problem.
// The kernel works on the caller's UNSCALED matrices -- the resident raw values Dev::Praw / Dev::Araw, or the caller's own per-problem values --
// so that every result is in the caller's units; what it shares with the forward's direct variant is the symbolic data of the banded factor
// (Engine::prepare_batch_direct: permutation, band slots, products).
constexpr int kAdjointRec = 4;          // doubles per problem in the adjoint record (OSQP_HIP_ADJOINT_REC): status, active rows, relative residual, reserved
constexpr double kAdjointTol = 1e-6;    // status 0: final relative residual of the unregularised system below this (OSQP_HIP_ADJOINT_TOL)
struct AdjointParams {
  int n = 0, m = 0, nbatch = 0, nzP = 0, nzA = 0;
  DevCsr A, B;                  // structure of A (CSR) and B = [P | A'] (CSR); their scaled values are not read
  const double *Praw = nullptr, *Araw = nullptr;      // shared UNSCALED values in the caller's CSC order (P: upper triangle)
  const double *Px_b = nullptr, *Ax_b = nullptr;      // per-problem values [nbatch][nzP] / [nbatch][nzA]; nullptr = the shared ones
  const int *Pi = nullptr, *Pj = nullptr, *Pm1 = nullptr, *Pm2 = nullptr, *Ai = nullptr, *Aj = nullptr, *AmA = nullptr, *AmB = nullptr;   // Dev's assembly maps
  const double *l = nullptr, *u = nullptr, *l0 = nullptr, *u0 = nullptr;      // [nbatch][m] or nullptr = the shared l0 / u0 [m]
  const double *x = nullptr, *y = nullptr, *dx = nullptr, *dy = nullptr;      // [nbatch][n] / [nbatch][m]; dy == nullptr: zero
  double *dP = nullptr, *dq = nullptr, *dA = nullptr, *dl = nullptr, *du = nullptr, *arec = nullptr;      // outputs, each optional
  double delta = 1e-6; int refine = 3;
  int bw = -1, nents = 0, ntri = 0;
  const int *perm = nullptr, *bp_slot = nullptr, *ke_slot = nullptr, *ke_ptr = nullptr, *kp_row = nullptr, *kp_a = nullptr, *kp_b = nullptr, *tri = nullptr;
};
// LDS of k_batch_adjoint (bytes): both matrices' values, seven n-vectors, six m-vectors, the reduction scratch and the padded band; 0: does not fit
inline size_t batch_adjoint_lds_bytes(int n, int m, int nzA, int nzB, int bw) {
  if (bw < 0 || bw > kBatchDirectMaxBw) return 0;
  const size_t b = sizeof(double) * ((size_t)((nzA + 1) & ~1) + (size_t)((nzB + 1) & ~1) + (size_t)7 * n + (size_t)6 * m + 16 + band_doubles(n, bw));
  return b <= 144 * 1024 ? b : 0;
}

// Adjoint derivatives of ONE QP on the PCG path (adjoint_hip.hip; Engine::adjoint_compute_pcg): device arrays in the engine's numbering and the
// caller's units.  The kernels read the scaled matrices and the raw bounds of Dev and write the recurrence's data into Dev itself.
constexpr int kAdjointPcgRec = 4;       // doubles of AdjointPcg::rec: active rows, max |g - K_a r|, max |g|, reserved
struct AdjointPcg {
  const double *x = nullptr, *y = nullptr, *dx = nullptr, *dy = nullptr;      // stored solution and incoming gradients (n / m); dy == nullptr: zero
  int *code = nullptr;                  // [m] per row: 0 inactive, 1 lower-active, 2 upper-active
  double *rx = nullptr, *ry = nullptr;  // [n], [m] solution of the adjoint system (r_y = 0 on inactive rows)
  double *dP = nullptr, *dA = nullptr, *dl = nullptr, *du = nullptr;          // [nzP], [nzA] in the CSC order of Dev::Pi / Ai; [m], [m]
  double *rec = nullptr;                // [kAdjointPcgRec]
  double c = 1.0, cinv = 1.0;           // cost scaling
  int rho_is_vec = 1;
};

// Lockstep batch route (lockstep_hip.hip; include/osqp_hip.h osqp_hip_batch_solve_lockstep): QPs that share the handle's scaled A / B and differ in
// q / l / u, at any size, kLsW problems at a time on block vectors (element (j, b) at j * kLsW + b: lanes are problems).
// (chunk width kLsW, the state's row counts, lockstep_grid and the work blocks' layout and sizes: lockstep_layout.h)
struct LockstepParams : BatchSettings {
  int n = 0, m = 0, count = 0;  // count: problems of this chunk (1 .. kLsW)
  DevCsr A, B;
  const double *D = nullptr, *Dinv = nullptr, *E = nullptr, *Einv = nullptr;
  double time_limit = 0;        // seconds this chunk may still take (<= 0: none)
  const double *q = nullptr, *l = nullptr, *u = nullptr;        // the chunk's rows of the UNSCALED [nbatch][n] / [nbatch][m] arrays, the CALLER's numbering; nullptr = the shared vector
  const double *q0 = nullptr, *l0 = nullptr, *u0 = nullptr;     // UNSCALED shared vectors, the ENGINE's numbering
  double *x = nullptr, *y = nullptr, *rec = nullptr;            // the chunk's rows: in UNSCALED warm start (if warm), out UNSCALED solution; [count][kBatchRec]
  const int *pc = nullptr, *pr = nullptr;                       // reordered handle: engine column / row -> the caller's; nullptr: identity
  double *ws = nullptr;         // lockstep_ws_doubles(n, m) doubles
  double pcg_rel = 0;           // > 0: the recurrence's PCG threshold ||r|| <= pcg_rel ||rhs|| (floor 1e-15, be::set_pcg_tol) in place of the cg_frac rule
  // adaptive rho by the single-QP path's rule (term_rules.h single_rho_rule) in place of batch_rho_rule: its tolerance (the setting's on the handle's
  // square-root scale, Engine::ctl_setup) and persistence test.  0: the batch family's rule (rho_tol).  Set by the direct route only.
  double rho_tol_single = 0; int rho_persist = 0;
  // polish of the chunk's SOLVED problems between the ADMM loop and the transposes out (lockstep_hip.hip "polish of a chunk"; Engine::polish's semantics):
  // on / off, rho_bar = 1 / delta_eff on the guessed-active rows, at least pol_min_steps = 1 + polish_refine_iter steps of the recurrence, its PCG to
  // ||r|| <= pol_pcg_rel ||rhs|| within pol_cg_max iterations, the polish work block (lockstep_polish_ws_doubles(n, m) doubles, device) and where the
  // chunk's polish statistics go (host, kLsPolStat doubles: problems attempted, accepted, rejected, recurrence steps of the slowest problem, PCG
  // iterations summed, kernel launches, GPU ms; nullptr: not wanted).  Set by Engine::run_lockstep_solve on both routes, for the shared and the
  // per-problem-matrix entries alike; the adjoints leave polish off.  The DIRECT route (lockstep_direct_chunk) has no PCG: pol_cg_max and pol_pcg_rel are not
  // read there and the PCG count is 0; pol_prod2 != 0 refreshes the dense rows of x and x~ in its recurrence by one two-operand product (k_lw_prod2),
  // 0 by two k_lw_prod launches -- the same bits (an A/B switch).
  int polish = 0, pol_min_steps = 1, pol_cg_max = 0, pol_prod2 = 1;
  double pol_rho = 0, pol_pcg_rel = 0;
  double *pol_ws = nullptr, *pol_stat = nullptr;
  // PER-PROBLEM MATRICES (lockstep_hip.hip "matrices of a chunk"; include/osqp_hip.h osqp_hip_batch_solve_lockstep_mat): mat_ws != nullptr switches the chunk to
  // its own matrix block (lockstep_mat_ws_doubles(n, m, nnz(A), nnz(B)) doubles, device): Aval[k * kLsW + b], Bval[k * kLsW + b], D, Dinv (n x kLsW), E, Einv
  // (m x kLsW), assembled from the chunk's rows Px / Ax of the caller's [nbatch][nnz(triu P)] / [nbatch][nnz(A)] arrays (the caller's CSC order; nullptr: the
  // handle's raw values for every problem) and equilibrated per problem in front of the transposes in; c and 1 / c are rows of the per-problem scalar
  // state.  pvmap / avmap: caller's position -> the engine's (reordered handle; nullptr: identity).  mat_iters: settings.scaling.  mat_stat (host,
  // kLsMatStat doubles, nullptr: not wanted): GPU ms and kernel launches of the assembly + equilibration.  Set by Engine::run_lockstep_solve and, for the
  // backward pass with per-problem matrices (osqp_hip_batch_adjoint_lockstep_mat), by Engine::run_lockstep_adjoint: lockstep_adjoint_chunk then prepares the
  // chunk's matrices in the same block by the same launches, with the handle's q for every problem (q == nullptr).
  double *mat_ws = nullptr, *mat_stat = nullptr;
  const double *Px = nullptr, *Ax = nullptr;
  const int *pvmap = nullptr, *avmap = nullptr;
  int mat_iters = 0;
};
constexpr int kLsPolStat = 7;
constexpr int kLsMatStat = 2;

// Adjoint derivatives of a chunk on the lockstep route (lockstep_hip.hip lockstep_adjoint_chunk; include/osqp_hip.h osqp_hip_batch_adjoint_lockstep):
// the recurrence of Engine::run_recurrence per problem on block vectors.  The base carries the matrices, the scalings, the permutations, the shared
// bounds l0 / u0, the chunk's rows of l / u and the settings the forward's kernels read (alpha = 1, cg_max = kMaxCg, pcg_rel = polish_pcg_tol, rho0 =
// 1 / delta_eff, eq_factor = 1); q / x / y / rec of the base are not used.  With mat_ws set the chunk runs on its problems' own matrices and scalings.
struct LockstepAdjointParams : LockstepParams {
  int nzP = 0, nzA = 0;
  const int *Pi = nullptr, *Pj = nullptr, *Ai = nullptr, *Aj = nullptr;       // Dev's assembly maps: row and column of every stored entry, the engine's CSC order
  const int *Pmap = nullptr, *Amap = nullptr;                                   // reordered handle: caller's position in P.x / A.x -> the engine's; nullptr: identity
  const double *sx = nullptr, *sy = nullptr, *gx = nullptr, *gy = nullptr;    // the chunk's rows of x, dx ([count][n]) and y, dy ([count][m]; gy == nullptr: zero), caller's numbering
  double *dP = nullptr, *dq = nullptr, *dA = nullptr, *dl = nullptr, *du = nullptr, *arec = nullptr;      // the chunk's rows of the outputs, each optional
  int min_steps = 1, max_steps = 60; double gain = 0.9;                        // RecurrenceRule{true, 0.9, 60} with 1 + polish_refine_iter
};

// The DIRECT lockstep route for a Woodbury handle whose K0 is diagonal (lockstep_hip.hip "lockstep DIRECT"; include/osqp_hip.h
// osqp_hip_batch_solve_lockstep_direct): the base's A / B are the handle's; Av is the view of A the row passes read -- the one-entry rows as they are, long
// row a as the single entry 1.0 at column n + a -- and WT / rows / islong are DevWb's (the dense transpose of the long rows, their indices, the row flags).
// PER-PROBLEM MATRICES on this route (the base's mat_ws / Px / Ax; include/osqp_hip.h osqp_hip_batch_solve_lockstep_direct_mat): mat_ws is then
// lockstep_direct_mat_ws_doubles(n, m, r, nnz(A), nnz(B), Av.nnz) doubles -- the matrix block, the chunk's own dense rows and view values -- and the chunk
// fills the latter two from the block's scaled values through wtpos ([n r]: where entry (long row a, column j) sits in A.val, at j r + a; -1: no entry)
// and vsrc ([Av.nnz]: where a view entry sits in A.val; -1: a long row's 1.0).
struct LockstepDirectView {
  int r = 0;                    // long rows (1 .. kWbMaxRows)
  DevCsr Av;
  const double *WT = nullptr; const int *rows = nullptr; const unsigned char *islong = nullptr;
  const int *wtpos = nullptr, *vsrc = nullptr;
};
struct LockstepDirectParams : LockstepParams { LockstepDirectView v; };

// Adjoint derivatives of a chunk on the DIRECT route (lockstep_hip.hip lockstep_direct_adjoint_chunk; include/osqp_hip.h
// osqp_hip_batch_adjoint_lockstep_direct): LockstepAdjointParams as Engine::run_lockstep_adjoint fills them (cg_max and pcg_rel are not read: there is
// no PCG), with LockstepDirectParams' view of A and the dense rows' data.
struct LockstepDirectAdjointParams : LockstepAdjointParams { LockstepDirectView v; };

namespace be {

// The direct route's chunk and the refresh of the view's values: weak as well (the host simulator declines).  stat[4]: ADMM iterations of the slowest
// problem, inversions of S summed over the problems, kernel launches, GPU ms.
int lockstep_direct_chunk(Dev &d, const LockstepDirectParams &p, void *stream, double *stat) __attribute__((weak));
int lockstep_direct_values(Dev &d, int nv, const int *src, double *out, void *stream) __attribute__((weak));
// The backward pass of such a chunk: weak as well.  stat[4]: recurrence steps of the slowest problem, inversions of S summed over the problems, kernel
// launches, GPU ms.
int lockstep_direct_adjoint_chunk(Dev &d, const LockstepDirectAdjointParams &p, void *stream, double *stat) __attribute__((weak));

// Weak, like adjoint_*: the host simulator has no such kernels and the driver answers OSQP_FUNC_NOT_IMPLEMENTED where the symbol is absent.  One chunk,
// start to finish, on `stream` (nullptr: d.stream); synchronises with that stream.  stat[4]: ADMM iterations of the slowest problem, PCG iterations
// summed over the problems, kernel launches, GPU ms.
int lockstep_chunk(Dev &d, const LockstepParams &p, void *stream, double *stat) __attribute__((weak));
// The backward pass of such a chunk: transposes in, classification, the recurrence, residual, gradients, transposes out; returns when the chunk's
// results are there.  stat[4]: recurrence steps of the slowest problem, PCG iterations summed, kernel launches, GPU ms.  Weak as well.
int lockstep_adjoint_chunk(Dev &d, const LockstepAdjointParams &p, void *stream, double *stat) __attribute__((weak));

// Weak, like batch_adjoint: the host simulator has no such kernels and the driver answers OSQP_FUNC_NOT_IMPLEMENTED where the symbols are absent.
// adjoint_load: classification of the rows (code, rec[0]) and the recurrence's data -- Dev::q = c D dx, l = u = z = -E dy on the active rows (free
// elsewhere), ctype, x = x~ = y = 0.  adjoint_residual: from the recurrence's (Dev::x, Dev::y) to rx, ry, dl, du and rec[1..2].  adjoint_gradients:
// dP, dA from (x, y, rx, ry).  All stream-ordered.
void adjoint_load(Dev &d, const AdjointPcg &a) __attribute__((weak));
void adjoint_residual(Dev &d, const AdjointPcg &a) __attribute__((weak));
void adjoint_gradients(Dev &d, const AdjointPcg &a) __attribute__((weak));

// stream == nullptr: on d.stream, synchronous; otherwise enqueued on that hipStream_t and not waited for.  Weak: the host simulator of the CPU test
// tier has no such kernel -- the driver answers OSQP_FUNC_NOT_IMPLEMENTED where the symbol is absent.
int batch_adjoint(Dev &d, const AdjointParams &p, void *stream) __attribute__((weak));
size_t batch_lds_bytes(int n, int m);                       // 0 if a problem does not fit one workgroup's LDS
// stream == nullptr: on d.stream, synchronous.  Otherwise enqueued on that hipStream_t and NOT waited for.  OSQP_FUNC_NOT_IMPLEMENTED if it does not fit.
// Sets d.batch_wave_ran.
int batch_solve(Dev &d, const BatchParams &p, void *stream = nullptr);
size_t batch_direct_lds_bytes(int n, int m, int nnz, int bw); // 0 if the banded factor does not fit next to the iterates
bool batch_direct_selected(const BatchParams &p);              // would batch_solve run a direct (banded LDL') variant for p?
void batch_release(Dev &d);                                    // the batch path's second stream and events
size_t batch_wave_lds_bytes(int n, int m, int steps);          // LDS of the wave-per-problem kernel (V + `steps` ELL steps of values + one staging vector per wave); 0: does not fit
void batch_products(Dev &d, int nprod, const int *a, const int *b, double *out);   // out[p] = A.val[a[p]] * A.val[b[p]]
// per-problem matrices: Px_b [nbatch][nnz(P as given at setup: upper triangle, CSC order)] / Ax_b [nbatch][nnz(A), CSC order], UNSCALED, device
// pointers; nullptr = the solver's own values for every problem.  Fills p.Aval_b .. p.kp_val_b (allocated by the caller) on `stream` (nullptr: d.stream).
// scaling_iters: the setting's `scaling`.  Returns OSQP_FUNC_NOT_IMPLEMENTED when a problem's matrices do not fit one workgroup's LDS.
int batch_prepare(Dev &d, const BatchParams &p, const double *Px_b, const double *Ax_b, int scaling_iters, void *stream);
void batch_order(Dev &d, int nbatch, const int *iters, int *order, void *stream);  // order = problems by descending iters (ties by index), on `stream`

const char *name();
int init(Dev &d, int device);            // select device, create stream; returns 0 or osqp_error_type
void destroy(Dev &d);
void *alloc(Dev &d, size_t bytes);       // zero-initialised device memory
void dfree(Dev &d, void *p);
void h2d(Dev &d, void *dst, const void *src, size_t bytes);
void d2h(Dev &d, void *dst, const void *src, size_t bytes);   // synchronous w.r.t. the solver stream
void zero(Dev &d, void *dst, size_t bytes);
void sync(Dev &d);
// hipEvent pair on the solver's stream around one osqp_solve ("hipEvent around solve"): mark(0) at its start, mark(1) at its end;
// ev_ms waits for the second event and returns the elapsed milliseconds (host simulator: wall clock)
void ev_mark(Dev &d, int which);
double ev_ms(Dev &d);
void activate(Dev &d);                  // make d.device current for the calling thread (HIP's current device is thread-local)
// Work enqueued on a CALLER's stream that reads solver-owned memory (batch_solve with a stream): ext_record marks its end on that
// stream, ext_wait makes the host wait for it before the solver overwrites or frees that memory (no-op when nothing is pending).
void ext_record(Dev &d, void *stream);
void ext_wait(Dev &d);

// ---- ADMM hot path (all asynchronous on d.stream) ----
// KB: x-part of the rhs and the PCG start, one pass over B (two sums per row):
//   rhs_j = sigma x_j - q_j + (A' v)_j                         (_osqp.py:649-650 folded into the reduced system)
//   r_j   = rhs_j - (B [xs; t0])_j ;  u_j = Minv_j r_j
//   partials: gamma0 = <r,u>, ||r||_inf, ||rhs||_inf ; resets F_DONE/F_ITERS
void kb_rhs(Dev &d);
// K1_i: if PCG already converged -> no-op.  Else test ||r_i||_inf <= max(tol_rel*||rhs||_inf, tol_abs); on success set
//   F_DONE, F_ITERS = i and return; otherwise t = rho .* (A u).
void k1(Dev &d, int i);
// K2_i: if !done: w = B [u; t] ; partial delta = <w,u>
void k2(Dev &d, int i);
// Kv_i: if !done: alpha_i,beta_i from (gamma_i, delta_i, gamma_{i-1}, alpha_{i-1});
//   p = u + beta p ; s = w + beta s ; xs += alpha p ; r -= alpha s ; u = Minv r ; partials gamma_{i+1}, ||r||_inf
void kv(Dev &d, int i);
// KA: after the PCG (budget = number of (K1,K2,Kv) triples that were enqueued):
//   z~ = A xs ; z,y update (_osqp.py:682-703) ; v = rho z - y ; t0 = rho z~ ; dy ; and, on extra workgroups,
//   x = alpha xs + (1-alpha) x ; dx (_osqp.py:660-668).  Also folds the PCG statistics of this ADMM iteration.
void ka(Dev &d, int budget);
// Slot form of a chunk (device-side scheduling of KB / K1 / K2F / K1F / KA; see backend_hip.hip): slot_begin(target, cap) once, then any
// number of slot_pair() launches; slot_done() = ADMM iterations the chunk had completed at the last fetch_flags / fetch_res_flags.
bool slots_supported(const Dev &d);
void slot_begin(Dev &d, int target, int cap);
void slot_pair(Dev &d);
int slot_done(Dev &d);
int slot_seq(Dev &d);                      // slots executed since slot_begin (consistency check of the record hand-over)
// launches one ADMM iteration with `pcg` PCG iterations needs in the slot form (a slot_pair() is two of them):
//   two-kernel form  2 (pcg + 2)   KB, K1, pcg x (K2F, K1F), the K2F that detects convergence, KA
//   F1 form          pcg + 2       F_0, F_1 .. F_pcg, KA (run by the launch whose scalar fold detects convergence; it also leaves the slices F_0 builds
//                                 r_0 from -- no KB launch) + one launch at the start of every chunk
//   Woodbury direct mode in two launches (wbdirect_hip.hip): 2 per iteration + one closing pair per chunk
//   K form           pcg + 3       KB (rhs and r_0 from B), F_0 .. F_pcg on the explicit K, KA (run by the launch whose fold detects convergence)
inline double slot_launches(const Dev &d, double pcg) { return (d.wb.on && d.wb.exact && d.wb.x.on && d.wb.x.slots) ? 2.16 : (d.f1.on ? pcg + 2.0 : (d.kf.on ? pcg + 3.0 : 2.0 * (pcg + 2.0))); }
bool kf_supported();                       // the K form exists (false: the host simulator)
void kf_values(Dev &d, int cond = 0);      // K.val <- term lists with the current rho / A.val / B.val (no-op without the form; cond: inside a boundary group, only when it updated rho)
void f1_refresh(Dev &d);                   // f1.pval <- B.val (no-op without a plan)
bool wb_supported();                       // Woodbury preconditioner available (false: the host simulator)
bool wbx_supported();                      // the two-launch direct mode exists (false: the host simulator)
void wbx_init(Dev &d);                     // once per handle, after the plan is uploaded (LDS attribute of its kernels on d.device)
void wbx_refresh(Dev &d);                  // tiles / one-entry-row values <- A.val
void wbx_factor(Dev &d, int cond = 0);     // tile2 = S^-1 A_L (after S^-1 has changed); cond: inside a boundary group, only when it updated rho
void wbx_slot_pair(Dev &d);                // the two launches as a pair of slots (device-side scheduling)
inline bool wbx_active(const Dev &d) { return d.wb.on && d.wb.exact && d.wb.x.on; }
inline bool wbx_slots(const Dev &d) { return wbx_active(d) && d.wb.x.slots; }
void wbx_chunk(Dev &d, int niter);         // niter ADMM iterations: X(rhs), { Y, X } x (niter - 1), Y, X(update): 2 niter + 1 launches on d.stream
bool wb_large_supported();                 // the device-factorised form exists (false: the host simulator)
void wb_refresh(Dev &d);                   // wb.AL / ALT / WT values <- A.val (after assembly / equilibration / matrix updates)
void wb_direct(Dev &d);                    // exact mode: x~ = x_g + M^-1 r_0 (after kb_rhs + wb_apply(0)); marks the solve as converged after one step
inline bool wbf_active(const Dev &d) { return d.wb.on && d.wb.exact && d.wb.dual && d.wb.fused; }
void wbf_iteration(Dev &d);                // one ADMM iteration of the fused column-space direct mode: seven launches (no KB, no KA)
void wb_apply(Dev &d, int parity, int direct = 0);   // direct: exact mode -- the last of the three kernels also forms x~ = x_g + u and marks the solve as converged after one step
//         // u = M^-1 r with the partials gamma = <r, u>, ||r||_inf in the slots of `parity` (after kb_rhs: 0, after kv(i): (i + 1) & 1)
// ---- device-driven chunk boundaries (policy.h; backend_hip.hip "boundary kernels").  The host uploads the state block once per solve,
// then only feeds launches: strings of slot launches and, after each chunk's worth, one boundary group -- conditional residual
// kernels, k_decide (the rules of policy.h on the device: termination, rho, tolerance, budget, next chunk), conditional rho update.
bool ctl_supported(const Dev &d);
void ctl_upload(Dev &d, const Ctl &c);     // host -> device copy of the state block (stream-ordered)
void ctl_begin(Dev &d);                    // start the chunk the state block describes (slot record, PCG tolerance, statistics reset)
void ctl_group(Dev &d, int diagonal);      // enqueue one boundary group (diagonal: the Jacobi preconditioner follows rho)
void ctl_poll(Dev &d, Ctl *out, int *seq, int *done);   // snapshot of the state block + slots executed + ADMM iterations of the chunk in flight, read on the side stream WITHOUT waiting for d.stream
void ctl_download(Dev &d, Ctl *out);       // after a stream synchronisation
constexpr int kSlotInts = 24;  // Dev::slot: two phase records of 8 words + the chunk epoch
void slot_poll(Dev &d, int *seq, int *done); // the same two numbers of the RUNNING chunk, read on a side stream without waiting for the launches

// ---- every check_termination iterations ----
// residual norms / objective pieces of (x,z,y) -> d.res[0 .. R_QDX]   (_osqp.py:705-794, 880-908)
void residuals(Dev &d);
void infeas_primal(Dev &d);                         // d.res[R_ATDY_*] = || (Dinv) A' dy ||_inf      (_osqp.py:815-818)
void infeas_dual(Dev &d, double thr, int unscaled);               // d.res[R_PDX_*], d.res[R_ADX_VIOL]              (_osqp.py:846-872)
void fetch_res(Dev &d, double *host_res);           // D2H of d.res + stream sync
void fetch_flags(Dev &d, int *host_flags);          // D2H of d.flags (+ reset of the F_STAT_* counters)
void fetch_res_flags(Dev &d, double *host_res, int *host_flags);   // both behind ONE stream synchronisation (per termination check)

// ---- rho / preconditioner ----
// rho_i by constraint type (_osqp.py:1590-1594), rho_inv, v = rho z - y, t0 = rho z~
void set_rho(Dev &d, double rho_bar);
// Minv_j = 1 / (B_jj + sum_i rho_i A_ij^2)   (diag of K; B_jj already contains sigma).  precond==0 -> Minv = 1
void precond(Dev &d, int diagonal);
void set_pcg_tol(Dev &d, double tol_rel, double tol_abs);

// full != 0 (after warm_start / cold_start, _osqp.py:1493-1509):  z = A x ; xs = x ; dx = dy = 0, then the refresh;
// refresh (always):  zt = A xs ; t0 = rho zt ; v = rho z - y   (state the PCG start of kb_rhs relies on)
void init_iterates(Dev &d, int full);

// tmp = z + y ; z = clip(tmp, l, u) ; y = tmp - z   (_osqp.py:676-680, used by polish :1780)
void project_normalcone(Dev &d);

// Two-kernel PCG iteration available?  When true the driver enqueues  k1(i); k2(i)  per iteration and kv(i) only after the
// last budgeted one: k1(i), i >= 1, performs the vector update of iteration i-1 itself (backend_hip.hip k_k1f).
bool pcg_fused(const Dev &d);

// ---- launch batching ----
bool graphs_supported();
void graph_begin(Dev &d);                 // start capturing d.stream
void *graph_end(Dev &d);                  // stop capturing, instantiate; returns executable-graph handle
void graph_launch(Dev &d, void *g);
void graph_free(Dev &d, void *g);

// ---- assembly / scaling on the device ----
// false: the driver scales on the host and uploads finished value arrays (the test-only host simulator).
bool device_assembly();
// A.val, B.val <- scatter of Araw / Praw through the maps, scaled as  E A D  and  c D P D  when scaled != 0, with sigma on B's
// diagonal when with_sigma != 0   (_osqp.py:432-436, 464, 1443, 1463)
void assemble(Dev &d, int scaled, double c, int with_sigma);
// Ruiz equilibration + cost normalisation (_osqp.py:389-497) of A.val, B.val (assembled unscaled, no sigma) and d.q IN PLACE:
// fills d.D, d.E, d.Dinv, d.Einv, adds sigma to B's diagonal, returns the cost scale c.  iters == 0: D = E = 1, c = 1.
double ruiz(Dev &d, int iters);

// ---- vector updates / warm start on the device ----
bool device_vec_updates();               // false: the host simulator (the driver scales on the host and uploads finished vectors)
// dst (device) <- src, asynchronous on the solver's stream; src_on_device = 0: host memory (reusable when the call returns)
void copy_in(Dev &d, void *dst, const void *src, size_t bytes, int src_on_device);
void stream_wait(Dev &d, void *caller_stream);       // the solver's stream waits for everything queued on caller_stream so far
void gather(Dev &d, double *dst_dev, const double *src_dev, const int *idx_dev, int cnt);   // dst[k] = src[idx[k]] (reordered problems: caller's numbering -> the engine's)
void scale_q(Dev &d, double c);                       // q = c D qraw                                  (_osqp.py:1328)
void scale_bounds(Dev &d, int rho_is_vec);            // l = E lraw, u = E uraw; ctype; cnt[0]       (:1357-1358, :505-518)
int count_bad_bounds(Dev &d, const double *l_dev, const double *u_dev);   // rows with !(l <= u) (:1348-1349); synchronises
void scale_warm(Dev &d, const double *x_dev, const double *y_dev, double c);   // x = Dinv x_in ; y = c Einv y_in  (:1493-1545); NULL: keep

// ---- probes / tests ----
bool ktrace_read(Dev &d, unsigned long long *out, int count);   // diagnostic build only (OSQP_HIP_KTRACE); false otherwise
void test_spmv(Dev &d, int which, const double *in_dev, double *out_dev);   // 0: out = A in ; 1: out = B in
// one routine of the dense fp64 kernels on the caller's DEVICE operands (include/osqp_hip.h osqp_hip_test_dense: op 0 dense_gemm, 1 dense_gemm_sym,
// 2 dense_spd_inverse with its own work space); runs on d.stream and synchronises; returns the smallest pivot (op 2; 0 otherwise).  Weak, like
// lockstep_chunk: a backend without it still links, and the driver answers OSQP_FUNC_NOT_IMPLEMENTED.
struct DenseProbe { int op, M, N, K; double alpha, beta; long as_i, as_k, bs_k, bs_j, cs_i, cs_j; const double *A, *B; double *C; };
double test_dense(Dev &d, const DenseProbe &p) __attribute__((weak));
// the band of band_ldl.h on the caller's DEVICE operands (include/osqp_hip.h osqp_hip_test_band, which has validated every field: nothing is checked
// here): one workgroup of `threads` clears the band, scatters `band`, factors with `tri` (band_tri_pairs(bw)) and solves the nrhs right-hand sides into x;
// image / dinv / bad receive the LDS image, 1 / D and band_factor's result.  Runs on d.stream and synchronises.  Weak like test_dense.
struct BandProbe {
  int n, bw, threads, guard, nrhs, ntri; double pivot_floor;
  const double *band; const int *perm, *tri; const double *rhs; double *x, *image, *dinv; int *bad;
};
// LDS of the probe's workgroup (bytes): the band and two vectors of band_cols(n); 0: above the cap of the product's own kernels (batch_direct_lds_bytes)
inline size_t test_band_lds_bytes(int n, int bw) {
  if (n < 1 || n > 144 * 1024 / 8 || bw < 0 || bw > kBatchDirectMaxBw) return 0;
  const size_t b = sizeof(double) * (band_doubles(n, bw) + (size_t)2 * band_cols(n));
  return b <= 144 * 1024 ? b : 0;
}
int test_band(Dev &d, const BandProbe &p) __attribute__((weak));
// the Woodbury correction of a handle with d.wb.on (include/osqp_hip.h osqp_hip_test_woodbury, which has validated every field: nothing is checked here).
// HOST vectors in the engine's numbering: r [n], x0 [n] (direct), u / xs / dinv0 [n], S / Sinv [order^2], rho [m].  wb_factor (refactor), r -> d.r,
// x0 -> d.xs, F_DONE cleared, wb_apply(parity, direct); d.r, d.uu, d.xs, the flags and the four gamma / rn partial slots are saved before and
// restored after.  gamma / rnorm: the kGrid partials of SL_GAMMA0 + parity / SL_RN0 + parity folded on the host in index order.  Weak like test_dense.
struct WbProbe {
  int refactor, parity, direct; const double *r, *x0; double *u, *xs, *dinv0, *S, *Sinv, *rho;
  int exact, info[2], done, iters; double gamma, rnorm;
};
int test_woodbury(Dev &d, WbProbe &p) __attribute__((weak));
// ---- dense KKT mode (DevDk; densekkt_hip.hip).  Weak like lockstep_chunk: the host simulator has none of it, and the driver answers
// OSQP_FUNC_NOT_IMPLEMENTED where the symbols are absent.
// dk_enable: the buffers, all or nothing (OSQP_MEM_ALLOC_ERROR: the device has no room; nothing stays allocated); d.dk.on = 1, no factorisation yet.
// dk_release: frees them, d.dk = DevDk().  dk_factor: W, K = W' W + P + sigma I, K^-1 in place, the probe; synchronous; sets d.dk.state (1 / 2), probe,
// minpiv and counts itself; K_out (host, n^2): K as formed, copied out before the inversion.  A fixed launch sequence without atomics on doubles:
// repeated factorisations of the same data are bit-identical.  Called by be::precond on a handle with the mode on and not suspended.
// dk_apply: u = K^-1 r_0 (Dev::r) into Dev::uu, x~ = x_g + u into Dev::xs, F_DONE = 1 / F_ITERS = 0 (ka then counts a converged solve of no PCG
// iteration); one launch on d.stream, capturable.
int dk_enable(Dev &d) __attribute__((weak));
void dk_release(Dev &d) __attribute__((weak));
void dk_factor(Dev &d, double *K_out = nullptr) __attribute__((weak));
void dk_apply(Dev &d) __attribute__((weak));
// the diagnostic entry (include/osqp_hip.h osqp_hip_test_dense_kkt, which has validated every field: nothing is checked here).  HOST vectors in the engine's
// numbering.  op 0 FORM: dk_factor with K [n^2] copied out before the inversion, rho [m].  op 1 APPLY: r -> d.r, xg -> d.xg, F_DONE cleared, dk_apply; xs, u
// [n], done / iters.  op 2 PROBE: the probe alone against the inverse in place.  d.r, d.uu, d.xs, d.xg and the flags are saved before and restored after.
struct DkProbe { int op; const double *r, *xg; double *K, *rho, *xs, *u; int done, iters, state; double probe, minpiv; };
int test_dense_kkt(Dev &d, DkProbe &p) __attribute__((weak));
// single launches of the lockstep kernels (include/osqp_hip.h osqp_hip_test_lockstep, which has validated every field, staged the caller's arrays and uploaded
// the blocks: nothing is checked here).  p: the parameters of a chunk as Engine::run_lockstep_solve builds them (ws / mat_ws: the route's resident blocks,
// q .. Ax: DEVICE arrays).  The body carves the blocks as lockstep_chunk does, launches ops[0 .. nops) -- OSQPHipLockstepOp, one kernel launch each, through
// the launch text of the drivers -- on d.stream, synchronises and answers hipGetLastError.  Weak like test_woodbury.
// direct: the direct route (p.v: the view as Engine::fill_lockstep_direct_view fills it, with wtpos / vsrc where mat).
struct LsProbe { LockstepDirectParams p; bool direct; int nops; const int *ops; };
int test_lockstep(Dev &d, const LsProbe &t) __attribute__((weak));
// the same for the kernels of the backward pass and of polish (include/osqp_hip.h osqp_hip_test_lockstep_back; OSQPHipLockstepBackOp).  polish == false: a is
// what Engine::run_lockstep_adjoint builds (a.ws: the route's adjoint work block; sx .. arec: DEVICE arrays), the carve is lockstep_adjoint_chunk's or the
// direct backward pass's.  polish == true: p is what a polishing Engine::run_lockstep_solve builds (p.ws, p.pol_ws: the route's forward block and the polish
// block), the carve is lockstep_chunk's / lockstep_direct_chunk's.  secs: what POL_END writes.  pol_max_steps (out): polish's step cap.  Weak as well.
struct LsBackProbe { LockstepDirectAdjointParams a; LockstepDirectParams p; bool polish, direct; int nops; const int *ops; double secs; int pol_max_steps; };
int test_lockstep_back(Dev &d, LsBackProbe &t) __attribute__((weak));
float time_kernel(Dev &d, int which, int reps);                             // mean ms per launch

}  // namespace be
}  // namespace osqp_hip
