#!/usr/bin/env python
"""Per-element matrices on the lockstep batch route against the per-element loop it replaces, on handles of the same process.

Problem: problems.banded_qp(n, window=40) at n = 400 and n = 2000; a batch of 64 / 256 elements, each with its own A values (x (1 + 0.1 N(0,1))), its own
diagonal of P (x (1 + 0.2 U(0,1))), its own q and bounds that are feasible by construction (tests/test_gpu_lockstep_mat.py's recipe), eps --eps.
Measured per (n, B): wall and GPU ms of ONE hip_batch_solve_lockstep(Px=, Ax=) call (median of --reps after --warmup), its launches and the share of the GPU
time spent in assembly + equilibration (lockstep_mat_last_record); and the loop the torch layer's default path runs for such a batch --
update(Px=, Ax=), update(q, l, u), solve() per element on ONE handle -- timed on the first min(B, --loop-sample) elements and scaled to B (one element
after the other: linear in B by construction); max |dx| between the two over the sampled elements, relative to the solution's scale.

    python tools/lockstep_mat_bench.py --out profiles/lockstep_mat_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'osqp-python_amd'))
sys.path.insert(0, ROOT)
import osqp_amd      # noqa: E402
import problems      # noqa: E402


def batch(P, q, A, l, u, B, seed=3):
    """(Px, Ax, Q, L, U) of B elements on the pattern of (triu P, A)."""
    n, m = len(q), len(l)
    Pu = sp.triu(P, format='csc'); Pu.sort_indices()
    rng = np.random.default_rng(seed)
    Ax = A.data * (1 + 0.1 * rng.standard_normal((B, A.nnz)))
    diag = np.repeat(np.arange(n), np.diff(Pu.indptr)) == Pu.indices
    Px = np.tile(Pu.data, (B, 1))
    Px[:, diag] *= 1 + 0.2 * rng.random((B, int(diag.sum())))
    Q = q + 0.05 * rng.standard_normal((B, n))
    xh = rng.standard_normal(n)
    s = 1 + rng.random(m)
    eq = l == u
    Z = np.stack([sp.csc_matrix((Ax[b], A.indices, A.indptr), shape=A.shape) @ xh for b in range(B)])
    return Px, Ax, Q, np.where(eq, Z, Z - s), np.where(eq, Z, Z + s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[400, 2000])
    ap.add_argument('--batches', type=int, nargs='+', default=[64, 256])
    ap.add_argument('--eps', type=float, default=1e-5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--loop-sample', type=int, default=16)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    SOLVED = int(osqp_amd.SolverStatus.OSQP_SOLVED)
    st = dict(verbose=False, eps_abs=a.eps, eps_rel=a.eps, max_iter=20000, warm_starting=False)
    rows = []
    for n in a.sizes:
        P, q, A, l, u = problems.banded_qp(n, window=40)
        A = sp.csc_matrix(A); A.sort_indices()
        for B in a.batches:
            Px, Ax, Q, L, U = batch(P, q, A, l, u, B)
            s = osqp_amd.OSQP(algebra='hip')
            s.setup(P, q, A, l, u, **st)
            wall, gpu, prep = [], [], []
            for r in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                x, y, rec = s._solver.hip_batch_solve_lockstep(q=Q, l=L, u=U, Px=Px, Ax=Ax)
                wall.append(1e3 * (time.perf_counter() - t0))
                last = s._solver.lockstep_mat_last_record()
                gpu.append(last['gpu_ms']); prep.append(last['prepare_gpu_ms'])
            wall, gpu, prep = (np.array(v[a.warmup:]) for v in (wall, gpu, prep))
            row = dict(n=n, m=len(l), B=B, eps=a.eps,
                       lockstep_mat=dict(wall_ms=float(np.median(wall)), wall_ms_min=float(wall.min()), wall_ms_max=float(wall.max()), gpu_ms=float(np.median(gpu)),
                                         prepare_gpu_ms=float(np.median(prep)), prepare_share=float(np.median(prep) / np.median(gpu)), kernel_launches=last['kernel_launches'],
                                         admm_iters_max=last['admm_iters_max'], pcg_iters=last['pcg_iters'], matrix_block_bytes=last['matrix_block_bytes'],
                                         solved=int((rec[:, 0] == SOLVED).sum())))
            # the loop on one handle (nn/torch.py::_loop: update(Px, Ax) + update(q, l, u) + solve() per element)
            h = osqp_amd.OSQP(algebra='hip')
            h.setup(P, q, A, l, u, **st)
            ns = min(B, a.loop_sample)
            tl, dev, nsolved = [], 0.0, 0
            for r in range(2):
                t0 = time.perf_counter()
                for b in range(ns):
                    h.update(Px=Px[b], Ax=Ax[b])
                    h.update(q=Q[b], l=L[b], u=U[b])
                    res = h.solve()
                    if r == 0:
                        dev = max(dev, float(np.abs(res.x - x[b]).max() / (1 + np.abs(res.x).max())))
                        nsolved += int(res.info.status_val == SOLVED)
                tl.append(1e3 * (time.perf_counter() - t0) * B / ns)
            row['loop'] = dict(wall_ms=float(tl[1]), wall_ms_first=float(tl[0]), sample=ns, solved_of_sample=nsolved)
            row['x_dev_max'] = dev
            row['loop_over_lockstep_mat'] = float(tl[1] / np.median(wall))
            print(json.dumps(row), flush=True)
            rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/lockstep_mat_bench.py', rows=rows), f, indent=1)


if __name__ == '__main__':
    main()
