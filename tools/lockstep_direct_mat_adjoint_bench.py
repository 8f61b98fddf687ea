#!/usr/bin/env python3
"""Direct lockstep adjoint with PER-PROBLEM MATRICES (the backward pass of a batch of factor-model QPs with one factor model per element, on a Woodbury handle
with a diagonal K0).  No other backward route takes such a batch, so the yardsticks are the forward call with per-element matrices and the shared-matrix
direct adjoint, both on the same handle and batch size in the same process.

problems.portfolio_qp(na, k) (n = na + k, m = na + k + 1, r = k + 1 dense rows), eps 1e-8, per-element q (mu redrawn) and tests/test_gpu_lockstep_direct_mat.py's
perturbation: rng = default_rng(3), Ax = A.data (1 + 0.1 N(0, 1)), then Px = triu(P).data (1 + 0.2 U(0, 1)).  The forward (x, y) come from
hip_batch_solve_lockstep_direct(Px=, Ax=); the incoming gradient is dx = x - 0.1 noise, dy = 0 (what a loss on x sends back).
Per B: milliseconds per hip_batch_adjoint_lockstep_direct(Px=, Ax=) call, per forward call with per-element matrices and per shared direct adjoint call
(each the median of --reps after --warmup, with the min-max spread), and from lockstep_direct_mat_adjoint_last_record: chunks, steps of the slowest element,
inversions of S, kernel launches, GPU ms, GPU ms of the preparation.
(profiles/lockstep_direct_mat_adjoint_prod2_ab.json is the output of an earlier form of this tool that held two handles, one launching the two dense-row
products of a step separately and one through a fused kernel that was measured and not kept: DESIGN.md section 6.)

    python tools/lockstep_direct_mat_adjoint_bench.py --na 2000 --k 4 --out profiles/lockstep_direct_mat_adjoint_bench.json
    python tools/lockstep_direct_mat_adjoint_bench.py --na 2000 --k 127 --batches 64 --out profiles/lockstep_direct_mat_adjoint_bench.json --append
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


def timed(call, warmup, reps):
    ts, out = [], None
    for _ in range(warmup + reps):
        t0 = time.perf_counter()
        out = call()
        ts.append(1e3 * (time.perf_counter() - t0))
    return np.array(ts[warmup:]), out


def stats(prefix, t):
    return {prefix + '_ms': float(np.median(t)), prefix + '_ms_min': float(t.min()), prefix + '_ms_max': float(t.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--na', type=int, default=2000)
    ap.add_argument('--k', type=int, default=4)
    ap.add_argument('--batches', type=int, nargs='+', default=[64, 256])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None)
    ap.add_argument('--append', action='store_true', help='keep the rows --out already holds (another shape: --na / --k)')
    a = ap.parse_args()
    P, q, A, l, u = problems.portfolio_qp(a.na, a.k)
    P, A = sp.csc_matrix(sp.triu(P)), sp.csc_matrix(A)
    P.sort_indices(); A.sort_indices()
    n, m = len(q), len(l)
    s = osqp_amd.OSQP(algebra='hip')
    s.setup(P, q, A, l, u, verbose=False, eps_abs=1e-8, eps_rel=1e-8, max_iter=50000, warm_starting=False)
    ext = s._solver
    r = int(ext.hip_stats()['woodbury_rows'])
    SOLVED = int(osqp_amd.SolverStatus.OSQP_SOLVED)
    rows = []
    for B in a.batches:
        rng = np.random.default_rng(1)
        Q = np.stack([np.concatenate([-rng.standard_normal(a.na), np.zeros(a.k)]) for _ in range(B)])
        rng = np.random.default_rng(3)
        Ax = A.data * (1.0 + 0.1 * rng.standard_normal((B, A.nnz)))
        Px = P.data * (1.0 + 0.2 * rng.random((B, P.nnz)))
        noise = 0.1 * np.random.default_rng(2).standard_normal((B, n))
        tf, (x, y, rec) = timed(lambda: ext.hip_batch_solve_lockstep_direct(q=Q, Px=Px, Ax=Ax), a.warmup, a.reps)
        fwd = ext.lockstep_direct_mat_last_record()
        dx = x - noise
        tb, g = timed(lambda: ext.hip_batch_adjoint_lockstep_direct(x, y, dx, Px=Px, Ax=Ax), a.warmup, a.reps)
        last = ext.lockstep_direct_mat_adjoint_last_record()
        xs, ys, recs = ext.hip_batch_solve_lockstep_direct(q=Q)
        dxs = xs - noise
        ts, gs = timed(lambda: ext.hip_batch_adjoint_lockstep_direct(xs, ys, dxs), a.warmup, a.reps)
        shared = ext.lockstep_direct_adjoint_last_record()
        ar = g['rec']
        ok = ar[:, 0] == 0
        row = dict(n=n, m=m, r=r, B=B, **stats('backward', tb), **stats('forward_mat', tf), **stats('shared_adjoint', ts),
                   backward_over_forward=float(np.median(tb) / np.median(tf)), mat_over_shared_adjoint=float(np.median(tb) / np.median(ts)),
                   forward_solved=int((rec[:, 0] == SOLVED).sum()), forward_admm_iters_max=fwd['admm_iters_max'], forward_gpu_ms=fwd['gpu_ms'],
                   shared_forward_solved=int((recs[:, 0] == SOLVED).sum()), shared_status0=int((gs['rec'][:, 0] == 0).sum()), shared_steps_max=shared['steps_max'],
                   shared_kernel_launches=shared['kernel_launches'], shared_gpu_ms=shared['gpu_ms'],
                   status0=int(ok.sum()), steps_min=int(ar[:, 3].min()), steps_median=float(np.median(ar[:, 3])),
                   residual_max_status0=float(ar[ok, 2].max()) if ok.any() else None, active_rows_min=int(ar[:, 1].min()), active_rows_max=int(ar[:, 1].max()),
                   **last)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        if a.append and os.path.exists(a.out):
            with open(a.out) as f:
                rows = json.load(f)['rows'] + rows
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/lockstep_direct_mat_adjoint_bench.py', problem='portfolio_qp(na, k): n = na + k, r = k + 1; Px, Ax per element', eps=1e-8, rows=rows), f, indent=1)


if __name__ == '__main__':
    main()
