#!/usr/bin/env python3
"""Direct lockstep route with PER-PROBLEM MATRICES against what the handle otherwise offers such a batch: update(Px, Ax, q) + solve() per element, on the
same handle in the same process.

problems.portfolio_qp(na, k) (n = na + k, m = na + k + 1, r = k + 1 dense rows), eps 1e-6, per-element q (mu redrawn) and per-element matrix values:
rng = default_rng(3), Ax = A.data (1 + 0.1 N(0, 1)), then Px = triu(P).data (1 + 0.2 U(0, 1)), per element and entry (tests/test_gpu_lockstep_direct_mat.py).
Per B: milliseconds per batch through hip_batch_solve_lockstep_direct(Px=, Ax=) (median of --reps after --warmup, with the min-max spread) and through
the loop (--loop-sample elements, one warm-up pass, median of --reps passes with the min-max spread, scaled to B), QP/s of both, and from
lockstep_direct_mat_last_record: chunks, ADMM iterations of the slowest element, inversions of S, kernel launches, GPU ms, the block's bytes and the
GPU ms of the preparation (assembly + equilibration + the fill of the dense rows) -- so launches and microseconds per ADMM iteration.  Per-kernel times
come from a kernel trace of one call:
    rocprofv3 --kernel-trace --stats -- python tools/lockstep_direct_mat_bench.py --batches 64 --reps 1 --warmup 0 --loop-sample 0

    python tools/lockstep_direct_mat_bench.py --out profiles/lockstep_direct_mat_bench.json
    python tools/lockstep_direct_mat_bench.py --na 2000 --k 127 --batches 64 --out profiles/lockstep_direct_mat_bench.json --append
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--na', type=int, default=2000)
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--batches', type=int, nargs='+', default=[64, 256])
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--loop-sample', type=int, default=32)
    ap.add_argument('--out', default=None)
    ap.add_argument('--append', action='store_true', help='keep the rows --out already holds (another shape: --na / --k)')
    a = ap.parse_args()
    P, q, A, l, u = problems.portfolio_qp(a.na, a.k)
    P, A = sp.csc_matrix(sp.triu(P)), sp.csc_matrix(A)
    P.sort_indices(); A.sort_indices()
    n, m = len(q), len(l)
    s = osqp_amd.OSQP(algebra='hip')
    s.setup(P, q, A, l, u, verbose=False, eps_abs=1e-6, eps_rel=1e-6, max_iter=20000, warm_starting=False)
    r = int(s._solver.hip_stats()['woodbury_rows'])
    SOLVED = int(osqp_amd.SolverStatus.OSQP_SOLVED)
    rows = []
    for B in a.batches:
        rng = np.random.default_rng(1)
        Q = np.stack([np.concatenate([-rng.standard_normal(a.na), np.zeros(a.k)]) for _ in range(B)])
        rng = np.random.default_rng(3)
        Ax = A.data * (1.0 + 0.1 * rng.standard_normal((B, A.nnz)))
        Px = P.data * (1.0 + 0.2 * rng.random((B, P.nnz)))
        ts = []
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            x, y, rec = s._solver.hip_batch_solve_lockstep_direct(q=Q, Px=Px, Ax=Ax)
            ts.append(1e3 * (time.perf_counter() - t0))
        ts = np.array(ts[a.warmup:])
        last = s._solver.lockstep_direct_mat_last_record()
        per = max(last['chunks'], 1) * max(last['admm_iters_max'], 1)
        row = dict(n=n, m=m, r=r, B=B, mat_ms=float(np.median(ts)), mat_ms_min=float(ts.min()), mat_ms_max=float(ts.max()),
                   mat_qp_per_s=float(1e3 * B / np.median(ts)), solved=int((rec[:, 0] == SOLVED).sum()), iters_mean=float(rec[:, 1].mean()),
                   launches_per_iter=last['kernel_launches'] / per, us_per_admm_iter=1e3 * (last['gpu_ms'] - last['prepare_gpu_ms']) / per,
                   prepare_gpu_ms_per_chunk=last['prepare_gpu_ms'] / max(last['chunks'], 1), **last)
        ns = min(B, a.loop_sample)
        if ns > 0:
            tl, dev, it, ok = [], 0.0, [], 0
            rho = s.settings.rho
            for rep in range(1 + a.reps):                  # (the first pass warms the loop up and gives the deviation and the iteration counts)
                t0 = time.perf_counter()
                for b in range(ns):
                    s.update(Px=Px[b], Ax=Ax[b], q=Q[b])
                    res = s.solve()
                    if rep == 0:
                        dev = max(dev, float(np.abs(res.x - x[b]).max() / (1 + np.abs(res.x).max()))); it.append(res.info.iter); ok += int(res.info.status_val == SOLVED)
                tl.append(1e3 * (time.perf_counter() - t0) * B / ns)
            tl = np.array(tl[1:])
            s.update(Px=P.data, Ax=A.data, q=q); s.update_settings(rho=rho)      # (the handle's own data back, for the next B)
            row.update(loop_ms=float(np.median(tl)), loop_ms_min=float(tl.min()), loop_ms_max=float(tl.max()), loop_sample=ns, loop_solved=ok, loop_qp_per_s=float(1e3 * B / np.median(tl)),
                       loop_ms_per_element=float(np.median(tl) / B), loop_iters_mean=float(np.mean(it)), speedup=float(np.median(tl) / np.median(ts)),
                       medians_apart=bool(ts.max() < tl.min() or tl.max() < ts.min()), x_dev_vs_loop=dev)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        if a.append and os.path.exists(a.out):
            with open(a.out) as f:
                rows = json.load(f)['rows'] + rows
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/lockstep_direct_mat_bench.py', problem='portfolio_qp(na, k): n = na + k, r = k + 1; Px, Ax per element', eps=1e-6, rows=rows), f, indent=1)


if __name__ == '__main__':
    main()
