#!/usr/bin/env python3
"""Direct lockstep adjoint (the backward pass of a direct lockstep batch on a Woodbury handle with a diagonal K0) against the forward call on the same
batch, on the same handle in the same process.  No other backward route takes such a handle, so the forward is the yardstick.

problems.portfolio_qp(na, k) (BASELINE configs[3]: n = na + k, m = na + k + 1, r = k + 1 dense rows), eps 1e-8, per-element q (mu redrawn).  The
forward (x, y) come from hip_batch_solve_lockstep_direct; the incoming gradient is dx = x - 0.1 noise, dy = 0 (what a loss on x sends back).
Per B: milliseconds per hip_batch_adjoint_lockstep_direct call and per hip_batch_solve_lockstep_direct call (each the median of --reps after --warmup,
with the min-max spread), their ratio, and from lockstep_direct_adjoint_last_record: chunks, recurrence steps of the slowest element, inversions of
S, kernel launches, GPU ms; the elements with status 0, the step counts and the record residuals.

    python tools/lockstep_direct_adjoint_bench.py --out profiles/lockstep_direct_adjoint_bench.json
    python tools/lockstep_direct_adjoint_bench.py --na 2000 --k 127 --batches 64 --out profiles/lockstep_direct_adjoint_bench.json --append
"""
import argparse
import json
import os
import sys
import time

import numpy as np

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--na', type=int, default=2000)
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--batches', type=int, nargs='+', default=[64, 256, 1024])
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None)
    ap.add_argument('--append', action='store_true', help='keep the rows --out already holds (another shape: --na / --k)')
    a = ap.parse_args()
    P, q, A, l, u = problems.portfolio_qp(a.na, a.k)
    n, m = len(q), len(l)
    s = osqp_amd.OSQP(algebra='hip')
    s.setup(P, q, A, l, u, verbose=False, eps_abs=1e-8, eps_rel=1e-8, max_iter=50000, warm_starting=False)
    ext = s._solver
    r = int(ext.hip_stats()['woodbury_rows'])
    rows = []
    for B in a.batches:
        rng = np.random.default_rng(1)
        Q = np.stack([np.concatenate([-rng.standard_normal(a.na), np.zeros(a.k)]) for _ in range(B)])
        tf, (x, y, rec) = timed(lambda: ext.hip_batch_solve_lockstep_direct(q=Q), a.warmup, a.reps)
        fwd = ext.lockstep_direct_last_record()
        solved = int((rec[:, 0] == int(osqp_amd.SolverStatus.OSQP_SOLVED)).sum())
        dx = x - 0.1 * np.random.default_rng(2).standard_normal(x.shape)
        tb, g = timed(lambda: ext.hip_batch_adjoint_lockstep_direct(x, y, dx), a.warmup, a.reps)
        last = ext.lockstep_direct_adjoint_last_record()
        ar = g['rec']
        ok = ar[:, 0] == 0
        row = dict(n=n, m=m, r=r, B=B, backward_ms=float(np.median(tb)), backward_ms_min=float(tb.min()), backward_ms_max=float(tb.max()),
                   forward_ms=float(np.median(tf)), forward_ms_min=float(tf.min()), forward_ms_max=float(tf.max()), backward_over_forward=float(np.median(tb) / np.median(tf)),
                   forward_solved=solved, forward_admm_iters_max=fwd['admm_iters_max'], forward_gpu_ms=fwd['gpu_ms'], status0=int(ok.sum()),
                   steps_min=int(ar[:, 3].min()), steps_median=float(np.median(ar[:, 3])), residual_max_status0=float(ar[ok, 2].max()) if ok.any() else None,
                   residual_median=float(np.median(ar[:, 2])), active_rows_min=int(ar[:, 1].min()), active_rows_max=int(ar[:, 1].max()),
                   launches_per_step=last['kernel_launches'] / max(last['chunks'], 1) / max(last['steps_max'], 1), **last)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        if a.append and os.path.exists(a.out):
            with open(a.out) as f:
                rows = json.load(f)['rows'] + rows
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/lockstep_direct_adjoint_bench.py', problem='portfolio_qp(na, k): n = na + k, r = k + 1', eps=1e-8, rows=rows), f, indent=1)


if __name__ == '__main__':
    main()
