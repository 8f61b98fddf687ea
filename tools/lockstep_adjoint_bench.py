#!/usr/bin/env python
"""Lockstep adjoint (the backward pass of a lockstep batch) against the per-element loop, on the same handle in the same process.

Problems: problems.banded_qp(n, window=40) for n in --sizes, q / l / u perturbed per element, eps 1e-8; batches of --batches elements.  The forward
(x, y) come from one hip_batch_solve_lockstep call; the incoming gradient is dx = x - 0.1 noise, dy = 0 (what a loss on x sends back).
Per (n, B): milliseconds per hip_batch_adjoint_lockstep call (median of --reps after --warmup, with the min-max spread) and through the loop the torch
layer ran before this route existed -- update(l, u) + adjoint_derivative_compute_at + the two getters, one element after the other.  The loop is timed
on the first min(B, --loop-sample) elements and scaled to B (it is linear in B by construction); the sample size is written next to the number.  Also
per (n, B): chunks, recurrence steps of the slowest element, PCG iterations, kernel launches, GPU ms (lockstep_adjoint_last_record), the elements with
status 0, and the largest relative deviation of dq between the two routes on the sampled elements.

    python tools/lockstep_adjoint_bench.py --out profiles/lockstep_adjoint_bench.json
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


def batch(q, l, u, nb, seed=1):
    rng = np.random.default_rng(seed)
    return (np.stack([q + 0.05 * rng.standard_normal(len(q)) for _ in range(nb)]), np.stack([l - 0.01 * (b % 64) for b in range(nb)]),
            np.stack([u + 0.01 * (b % 64) for b in range(nb)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[500, 2000])
    ap.add_argument('--batches', type=int, nargs='+', default=[8, 64, 256])
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--loop-sample', type=int, default=8)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rows = []
    for n in a.sizes:
        P, q, A, l, u = problems.banded_qp(n, window=40)
        s = osqp_amd.OSQP(algebra='hip')
        s.setup(P, q, A, l, u, verbose=False, eps_abs=1e-8, eps_rel=1e-8, max_iter=50000, warm_starting=False)
        ext = s._solver
        m = len(l)
        for B in a.batches:
            Q, L, U = batch(q, l, u, B)
            x, y, rec = ext.hip_batch_solve_lockstep(q=Q, l=L, u=U)
            solved = int((rec[:, 0] == int(osqp_amd.SolverStatus.OSQP_SOLVED)).sum())
            dx = x - 0.1 * np.random.default_rng(2).standard_normal(x.shape)
            ts = []
            for r in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                g = ext.hip_batch_adjoint_lockstep(x, y, dx, None, l=L, u=U)
                ts.append(1e3 * (time.perf_counter() - t0))
            ts = np.array(ts[a.warmup:])
            last = ext.lockstep_adjoint_last_record()
            ns = min(B, a.loop_sample)
            tl, dev = [], 0.0
            for r in range(2):                                                  # one warm-up pass, one timed
                t0 = time.perf_counter()
                for b in range(ns):
                    s.update(l=L[b], u=U[b])
                    st = ext.adjoint_derivative_compute_at(x[b], y[b], dx[b])
                    dP, dA = s.ext.CSC(s._derivative_cache['P'].copy()), s.ext.CSC(s._derivative_cache['A'].copy())
                    dq, dl, du = np.empty(n), np.zeros(m), np.zeros(m)
                    st = st or ext.adjoint_derivative_get_mat(dP, dA) or ext.adjoint_derivative_get_vec(dq, dl, du)
                    if r == 0 and not st:
                        dev = max(dev, float(np.abs(dq - g['dq'][b]).max() / (1e-300 + np.abs(dq).max())))
                tl.append(1e3 * (time.perf_counter() - t0) * B / ns)
            s.update(l=l, u=u)
            row = dict(n=n, m=m, B=B, lockstep_ms=float(np.median(ts)), lockstep_ms_min=float(ts.min()), lockstep_ms_max=float(ts.max()),
                       loop_ms=float(tl[1]), loop_sample=ns, ratio=float(tl[1] / np.median(ts)), forward_solved=solved,
                       status0=int((g['rec'][:, 0] == 0).sum()), residual_max=float(g['rec'][:, 2].max()), dq_dev_vs_loop=dev, **last)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/lockstep_adjoint_bench.py', eps=1e-8, rows=rows), f, indent=1)


if __name__ == '__main__':
    main()
