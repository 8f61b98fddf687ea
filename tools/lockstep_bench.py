#!/usr/bin/env python
"""Lockstep batch route against the sequential update + solve loop, on the same handle in the same process.

Problems: problems.banded_qp(n, window=40) for n in --sizes, q / l / u perturbed per element, eps 1e-6; batches of --batches elements.
Per (n, B): milliseconds per batch through hip_batch_solve_lockstep (median of --reps after --warmup, with the min-max spread) and through the
loop `update(q, l, u); solve()` over the elements.  The loop is timed on the first min(B, --loop-sample) elements and scaled to B (it is linear in
B by construction: one element after the other); the sample size is written next to the number.  Also reported per (n, B): chunks, ADMM iterations
of the slowest element, PCG iterations, kernel launches, GPU ms (lockstep_last_record), and the bytes one product launch moves at the least
(matrix once + one block vector in, one out) next to the mean time of a launch.  Per-kernel times come from a `rocprofv3 --kernel-trace --stats`
run of this script with one size and one batch (k_ls_kp and k_ls_t are the two product kernels of a PCG iteration).

    python tools/lockstep_bench.py --out profiles/lockstep_bench.json
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
    ap.add_argument('--sizes', type=int, nargs='+', default=[500, 2000, 8000])
    ap.add_argument('--batches', type=int, nargs='+', default=[8, 64, 256, 1024])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--loop-sample', type=int, default=32)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rows = []
    for n in a.sizes:
        P, q, A, l, u = problems.banded_qp(n, window=40)
        m = len(l)
        s = osqp_amd.OSQP(algebra='hip')
        s.setup(P, q, A, l, u, verbose=False, eps_abs=1e-6, eps_rel=1e-6, max_iter=20000, warm_starting=False)
        nnzA, nnzB = A.nnz, (P + P.T).nnz + A.nnz
        for B in a.batches:
            Q, L, U = batch(q, l, u, B)
            ts = []
            for r in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                x, y, rec = s._solver.hip_batch_solve_lockstep(q=Q, l=L, u=U)
                ts.append(1e3 * (time.perf_counter() - t0))
            ts = np.array(ts[a.warmup:])
            last = s._solver.lockstep_last_record()
            solved = int((rec[:, 0] == int(osqp_amd.SolverStatus.OSQP_SOLVED)).sum())
            ns = min(B, a.loop_sample)
            tl, dev = [], 0.0
            for r in range(1 + max(1, a.reps // 2)):
                t0 = time.perf_counter()
                for b in range(ns):
                    s.update(q=Q[b], l=L[b], u=U[b])
                    res = s.solve()
                    if r == 0:
                        dev = max(dev, float(np.abs(res.x - x[b]).max() / (1 + np.abs(res.x).max())))
                tl.append(1e3 * (time.perf_counter() - t0) * B / ns)
            tl = np.array(tl[1:])
            # least traffic of one product launch over B = [P + sigma I | A'] with a full chunk: 12 bytes per entry + n + m rows in, n rows out, 512 bytes each
            bytes_b = 12 * nnzB + 512 * (2 * n + m)
            row = dict(n=n, m=m, B=B, lockstep_ms=float(np.median(ts)), lockstep_ms_min=float(ts.min()), lockstep_ms_max=float(ts.max()),
                       loop_ms=float(np.median(tl)), loop_ms_min=float(tl.min()), loop_ms_max=float(tl.max()), loop_sample=ns,
                       speedup=float(np.median(tl) / np.median(ts)), solved=solved, x_dev_vs_loop=dev, nnzA=int(nnzA), nnzB=int(nnzB),
                       product_B_min_bytes=int(bytes_b), mean_launch_us=1e3 * last['gpu_ms'] / max(last['kernel_launches'], 1), **last)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/lockstep_bench.py', eps=1e-6, rows=rows), f, indent=1)


if __name__ == '__main__':
    main()
