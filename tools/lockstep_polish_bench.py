#!/usr/bin/env python
"""Polish on the lockstep batch route: what it costs, and the per-element loop it replaces, on handles of the same process.

Problem: problems.banded_qp(n, window=40), q / l / u perturbed per element as tools/lockstep_bench.py does, eps --eps; one batch of --batch elements.
Measured: GPU ms (lockstep_last_record + lockstep_polish_last_record) and wall ms of hip_batch_solve_lockstep with polishing off and on (median of
--reps after --warmup, with the min-max spread); the polish's recurrence steps, PCG iterations, launches and accept / reject counts from the polish
record; and the loop `update(q, l, u); solve()` over the elements on ONE handle with polishing=True -- what a caller had to run for polished points
before.  The loop is timed on the first min(B, --loop-sample) elements and scaled to B (one element after the other: linear in B by construction).

    python tools/lockstep_polish_bench.py --out profiles/lockstep_polish_bench.json
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
from lockstep_bench import batch      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=2000)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--eps', type=float, default=1e-4)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--loop-sample', type=int, default=16)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    n, B = a.size, a.batch
    P, q, A, l, u = problems.banded_qp(n, window=40)
    Q, L, U = batch(q, l, u, B)
    st = dict(verbose=False, eps_abs=a.eps, eps_rel=a.eps, max_iter=20000, warm_starting=False)
    SOLVED = int(osqp_amd.SolverStatus.OSQP_SOLVED)
    row = dict(n=n, m=len(l), B=B, eps=a.eps)
    keep = {}
    for name, pol in (('off', False), ('on', True)):
        s = osqp_amd.OSQP(algebra='hip')
        s.setup(P, q, A, l, u, polishing=pol, **st)
        wall, gpu, pgpu = [], [], []
        for r in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            x, y, rec = s._solver.hip_batch_solve_lockstep(q=Q, l=L, u=U)
            wall.append(1e3 * (time.perf_counter() - t0))
            gpu.append(s._solver.lockstep_last_record()['gpu_ms']); pgpu.append(s._solver.lockstep_polish_last_record()['gpu_ms'])
        wall, gpu, pgpu = (np.array(v[a.warmup:]) for v in (wall, gpu, pgpu))
        last, plast = s._solver.lockstep_last_record(), s._solver.lockstep_polish_last_record()
        keep[name] = (x, y, rec)
        row[name] = dict(wall_ms=float(np.median(wall)), wall_ms_min=float(wall.min()), wall_ms_max=float(wall.max()),
                         admm_gpu_ms=float(np.median(gpu)), polish_gpu_ms=float(np.median(pgpu)), polish_gpu_ms_min=float(pgpu.min()), polish_gpu_ms_max=float(pgpu.max()),
                         solved=int((rec[:, 0] == SOLVED).sum()), status_polish_1=int((rec[:, 8] == 1).sum()), status_polish_m1=int((rec[:, 8] == -1).sum()),
                         prim_res_max=float(rec[:, 3].max()), dual_res_max=float(rec[:, 4].max()), admm=last, polish=plast)
        print(json.dumps({name: row[name]}), flush=True)
    # the loop on one polishing handle
    s = osqp_amd.OSQP(algebra='hip')
    s.setup(P, q, A, l, u, polishing=True, **st)
    ns = min(B, a.loop_sample)
    tl, dev, npol = [], 0.0, 0
    xp = keep['on'][0]
    for r in range(2):
        t0 = time.perf_counter()
        for b in range(ns):
            s.update(q=Q[b], l=L[b], u=U[b])
            res = s.solve()
            if r == 0:
                dev = max(dev, float(np.abs(res.x - xp[b]).max() / (1 + np.abs(res.x).max())))
                npol += int(res.info.status_polish == 1)
        tl.append(1e3 * (time.perf_counter() - t0) * B / ns)
    row['loop'] = dict(wall_ms=float(tl[1]), wall_ms_first=float(tl[0]), sample=ns, status_polish_1=npol, x_dev_vs_lockstep=dev)
    print(json.dumps({'loop': row['loop']}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/lockstep_polish_bench.py', **row), f, indent=1)


if __name__ == '__main__':
    main()
