#!/usr/bin/env python
"""Polish on the lockstep batch route with per-element matrices: what it costs, and the per-element loop it replaces, on handles of the same process.

Problem and batch: tools/lockstep_mat_bench.py's -- problems.banded_qp(n, window=40) at n = 400 and n = 2000, 64 / 256 elements, each with its own A
values, its own diagonal of P, its own q and bounds feasible by construction; eps --eps.
Measured per (n, B), with polishing off and on: wall ms of ONE hip_batch_solve_lockstep(Px=, Ax=) call (median of --reps after --warmup, with the
min-max spread); GPU ms of the ADMM part, of the preparation inside it (lockstep_mat_last_record) and of polish (lockstep_polish_last_record); launches
and PCG iterations of each part; attempted / accepted / rejected; GPU ms per launch of polish.  And the loop a caller had to run for polished points on
per-element matrices before: update(Px=, Ax=), update(q, l, u), solve() per element on ONE handle with polishing=True, timed on the first
min(B, --loop-sample) elements and scaled to B (one element after the other: linear in B by construction).

    python tools/lockstep_mat_polish_bench.py --out profiles/lockstep_mat_polish_bench.json
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import osqp_amd      # noqa: E402
import problems      # noqa: E402
from lockstep_mat_bench import batch      # noqa: E402


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
            row = dict(n=n, m=len(l), B=B, eps=a.eps)
            xp = None
            for name, pol in (('off', False), ('on', True)):
                s = osqp_amd.OSQP(algebra='hip')
                s.setup(P, q, A, l, u, polishing=pol, **st)
                wall, gpu, prep, pgpu = [], [], [], []
                for r in range(a.warmup + a.reps):
                    t0 = time.perf_counter()
                    x, y, rec = s._solver.hip_batch_solve_lockstep(q=Q, l=L, u=U, Px=Px, Ax=Ax)
                    wall.append(1e3 * (time.perf_counter() - t0))
                    last, plast = s._solver.lockstep_mat_last_record(), s._solver.lockstep_polish_last_record()
                    gpu.append(last['gpu_ms']); prep.append(last['prepare_gpu_ms']); pgpu.append(plast['gpu_ms'])
                wall, gpu, prep, pgpu = (np.array(v[a.warmup:]) for v in (wall, gpu, prep, pgpu))
                xp = x
                row[name] = dict(wall_ms=float(np.median(wall)), wall_ms_min=float(wall.min()), wall_ms_max=float(wall.max()),
                                 admm_gpu_ms=float(np.median(gpu)), prepare_gpu_ms=float(np.median(prep)),
                                 polish_gpu_ms=float(np.median(pgpu)), polish_gpu_ms_min=float(pgpu.min()), polish_gpu_ms_max=float(pgpu.max()),
                                 polish_gpu_ms_per_launch=float(np.median(pgpu) / plast['kernel_launches']) if plast['kernel_launches'] else 0.0,
                                 admm_gpu_ms_per_launch=float(np.median(gpu) / last['kernel_launches']),
                                 solved=int((rec[:, 0] == SOLVED).sum()), status_polish_1=int((rec[:, 8] == 1).sum()), status_polish_m1=int((rec[:, 8] == -1).sum()),
                                 prim_res_max=float(rec[:, 3].max()), dual_res_max=float(rec[:, 4].max()), admm=last, polish=plast)
            # the shared route's polish on the same (polishing) handle, the same q and the handle's own bounds (feasible on its own A), for the per-launch
            # figure: broadcast values in place of per-lane ones
            pg = []
            for r in range(a.warmup + a.reps):
                s._solver.hip_batch_solve_lockstep(q=Q)
                ps = s._solver.lockstep_polish_last_record()
                pg.append(ps['gpu_ms'])
            pg = np.array(pg[a.warmup:])
            row['shared_polish'] = dict(polish_gpu_ms=float(np.median(pg)), polish_gpu_ms_per_launch=float(np.median(pg) / ps['kernel_launches']) if ps['kernel_launches'] else 0.0, polish=ps)
            # the loop on one polishing handle (nn/torch.py::_loop: update(Px, Ax) + update(q, l, u) + solve() per element)
            h = osqp_amd.OSQP(algebra='hip')
            h.setup(P, q, A, l, u, polishing=True, **st)
            ns = min(B, a.loop_sample)
            tl, dev, npol = [], 0.0, 0
            for r in range(2):
                t0 = time.perf_counter()
                for b in range(ns):
                    h.update(Px=Px[b], Ax=Ax[b])
                    h.update(q=Q[b], l=L[b], u=U[b])
                    res = h.solve()
                    if r == 0:
                        dev = max(dev, float(np.abs(res.x - xp[b]).max() / (1 + np.abs(res.x).max())))
                        npol += int(res.info.status_polish == 1)
                tl.append(1e3 * (time.perf_counter() - t0) * B / ns)
            row['loop'] = dict(wall_ms=float(tl[1]), wall_ms_first=float(tl[0]), sample=ns, status_polish_1=npol, x_dev_vs_lockstep=dev)
            row['loop_over_lockstep_mat_polish'] = float(tl[1] / row['on']['wall_ms'])
            print(json.dumps(row), flush=True)
            rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/lockstep_mat_polish_bench.py', rows=rows), f, indent=1)


if __name__ == '__main__':
    main()
