#!/usr/bin/env python3
"""Polish on the direct lockstep route: what it costs, and the two forms of its recurrence's dense-row refresh, each case in a child process of its own.

problems.portfolio_qp(na, k) (n = na + k, m = na + k + 1, r = k + 1 dense rows), eps 1e-6, B elements with q redrawn per element (default_rng(1)) --
with the handle's matrices ("shared") and with per-element values (default_rng(3): Ax = A.data (1 + 0.1 N(0, 1)), then Px = triu(P).data (1 + 0.2 U(0, 1)),
as tools/lockstep_direct_mat_bench.py draws them, "mat").
Cases per shape: polishing off; polishing on with OSQP_HIP_LS_POL_PROD2=0 (the dense rows of x and x~ by two k_lw_prod launches per step) and =1 (one
k_lw_prod2 launch, the default).  The switch is read once per process, so every case runs in a child; the children of a shape are run --repeats times,
INTERLEAVED (off, prod2=0, prod2=1, off, ...), and a case's figure is the median over its children of the child's own median over --reps calls after
--warmup.  Columns: wall ms, ADMM GPU ms (lockstep_direct_last_record), polish GPU ms, recurrence steps of the slowest problem, polish launches,
accepted / rejected (lockstep_polish_last_record).

    python tools/lockstep_direct_polish_bench.py --out profiles/lockstep_direct_polish_bench.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'osqp-python_amd'))
sys.path.insert(0, ROOT)

CASES = (('off', False, None), ('on_prod2_0', True, '0'), ('on_prod2_1', True, '1'))


def child(a):
    import osqp_amd
    import problems
    P, q, A, l, u = problems.portfolio_qp(a.na, a.k)
    P, A = sp.csc_matrix(sp.triu(P)), sp.csc_matrix(A)
    P.sort_indices(); A.sort_indices()
    s = osqp_amd.OSQP(algebra='hip')
    s.setup(P, q, A, l, u, verbose=False, eps_abs=1e-6, eps_rel=1e-6, max_iter=20000, warm_starting=False, polishing=bool(a.polishing))
    B = a.batch
    rng = np.random.default_rng(1)
    kw = dict(q=np.stack([np.concatenate([-rng.standard_normal(a.na), np.zeros(a.k)]) for _ in range(B)]))
    if a.mat:
        rng = np.random.default_rng(3)
        kw['Ax'] = A.data * (1.0 + 0.1 * rng.standard_normal((B, A.nnz)))
        kw['Px'] = P.data * (1.0 + 0.2 * rng.random((B, P.nnz)))
    wall, gpu, pgpu = [], [], []
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        x, y, rec = s._solver.hip_batch_solve_lockstep_direct(**kw)
        wall.append(1e3 * (time.perf_counter() - t0))
        gpu.append(s._solver.lockstep_direct_last_record()['gpu_ms']); pgpu.append(s._solver.lockstep_polish_last_record()['gpu_ms'])
    wall, gpu, pgpu = (np.array(v[a.warmup:]) for v in (wall, gpu, pgpu))
    last, plast = s._solver.lockstep_direct_last_record(), s._solver.lockstep_polish_last_record()
    print('RESULT ' + json.dumps(dict(n=len(q), m=len(l), r=int(s._solver.hip_stats()['woodbury_rows']), B=B, wall_ms=float(np.median(wall)), admm_gpu_ms=float(np.median(gpu)),
                                      polish_gpu_ms=float(np.median(pgpu)), polish_gpu_ms_min=float(pgpu.min()), polish_gpu_ms_max=float(pgpu.max()),
                                      steps=plast['steps_max'], polish_launches=plast['kernel_launches'], accepted=plast['accepted'], rejected=plast['rejected'],
                                      solved=int((rec[:, 0] == int(osqp_amd.SolverStatus.OSQP_SOLVED)).sum()), admm_launches=last['kernel_launches'],
                                      prim_res_max=float(rec[:, 3].max()), dual_res_max=float(rec[:, 4].max()))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--na', type=int, default=2000)
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=3, help='children per case, interleaved')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--mat', type=int, default=0)
    ap.add_argument('--polishing', type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = []
    for mat in (0, 1):
        runs = {name: [] for name, _, _ in CASES}
        for rep in range(a.repeats):
            for name, pol, flag in CASES:
                env = dict(os.environ)
                env.pop('OSQP_HIP_LS_POL_PROD2', None)
                if flag is not None:
                    env['OSQP_HIP_LS_POL_PROD2'] = flag
                cmd = [sys.executable, os.path.abspath(__file__), '--child', '--mat', str(mat), '--polishing', str(int(pol)), '--na', str(a.na), '--k', str(a.k),
                       '--batch', str(a.batch), '--reps', str(a.reps), '--warmup', str(a.warmup)]
                o = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
                if o.returncode != 0:
                    sys.exit('child %s failed (%d): %s' % (name, o.returncode, o.stderr[-2000:]))
                runs[name].append(json.loads([ln for ln in o.stdout.splitlines() if ln.startswith('RESULT ')][-1][7:]))
        row = dict(matrices='per-problem' if mat else 'shared')
        for name, rs in runs.items():
            med = {k: (float(np.median([r[k] for r in rs])) if isinstance(rs[0][k], float) else rs[0][k]) for k in rs[0]}
            med['polish_gpu_ms_children'] = [r['polish_gpu_ms'] for r in rs]
            row[name] = med
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/lockstep_direct_polish_bench.py', problem='portfolio_qp(%d, %d), B = %d' % (a.na, a.k, a.batch), eps=1e-6, repeats=a.repeats, reps=a.reps, rows=rows), f, indent=1)


if __name__ == '__main__':
    main()
