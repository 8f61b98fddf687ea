#!/usr/bin/env python
"""Lockstep adjoint with per-element matrices (the backward pass of hip_batch_solve_lockstep(Px=, Ax=)) against the per-element loop it replaces in the
torch layer, on handles of the same process.

Problem: problems.banded_qp(n, window=40) at n = 2000; a batch of 64 / 256 elements, each with its own A values, its own diagonal of P, its own q and
bounds (tools/lockstep_mat_bench.py's recipe), eps --eps.  The forward (x, y) come from one hip_batch_solve_lockstep(Px=, Ax=) call; the incoming
gradient is dx = x - 0.1 noise, dy = 0 (what a loss on x sends back).
Measured per (n, B): wall and GPU ms of ONE hip_batch_adjoint_lockstep(Px=, Ax=) call (median of --reps after --warmup, with the min-max spread), its
launches, recurrence steps, PCG iterations and the share of the GPU time spent in assembly + equilibration (lockstep_mat_adjoint_last_record); and the
loop nn/torch.py::_backward_loop runs for such a batch -- update(Px=, Ax=), update(l, u), adjoint_derivative_compute_at and the two getters per element
on ONE handle -- timed on the first min(B, --loop-sample) elements and scaled to B (one element after the other: linear in B by construction); the
largest relative deviation of dq between the two routes over the sampled elements.

    python tools/lockstep_mat_adjoint_bench.py --out profiles/lockstep_mat_adjoint_bench.json
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
    ap.add_argument('--sizes', type=int, nargs='+', default=[2000])
    ap.add_argument('--batches', type=int, nargs='+', default=[64, 256])
    ap.add_argument('--eps', type=float, default=1e-8)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--loop-sample', type=int, default=8)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    SOLVED = int(osqp_amd.SolverStatus.OSQP_SOLVED)
    st = dict(verbose=False, eps_abs=a.eps, eps_rel=a.eps, max_iter=50000, warm_starting=False)
    rows = []
    for n in a.sizes:
        P, q, A, l, u = problems.banded_qp(n, window=40)
        A = sp.csc_matrix(A); A.sort_indices()
        m = len(l)
        for B in a.batches:
            Px, Ax, Q, L, U = batch(P, q, A, l, u, B)
            s = osqp_amd.OSQP(algebra='hip')
            s.setup(P, q, A, l, u, **st)
            ext = s._solver
            x, y, rec = ext.hip_batch_solve_lockstep(q=Q, l=L, u=U, Px=Px, Ax=Ax)
            dx = x - 0.1 * np.random.default_rng(2).standard_normal(x.shape)
            wall, gpu, prep = [], [], []
            for r in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                g = ext.hip_batch_adjoint_lockstep(x, y, dx, None, l=L, u=U, Px=Px, Ax=Ax)
                wall.append(1e3 * (time.perf_counter() - t0))
                last = ext.lockstep_mat_adjoint_last_record()
                gpu.append(last['gpu_ms']); prep.append(last['prepare_gpu_ms'])
            wall, gpu, prep = (np.array(v[a.warmup:]) for v in (wall, gpu, prep))
            row = dict(n=n, m=m, B=B, eps=a.eps, forward_solved=int((rec[:, 0] == SOLVED).sum()),
                       lockstep_mat_adjoint=dict(wall_ms=float(np.median(wall)), wall_ms_min=float(wall.min()), wall_ms_max=float(wall.max()), gpu_ms=float(np.median(gpu)),
                                                 prepare_gpu_ms=float(np.median(prep)), prepare_share=float(np.median(prep) / np.median(gpu)),
                                                 kernel_launches=last['kernel_launches'], chunks=last['chunks'], steps_max=last['steps_max'], pcg_iters=last['pcg_iters'],
                                                 matrix_block_bytes=last['matrix_block_bytes'], status0=int((g['rec'][:, 0] == 0).sum()),
                                                 residual_max=float(g['rec'][:, 2].max())))
            # the loop on one handle (nn/torch.py::_backward_loop: update(Px, Ax) + update(l, u) + adjoint_derivative_compute_at + the getters per element)
            h = osqp_amd.OSQP(algebra='hip')
            h.setup(P, q, A, l, u, **st)
            hx = h._solver
            ns = min(B, a.loop_sample)
            tl, dev, ok = [], 0.0, 0
            for r in range(2):                                                      # one warm-up pass, one timed
                t0 = time.perf_counter()
                for b in range(ns):
                    h.update(Px=Px[b], Ax=Ax[b])
                    h.update(l=L[b], u=U[b])
                    e = hx.adjoint_derivative_compute_at(x[b], y[b], dx[b])
                    dP, dA = h.ext.CSC(h._derivative_cache['P'].copy()), h.ext.CSC(h._derivative_cache['A'].copy())
                    dq, dl, du = np.empty(n), np.zeros(m), np.zeros(m)
                    e = e or hx.adjoint_derivative_get_mat(dP, dA) or hx.adjoint_derivative_get_vec(dq, dl, du)
                    if r == 0 and not e:
                        ok += 1
                        dev = max(dev, float(np.abs(dq - g['dq'][b]).max() / (1e-300 + np.abs(dq).max())))
                tl.append(1e3 * (time.perf_counter() - t0) * B / ns)
            row['loop'] = dict(wall_ms=float(tl[1]), wall_ms_first=float(tl[0]), sample=ns, status0_of_sample=ok)
            row['dq_dev_vs_loop'] = dev
            row['loop_over_lockstep_mat_adjoint'] = float(tl[1] / np.median(wall))
            print(json.dumps(row), flush=True)
            rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(dict(tool='tools/lockstep_mat_adjoint_bench.py', rows=rows), f, indent=1)


if __name__ == '__main__':
    main()
