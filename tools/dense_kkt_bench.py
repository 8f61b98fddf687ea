#!/usr/bin/env python
"""Sweep of the dense KKT mode (include/osqp_hip.h osqp_hip_dense_kkt) against the same handle with the mode off.

Two families -- banded (problems.banded_qp: the one-launch PCG form's home ground) and unstructured (problems.random_qp-like: sparse random A and
P = M M' + 0.01 I with a density that keeps m n under the work matrix' cap and the rows short of the Woodbury threshold) -- at n = 500, 1 000, 2 000,
4 000, m = 2 n.  Per size, on ONE handle in ONE process, blocks of cold solves alternate between the mode off and on (off, on, off, on: a drift of the
machine shows as a difference between the two blocks of one arm); every solve starts from zero iterates and from the setting's rho.  Reported:

  off_ms / on_ms          median wall-clock ms per cold solve (host clock around osqp_solve, which ends in a stream synchronisation), with min and max
  off_iter / on_iter      ADMM iterations of each
  factor_ms               ms per factorisation (W, W' W, + P + sigma I, the inverse, the probe; median over the rho resets and the solves' rho updates)
  apply_us                microseconds per k_dk_apply launch, back-to-back launches between a hipEvent pair (osqp_hip_time_kernel 24)
  iteration_us            microseconds per ADMM iteration of the mode (KB, k_dk_apply, KA): a captured chunk replayed between a hipEvent pair (25)
  off_launches            kernel launches of an off solve (what the mode's 3 per iteration replace)

Results: one JSON document (default profiles/dense_kkt_bench.json).  A run without a GPU fails: there is no other way to obtain these numbers."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'osqp-python_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)
import osqp_amd          # noqa: E402
import problems          # noqa: E402

warnings.simplefilter('ignore')
RHO0 = 0.1


def unstructured(n, seed=0, per_row=12):
    """random_qp's construction at a density of per_row entries per row / column; bounds around a feasible point"""
    rng = np.random.default_rng(seed)
    m = 2 * n
    M = sp.random(n, n, density=min(1.0, 3.0 / n), random_state=rng, data_rvs=rng.standard_normal)
    P = (M @ M.T + 1e-2 * sp.eye(n)).tocsc(); P.sort_indices()
    A = sp.random(m, n, density=min(1.0, per_row / n), random_state=rng, data_rvs=rng.standard_normal, format='csc'); A.sort_indices()
    q = rng.standard_normal(n)
    ax = A @ (0.1 * rng.standard_normal(n))
    return P, q, A, ax - rng.random(m), ax + rng.random(m)


FAMILIES = {'banded': lambda n: problems.banded_qp(n, window=min(200, n)), 'unstructured': unstructured}


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), n=len(v))


def cold_solves(m, reps):
    """reps cold solves from the setting's rho; returns (ms per solve, iterations, the update_settings times in ms)"""
    ms, it, reset = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter(); m.update_settings(rho=RHO0); reset.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter(); r = m.solve(); ms.append(1e3 * (time.perf_counter() - t0))
        assert r.info.status_val == 1, r.info.status
        it.append(int(r.info.iter))
    return ms, it, reset


def run(family, n, reps, eps):
    P, q, A, l, u = FAMILIES[family](n)
    m = osqp_amd.OSQP(algebra='hip')
    m.setup(P, q, A, l, u, verbose=False, eps_abs=eps, eps_rel=eps, max_iter=20000, warm_starting=False, rho=RHO0)
    s = m._solver
    out = dict(family=family, n=int(n), m=int(A.shape[0]), nnzA=int(A.nnz), eps=eps, woodbury_rows=int(s.hip_stats()['woodbury_rows']), reordered=int(s.hip_stats()['reordered']))
    off, on, off_it, on_it, fac, launches = [], [], [], [], [], []
    cold_solves(m, 2)                                        # warm-up of the off path (graphs, code objects)
    for block in range(2):
        a, b, _ = cold_solves(m, reps); off += a; off_it += b
        launches.append(float(s.hip_stats()['kernel_launches']))
        st = s.hip_dense_kkt(True)
        if st != 0:
            out.update(declined=st)
            return out
        if block == 0:
            cold_solves(m, 2)                                # warm-up of the on path
        n0 = s.hip_dense_kkt_record()['factorisations']
        a, b, reset = cold_solves(m, reps); on += a; on_it += b
        rec = s.hip_dense_kkt_record()
        fac += reset                                         # (with the mode on, update_settings(rho) IS one factorisation, synchronous)
        out.update(state=rec['state'], probe=rec['probe'], min_pivot=rec['min_pivot'], device_bytes=rec['device_bytes'],
                   on_pcg_iters=float(s.hip_stats()['pcg_iters_total']), factorisations_per_solve=(rec['factorisations'] - n0) / reps - 1.0)
        if rec['state'] == 1:
            out.update(apply_us=1e3 * s.hip_time_kernel(24, 200), iteration_us=1e3 * s.hip_time_kernel(25, 200))
        assert s.hip_dense_kkt(False) == 0
    out.update(off_ms=spread(off), on_ms=spread(on), off_iter=spread(off_it), on_iter=spread(on_it), factor_ms=spread(fac), off_launches=statistics.median(launches),
               off_ms_blocks=[statistics.median(off[:reps]), statistics.median(off[reps:])], on_ms_blocks=[statistics.median(on[:reps]), statistics.median(on[reps:])])
    out['speedup'] = out['off_ms']['median'] / out['on_ms']['median']
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--sizes', type=int, nargs='+', default=[500, 1000, 2000, 4000])
    ap.add_argument('--families', nargs='+', default=list(FAMILIES))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--eps', type=float, default=1e-5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dense_kkt_bench.json'))
    a = ap.parse_args()
    assert osqp_amd._lib.handle().osqp_hip_backend() == b'hip-gfx950'
    rows = []
    for fam in a.families:
        for n in a.sizes:
            r = run(fam, n, a.reps, a.eps)
            rows.append(r)
            if 'off_ms' in r:
                print('%-13s n=%5d  off %8.2f ms (%d it, %d launches)  on %8.2f ms (%d it)  x%.2f  factor %.2f ms  apply %.1f us  iteration %.1f us  state %d' % (
                    fam, n, r['off_ms']['median'], r['off_iter']['median'], r['off_launches'], r['on_ms']['median'], r['on_iter']['median'], r['speedup'],
                    r['factor_ms']['median'], r.get('apply_us', float('nan')), r.get('iteration_us', float('nan')), r['state']), flush=True)
            else:
                print('%-13s n=%5d  declined (%s)' % (fam, n, r.get('declined')), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(dict(tool='tools/dense_kkt_bench.py', reps_per_block=a.reps, blocks=2, eps=a.eps, rho=RHO0, rows=rows), f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
