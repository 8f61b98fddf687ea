"""Forward and backward of the MPC batch through the device-pointer path, timed with a hipEvent pair each (torch.cuda.Event on torch's current
stream, after a warm-up, over several repetitions; median and spread reported).

    python tools/adjoint_bench.py [--batch 4096] [--reps 20] [--warmup 5] [--out profiles/NAME.json]
    python tools/adjoint_bench.py --single [--n 100000] [--eps 1e-8] [--reps 20] [--warmup 5] [--out profiles/NAME.json]      (see single())
    python tools/adjoint_bench.py --single --woodbury [--eps 1e-8] [--reps 5] [--warmup 1] [--only TEXT] [--out profiles/NAME.json]      (see woodbury())

forward  = osqp_hip_batch_solve_device (every solve launch of the batch);  backward = osqp_hip_batch_adjoint_device (ONE launch: k_batch_adjoint)
with all five gradients, and with dq alone (what the dP / dA stores of nbatch x (nnz(P) + nnz(A)) doubles cost).  One JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'osqp-python_amd')]


def single(a):
    """--single: the backward of ONE large QP on the PCG path (BASELINE configs[1], problems.banded_qp(n)): osqp_adjoint_derivative_compute after a
    solve at --eps, wall time per call (the call synchronises) -- median over --reps after --warmup -- with the engine's own split into the
    recurrence and the gradient kernel (osqp_hip_adjoint_last_record), and the same handle's polish time for comparison (the same recurrence,
    started from the solution instead of zero).  Gradient kernel traffic: per stored entry two 4-byte indices and one 8-byte store, plus the
    gathered vectors once (3 n + 2 m doubles), against 8 TB/s."""
    import time
    import osqp_amd
    import problems
    P, q, A, l, u = problems.banded_qp(a.n, seed=12345)
    n, m = len(q), len(l)
    st = dict(eps_abs=a.eps, eps_rel=a.eps, verbose=False, max_iter=200000)
    s = osqp_amd.OSQP(algebra='hip')
    s.setup(P, q, A, l, u, **st)
    r = s.solve()
    assert r.info.status_val == osqp_amd.SolverStatus.OSQP_SOLVED
    dx = r.x - 0.1 * np.random.default_rng(7).standard_normal(n)
    tot, rec_s, grad_s = [], [], []
    for k in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        s.adjoint_derivative_compute(dx=dx)
        t1 = time.perf_counter()
        rec = s.adjoint_last_record()
        if k >= a.warmup:
            tot.append(t1 - t0); rec_s.append(rec['recurrence_s']); grad_s.append(rec['gradient_s'])
    sp_ = osqp_amd.OSQP(algebra='hip')
    sp_.setup(P, q, A, l, u, polishing=True, **st)
    pol = [sp_.solve().info.polish_time for _ in range(3)]
    import scipy.sparse as spa
    nzP, nzA = spa.triu(P).nnz, A.nnz
    gbytes = 16.0 * (nzP + nzA) + 8.0 * (3 * n + 2 * m)
    med = lambda v: float(np.median(v))
    line = dict(tool='adjoint_bench --single', n=n, m=m, nnzP_triu=int(nzP), nnzA=int(nzA), eps=a.eps, reps=a.reps, warmup=a.warmup, iter=int(r.info.iter),
                backward_ms_median=1e3 * med(tot), backward_ms_min=1e3 * min(tot), backward_ms_max=1e3 * max(tot),
                recurrence_ms_median=1e3 * med(rec_s), gradient_kernel_ms_median=1e3 * med(grad_s), recurrence_steps=rec['steps'], active_rows=rec['active_rows'],
                residual=rec['residual'], polish_ms=[1e3 * p for p in pol], recurrence_over_polish=med(rec_s) / float(np.median(pol)),
                gradient_bytes=gbytes, gradient_fraction_of_8TBs=gbytes / max(med(grad_s), 1e-12) / 8e12)
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


def woodbury(a):
    """--single --woodbury: the backward of ONE QP whose linear solve runs the Woodbury-corrected preconditioner (OSQPHipPolicy::adjoint_woodbury = 1):
    the four problems of tests/test_gpu_adjoint_woodbury.py and BASELINE configs[2] / configs[3] at full size, the lasso also with the inverse cache
    off (putting rho back is then a second factorisation instead of a look-up).  Per problem: the mode, one cold solve of the handle (wall time of
    its first solve), then osqp_adjoint_derivative_compute with a random dy -- wall time per call, median over --reps after --warmup -- with the
    record's split (recurrence, gradient kernels), the recurrence's steps and its PCG iterations per step.  One JSON object, a list under "problems"."""
    import time
    import scipy.sparse as spa
    import osqp_amd
    import problems

    def banded_dense():
        P, q, A, l, u = problems.banded_qp(3000, window=30)
        rng = np.random.default_rng(1)
        dense = spa.random(6, 3000, density=0.3, random_state=rng, data_rvs=rng.standard_normal, format='csc')
        x0 = 0.1 * rng.standard_normal(3000)
        half = np.array([1.0, 1.0, 1.0, 1e3, 1e3, 1e3])
        return P, q, spa.vstack([A, dense], format='csc'), np.concatenate([l, dense @ x0 - half]), np.concatenate([u, dense @ x0 + half])
    full = []

    def lasso_full():                                  # (generated once: 50 M entries)
        if not full:
            full.append(problems.lasso_qp(5000, 10000))
        return full[0]
    cases = [('portfolio_qp(600, 4)', lambda: problems.portfolio_qp(600, 4), {}), ('portfolio_qp(2000, 20)', lambda: problems.portfolio_qp(2000, 20), {}),
             ('lasso_qp(300, 600)', lambda: problems.lasso_qp(300, 600), {}), ('banded_qp(3000, window=30) + 6 dense rows', banded_dense, {}),
             ('configs[3] portfolio_qp(10000, 100)', lambda: problems.portfolio_qp(10000, 100), {}),
             ('configs[2] lasso_qp(5000, 10000)', lambda: lasso_full(), {}),
             ('configs[2] lasso_qp(5000, 10000), inverse cache off', lambda: lasso_full(), {'OSQP_HIP_WOODBURY_CACHE': '0'})]
    if a.only:
        cases = [c for c in cases if a.only in c[0]]
    os.environ['OSQP_HIP_SMALL_DIRECT'] = '0'
    med = lambda v: float(np.median(v))
    out = []
    for name, make, env in cases:
        P, q, A, l, u = make()
        n, m = len(q), len(l)
        os.environ.update(env)
        try:
            s = osqp_amd.OSQP(algebra='hip')
            s.setup(P, q, A, l, u, eps_abs=a.eps, eps_rel=a.eps, verbose=False, max_iter=200000)
        finally:
            for k in env:
                os.environ.pop(k)
        s._solver.set_policy(adjoint_woodbury=1)
        t0 = time.perf_counter()
        r = s.solve()
        cold = time.perf_counter() - t0
        st = s._solver.hip_stats()
        assert r.info.status_val == osqp_amd.SolverStatus.OSQP_SOLVED and st['woodbury_rows'] > 0
        rng = np.random.default_rng(7)
        dx, dy = r.x - 0.1 * rng.standard_normal(n), rng.standard_normal(m)
        tot, rec_s, grad_s, rec, err = [], [], [], None, None
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            try:
                s.adjoint_derivative_compute(dx=dx, dy=dy)
            except ArithmeticError as e:            # the recurrence stalled above the threshold: the record says where
                err = str(e)
            t1 = time.perf_counter()
            rec = s.adjoint_last_record()
            if k >= a.warmup:
                tot.append(t1 - t0); rec_s.append(rec['recurrence_s']); grad_s.append(rec['gradient_s'])
        after = s._solver.hip_stats()
        line = dict(problem=name, n=n, m=m, nnzA=int(A.nnz), eps=a.eps, woodbury_rows=int(st['woodbury_rows']), woodbury_direct=int(st['woodbury_direct']),
                    woodbury_dual_cols=int(st['woodbury_dual_cols']), woodbury_one_launch=int(st['woodbury_one_launch']), preconditioner=s._solver.hip_preconditioner(),
                    solve_iter=int(r.info.iter), cold_solve_ms=1e3 * cold, solve_factorisations=int(st['woodbury_factorisations']), solve_cache_hits=int(st['woodbury_cache_hits']),
                    status=rec['status'], active_rows=rec['active_rows'], residual=rec['residual'], recurrence_steps=rec['steps'], pcg_iters=rec['pcg_iters'],
                    pcg_iters_per_step=rec['pcg_iters'] / max(rec['steps'], 1), backward_ms_median=1e3 * med(tot), backward_ms_min=1e3 * min(tot), backward_ms_max=1e3 * max(tot),
                    recurrence_ms_median=1e3 * med(rec_s), gradient_kernel_ms_median=1e3 * med(grad_s), backward_over_cold_solve=med(tot) / cold,
                    stats_unchanged_by_the_calls=all(after[k] == st[k] for k in ('woodbury_rows', 'woodbury_direct', 'woodbury_factorisations', 'woodbury_cache_hits')))
        if err:
            line['error'] = err
        print(json.dumps(line), flush=True)
        out.append(line)
        del s
    text = json.dumps(dict(tool='adjoint_bench --single --woodbury', reps=a.reps, warmup=a.warmup, problems=out), indent=1)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--single', action='store_true', help='one large QP on the PCG path instead of the MPC batch')
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--eps', type=float, default=1e-6)
    ap.add_argument('--out', default=None)
    ap.add_argument('--woodbury', action='store_true', help='with --single: the QPs with dense rows (Woodbury handles) instead of the banded QP')
    ap.add_argument('--only', default=None, help='with --woodbury: the problems whose name contains this text')
    a = ap.parse_args()
    if a.single and a.woodbury:
        return woodbury(a)
    if a.single:
        return single(a)
    import torch
    import osqp_amd
    import problems
    B = a.batch
    P, q, A, L, U = problems.mpc_batch(B)
    n, m = P.shape[0], A.shape[0]
    s = osqp_amd.OSQP(algebra='hip')
    s.setup(P, q, A, L[0], U[0], eps_abs=a.eps, eps_rel=a.eps, verbose=False, max_iter=4000)
    sv = s._solver
    dev = torch.device('cuda', 0)
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64, device=dev)
    Ld, Ud = t(L), t(U)
    x, y = torch.zeros((B, n), dtype=torch.float64, device=dev), torch.zeros((B, m), dtype=torch.float64, device=dev)
    rec, arec = torch.zeros((B, sv.BATCH_REC), dtype=torch.float64, device=dev), torch.zeros((B, sv.ADJOINT_REC), dtype=torch.float64, device=dev)
    dx = t(np.random.default_rng(5).standard_normal((B, n)))
    dP, dq, dA = (torch.zeros((B, w), dtype=torch.float64, device=dev) for w in (sv.nnz_P, n, sv.nnz_A))
    dl, du = torch.zeros((B, m), dtype=torch.float64, device=dev), torch.zeros((B, m), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def forward():
        sv.hip_batch_solve_device(B, None, Ld.data_ptr(), Ud.data_ptr(), x.data_ptr(), y.data_ptr(), rec.data_ptr(), warm=False, stream=stream)

    def backward(full=True):
        sv.hip_batch_adjoint_device(B, x.data_ptr(), y.data_ptr(), dx.data_ptr(), None, Ld.data_ptr(), Ud.data_ptr(), None, None,
                                    dP.data_ptr() if full else None, dq.data_ptr(), dA.data_ptr() if full else None,
                                    dl.data_ptr() if full else None, du.data_ptr() if full else None, arec.data_ptr(), stream=stream)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms = np.array(ms)
        return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()))
    fwd = timed(forward)
    assert int((rec[:, 0] != 1).sum()) == 0, 'unsolved problems in the batch'
    bwd, bwd_dq = timed(backward), timed(lambda: backward(False))
    st = arec.cpu().numpy()
    line = dict(tool='adjoint_bench', batch=B, n=n, m=m, nnz_P=sv.nnz_P, nnz_A=sv.nnz_A, eps=a.eps, reps=a.reps, warmup=a.warmup,
                forward=fwd, backward=bwd, backward_dq_only=bwd_dq, mean_forward_iter=float(rec[:, 1].mean().item()),
                backward_over_forward=bwd['median_ms'] / fwd['median_ms'], adjoint_status_nonzero=int((st[:, 0] != 0).sum()),
                adjoint_worst_residual=float(st[:, 2].max()), gradient_bytes=int(8 * B * (sv.nnz_P + sv.nnz_A + n + 2 * m)))
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
