"""Forward and backward of the MPC batch through the device-pointer path, timed with a hipEvent pair each (torch.cuda.Event on torch's current
stream, after a warm-up, over several repetitions; median and spread reported).

    python tools/adjoint_bench.py [--batch 4096] [--reps 20] [--warmup 5] [--out profiles/NAME.json]

forward  = osqp_hip_batch_solve_device (every solve launch of the batch);  backward = osqp_hip_batch_adjoint_device (ONE launch: k_batch_adjoint)
with all five gradients, and with dq alone (what the dP / dA stores of nbatch x (nnz(P) + nnz(A)) doubles cost).  One JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'osqp-python_amd')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--eps', type=float, default=1e-6)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
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
