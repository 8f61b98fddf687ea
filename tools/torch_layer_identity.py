#!/usr/bin/env python
"""Bit identity of the torch layer (osqp_amd.nn.torch.OSQP) between two versions of the Python package on ONE built library.

Only the layer's public surface is used -- the constructor's keywords, forward, backward, last_rec, last_adjoint_rec and the launch counters -- so the
same file runs on either version: ``--package DIR`` names the directory that holds the ``osqp_amd`` package to import (default: this checkout's
osqp-python_amd; a copy of another commit's package next to the same libosqp_hip.so gives the other side).

  --dump FILE      run the fixed cases below and write FILE (.npz): per case x, every gradient, last_rec, last_adjoint_rec and all counters -- or the
                   type and text of the exception the case ends in
  --compare A B    bit equality of every array and equality of every counter; prints the case count and the differences, exits non-zero on any
  --time REPS      host time of the layer: ms of one forward and one backward call, median [min, max] over REPS after one warm-up, on (a) the
                   batch benchmark's shape (problems.mpc_batch(4096): shared matrices, l / u as ROCm tensors, the zero-copy one-launch route) and
                   (b) tools/lockstep_mat_adjoint_bench.py's shape (banded_qp(2000, window=40), 64 elements with their own matrices, the lockstep
                   route forward and backward, eps 1e-8).  One JSON line.

Cases: every row of the route table in the layer's module docstring with host and with ROCm tensors, forward and backward (large_backward =
large_batch), a batch of 3: a QP that fits one workgroup (banded_qp(40, window=8)), one that does not (banded_qp(400, window=40)) and the Woodbury
handle with a diagonal K0 (portfolio_qp(600, 4)); shared and per-element matrices; the cells in which a decline comes out of the layer included.
(`profiles/torch_layer_refactor.txt`)"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ('setup_count', 'adjoint_launches', 'mat_batch_launches', 'mat_lockstep_launches', 'mat_lockstep_direct_launches',
            'mat_lockstep_adjoint_launches', 'mat_lockstep_direct_adjoint_launches')
NB = 3
# (problem, large_batch = large_backward)
CASES = [('small', 'loop'), ('large', 'loop'), ('large', 'lockstep'), ('large', 'lockstep_direct'), ('woodbury', 'lockstep'), ('woodbury', 'lockstep_direct')]


def _problem(name):
    import problems
    P, q, A, l, u = dict(small=lambda: problems.banded_qp(40, window=8), large=lambda: problems.banded_qp(400, window=40),
                         woodbury=lambda: problems.portfolio_qp(600, 4))[name]()
    P, A = sp.csc_matrix(P), sp.csc_matrix(A)
    P.sort_indices(); A.sort_indices()
    rng = np.random.default_rng(13)
    Q = np.stack([q + 0.05 * b * rng.standard_normal(len(q)) for b in range(NB)])
    scale = 1 + 0.01 * np.arange(NB)[:, None]             # per-element matrices: x / scale of a feasible x stays feasible
    return P, A, Q, np.tile(l, (NB, 1)), np.tile(u, (NB, 1)), P.data * scale, A.data * scale


def _layer(P, A, **kw):
    from osqp_amd.nn.torch import OSQP as Layer
    pco, aco = P.tocoo(), A.tocoo()
    return Layer((pco.row, pco.col), P.shape, (aco.row, aco.col), A.shape, **kw)


def _host(v):
    import torch
    return None if v is None else torch.as_tensor(v).detach().cpu().numpy()


def dump(path):
    import torch
    out = {}
    for name, mode in CASES:
        P, A, Q, L, U, Pv, Av = _problem(name)
        for per_element in (False, True):
            for device in ('cpu', 'cuda'):
                tag = '%s/%s/%s/%s' % (name, 'per_element' if per_element else 'shared', mode, device)
                layer = _layer(P, A, eps_rel=1e-6, eps_abs=1e-6, max_iter=200000, large_batch=mode, large_backward=mode)
                vals = [Pv if per_element else P.data, Q, Av if per_element else A.data, L, U]
                ts = [torch.tensor(np.array(v), dtype=torch.float64, device=device, requires_grad=True) for v in vals]
                try:
                    x = layer(*ts)
                    out[tag + '/x'] = _host(x)
                    (0.5 * (x ** 2).sum()).backward()
                    for key, t in zip(('dP', 'dq', 'dA', 'dl', 'du'), ts):
                        out[tag + '/' + key] = _host(t.grad)
                except Exception as e:      # a decline that comes out of the layer is part of the table
                    out[tag + '/error'] = np.array('%s: %s' % (type(e).__name__, e))
                for key in ('last_rec', 'last_adjoint_rec'):
                    v = _host(getattr(layer, key))
                    if v is not None:
                        out[tag + '/' + key] = v
                out[tag + '/counters'] = np.array([getattr(layer, k, 0) for k in COUNTERS], dtype=np.int64)
                print(tag, str(out.get(tag + '/error', 'ok')), dict(zip(COUNTERS, out[tag + '/counters'].tolist())), flush=True)
    np.savez(path, **out)
    print('%d cases, %d arrays -> %s' % (len({k.rsplit('/', 1)[0] for k in out}), len(out), path))


def compare(a, b):
    A, B = np.load(a), np.load(b)
    cases = sorted({k.rsplit('/', 1)[0] for k in set(A.files) | set(B.files)})
    diffs = []
    for k in sorted(set(A.files) | set(B.files)):
        if k not in A.files or k not in B.files:
            diffs.append('%s: only in %s' % (k, a if k in A.files else b))
        elif A[k].shape != B[k].shape or A[k].dtype != B[k].dtype or A[k].tobytes() != B[k].tobytes():
            diffs.append('%s: differs' % k)
    for d in diffs:
        print(d)
    print('%d cases, %d arrays compared, %d differences' % (len(cases), len(set(A.files) | set(B.files)), len(diffs)))
    return 1 if diffs else 0


def _ms(fn, reps, sync):
    t = []
    for r in range(reps + 1):
        sync(); t0 = time.perf_counter()
        fn()
        sync(); t.append(1e3 * (time.perf_counter() - t0))
    t = np.array(t[1:])
    return [float(np.median(t)), float(t.min()), float(t.max())]


def timing(reps):
    import torch
    import problems
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from lockstep_mat_bench import batch
    row = {}
    dev = torch.device('cuda', 0)
    sync = lambda: torch.cuda.synchronize(dev)
    # (a) shared matrices, ROCm tensors, one launch
    P, q, A, L, U = problems.mpc_batch(4096)
    P, A = sp.csc_matrix(P), sp.csc_matrix(A)
    P.sort_indices(); A.sort_indices()
    layer = _layer(P, A, eps_rel=1e-6, eps_abs=1e-6)
    ts = [torch.tensor(np.array(v), dtype=torch.float64, device=dev) for v in (P.data, q, A.data, L, U)]
    ts[3].requires_grad_(True)
    hold = {}

    def forward():
        hold['x'] = layer(*ts)
    row['mpc4096_forward_ms'] = _ms(forward, reps, sync)
    row['mpc4096_backward_ms'] = _ms(lambda: hold['x'].sum().backward(retain_graph=True), reps, sync)
    # (b) per-element matrices on the lockstep route, host tensors
    P, q, A, l, u = problems.banded_qp(2000, window=40)
    P, A = sp.csc_matrix(P), sp.csc_matrix(A)
    P.sort_indices(); A.sort_indices()
    Px, Ax, Q, L, U = batch(P, q, A, l, u, 64)
    layer = _layer(P, A, eps_rel=1e-8, eps_abs=1e-8, max_iter=50000, large_batch='lockstep', large_backward='lockstep')
    ts = [torch.tensor(np.array(v), dtype=torch.float64) for v in (np.tile(P.data, (64, 1)), Q, Ax, L, U)]
    ts[1].requires_grad_(True)
    row['banded2000x64_forward_ms'] = _ms(forward, reps, sync)
    row['banded2000x64_backward_ms'] = _ms(lambda: hold['x'].sum().backward(retain_graph=True), reps, sync)
    row['counters'] = {k: getattr(layer, k, 0) for k in COUNTERS}
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--package', default=os.path.join(ROOT, 'osqp-python_amd'))
    ap.add_argument('--dump')
    ap.add_argument('--compare', nargs=2)
    ap.add_argument('--time', type=int)
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    warnings.simplefilter('ignore')
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.abspath(a.package))
    if a.dump:
        dump(a.dump)
    if a.time:
        timing(a.time)
    return 0


if __name__ == '__main__':
    sys.exit(main())
