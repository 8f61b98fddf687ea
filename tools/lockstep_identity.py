#!/usr/bin/env python3
"""Bit identity of the lockstep routes between two builds of the engine: what a change of the host drivers (lockstep_hip.hip's chunk functions,
Engine::run_lockstep_solve / run_lockstep_adjoint and the entry points over them) must leave exactly as it was.

--dump FILE runs, with fixed seeds and no time limit, on problems.banded_qp(400, window=40) at B = 70 and eps 1e-8 (one full chunk and a ragged one):
the forward route, the forward with polishing, the forward with per-element Px / Ax (and that with polishing: its ADMM part, the polished result, and
the same handle with polishing switched off), the adjoint, the adjoint with per-element Px / Ax; on problems.portfolio_qp(200, 10) and (600, 4) at
B = 70: the direct forward and the direct adjoint, both also with per-element Px / Ax drawn as tests/test_gpu_lockstep_direct_mat.py draws them (a handle
the direct route declines -- (200, 10): no dense row -- is kept as its return code), and the direct forward on a polishing handle, shared and with
per-element matrices (its ADMM part, the polished result, and the same handle with polishing switched off); and the m = 0 tridiagonal case at n = 900, B = 3, with polish.  On both
routes there is one forward call each with only Px and only Ax, and every case above is run again through its *_device entry, the same inputs as torch
tensors on torch's current stream (tags <tag>_dev).  A call with per-element matrices is kept with its own record and its route's base record
(<tag>_base).  The tool's Python is the same text for both dumps: the C ABI is what two builds share.  Every returned array and every *_last_record
field except the timings goes into an .npz.  --compare A B exits non-zero unless every array is equal (NaNs in the same places) and every record field
is equal: kernel launches, iteration / step counts, PCG iterations, inversions, polish counts, workspace bytes.  --feature TAG ..: entries under these
tags are what build B is meant to change (mat_polish, when A is a build from before polish reached the per-element-matrix entry; direct_600_4_polish and
direct_600_4_mat_polish, when A is a build from before polish reached the direct route); they are printed with both sides' figures and not counted.

    python tools/lockstep_identity.py --dump prof_out/identity_this.npz          (OSQP_HIP_LIBRARY selects the other build)
    python tools/lockstep_identity.py --compare prof_out/identity_parent.npz prof_out/identity_this.npz [--feature mat_polish direct_600_4_polish ..]
"""
import argparse
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'osqp-python_amd'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

TIMINGS = ('gpu_ms', 'seconds', 'prepare_gpu_ms')
REC_SECONDS = 9          # column of a batch record that holds the polish seconds


def outer(P, q, A, l, u, **kw):
    import osqp_amd
    s = osqp_amd.OSQP(algebra='hip')
    st = dict(verbose=False, eps_abs=1e-8, eps_rel=1e-8, max_iter=20000, warm_starting=False)
    st.update(kw)
    s.setup(P, q, A, l, u, **st)
    return s


def handle(P, q, A, l, u, **kw):
    return outer(P, q, A, l, u, **kw)._solver


def dump(path):
    import problems
    from lockstep_mat_bench import batch
    out = {}

    def keep(tag, arrays, record):
        for k, v in arrays.items():
            out['%s/%s' % (tag, k)] = np.asarray(v)
        for k, v in record.items():
            if k not in TIMINGS:
                out['%s/last.%s' % (tag, k)] = np.float64(v)

    def fwd(x, y, rec):
        rec = rec.copy(); rec[:, REC_SECONDS] = 0.0          # (wall time of the polish)
        return dict(x=x, y=y, rec=rec)

    # the *_device entries: the same inputs as torch ROCm tensors, the work on torch's current stream (None stays None: the handle's own values)
    def dev(*arrays):
        import torch
        return [None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda') for a in arrays]

    def ptr(t):
        return None if t is None else t.data_ptr()

    def stream():
        import torch
        return torch.cuda.current_stream().cuda_stream

    def fwd_dev(entry, e, nb, q=None, l=None, u=None, Px=None, Ax=None):
        q, l, u, Px, Ax = dev(q, l, u, Px, Ax)
        x, y, rec = dev(np.zeros((nb, e.n)), np.zeros((nb, e.m)), np.zeros((nb, e.BATCH_REC)))
        entry(nb, ptr(q), ptr(l), ptr(u), ptr(x), ptr(y), ptr(rec), warm=False, stream=stream(), Px_ptr=ptr(Px), Ax_ptr=ptr(Ax))
        return fwd(*(t.cpu().numpy() for t in (x, y, rec)))

    def adj_dev(entry, e, x, y, dx, dy=None, l=None, u=None, Px=None, Ax=None):
        nb = x.shape[0]
        x, y, dx, dy, l, u, Px, Ax = dev(x, y, dx, dy, l, u, Px, Ax)
        names = ('dP', 'dq', 'dA', 'dl', 'du', 'rec')
        outs = dev(*(np.zeros((nb, w)) for w in (e.nnz_P, e.n, e.nnz_A, e.m, e.m, e.ADJOINT_REC)))
        entry(nb, ptr(x), ptr(y), ptr(dx), ptr(dy), ptr(l), ptr(u), *(ptr(t) for t in outs), stream=stream(), Px_ptr=ptr(Px), Ax_ptr=ptr(Ax))
        return {k: t.cpu().numpy() for k, t in zip(names, outs)}

    B = 70
    P, q, A, l, u = problems.banded_qp(400, window=40)
    A = sp.csc_matrix(A); A.sort_indices()
    Px, Ax, Q, L, U = batch(P, q, A, l, u, B)
    e = handle(P, q, A, l, u)
    x, y, rec = e.hip_batch_solve_lockstep(q=Q, l=L, u=U)
    keep('forward', fwd(x, y, rec), e.lockstep_last_record())
    dx = x - 0.1 * np.random.default_rng(2).standard_normal(x.shape)
    dy = 0.1 * np.random.default_rng(4).standard_normal(y.shape)
    keep('adjoint', e.hip_batch_adjoint_lockstep(x, y, dx, dy, l=L, u=U), e.lockstep_adjoint_last_record())
    xm, ym, recm = e.hip_batch_solve_lockstep(q=Q, l=L, u=U, Px=Px, Ax=Ax)
    keep('mat', fwd(xm, ym, recm), e.lockstep_mat_last_record())
    keep('mat_base', {}, e.lockstep_last_record())
    dxm = xm - 0.1 * np.random.default_rng(2).standard_normal(xm.shape)
    keep('mat_adjoint', e.hip_batch_adjoint_lockstep(xm, ym, dxm, dy, l=L, u=U, Px=Px, Ax=Ax), e.lockstep_mat_adjoint_last_record())
    keep('mat_adjoint_base', {}, e.lockstep_adjoint_last_record())
    for tag, kw in (('mat_px_only', dict(Px=Px)), ('mat_ax_only', dict(Ax=Ax))):        # one-sided: the other side is the handle's own values
        keep(tag, fwd(*e.hip_batch_solve_lockstep(q=Q, l=L, u=U, **kw)), e.lockstep_mat_last_record())
    keep('forward_dev', fwd_dev(e.hip_batch_solve_lockstep_device, e, B, Q, L, U), e.lockstep_last_record())
    keep('adjoint_dev', adj_dev(e.hip_batch_adjoint_lockstep_device, e, x, y, dx, dy, L, U), e.lockstep_adjoint_last_record())
    keep('mat_dev', fwd_dev(e.hip_batch_solve_lockstep_device, e, B, Q, L, U, Px, Ax), e.lockstep_mat_last_record())
    keep('mat_dev_base', {}, e.lockstep_last_record())
    keep('mat_adjoint_dev', adj_dev(e.hip_batch_adjoint_lockstep_device, e, xm, ym, dxm, dy, L, U, Px, Ax), e.lockstep_mat_adjoint_last_record())
    keep('mat_adjoint_dev_base', {}, e.lockstep_adjoint_last_record())
    so = outer(P, q, A, l, u, polishing=True)
    e = so._solver
    keep('polish', fwd(*e.hip_batch_solve_lockstep(q=Q, l=L, u=U)), e.lockstep_last_record())
    keep('polish_part', {}, e.lockstep_polish_last_record())
    # per-element matrices on the polishing handle.  mat_polish_admm: the ADMM part of that call (record fields status, iter, rho, rho_updates, pcg_iters,
    # rho_estimate; lockstep_mat_last_record), which polish must leave as the unpolished call has it.  mat_polish_off: the same handle with polishing
    # switched off.  mat_polish (FEATURE below): the polished x, y, rec and the polish record -- a build from before polish reached this entry returns the
    # ADMM point there.
    xq, yq, recq = e.hip_batch_solve_lockstep(q=Q, l=L, u=U, Px=Px, Ax=Ax)
    keep('mat_polish', fwd(xq, yq, recq), e.lockstep_polish_last_record())
    keep('mat_polish_admm', dict(rec=recq[:, [0, 1, 5, 6, 7, 10]]), e.lockstep_mat_last_record())
    so.update_settings(polishing=False)
    keep('mat_polish_off', fwd(*e.hip_batch_solve_lockstep(q=Q, l=L, u=U, Px=Px, Ax=Ax)), e.lockstep_mat_last_record())
    keep('mat_polish_off_part', {}, e.lockstep_polish_last_record())

    # portfolio_qp(200, 10) has no row past kLongRow entries, so the handle is no Woodbury one and the direct route declines it: the answer is what is kept.
    # portfolio_qp(600, 4) (the GPU suites' shape: r = 5) is the handle the direct drivers run on.
    for na, k in ((200, 10), (600, 4)):
        tag = 'direct_%d_%d' % (na, k)
        P, q, A, l, u = problems.portfolio_qp(na, k)
        rng = np.random.default_rng(1)
        Q = np.stack([np.concatenate([-rng.standard_normal(na), np.zeros(k)]) for _ in range(B)])
        e = handle(P, q, A, l, u, max_iter=50000)
        try:
            x, y, rec = e.hip_batch_solve_lockstep_direct(q=Q)
        except ValueError as err:
            keep(tag, dict(declined=err.code), {})
            print('%s: declined (%s)' % (tag, err.code))
            continue
        keep(tag, fwd(x, y, rec), e.lockstep_direct_last_record())
        dx = x - 0.1 * np.random.default_rng(2).standard_normal(x.shape)
        keep(tag + '_adjoint', e.hip_batch_adjoint_lockstep_direct(x, y, dx), e.lockstep_direct_adjoint_last_record())
        # per-element Px / Ax as tests/test_gpu_lockstep_direct_mat.py builds them: Ax first, then Px, from one default_rng(3)
        Pt, Ac = sp.csc_matrix(sp.triu(P)), sp.csc_matrix(A)
        Pt.sort_indices(); Ac.sort_indices()
        rng = np.random.default_rng(3)
        Ax = Ac.data * (1.0 + 0.1 * rng.standard_normal((B, Ac.nnz)))
        Px = Pt.data * (1.0 + 0.2 * rng.random((B, Pt.nnz)))
        xm, ym, recm = e.hip_batch_solve_lockstep_direct(q=Q, Px=Px, Ax=Ax)
        keep(tag + '_mat', fwd(xm, ym, recm), e.lockstep_direct_mat_last_record())
        keep(tag + '_mat_base', {}, e.lockstep_direct_last_record())
        dxm = xm - 0.1 * np.random.default_rng(2).standard_normal(xm.shape)
        keep(tag + '_mat_adjoint', e.hip_batch_adjoint_lockstep_direct(xm, ym, dxm, Px=Px, Ax=Ax), e.lockstep_direct_mat_adjoint_last_record())
        keep(tag + '_mat_adjoint_base', {}, e.lockstep_direct_adjoint_last_record())
        for side, kw in (('_mat_px_only', dict(Px=Px)), ('_mat_ax_only', dict(Ax=Ax))):
            keep(tag + side, fwd(*e.hip_batch_solve_lockstep_direct(q=Q, **kw)), e.lockstep_direct_mat_last_record())
        keep(tag + '_dev', fwd_dev(e.hip_batch_solve_lockstep_direct_device, e, B, Q), e.lockstep_direct_last_record())
        keep(tag + '_adjoint_dev', adj_dev(e.hip_batch_adjoint_lockstep_direct_device, e, x, y, dx), e.lockstep_direct_adjoint_last_record())
        keep(tag + '_mat_dev', fwd_dev(e.hip_batch_solve_lockstep_direct_device, e, B, Q, Px=Px, Ax=Ax), e.lockstep_direct_mat_last_record())
        keep(tag + '_mat_dev_base', {}, e.lockstep_direct_last_record())
        keep(tag + '_mat_adjoint_dev', adj_dev(e.hip_batch_adjoint_lockstep_direct_device, e, xm, ym, dxm, Px=Px, Ax=Ax), e.lockstep_direct_mat_adjoint_last_record())
        keep(tag + '_mat_adjoint_dev_base', {}, e.lockstep_direct_adjoint_last_record())
        # the polishing direct handle, shared and per-element matrices.  <tag>_polish / <tag>_mat_polish (FEATURE below): the polished x, y, rec and the polish
        # record -- a build from before polish reached the direct route returns the ADMM point and status_polish 0 there.  *_admm: the ADMM part of those calls
        # (record fields status, iter, rho, rho_updates, pcg_iters, rho_estimate; the direct records), which polish must leave as it was.  *_off: the same
        # handle with polishing switched off.
        so = outer(P, q, A, l, u, max_iter=50000, polishing=True)
        e = so._solver
        for t, kw, last in ((tag + '_polish', dict(), e.lockstep_direct_last_record), (tag + '_mat_polish', dict(Px=Px, Ax=Ax), e.lockstep_direct_mat_last_record)):
            xq, yq, recq = e.hip_batch_solve_lockstep_direct(q=Q, **kw)
            keep(t, fwd(xq, yq, recq), e.lockstep_polish_last_record())
            keep(t + '_admm', dict(rec=recq[:, [0, 1, 5, 6, 7, 10]]), last())
        so.update_settings(polishing=False)
        for t, kw, last in ((tag + '_polish_off', dict(), e.lockstep_direct_last_record), (tag + '_mat_polish_off', dict(Px=Px, Ax=Ax), e.lockstep_direct_mat_last_record)):
            keep(t, fwd(*e.hip_batch_solve_lockstep_direct(q=Q, **kw)), last())
            keep(t + '_part', {}, e.lockstep_polish_last_record())

    n = 900
    rng = np.random.default_rng(3)
    d = 1.0 + rng.random(n)
    off = 0.3 * rng.standard_normal(n - 1)
    P = sp.diags([off, d + 1.0, off], [-1, 0, 1], format='csc')
    q = rng.standard_normal(n)
    Q = np.stack([q + 0.1 * b * rng.standard_normal(n) for b in range(3)])
    e = handle(P, q, sp.csc_matrix((0, n)), np.zeros(0), np.zeros(0), polishing=True, max_iter=4000, check_termination=25)
    keep('m0', fwd(*e.hip_batch_solve_lockstep(q=Q)), e.lockstep_last_record())
    keep('m0_polish_part', {}, e.lockstep_polish_last_record())

    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **out)
    print('%d entries -> %s' % (len(out), path))


def compare(pa, pb, feature=()):
    a, b = np.load(pa), np.load(pb)
    own = lambda k: k.split('/')[0] in feature
    bad = sorted(k for k in set(a.files) ^ set(b.files) if not own(k))
    new = []
    for k in sorted(set(a.files) & set(b.files)):
        if a[k].shape != b[k].shape or not np.array_equal(a[k], b[k], equal_nan=True):
            (new if own(k) else bad).append(k)
    for k in bad:
        print('DIFFERS: %s' % k)
    for k in new:                                        # (what the feature is: shown with both sides' figures, not counted)
        va, vb = a[k], b[k]
        print('FEATURE: %s  %s -> %s' % (k, *(('%g' % v) if v.ndim == 0 else 'array%s' % (v.shape,) for v in (va, vb))))
    for tag in feature:
        k = '%s/rec' % tag
        if k in a.files and k in b.files:
            print('FEATURE: %s status_polish == 1: %d -> %d of %d' % (tag, int((a[k][:, 8] == 1).sum()), int((b[k][:, 8] == 1).sum()), len(b[k])))
    ncmp = len([k for k in set(a.files) | set(b.files) if not own(k)])
    print('%d entries compared, %d differences; %d feature entries differ' % (ncmp, len(bad), len(new)))
    return 1 if bad else 0


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--dump', metavar='FILE')
    ap.add_argument('--compare', nargs=2, metavar=('A', 'B'))
    ap.add_argument('--feature', nargs='*', default=[], metavar='TAG', help='tags whose entries B is meant to change: reported, not counted as differences')
    args = ap.parse_args()
    if args.dump:
        dump(args.dump)
    sys.exit(compare(*args.compare, feature=tuple(args.feature)) if args.compare else 0)
