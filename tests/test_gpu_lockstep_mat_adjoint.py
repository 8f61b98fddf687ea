"""GPU tier: adjoint derivatives on the lockstep route with PER-PROBLEM MATRICES (include/osqp_hip.h osqp_hip_batch_adjoint_lockstep_mat[_device];
osqp-python_amd/csrc/lockstep_hip.hip lockstep_adjoint_chunk with a matrix block) -- the backward pass of osqp_hip_batch_solve_lockstep_mat: every element's
adjoint system on its own P_b, A_b under its own D_b, E_b, c_b.

Shape and data are test_gpu_lockstep_mat.py's Base: banded_qp(400, window=40) (n = 400, m = 800, nnz(A) = 4000, 600 stored entries of triu P), B = 70 (a full
chunk and a ragged one of 6), the rng(3) batch, eps 1e-8; (x, y) come from that file's ONE forward call with per-element matrices.  dx = x - 0.1 N(0,1) and
dy = N(0,1) from default_rng(7), drawn in that order.  Input conditions, asserted per element on the element's own matrices: every inequality row keeps a
class margin min(|(z - l) + y|, |(u - z) - y|) >= 1e-9 and the active rows stay below n.  The checks and their bounds are test_gpu_lockstep_adjoint.py's
(certificate below OSQP_HIP_ADJOINT_TOL, the sparse yardstick, dP / dA to 1e-13 of max |value|, _pair_bound between two certified solutions), each taken
on the element's OWN P_of(b) / A_of(b)."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import adjoint_sparse_ref as ref
import osqp_amd
import problems
from osqp_amd import ext_hip
from util import record_deviation
from test_gpu_lockstep_mat import Base
from test_gpu_lockstep_adjoint import TOL, B, PICK, KEYS, EPS, _margin, _pair_bound, _handle

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
S = osqp_amd.SolverStatus
NOT_IMPL = ext_hip.osqp_error_type.OSQP_FUNC_NOT_IMPLEMENTED
NOT_INIT = ext_hip.osqp_error_type.OSQP_DATA_NOT_INITIALIZED
TAG = 'test_gpu_lockstep_mat_adjoint'


class AdjBase(Base):
    def __init__(self):
        super().__init__()
        assert (self.rec[:, 0] == S.OSQP_SOLVED).all()
        rng = np.random.default_rng(7)
        self.noise = 0.1 * rng.standard_normal((B, self.n))
        self.dx = self.x - self.noise
        self.dy = rng.standard_normal((B, self.m))
        ext = self.s._solver
        self.g = {wd: ext.hip_batch_adjoint_lockstep(self.x, self.y, self.dx, self.dy if wd else None, l=self.L, u=self.U, Px=self.Px, Ax=self.Ax) for wd in (False, True)}
        self.adj_last = ext.lockstep_mat_adjoint_last_record()
        self.adj_last_shared = ext.lockstep_adjoint_last_record()
        self.cert = {}                       # (with_dy, b) -> (host residual, g, r, active rows) on the element's own matrices: computed once, shared

    def certificate(self, wd, b):
        if (wd, b) not in self.cert:
            g = self.g[wd]
            self.cert[(wd, b)] = ref.certificate(self.P_of(b), self.A_of(b), self.L[b], self.U[b], self.x[b], self.y[b], self.dx[b], self.dy[b] if wd else None,
                                                 g['dq'][b], g['dl'][b], g['du'][b])
        return self.cert[(wd, b)]

    def call(self, sl, **kw):
        """the mat adjoint on the base batch's rows sl, with dy"""
        return self.s._solver.hip_batch_adjoint_lockstep(self.x[sl], self.y[sl], self.dx[sl], self.dy[sl], l=self.L[sl], u=self.U[sl], Px=self.Px[sl], Ax=self.Ax[sl], **kw)


@pytest.fixture(scope='module')
def base():
    return AdjBase()


def _certified(tag, P, A, l, u, x, y, dx, dy, g, b, rec):
    """test 1's check of one element: certificate below TOL on (P, A), status 0, the host's active rows, the record's residual within x10 of the host's."""
    margin = _margin(A, l, u, x, y)
    assert margin >= 1e-9, (tag, b, margin)
    host_res, gv, rv, nact = ref.certificate(P, A, l, u, x, y, dx, dy, g['dq'][b], g['dl'][b], g['du'][b])
    print('%s element %d: host residual %.3e, record %s' % (tag, b, host_res, rec))
    assert nact < len(x), (tag, b, nact)
    assert host_res < TOL, (tag, b, host_res)
    assert rec[0] == 0 and rec[1] == nact, (tag, b, rec, nact)
    assert rec[2] < TOL and rec[2] <= 10 * host_res and host_res <= 10 * rec[2], (tag, b, rec[2], host_res)
    return host_res, gv, rv, nact


def test_certificate_every_element(base):
    """1. Every element, with and without dy, on its OWN matrices: certificate below the threshold, status 0, the host's active rows, the record's residual
    within a factor 10 of the host's, both ways; hip_batch_adjoint still declines the shape; the last record."""
    last = base.adj_last
    print('lockstep-mat adjoint B=70: %s' % last)
    assert last['chunks'] == 2 and last['width'] == 64 and last['matrix_block_bytes'] > 0 and 0 < last['prepare_gpu_ms'] < last['gpu_ms'], last
    assert base.adj_last_shared['chunks'] == 2 and base.adj_last_shared['kernel_launches'] == last['kernel_launches'] and base.adj_last_shared['steps_max'] == last['steps_max']
    worst = 0.0
    for b in range(B):
        margin = _margin(base.A_of(b), base.L[b], base.U[b], base.x[b], base.y[b])
        assert margin >= 1e-9, (b, margin)
    for wd in (False, True):
        rec = base.g[wd]['rec']
        for b in range(B):
            host_res, gv, rv, nact = base.certificate(wd, b)
            worst = max(worst, host_res)
            assert nact < base.n, (b, nact)
            assert host_res < TOL, (wd, b, host_res)
            assert rec[b, 0] == 0 and rec[b, 1] == nact, (wd, b, rec[b], nact)
            assert rec[b, 2] < TOL and rec[b, 2] <= 10 * host_res and host_res <= 10 * rec[b, 2], (wd, b, rec[b, 2], host_res)
    record_deviation(TAG, 'certificate, 70 elements x (dy, no dy)', worst_host_residual=worst, tol=TOL, steps_max=last['steps_max'], pcg_iters=last['pcg_iters'],
                     kernel_launches=last['kernel_launches'], gpu_ms=last['gpu_ms'], prepare_gpu_ms=last['prepare_gpu_ms'])
    print('worst host residual %.3e' % worst)
    with pytest.raises(ValueError) as e:
        base.s._solver.hip_batch_adjoint(base.x, base.y, base.dx, l=base.L, u=base.U, Px=base.Px, Ax=base.Ax)
    assert e.value.code == NOT_IMPL


@pytest.mark.parametrize('with_dy', [False, True])
def test_yardstick(base, with_dy):
    """2. |r - r_ref| / |r_ref| <= 10 res |g| / (sigma_min |r_ref|) against the sparse reference on the element's own matrices (the bound of
    test_gpu_lockstep_adjoint.py::test_yardstick); dP / dA against the host formulas to 1e-13 of max |value|."""
    g = base.g[with_dy]
    for b in PICK:
        Pb, Ab = base.P_of(b), base.A_of(b)
        host_res, gv, rv, nact = base.certificate(with_dy, b)
        y0 = ref.adjoint(Pb, Ab, base.L[b], base.U[b], base.x[b], base.y[b], base.dx[b], base.dy[b] if with_dy else None)
        r_ref = np.concatenate([y0['r_x'], y0['r_y'][y0['act']]])
        dev = float(np.linalg.norm(rv - r_ref) / np.linalg.norm(r_ref))
        bound = 10 * host_res * np.linalg.norm(gv) / (y0['sigma_min'] * np.linalg.norm(r_ref))
        record_deviation(TAG, 'banded n=400 own matrices, element %d dy=%s' % (b, with_dy), r_rel_dev=dev, bound=float(bound), host_residual=host_res,
                         record_residual=float(g['rec'][b, 2]), active_rows=nact, steps=int(g['rec'][b, 3]), sigma_min=y0['sigma_min'])
        print('element %d dy=%s: |r - r_ref| / |r_ref| = %.3e (bound %.3e), sigma_min %.3e, steps %d' % (b, with_dy, dev, bound, y0['sigma_min'], g['rec'][b, 3]))
        assert dev <= bound, (b, dev, bound)
        dP, dA = ref.gradients(Pb, Ab, base.x[b], base.y[b], g['dq'][b], -(g['dl'][b] + g['du'][b]))
        for name, got, want in (('dP', g['dP'][b], dP), ('dA', g['dA'][b], dA)):
            assert got.shape == want.shape
            rel = float(np.abs(got - want).max() / np.abs(want).max())
            record_deviation(TAG, '%s at the stored entries, element %d dy=%s' % (name, b, with_dy), rel_dev=rel, bound=1e-13)
            assert rel <= 1e-13, (b, name, rel)


def test_independence(base):
    """3. An element's outputs and record do not depend on what else is in the batch or where in it the element sits; its matrices are part of the element."""
    g = base.g[True]
    for b in PICK:
        g1 = base.call(slice(b, b + 1))
        for k in KEYS:
            assert np.array_equal(g1[k][0], g[k][b]), (b, k)
    r = lambda a: a[::-1].copy()
    gr = base.s._solver.hip_batch_adjoint_lockstep(r(base.x), r(base.y), r(base.dx), r(base.dy), l=r(base.L), u=r(base.U), Px=r(base.Px), Ax=r(base.Ax))
    for k in KEYS:
        assert np.array_equal(gr[k][::-1], g[k]), k


def test_one_side_only(base):
    """4. Ax alone and Px alone (the other side is the handle's own), at the (x, y) of the matching forward: certified as in test 1 on the matrices the element
    was solved with.  Tiles of the handle's own values against the shared adjoint at the same inputs: same statuses and active rows, r within _pair_bound;
    whether the two are bitwise equal is recorded, not required."""
    ext = base.s._solver
    nb = 7
    sl = slice(0, nb)
    x, y, rec = ext.hip_batch_solve_lockstep(q=base.Q[sl], l=base.L[sl], u=base.U[sl], Ax=base.Ax[sl])
    assert (rec[:, 0] == S.OSQP_SOLVED).all()
    dx = x - base.noise[sl]
    g = ext.hip_batch_adjoint_lockstep(x, y, dx, base.dy[sl], l=base.L[sl], u=base.U[sl], Ax=base.Ax[sl])
    for b in range(nb):
        _certified('Ax alone', base.P, base.A_of(b), base.L[b], base.U[b], x[b], y[b], dx[b], base.dy[b], g, b, g['rec'][b])
    L0, U0 = np.tile(base.l_own, (nb, 1)), np.tile(base.u_own, (nb, 1))
    x, y, rec = ext.hip_batch_solve_lockstep(q=base.Q[sl], l=L0, u=U0, Px=base.Px[sl])
    assert (rec[:, 0] == S.OSQP_SOLVED).all()
    dx = x - base.noise[sl]
    g = ext.hip_batch_adjoint_lockstep(x, y, dx, base.dy[sl], l=L0, u=U0, Px=base.Px[sl])
    for b in range(nb):
        _certified('Px alone', base.P_of(b), base.A, L0[b], U0[b], x[b], y[b], dx[b], base.dy[b], g, b, g['rec'][b])
    xs, ys, rs = ext.hip_batch_solve_lockstep(q=base.Q[sl], l=L0, u=U0)
    assert (rs[:, 0] == S.OSQP_SOLVED).all()
    dx = xs - base.noise[sl]
    gs = ext.hip_batch_adjoint_lockstep(xs, ys, dx, base.dy[sl], l=L0, u=U0)
    gt = ext.hip_batch_adjoint_lockstep(xs, ys, dx, base.dy[sl], l=L0, u=U0, Px=np.tile(base.Pu.data, (nb, 1)), Ax=np.tile(base.A.data, (nb, 1)))
    assert np.array_equal(gt['rec'][:, 0], gs['rec'][:, 0]) and (gs['rec'][:, 0] == 0).all() and np.array_equal(gt['rec'][:, 1], gs['rec'][:, 1])
    bitwise = all(np.array_equal(gt[k], gs[k]) for k in KEYS)
    for b in range(nb):
        res_t = ref.certificate(base.P, base.A, L0[b], U0[b], xs[b], ys[b], dx[b], base.dy[b], gt['dq'][b], gt['dl'][b], gt['du'][b])
        res_s = ref.certificate(base.P, base.A, L0[b], U0[b], xs[b], ys[b], dx[b], base.dy[b], gs['dq'][b], gs['dl'][b], gs['du'][b])
        smin = ref.adjoint(base.P, base.A, L0[b], U0[b], xs[b], ys[b], dx[b], base.dy[b])['sigma_min']
        dev = float(np.linalg.norm(res_t[2] - res_s[2]) / np.linalg.norm(res_s[2]))
        bound = _pair_bound(res_t, res_s, smin)
        record_deviation(TAG, 'tiles of the handle\'s values against the shared adjoint, element %d' % b, r_rel_dev=dev, bound=float(bound), bitwise=bool(bitwise))
        assert res_t[0] < TOL and res_t[3] == res_s[3] and dev <= bound, (b, dev, bound)
    print('tiles against the shared adjoint: bitwise equal = %s' % bitwise)


def test_device_pointers(base):
    """5. The device entry on torch tensors (the ragged chunk's 6) gives the host entry's bits; the nbatch == 0 query."""
    import torch
    dev = torch.device('cuda', 0)
    nb = 6
    t = lambda a: torch.tensor(a[64:64 + nb], dtype=torch.float64, device=dev).contiguous()
    xd, yd, gx, gy, ld, ud, pd, ad = t(base.x), t(base.y), t(base.dx), t(base.dy), t(base.L), t(base.U), t(base.Px), t(base.Ax)
    ext = base.s._solver
    widths = dict(dP=ext.nnz_P, dq=base.n, dA=ext.nnz_A, dl=base.m, du=base.m, rec=4)
    out = {k: torch.empty((nb, w), dtype=torch.float64, device=dev) for k, w in widths.items()}
    ext.hip_batch_adjoint_lockstep_device(0, None, None, None, Px_ptr=pd.data_ptr(), Ax_ptr=ad.data_ptr())      # the applicability query: no exception
    ext.hip_batch_adjoint_lockstep_device(nb, xd.data_ptr(), yd.data_ptr(), gx.data_ptr(), gy.data_ptr(), ld.data_ptr(), ud.data_ptr(),
                                          out['dP'].data_ptr(), out['dq'].data_ptr(), out['dA'].data_ptr(), out['dl'].data_ptr(), out['du'].data_ptr(), out['rec'].data_ptr(),
                                          stream=torch.cuda.current_stream(dev).cuda_stream, Px_ptr=pd.data_ptr(), Ax_ptr=ad.data_ptr())
    for k in KEYS:
        assert np.array_equal(out[k].cpu().numpy(), base.g[True][k][64:64 + nb]), k
    P, q, A, l, u = problems.portfolio_qp(200, 10)
    s1 = osqp_amd.OSQP(algebra='hip'); s1.setup(P, q, A, l, u, verbose=False, eps_abs=1e-6, eps_rel=1e-6, max_iter=20000)
    with pytest.raises(ValueError) as e:
        s1._solver.hip_batch_adjoint_lockstep_device(0, None, None, None, Px_ptr=0, Ax_ptr=0)
    assert e.value.code == NOT_IMPL


def test_reordered_handle(base, monkeypatch):
    """6. A handle that works on a permuted copy: certified on the element's own matrices, dP / dA at the caller's entries, agreement with the handle as numbered."""
    nb = 5
    monkeypatch.setenv('OSQP_HIP_REORDER', '2')
    s = _handle(base.P, base.q, base.A, base.l, base.u)
    assert s._solver.hip_stats()['reordered'] == 1
    sl = slice(0, nb)
    g = s._solver.hip_batch_adjoint_lockstep(base.x[sl], base.y[sl], base.dx[sl], base.dy[sl], l=base.L[sl], u=base.U[sl], Px=base.Px[sl], Ax=base.Ax[sl])
    for b in range(nb):
        Pb, Ab = base.P_of(b), base.A_of(b)
        res1 = ref.certificate(Pb, Ab, base.L[b], base.U[b], base.x[b], base.y[b], base.dx[b], base.dy[b], g['dq'][b], g['dl'][b], g['du'][b])
        res0 = base.certificate(True, b)
        assert res1[0] < TOL and g['rec'][b, 0] == 0 and g['rec'][b, 1] == res1[3] == res0[3], (b, res1[0], g['rec'][b])
        dP, dA = ref.gradients(Pb, Ab, base.x[b], base.y[b], g['dq'][b], -(g['dl'][b] + g['du'][b]))
        for got, want in ((g['dP'][b], dP), (g['dA'][b], dA)):
            assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), b
        smin = ref.adjoint(Pb, Ab, base.L[b], base.U[b], base.x[b], base.y[b], base.dx[b], base.dy[b])['sigma_min']
        dev = float(np.linalg.norm(res1[2] - res0[2]) / np.linalg.norm(res0[2]))
        bound = _pair_bound(res1, res0, smin)
        record_deviation(TAG, 'reordered against as numbered, element %d' % b, r_rel_dev=dev, bound=float(bound))
        assert dev <= bound, (b, dev, bound)


def test_statuses_in_one_chunk():
    """7. test_gpu_lockstep_adjoint.py::test_statuses_in_one_chunk (n = 420, P = diag, A = [I; I], caller-supplied x, y) with every element on its own
    Px = d_b and Ax = f_b A.data, f = (1, 3, 0.5, 2): bounds times f_b and duals over f_b keep each x that element's exact solution.  Statuses 0 / 2 / 3 / 0;
    the two solved elements certified on their own matrices, with the bits of their solo calls."""
    n = 420
    rng = np.random.default_rng(7)
    d0 = 0.5 + rng.random(n)
    P = sp.diags(d0, format='csc'); A = sp.vstack([sp.identity(n), sp.identity(n)], format='csc')
    l = np.concatenate([-np.ones(n), -2 * np.ones(n)]); u = np.concatenate([np.ones(n), 2 * np.ones(n)])
    s = osqp_amd.OSQP(algebra='hip'); s.setup(P, rng.standard_normal(n), A, l, u, verbose=False, eps_abs=1e-6, eps_rel=1e-6)
    nb, m = 4, 2 * n
    f = np.array([1.0, 3.0, 0.5, 2.0])
    Px = 0.5 + rng.random((nb, n))                                               # every element's own diagonal d_b
    Ax = f[:, None] * np.tile(A.data, (nb, 1))
    Ab = [sp.csc_matrix((Ax[b], A.indices, A.indptr), shape=A.shape) for b in range(nb)]
    Pb = [sp.diags(Px[b], format='csc') for b in range(nb)]
    L, U = f[:, None] * np.tile(l, (nb, 1)), f[:, None] * np.tile(u, (nb, 1))
    X, Y, DX, DY = np.zeros((nb, n)), np.zeros((nb, m)), rng.standard_normal((nb, n)), np.zeros((nb, m))
    for b in (0, 3):                     # the box problems' exact solutions: x = clip(-q / d_b, -1, 1), f_b y from stationarity d_b x + q + f_b y = 0
        q = 2.0 * rng.standard_normal(n)
        X[b] = np.clip(-q / Px[b], -1.0, 1.0)
        Y[b, :n] = np.where(np.abs(X[b]) == 1.0, -(Px[b] * X[b] + q), 0.0) / f[b]
        DY[b] = rng.standard_normal(m)
        assert 0 < np.count_nonzero(Y[b]) < n and _margin(Ab[b], L[b], U[b], X[b], Y[b]) >= 1e-9
        low, upp = ref.active_set(Ab[b], L[b], U[b], X[b], Y[b])
        assert int((low | upp).sum()) == np.count_nonzero(Y[b])
    X[1] = rng.standard_normal(n); L[1] = U[1] = f[1] * np.concatenate([X[1], X[1]]); Y[1] = rng.standard_normal(m) / f[1]      # every row an equality at a consistent b
    L[2] = -np.inf; U[2] = np.inf; L[2, [0, n]] = U[2, [0, n]] = 0.0; DY[2, 0], DY[2, n] = 1.0, -1.0                          # f x_0 = -1 and f x_0 = +1
    ext = s._solver
    g = ext.hip_batch_adjoint_lockstep(X, Y, DX, DY, l=L, u=U, Px=Px, Ax=Ax)
    rec = g['rec']
    print(rec)
    assert list(rec[:, 0]) == [0, 2, 3, 0], rec
    assert rec[1, 1] == 2 * n and rec[1, 3] == 0 and rec[2, 1] == 2 and rec[2, 3] > 0 and not (rec[2, 2] < TOL)
    for b in (0, 3):
        res = ref.certificate(Pb[b], Ab[b], L[b], U[b], X[b], Y[b], DX[b], DY[b], g['dq'][b], g['dl'][b], g['du'][b])
        assert res[0] < TOL and rec[b, 1] == res[3], (b, res[0], rec[b])
        sl = slice(b, b + 1)
        g1 = ext.hip_batch_adjoint_lockstep(X[sl], Y[sl], DX[sl], DY[sl], l=L[sl], u=U[sl], Px=Px[sl], Ax=Ax[sl])
        for k in KEYS:
            assert np.array_equal(g1[k][0], g[k][b]), (b, k)


def test_handle_is_left_alone(base):
    """8. solve(), update(q), solve(), a warm start and a third solve with the mat adjoint called in between, against a twin that never calls it: the
    handle's results, its scaling and the forward lockstep record do not move."""
    out = []
    q2 = base.Q[5]
    for call in (False, True):
        s = _handle(base.P, base.q, base.A, base.l, base.u, eps_abs=1e-6, eps_rel=1e-6)
        sc_a = s._solver.hip_scaling()
        adj = (lambda: s._solver.hip_batch_adjoint_lockstep(base.x[:3], base.y[:3], base.dx[:3], base.dy[:3], l=base.L[:3], u=base.U[:3], Px=base.Px[:3], Ax=base.Ax[:3])) \
            if call else (lambda: None)
        adj()
        ra = s.solve()
        adj()
        s.update(q=q2)
        rb = s.solve()
        adj()
        s.warm_start(x=ra.x, y=ra.y)
        adj()
        rc = s.solve()
        sc_b = s._solver.hip_scaling()
        assert np.array_equal(sc_a[0], sc_b[0]) and np.array_equal(sc_a[1], sc_b[1]) and sc_a[2] == sc_b[2]
        out.append((ra, rb, rc, s._solver.lockstep_last_record(), sc_b))
    for a, b in zip(out[0][:3], out[1][:3]):
        assert a.info.status_val == b.info.status_val == S.OSQP_SOLVED and a.info.iter == b.info.iter
        assert np.array_equal(a.x, b.x) and np.array_equal(a.y, b.y)
    assert out[0][3] == out[1][3] and out[1][3]['chunks'] == 0                   # the forward route's record has not moved
    assert np.array_equal(out[0][4][0], out[1][4][0]) and np.array_equal(out[0][4][1], out[1][4][1]) and out[0][4][2] == out[1][4][2]


def test_forward_unaffected(base):
    """9. forward mat call, mat adjoint call, the same forward again: the two forwards return the same bits; lockstep_mat_scaling is withdrawn by the
    adjoint call (it overwrites the matrix block) and answers again after the second forward."""
    ext = base.s._solver
    nb = 6
    sl = slice(64, 64 + nb)
    fwd = lambda: ext.hip_batch_solve_lockstep(q=base.Q[sl], l=base.L[sl], u=base.U[sl], Px=base.Px[sl], Ax=base.Ax[sl])
    x1, y1, r1 = fwd()
    sc1 = ext.lockstep_mat_scaling(0)
    g = base.call(slice(0, 3))
    assert (g['rec'][:, 0] == 0).all()
    with pytest.raises(ValueError) as e:
        ext.lockstep_mat_scaling(0)
    assert e.value.code == NOT_INIT
    x2, y2, r2 = fwd()
    sc2 = ext.lockstep_mat_scaling(0)
    assert np.array_equal(x1, x2) and np.array_equal(y1, y2) and np.array_equal(r1, r2)
    assert np.array_equal(sc1[0], sc2[0]) and np.array_equal(sc1[1], sc2[1]) and sc1[2] == sc2[2]
    assert np.array_equal(x1, base.x[sl]) and np.array_equal(r1, base.rec[sl])


@pytest.mark.parametrize('device', ['cpu', 'cuda'])
def test_torch_layer(base, device):
    """10. 2-D P_val / A_val / q / l / u, all requiring grad, loss 0.5 sum x^2: large_backward='lockstep' makes ONE call of the mat adjoint; every element
    certified on its own matrices, grad P_val / grad A_val per element against the host formulas; large_backward='loop' makes nb calls and agrees."""
    import torch
    from osqp_amd.nn.torch import OSQP as Layer
    nb = 3
    Pc = sp.csc_matrix(base.P); Pc.sort_indices()
    Ac = sp.csc_matrix(base.A); Ac.sort_indices()
    pco, aco = Pc.tocoo(), Ac.tocoo()
    mk = lambda **kw: Layer((pco.row, pco.col), Pc.shape, (aco.row, aco.col), Ac.shape, eps_rel=EPS, eps_abs=EPS, max_iter=200000, **kw)
    Pfull = np.stack([base.P_of(b).tocoo().data for b in range(nb)])              # (the pattern of every P_b is P's: same order of entries)
    assert all(np.array_equal(base.P_of(b).indices, Pc.indices) for b in (0, nb - 1)) and Pfull.shape == (nb, Pc.nnz)
    vals = [Pfull, base.Q[:nb], base.Ax[:nb], base.L[:nb], base.U[:nb]]
    got = {}
    for mode, kw, calls, mat_calls in (('lockstep', dict(large_batch='lockstep', large_backward='lockstep'), 1, 1), ('loop', dict(large_batch='lockstep', large_backward='loop'), nb, 0)):
        layer = mk(**kw)
        ts = [torch.tensor(np.array(v), dtype=torch.float64, device=device, requires_grad=True) for v in vals]
        x = layer(*ts)
        before = layer.adjoint_launches
        (0.5 * (x ** 2).sum()).backward()
        assert layer.adjoint_launches == before + calls and layer.mat_lockstep_adjoint_launches == mat_calls, (mode, layer.adjoint_launches - before, layer.mat_lockstep_adjoint_launches)
        rec = torch.as_tensor(layer.last_adjoint_rec).cpu().numpy()
        assert rec.shape == (nb, 4) and (rec[:, 0] == 0).all(), rec
        for t in ts:
            assert t.grad is not None and t.grad.shape == t.shape and t.grad.device == t.device and bool(torch.isfinite(t.grad).all())
        got[mode] = (x.detach().cpu().numpy(), torch.as_tensor(layer.last_dual).cpu().numpy(), [t.grad.cpu().numpy() for t in ts], rec, layer)
    X, Y, (gP, dq, gA, dl, du), rec, layer = got['lockstep']
    Xl, Yl, (gPl, dql, gAl, dll, dul), recl, _ = got['loop']
    assert np.array_equal(X, Xl) and np.array_equal(Y, Yl)                       # (the same forward call: both backwards start from the same (x, y))
    p_map = layer._p_map(Pc.nnz)
    for b in range(nb):
        Pb, Ab = base.P_of(b), base.A_of(b)
        res = ref.certificate(Pb, Ab, base.L[b], base.U[b], X[b], Y[b], X[b], None, dq[b], dl[b], du[b])
        assert res[0] < TOL and rec[b, 1] == res[3], (b, res[0], rec[b], res[3])
        dP, dA = ref.gradients(Pb, Ab, X[b], Y[b], dq[b], -(dl[b] + du[b]))
        assert np.abs(gP[b] - dP[p_map]).max() <= 1e-13 * np.abs(dP).max(), (b, np.abs(gP[b] - dP[p_map]).max() / np.abs(dP).max())
        assert np.abs(gA[b] - dA).max() <= 1e-13 * np.abs(dA).max(), (b, np.abs(gA[b] - dA).max() / np.abs(dA).max())
        resl = ref.certificate(Pb, Ab, base.L[b], base.U[b], X[b], Y[b], X[b], None, dql[b], dll[b], dul[b])
        smin = ref.adjoint(Pb, Ab, base.L[b], base.U[b], X[b], Y[b], X[b], None)['sigma_min']
        dev = float(np.linalg.norm(res[2] - resl[2]) / np.linalg.norm(resl[2]))
        bound = _pair_bound(res, resl, smin)
        record_deviation(TAG, 'torch layer (%s): one call against the per-element loop, element %d' % (device, b), r_rel_dev=dev, bound=float(bound))
        assert resl[0] < TOL and res[3] == resl[3] and dev <= bound, (b, dev, bound, resl[0])


def test_declines():
    """What osqp_hip_batch_solve_lockstep_mat declines, this entry declines: a repeated (j, j) entry in the stored upper triangle of P (the construction of
    test_gpu_lockstep_mat_declines.py) and a Woodbury handle -- for the host entry and the query, leaving the record zero."""
    n, m, nb = 6, 8, 3
    rng = np.random.default_rng(2)
    A = sp.random(m, n, density=0.5, random_state=rng, data_rvs=rng.standard_normal, format='csc')
    q = rng.standard_normal(n); l = -np.ones(m); u = np.ones(m)
    indptr, indices, data = [0], [], []
    for j in range(n):                                   # column j: (0, j) [j > 0], then the diagonal stored TWICE
        if j > 0:
            indices.append(0); data.append(0.1)
        indices += [j, j]; data += [0.7, 0.5]
        indptr.append(len(indices))
    Pdup = sp.csc_matrix((np.array(data), np.array(indices), np.array(indptr)), shape=(n, n))
    ext = osqp_amd.interface._backend('hip')
    st = ext.OSQPSettings(); ext.osqp_set_default_settings(st)
    st.verbose = 0; st.eps_abs = st.eps_rel = 1e-7
    solver = ext.OSQPSolver(ext.CSC(Pdup), q, ext.CSC(A), l, u, m, n, st)          # straight through the C ABI: the duplicates stay
    with pytest.raises(ValueError) as e:
        solver.hip_batch_adjoint_lockstep(np.zeros((nb, n)), np.zeros((nb, m)), np.ones((nb, n)), Ax=np.tile(A.data, (nb, 1)))
    assert e.value.code == NOT_IMPL
    with pytest.raises(ValueError) as e:
        solver.hip_batch_adjoint_lockstep_device(0, None, None, None, Px_ptr=0, Ax_ptr=0)
    assert e.value.code == NOT_IMPL
    assert all(v == 0 for v in solver.lockstep_mat_adjoint_last_record().values())
    solver.hip_batch_adjoint_lockstep_device(0, None, None, None)                  # (the shared adjoint serves this handle)
    P, q, A, l, u = problems.portfolio_qp(200, 10)
    s = osqp_amd.OSQP(algebra='hip'); s.setup(P, q, A, l, u, verbose=False, eps_abs=1e-6, eps_rel=1e-6, max_iter=20000)
    assert s._solver.hip_stats()['woodbury_rows'] > 0
    with pytest.raises(ValueError) as e:
        s._solver.hip_batch_adjoint_lockstep(np.zeros((nb, len(q))), np.zeros((nb, len(l))), np.ones((nb, len(q))), Ax=np.tile(sp.csc_matrix(A).data, (nb, 1)))
    assert e.value.code == NOT_IMPL
