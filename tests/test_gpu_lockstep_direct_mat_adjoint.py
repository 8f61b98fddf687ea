"""GPU tier: adjoint derivatives on the direct lockstep route with PER-PROBLEM MATRICES (include/osqp_hip.h osqp_hip_batch_adjoint_lockstep_direct_mat[_device];
osqp-python_amd/csrc/lockstep_hip.hip lockstep_direct_adjoint_chunk with a matrix block) -- the backward pass of osqp_hip_batch_solve_lockstep_direct_mat: a
batch of factor-model portfolio QPs on a Woodbury handle with a diagonal K0, every element's adjoint system on its own P_b, A_b (dense rows included) under
its own D_b, E_b, c_b.

Shape and data are test_gpu_lockstep_direct_mat.py's Base: portfolio_qp(600, 4) (n = 604, m = 605, r = 5), B = 70 (a full chunk and a ragged one of 6), that
file's _perturb, eps 1e-8; (x, y) come from its ONE forward call with per-element matrices.  dx = x - 0.1 N(0, 1), then dy = N(0, 1), both from
default_rng(7).  Input conditions, asserted per element on the element's own matrices: every inequality row keeps a class margin
min(|(z - l) + y|, |(u - z) - y|) >= 1e-9 and the active rows stay below n.  The checks and their bounds are test_gpu_lockstep_adjoint.py's (certificate
below OSQP_HIP_ADJOINT_TOL, the sparse yardstick, dP / dA to 1e-13 of max |value|, _pair_bound between two certified solutions), each taken on the element's
OWN matrices."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import adjoint_sparse_ref as ref
import osqp_amd
import problems
import test_gpu_lockstep_direct as fwd_shared
from osqp_amd import ext_hip
from util import record_deviation
from test_gpu_lockstep_direct_mat import Base, _perturb, _own, _csc
from test_gpu_lockstep_adjoint import TOL, B, PICK, KEYS, EPS, _margin, _pair_bound
from test_gpu_lockstep_direct_adjoint import _factor_qp, _one_dense_row

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
S = osqp_amd.SolverStatus
NOT_IMPL = ext_hip.osqp_error_type.OSQP_FUNC_NOT_IMPLEMENTED
TAG = 'test_gpu_lockstep_direct_mat_adjoint'
_handle = fwd_shared._handle


class AdjBase(Base):
    def __init__(self):
        super().__init__()
        assert (self.rec[:, 0] == S.OSQP_SOLVED).all()
        rng = np.random.default_rng(7)
        self.noise = 0.1 * rng.standard_normal((B, self.n))
        self.dx = self.x - self.noise
        self.dy = rng.standard_normal((B, self.m))
        ext = self.s._solver
        self.g, self.adj_last, self.adj_last_direct = {}, {}, {}
        for wd in (False, True):
            self.g[wd] = ext.hip_batch_adjoint_lockstep_direct(self.x, self.y, self.dx, self.dy if wd else None, l=self.L, u=self.U, Px=self.Px, Ax=self.Ax)
            self.adj_last[wd] = ext.lockstep_direct_mat_adjoint_last_record()
            self.adj_last_direct[wd] = ext.lockstep_direct_adjoint_last_record()
        self.cert = {}                       # (with_dy, b) -> (host residual, g, r, active rows) on the element's own matrices: computed once, shared

    def certificate(self, wd, b):
        if (wd, b) not in self.cert:
            g = self.g[wd]
            Pb, Ab = self.own(b)
            self.cert[(wd, b)] = ref.certificate(Pb, Ab, self.L[b], self.U[b], self.x[b], self.y[b], self.dx[b], self.dy[b] if wd else None,
                                                 g['dq'][b], g['dl'][b], g['du'][b])
        return self.cert[(wd, b)]

    def call(self, sl, ext=None, **kw):
        """the mat adjoint on the base batch's rows sl, with dy"""
        ext = ext or self.s._solver
        return ext.hip_batch_adjoint_lockstep_direct(self.x[sl], self.y[sl], self.dx[sl], self.dy[sl], l=self.L[sl], u=self.U[sl], Px=self.Px[sl], Ax=self.Ax[sl], **kw)


@pytest.fixture(scope='module')
def base():
    return AdjBase()


def _certified(tag, P, A, l, u, x, y, dx, dy, g, b):
    """test 1's check of one element: the input conditions, certificate below TOL on (P, A), status 0, the host's active rows, the record's residual within
    x10 of the host's both ways."""
    rec = g['rec'][b]
    margin = _margin(A, l, u, x, y)
    assert margin >= 1e-9, (tag, b, margin)
    host_res, gv, rv, nact = ref.certificate(P, A, l, u, x, y, dx, dy, g['dq'][b], g['dl'][b], g['du'][b])
    print('%s element %d: margin %.2e, host residual %.3e, record %s' % (tag, b, margin, host_res, rec))
    assert nact < len(x), (tag, b, nact)
    assert host_res < TOL, (tag, b, host_res)
    assert rec[0] == 0 and rec[1] == nact, (tag, b, rec, nact)
    assert rec[2] < TOL and rec[2] <= 10 * host_res and host_res <= 10 * rec[2], (tag, b, rec[2], host_res)
    return host_res, gv, rv, nact


def test_certificate_every_element(base):
    """1. Every element, with and without dy, on its OWN matrices: certificate below the threshold, status 0, the host's active rows, the record's residual
    within a factor 10 of the host's, both ways; the record (one inversion of S per problem), the direct adjoint record moving with it; hip_batch_adjoint
    and hip_batch_adjoint_lockstep(Px=, Ax=) still decline the handle."""
    assert (base.n, base.m) == (604, 605) and base.s._solver.hip_stats()['woodbury_rows'] == 5
    for b in range(B):
        Pb, Ab = base.own(b)
        margin = _margin(Ab, base.L[b], base.U[b], base.x[b], base.y[b])
        assert margin >= 1e-9, (b, margin)
    worst = 0.0
    for wd in (False, True):
        last, direct, rec = base.adj_last[wd], base.adj_last_direct[wd], base.g[wd]['rec']
        print('direct lockstep-mat adjoint B=70 dy=%s: %s' % (wd, last))
        assert last['chunks'] == 2 and last['width'] == 64 and last['inversions'] == B and last['matrix_block_bytes'] > 0, last
        assert 0 < last['prepare_gpu_ms'] < last['gpu_ms'], last
        assert all(direct[k] == last[k] for k in ('chunks', 'width', 'steps_max', 'inversions', 'kernel_launches', 'gpu_ms')), (direct, last)
        for b in range(B):
            host_res, gv, rv, nact = base.certificate(wd, b)
            worst = max(worst, host_res)
            assert nact < base.n, (b, nact)
            assert host_res < TOL, (wd, b, host_res)
            assert rec[b, 0] == 0 and rec[b, 1] == nact, (wd, b, rec[b], nact)
            assert rec[b, 2] < TOL and rec[b, 2] <= 10 * host_res and host_res <= 10 * rec[b, 2], (wd, b, rec[b, 2], host_res)
        assert last['steps_max'] == rec[:, 3].max()
        record_deviation(TAG, 'certificate, 70 elements, dy=%s' % wd, worst_host_residual=worst, tol=TOL, steps_max=last['steps_max'], inversions=last['inversions'],
                         kernel_launches=last['kernel_launches'], gpu_ms=last['gpu_ms'], prepare_gpu_ms=last['prepare_gpu_ms'])
    print('worst host residual %.3e' % worst)
    ext = base.s._solver
    for route in (ext.hip_batch_adjoint, ext.hip_batch_adjoint_lockstep):
        with pytest.raises(ValueError) as e:
            route(base.x, base.y, base.dx, l=base.L, u=base.U, Px=base.Px, Ax=base.Ax)
        assert e.value.code == NOT_IMPL


@pytest.mark.parametrize('with_dy', [False, True])
def test_yardstick(base, with_dy):
    """2. |r - r_ref| / |r_ref| <= 10 res |g| / (sigma_min |r_ref|) against the sparse reference on the element's own matrices; dP / dA at every stored
    entry -- the dense rows' on their own as well -- against the host formulas to 1e-13 of max |value|."""
    g = base.g[with_dy]
    dense = np.diff(sp.csr_matrix(base.A).indptr) > 128
    assert int(dense.sum()) == 5
    in_dense = dense[base.A.tocoo().row]      # (tocoo of a CSC matrix keeps the CSC order: adjoint_sparse_ref.stored_entries)
    for b in PICK:
        Pb, Ab = base.own(b)
        host_res, gv, rv, nact = base.certificate(with_dy, b)
        y0 = ref.adjoint(Pb, Ab, base.L[b], base.U[b], base.x[b], base.y[b], base.dx[b], base.dy[b] if with_dy else None)
        r_ref = np.concatenate([y0['r_x'], y0['r_y'][y0['act']]])
        dev = float(np.linalg.norm(rv - r_ref) / np.linalg.norm(r_ref))
        bound = 10 * host_res * np.linalg.norm(gv) / (y0['sigma_min'] * np.linalg.norm(r_ref))
        record_deviation(TAG, 'portfolio 600x4 own matrices, element %d dy=%s' % (b, with_dy), r_rel_dev=dev, bound=float(bound), host_residual=host_res,
                         record_residual=float(g['rec'][b, 2]), active_rows=nact, steps=int(g['rec'][b, 3]), sigma_min=y0['sigma_min'])
        print('element %d dy=%s: |r - r_ref| / |r_ref| = %.3e (bound %.3e), sigma_min %.3e, steps %d' % (b, with_dy, dev, bound, y0['sigma_min'], g['rec'][b, 3]))
        assert dev <= bound, (b, dev, bound)
        dP, dA = ref.gradients(Pb, Ab, base.x[b], base.y[b], g['dq'][b], -(g['dl'][b] + g['du'][b]))
        for name, got, want in (('dP', g['dP'][b], dP), ('dA', g['dA'][b], dA), ('dA dense rows', g['dA'][b][in_dense], dA[in_dense])):
            assert got.shape == want.shape and got.size > 0
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
    gr = base.call(slice(None, None, -1))
    for k in KEYS:
        assert np.array_equal(gr[k][::-1], g[k]), k


def test_one_side_only(base):
    """4. Ax alone and Px alone (the other side is the handle's own), at the (x, y) of the matching forward: certified as in test 1 on the matrices the element
    was solved with.  Tiles of the handle's own values against the shared direct adjoint at the same inputs: same statuses and active rows, r within
    _pair_bound; whether the two are bitwise equal is recorded, not required."""
    ext = base.s._solver
    nb = 6
    sl = slice(0, nb)
    kw = dict(q=base.Q[sl], l=base.L[sl], u=base.U[sl])
    for side in ('Ax', 'Px'):
        mk = {side: getattr(base, side)[sl]}
        x, y, rec = ext.hip_batch_solve_lockstep_direct(**kw, **mk)
        assert (rec[:, 0] == S.OSQP_SOLVED).all(), (side, rec[:, 0])
        dx = x - base.noise[sl]
        g = ext.hip_batch_adjoint_lockstep_direct(x, y, dx, base.dy[sl], l=base.L[sl], u=base.U[sl], **mk)
        assert ext.lockstep_direct_mat_adjoint_last_record()['inversions'] == nb
        for b in range(nb):
            Pb, Ab = base.own(b)
            _certified(side + ' alone', Pb if side == 'Px' else base.P, Ab if side == 'Ax' else base.A, base.L[b], base.U[b], x[b], y[b], dx[b], base.dy[b], g, b)
    nt = 3
    st = slice(0, nt)
    xs, ys, rs = ext.hip_batch_solve_lockstep_direct(q=base.Q[st], l=base.L[st], u=base.U[st])
    assert (rs[:, 0] == S.OSQP_SOLVED).all()
    dx = xs - base.noise[st]
    gs = ext.hip_batch_adjoint_lockstep_direct(xs, ys, dx, base.dy[st], l=base.L[st], u=base.U[st])
    gt = ext.hip_batch_adjoint_lockstep_direct(xs, ys, dx, base.dy[st], l=base.L[st], u=base.U[st], Px=np.tile(base.P.data, (nt, 1)), Ax=np.tile(base.A.data, (nt, 1)))
    assert np.array_equal(gt['rec'][:, 0], gs['rec'][:, 0]) and (gs['rec'][:, 0] == 0).all() and np.array_equal(gt['rec'][:, 1], gs['rec'][:, 1])
    bitwise = all(np.array_equal(gt[k], gs[k]) for k in KEYS)
    for b in range(nt):
        res_t = ref.certificate(base.P, base.A, base.L[b], base.U[b], xs[b], ys[b], dx[b], base.dy[b], gt['dq'][b], gt['dl'][b], gt['du'][b])
        res_s = ref.certificate(base.P, base.A, base.L[b], base.U[b], xs[b], ys[b], dx[b], base.dy[b], gs['dq'][b], gs['dl'][b], gs['du'][b])
        smin = ref.adjoint(base.P, base.A, base.L[b], base.U[b], xs[b], ys[b], dx[b], base.dy[b])['sigma_min']
        dev = float(np.linalg.norm(res_t[2] - res_s[2]) / np.linalg.norm(res_s[2]))
        bound = _pair_bound(res_t, res_s, smin)
        record_deviation(TAG, 'tiles of the handle\'s values against the shared direct adjoint, element %d' % b, r_rel_dev=dev, bound=float(bound), bitwise=bool(bitwise))
        assert res_t[0] < TOL and res_s[0] < TOL and res_t[3] == res_s[3] and dev <= bound, (b, dev, bound)
    print('tiles against the shared direct adjoint: bitwise equal = %s' % bitwise)


def _edge(P, q, A, l, u, r):
    """5. test_gpu_lockstep_direct_mat.py _edge's three perturbed elements: SOLVED by the forward with own matrices, then the backward on them: certified on the
    element's own matrices, one inversion of S each."""
    P, A = _csc(sp.triu(P)), _csc(A)
    n, m = len(q), len(l)
    rng = np.random.default_rng(5)
    Q = np.stack([q * (1.0 + 0.3 * b) + 0.1 * b * rng.standard_normal(n) * (q != 0) for b in range(3)])
    L, U = np.tile(l, (3, 1)), np.tile(u, (3, 1))
    Px, Ax = _perturb(P, A, 3)
    s = _handle(P, q, A, l, u)
    assert s._solver.hip_stats()['woodbury_rows'] == r
    x, y, rec = s._solver.hip_batch_solve_lockstep_direct(q=Q, l=L, u=U, Px=Px, Ax=Ax)
    assert (rec[:, 0] == S.OSQP_SOLVED).all(), rec[:, 0]
    rng = np.random.default_rng(7)
    dx = x - 0.1 * rng.standard_normal((3, n))
    dy = rng.standard_normal((3, m))
    g = s._solver.hip_batch_adjoint_lockstep_direct(x, y, dx, dy, l=L, u=U, Px=Px, Ax=Ax)
    last = s._solver.lockstep_direct_mat_adjoint_last_record()
    print('r = %d: %s' % (r, last))
    assert last['chunks'] == 1 and last['inversions'] == 3, last
    for b in range(3):
        Pb, Ab = _own(P, A, Px, Ax, b)
        host_res, gv, rv, nact = _certified('r = %d' % r, Pb, Ab, L[b], U[b], x[b], y[b], dx[b], dy[b], g, b)
        record_deviation(TAG, 'r = %d element %d' % (r, b), host_residual=host_res, record_residual=float(g['rec'][b, 2]), active_rows=nact, steps=int(g['rec'][b, 3]), tol=TOL)


def test_one_dense_row():
    P, q, A, l, u = _one_dense_row()
    assert int((np.diff(sp.csr_matrix(A).indptr) > 128).sum()) == 1
    _edge(P, q, A, l, u, 1)


def test_128_dense_rows():
    P, q, A, l, u = _factor_qp(400, 127, 0.7)
    assert len(q) == 527 and int((np.diff(sp.csr_matrix(A).indptr) > 128).sum()) == 128
    _edge(P, q, A, l, u, 128)


def test_statuses_in_one_chunk():
    """6. test_gpu_lockstep_direct_adjoint.py::test_statuses_in_one_chunk (n = 500, P diagonal, A = [budget; I; e_0'], r = 1) with every element on its own
    Px = d_b and Ax = f_b A.data, f = (1, 3, 0.5, 2), bounds times f_b: an element solved by the forward on its own matrices (status 0), every row an equality
    at a consistent point (status 2, no step), the two copies of the row of x_0 as equalities with contradicting dy (status 3), another solved element;
    the two solved elements are certified on their own matrices and carry the bits of their solo calls."""
    n = 500
    rng = np.random.default_rng(2)
    P = sp.diags(0.5 + rng.random(n), format='csc')
    budget = sp.csc_matrix((np.ones(200), (np.zeros(200, dtype=int), np.arange(0, 400, 2))), shape=(1, n))
    e0 = sp.csc_matrix(([1.0], ([0], [0])), shape=(1, n))
    A = _csc(sp.vstack([budget, sp.identity(n), e0], format='csc'))
    q = rng.standard_normal(n)
    l, u = np.concatenate([[1.0], np.zeros(n), [-10.0]]), np.concatenate([[1.0], np.ones(n), [10.0]])
    nb, m = 4, n + 2
    s = _handle(P, q, A, l, u)
    ext = s._solver
    assert ext.hip_stats()['woodbury_rows'] == 1
    f = np.array([1.0, 3.0, 0.5, 2.0])
    Px = 0.5 + rng.random((nb, n))                                               # every element's own diagonal d_b
    Ax = f[:, None] * np.tile(A.data, (nb, 1))
    Ab = [sp.csc_matrix((Ax[b], A.indices, A.indptr), shape=A.shape) for b in range(nb)]
    Pb = [sp.diags(Px[b], format='csc') for b in range(nb)]
    Q = np.stack([q, q, q, 1.3 * q + 0.1 * rng.standard_normal(n)])
    L, U = f[:, None] * np.tile(l, (nb, 1)), f[:, None] * np.tile(u, (nb, 1))
    ok = [0, 3]
    xf, yf, recf = ext.hip_batch_solve_lockstep_direct(q=Q[ok], l=L[ok], u=U[ok], Px=Px[ok], Ax=Ax[ok])
    assert (recf[:, 0] == S.OSQP_SOLVED).all(), recf[:, 0]
    X, Y, DX, DY = np.zeros((nb, n)), np.zeros((nb, m)), rng.standard_normal((nb, n)), np.zeros((nb, m))
    for k, b in enumerate(ok):
        X[b], Y[b], DY[b] = xf[k], yf[k], rng.standard_normal(m)
        assert _margin(Ab[b], L[b], U[b], X[b], Y[b]) >= 1e-9
    X[1] = rng.standard_normal(n); L[1] = U[1] = Ab[1] @ X[1]; Y[1] = rng.standard_normal(m)                      # every row an equality at a consistent point
    L[2] = -np.inf; U[2] = np.inf; L[2, [1, n + 1]] = U[2, [1, n + 1]] = 0.0; DY[2, 1], DY[2, n + 1] = 1.0, -1.0      # f x_0 = -1 and f x_0 = +1
    call = lambda sl: ext.hip_batch_adjoint_lockstep_direct(X[sl], Y[sl], DX[sl], DY[sl], l=L[sl], u=U[sl], Px=Px[sl], Ax=Ax[sl])
    g = call(slice(None))
    rec = g['rec']
    print(rec)
    assert list(rec[:, 0]) == [0, 2, 3, 0], rec
    assert rec[1, 1] == n + 2 and rec[1, 3] == 0 and rec[2, 1] == 2 and rec[2, 3] > 0 and not (rec[2, 2] < TOL)
    for b in ok:
        res = ref.certificate(Pb[b], Ab[b], L[b], U[b], X[b], Y[b], DX[b], DY[b], g['dq'][b], g['dl'][b], g['du'][b])
        assert res[0] < TOL and rec[b, 1] == res[3], (b, res[0], rec[b])
        g1 = call(slice(b, b + 1))
        for k in KEYS:
            assert np.array_equal(g1[k][0], g[k][b]), (b, k)


def test_device_pointers(base):
    """7. The device entry on torch tensors (the ragged chunk's 6) gives the host entry's bits; the nbatch == 0 query answers."""
    import torch
    dev = torch.device('cuda', 0)
    nb = 6
    t = lambda a: torch.tensor(a[64:64 + nb], dtype=torch.float64, device=dev).contiguous()
    xd, yd, gx, gy, ld, ud, pd, ad = t(base.x), t(base.y), t(base.dx), t(base.dy), t(base.L), t(base.U), t(base.Px), t(base.Ax)
    ext = base.s._solver
    widths = dict(dP=ext.nnz_P, dq=base.n, dA=ext.nnz_A, dl=base.m, du=base.m, rec=4)
    out = {k: torch.empty((nb, w), dtype=torch.float64, device=dev) for k, w in widths.items()}
    ext.hip_batch_adjoint_lockstep_direct_device(0, None, None, None, Px_ptr=pd.data_ptr(), Ax_ptr=ad.data_ptr())      # the applicability query: no exception
    torch.cuda.synchronize()
    ext.hip_batch_adjoint_lockstep_direct_device(nb, xd.data_ptr(), yd.data_ptr(), gx.data_ptr(), gy.data_ptr(), ld.data_ptr(), ud.data_ptr(),
                                                 out['dP'].data_ptr(), out['dq'].data_ptr(), out['dA'].data_ptr(), out['dl'].data_ptr(), out['du'].data_ptr(), out['rec'].data_ptr(),
                                                 stream=torch.cuda.current_stream(dev).cuda_stream, Px_ptr=pd.data_ptr(), Ax_ptr=ad.data_ptr())
    for k in KEYS:
        assert np.array_equal(out[k].cpu().numpy(), base.g[True][k][64:64 + nb]), k


def test_declines(base, monkeypatch):
    """8. A banded handle, r = 129, a repeated (j, j) entry in the stored triangle of P (through the C ABI) and a reordered handle: both entries and the
    query answer OSQP_FUNC_NOT_IMPLEMENTED and the new record stays zero."""
    def declined(solver, n, m, nzA):
        for call in (lambda: solver.hip_batch_adjoint_lockstep_direct(np.zeros((3, n)), np.zeros((3, m)), np.ones((3, n)), Ax=np.ones((3, nzA))),
                     lambda: solver.hip_batch_adjoint_lockstep_direct_device(3, 0, 0, 0, Px_ptr=0, Ax_ptr=0),
                     lambda: solver.hip_batch_adjoint_lockstep_direct_device(0, None, None, None, Px_ptr=0, Ax_ptr=0)):
            with pytest.raises(ValueError) as e:
                call()
            assert e.value.code == NOT_IMPL
        assert all(v == 0 for v in solver.lockstep_direct_mat_adjoint_last_record().values())

    for data, rows in ((problems.banded_qp(400, window=40), 0), (_factor_qp(400, 128, 0.7), None)):
        P, q, A, l, u = data
        if rows is None:
            assert int((np.diff(sp.csr_matrix(A).indptr) > 128).sum()) == 129
        s = _handle(P, q, _csc(A), l, u, eps_abs=1e-6, eps_rel=1e-6)
        if rows is not None:
            assert s._solver.hip_stats()['woodbury_rows'] == rows
        declined(s._solver, len(q), len(l), _csc(A).nnz)
    d = base.P.diagonal()                     # a repeated (j, j), straight through the C ABI (the duplicates stay): test_gpu_lockstep_direct_mat.py test_declines
    Pdup = sp.csc_matrix((np.repeat(0.5 * d, 2), np.repeat(np.arange(base.n), 2), 2 * np.arange(base.n + 1)), shape=(base.n, base.n))
    ext = osqp_amd.interface._backend('hip')
    st = ext.OSQPSettings(); ext.osqp_set_default_settings(st)
    st.verbose = 0; st.eps_abs = st.eps_rel = 1e-7
    solver = ext.OSQPSolver(ext.CSC(Pdup), base.q, ext.CSC(base.A), base.l, base.u, base.m, base.n, st)
    declined(solver, base.n, base.m, base.A.nnz)
    monkeypatch.setenv('OSQP_HIP_REORDER', '2')
    s = _handle(base.P, base.q, base.A, base.l, base.u)
    assert s._solver.hip_stats()['reordered'] == 1 and s._solver.hip_stats()['woodbury_rows'] == 5
    declined(s._solver, base.n, base.m, base.A.nnz)


def test_handle_and_forward_left_alone(base):
    """9. solve(), update(q), solve(), a warm start and a third solve with the new call in between, against a twin that never calls it: identical bits and
    scaling, the forward records unmoved.  And the forward call with per-element matrices before and after an adjoint call returns the same bits."""
    out = []
    q2 = base.Q[5]
    for call in (False, True):
        s = _handle(base.P, base.q, base.A, base.l, base.u, eps_abs=1e-6, eps_rel=1e-6, warm_starting=True)
        sc_a = s._solver.hip_scaling()
        adj = (lambda: base.call(slice(0, 3), ext=s._solver)) if call else (lambda: None)
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
        out.append((ra, rb, rc, (s._solver.lockstep_direct_last_record(), s._solver.lockstep_direct_mat_last_record()), sc_b, s._solver.lockstep_direct_mat_adjoint_last_record()))
    for a, b in zip(out[0][:3], out[1][:3]):
        assert a.info.status_val == b.info.status_val == S.OSQP_SOLVED and a.info.iter == b.info.iter
        assert np.array_equal(a.x, b.x) and np.array_equal(a.y, b.y)
    assert out[0][3] == out[1][3] and all(r['chunks'] == 0 for r in out[1][3])                   # the forward routes' records have not moved
    assert np.array_equal(out[0][4][0], out[1][4][0]) and np.array_equal(out[0][4][1], out[1][4][1]) and out[0][4][2] == out[1][4][2]
    assert out[0][5]['chunks'] == 0 and out[1][5]['chunks'] == 1 and out[1][5]['inversions'] == 3
    ext = base.s._solver
    sl = slice(64, 70)
    x1, y1, r1 = ext.hip_batch_solve_lockstep_direct(**base.rows(sl))
    recs = (ext.lockstep_direct_last_record(), ext.lockstep_direct_mat_last_record())
    g = base.call(slice(0, 3))
    assert (g['rec'][:, 0] == 0).all()
    assert recs == (ext.lockstep_direct_last_record(), ext.lockstep_direct_mat_last_record())
    x2, y2, r2 = ext.hip_batch_solve_lockstep_direct(**base.rows(sl))
    assert np.array_equal(x1, x2) and np.array_equal(y1, y2) and np.array_equal(r1, r2)
    assert np.array_equal(x1, base.x[sl]) and np.array_equal(r1, base.rec[sl])


@pytest.mark.parametrize('device', ['cpu', 'cuda'])
def test_torch_layer(base, device):
    """10. 2-D P_val / q / A_val / l / u, all requiring grad, loss 0.5 sum x^2, large_batch = large_backward = 'lockstep_direct': the backward makes ONE call
    of the direct adjoint with per-element matrices; every element certified on its own matrices, grad P_val / grad A_val per element against the host
    formulas.  (On the parent commit this backward raises NotImplementedError.)"""
    import torch
    from osqp_amd.nn.torch import OSQP as Layer
    nb = 3
    Pc, Ac = base.P, base.A                                                           # (P is diagonal: its full pattern is its upper triangle)
    pco, aco = Pc.tocoo(), Ac.tocoo()
    layer = Layer((pco.row, pco.col), Pc.shape, (aco.row, aco.col), Ac.shape, eps_rel=EPS, eps_abs=EPS, max_iter=200000, large_batch='lockstep_direct', large_backward='lockstep_direct')
    vals = [base.Px[:nb], base.Q[:nb], base.Ax[:nb], base.L[:nb], base.U[:nb]]
    ts = [torch.tensor(np.array(v), dtype=torch.float64, device=device, requires_grad=True) for v in vals]
    x = layer(*ts)
    assert layer.mat_lockstep_direct_launches == 1
    before = layer.adjoint_launches
    (0.5 * (x ** 2).sum()).backward()
    assert layer.adjoint_launches == before + 1 and layer.mat_lockstep_direct_adjoint_launches == 1 and layer.mat_lockstep_adjoint_launches == 0
    last = layer._solver._solver.lockstep_direct_mat_adjoint_last_record()
    assert last['chunks'] == 1 and last['inversions'] == nb, last
    rec = torch.as_tensor(layer.last_adjoint_rec).cpu().numpy()
    assert rec.shape == (nb, 4) and (rec[:, 0] == 0).all(), rec
    for t in ts:
        assert t.grad is not None and t.grad.shape == t.shape and t.grad.device == t.device and bool(torch.isfinite(t.grad).all())
    X, Y = x.detach().cpu().numpy(), torch.as_tensor(layer.last_dual).cpu().numpy()
    gP, dq, gA, dl, du = (t.grad.cpu().numpy() for t in ts)
    p_map = layer._p_map(Pc.nnz)
    for b in range(nb):
        Pb, Ab = base.own(b)
        assert _margin(Ab, base.L[b], base.U[b], X[b], Y[b]) >= 1e-9
        res = ref.certificate(Pb, Ab, base.L[b], base.U[b], X[b], Y[b], X[b], None, dq[b], dl[b], du[b])
        assert res[0] < TOL and rec[b, 1] == res[3] and res[3] < base.n, (b, res[0], rec[b], res[3])
        dP, dA = ref.gradients(Pb, Ab, X[b], Y[b], dq[b], -(dl[b] + du[b]))
        assert np.abs(gP[b] - dP[p_map]).max() <= 1e-13 * np.abs(dP).max(), (b, np.abs(gP[b] - dP[p_map]).max() / np.abs(dP).max())
        assert np.abs(gA[b] - dA).max() <= 1e-13 * np.abs(dA).max(), (b, np.abs(gA[b] - dA).max() / np.abs(dA).max())
