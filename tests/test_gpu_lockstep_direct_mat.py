"""GPU tier: the direct lockstep route with PER-PROBLEM MATRICES (osqp_hip_batch_solve_lockstep_direct_mat[_device]; osqp-python_amd/csrc/lockstep_hip.hip
lockstep_direct_chunk with mat_ws) -- a batch of factor-model portfolio QPs on a Woodbury handle with a diagonal K0 whose elements have their own values
of P and A on the handle's pattern: element b is solved as a handle set up with (P_b, q_b, A_b, l_b, u_b) alone would solve it.

Yardsticks: those of test_gpu_lockstep_direct.py -- eps = 1e-8, check_termination = 25, adaptive_rho_interval = 50, ATOL = 2e-6 relative to the solution's
scale between two eps = 1e-8 iterates of one QP, and that file's _certify rule evaluated on the element's OWN P_b, A_b.

Inputs: problems.portfolio_qp(600, 4) (n = 604, m = 605, r = 5, nnz(A) = 2404, 604 stored entries of P), B = 70 (one full chunk and a ragged one of 6);
rng = default_rng(3): Ax = A.data (1 + 0.1 N(0, 1)), then Px = triu(P).data (1 + 0.2 U(0, 1)), per element and entry; Q is that file's, L, U the base's.
On the CPU oracle the elements 0, 5, 63, 64, 69 of exactly this batch end SOLVED at eps 1e-8 in 425-1675 iterations; the three elements of the r = 1 and
of the r = 128 batch below (the same perturbation, unnarrowed) end SOLVED there too (r = 1: 825 / 1050 / 1225 iterations, r = 128: 475 / 300 / 550)."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_amd
import problems
import test_gpu_lockstep_direct as shared
from osqp_amd import ext_hip
from oracle import Oracle, SOLVED
from util import record_deviation

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
S = osqp_amd.SolverStatus
NOT_IMPL = ext_hip.osqp_error_type.OSQP_FUNC_NOT_IMPLEMENTED
EPS, ATOL, B, PICK, ST = shared.EPS, shared.ATOL, shared.B, shared.PICK, shared.ST
REC_STATUS, REC_ITER, REC_OBJ, REC_PCG = shared.REC_STATUS, shared.REC_ITER, shared.REC_OBJ, shared.REC_PCG
_handle, _certify, _close = shared._handle, shared._certify, shared._close


def _csc(M):
    M = sp.csc_matrix(M)
    M.sort_indices()
    return M


def _perturb(P, A, nb, a_width=0.1):
    """(Px, Ax): nb rows of values on the patterns of triu(P) and A -- Ax first, then Px, from one default_rng(3)"""
    rng = np.random.default_rng(3)
    Ax = A.data * (1.0 + a_width * rng.standard_normal((nb, A.nnz)))
    Px = P.data * (1.0 + 0.2 * rng.random((nb, P.nnz)))
    return Px, Ax


def _own(P, A, Px, Ax, b):
    """element b's own matrices"""
    return sp.csc_matrix((Px[b], P.indices, P.indptr), shape=P.shape), sp.csc_matrix((Ax[b], A.indices, A.indptr), shape=A.shape)


class Base:
    NA, K = 600, 4

    def __init__(self):
        P, self.q, A, self.l, self.u = problems.portfolio_qp(self.NA, self.K)
        self.P, self.A = _csc(sp.triu(P)), _csc(A)
        self.n, self.m = len(self.q), len(self.l)
        rng = np.random.default_rng(17)
        self.Q = np.stack([np.concatenate([-rng.standard_normal(self.NA) / (1.0 + 0.05 * b), np.zeros(self.K)]) for b in range(B)])      # test_gpu_lockstep_direct.py Base
        self.L, self.U = np.tile(self.l, (B, 1)), np.tile(self.u, (B, 1))
        self.Px, self.Ax = _perturb(self.P, self.A, B)
        self.s = _handle(self.P, self.q, self.A, self.l, self.u)
        self.kw = dict(q=self.Q, l=self.L, u=self.U, Px=self.Px, Ax=self.Ax)
        self.x, self.y, self.rec = self.s._solver.hip_batch_solve_lockstep_direct(**self.kw)
        self.last = self.s._solver.lockstep_direct_mat_last_record()
        self.last_direct = self.s._solver.lockstep_direct_last_record()

    def own(self, b):
        return _own(self.P, self.A, self.Px, self.Ax, b)

    def rows(self, idx):
        return dict(q=self.Q[idx], l=self.L[idx], u=self.U[idx], Px=self.Px[idx], Ax=self.Ax[idx])


@pytest.fixture(scope='module')
def base():
    return Base()


def _fresh(Pb, q, Ab, l, u, **kw):
    """a handle set up with the element's data alone, solved by the shared direct call on a batch of one: x, y, record"""
    s = _handle(Pb, q, Ab, l, u, **kw)
    x, y, rec = s._solver.hip_batch_solve_lockstep_direct(nbatch=1)
    return x[0], y[0], rec[0]


def test_the_route(base):
    """hip_batch_solve and hip_batch_solve_lockstep decline such a batch; the new call solves all 70 and every element is certified on its OWN matrices;
    four of them are held to the oracle at eps 1e-9 on their own matrices.  (On the parent commit the keyword does not exist.)"""
    assert (base.n, base.m, base.A.nnz, base.P.nnz) == (604, 605, 2404, 604)
    assert base.s._solver.hip_stats()['woodbury_rows'] == 5
    for route in (base.s._solver.hip_batch_solve, base.s._solver.hip_batch_solve_lockstep):
        with pytest.raises(ValueError) as e:
            route(**base.kw)
        assert e.value.code == NOT_IMPL
    base.s._solver.hip_batch_solve_lockstep_direct_device(0, None, None, None, None, None, None, Px_ptr=0, Ax_ptr=0)      # the applicability query: no exception
    assert (base.rec[:, REC_STATUS] == S.OSQP_SOLVED).all(), base.rec[:, REC_STATUS]
    assert (base.rec[:, REC_PCG] == 0).all()
    last = base.last
    print('record', last)
    assert last['chunks'] == 2 and last['width'] == 64 and last['admm_iters_max'] == base.rec[:, REC_ITER].max()
    assert last['matrix_block_bytes'] > 0 and 0 < last['prepare_gpu_ms'] < last['gpu_ms']
    assert all(base.last_direct[k] == last[k] for k in ('chunks', 'width', 'admm_iters_max', 'factorisations', 'kernel_launches', 'gpu_ms'))      # the direct route's own record moves too
    for b in range(B):
        Pb, Ab = base.own(b)
        _certify(Pb, base.Q[b], Ab, base.L[b], base.U[b], base.x[b], base.y[b], base.rec[b, REC_OBJ])
    for b in PICK:
        Pb, Ab = base.own(b)
        st = dict(ST, eps_abs=1e-9, eps_rel=1e-9); st.pop('warm_starting')
        xo, yo, io = Oracle().setup(Pb, base.Q[b], Ab, base.L[b], base.U[b], **st).solve()
        assert io.status_val == SOLVED
        ex, ey = _close(base.x[b], xo), _close(base.y[b], yo)
        record_deviation('lockstep_direct_mat_vs_oracle', 'portfolio 600x4 element %d' % b, dx_rel=ex, dy_rel=ey, iters=int(base.rec[b, REC_ITER]), oracle_iters=io.iter, atol=ATOL)
        print('element %d: direct lockstep (own matrices) %d iterations, oracle %d; |dx| %.2e |dy| %.2e (relative)' % (b, base.rec[b, REC_ITER], io.iter, ex, ey))
        assert ex <= ATOL and ey <= ATOL


def test_the_elements_own_handle(base):
    """Elements 0 and 5 of a batch of 6 against a FRESH handle set up with that element's data (the shared direct call, nbatch = 1): x, y at ATOL.  The rho
    rule and the scaling are the same, so equal iteration counts are expected; both are printed and recorded."""
    x, y, rec = base.s._solver.hip_batch_solve_lockstep_direct(**base.rows(slice(0, 6)))
    assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all()
    for b in (0, 5):
        Pb, Ab = base.own(b)
        xf, yf, rf = _fresh(Pb, base.Q[b], Ab, base.L[b], base.U[b])
        assert rf[REC_STATUS] == S.OSQP_SOLVED
        ex, ey = _close(x[b], xf), _close(y[b], yf)
        record_deviation('lockstep_direct_mat_vs_own_handle', 'portfolio 600x4 element %d' % b, dx_rel=ex, dy_rel=ey, iters=int(rec[b, REC_ITER]), own_handle_iters=int(rf[REC_ITER]), atol=ATOL)
        print('element %d: %d iterations, its own handle %d; |dx| %.2e |dy| %.2e (relative); bits equal: %s' % (b, rec[b, REC_ITER], rf[REC_ITER], ex, ey, np.array_equal(x[b], xf) and np.array_equal(y[b], yf)))
        assert ex <= ATOL and ey <= ATOL, (b, ex, ey)


def test_own_values_tiled(base):
    """Px, Ax = the handle's own values repeated: against the shared direct call on the same q, l, u at ATOL; iteration counts and bit equality reported."""
    nb = 6
    kw = dict(q=base.Q[:nb], l=base.L[:nb], u=base.U[:nb])
    xs, ys, rs = base.s._solver.hip_batch_solve_lockstep_direct(**kw)
    xm, ym, rm = base.s._solver.hip_batch_solve_lockstep_direct(Px=np.tile(base.P.data, (nb, 1)), Ax=np.tile(base.A.data, (nb, 1)), **kw)
    assert (rs[:, REC_STATUS] == S.OSQP_SOLVED).all() and (rm[:, REC_STATUS] == S.OSQP_SOLVED).all()
    bits = np.array_equal(xs, xm) and np.array_equal(ys, ym) and np.array_equal(rs, rm)
    print('iterations shared', rs[:, REC_ITER].astype(int), 'own values tiled', rm[:, REC_ITER].astype(int), '; bits equal:', bits)
    for b in range(nb):
        ex, ey = _close(xm[b], xs[b]), _close(ym[b], ys[b])
        record_deviation('lockstep_direct_mat_tiled_vs_shared', 'portfolio 600x4 element %d' % b, dx_rel=ex, dy_rel=ey, iters=int(rm[b, REC_ITER]), shared_iters=int(rs[b, REC_ITER]), bits_equal=int(bits), atol=ATOL)
        assert ex <= ATOL and ey <= ATOL, (b, ex, ey)


def test_one_side_only(base):
    """Ax alone (P: the handle's) and Px alone (A: the handle's): every element certified on the matrices it was given."""
    nb = 6
    for side in ('Ax', 'Px'):
        kw = dict(q=base.Q[:nb], l=base.L[:nb], u=base.U[:nb])
        kw[side] = getattr(base, side)[:nb]
        x, y, rec = base.s._solver.hip_batch_solve_lockstep_direct(**kw)
        assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all(), (side, rec[:, REC_STATUS])
        for b in range(nb):
            Pb, Ab = base.own(b)
            _certify(Pb if side == 'Px' else base.P, base.Q[b], Ab if side == 'Ax' else base.A, base.L[b], base.U[b], x[b], y[b], rec[b, REC_OBJ])


def test_independence(base):
    """A problem alone, at lane 0, at lane 63 and in the ragged chunk, among different neighbours: x, y and record are bit-identical."""
    solve = base.s._solver.hip_batch_solve_lockstep_direct
    for b in PICK:
        x1, y1, r1 = solve(**base.rows(slice(b, b + 1)))
        assert np.array_equal(x1[0], base.x[b]) and np.array_equal(y1[0], base.y[b]) and np.array_equal(r1[0], base.rec[b]), b
    xr, yr, rr = solve(**{k: v[::-1].copy() for k, v in base.kw.items()})          # lane 0 <-> the ragged chunk's last, other neighbours
    assert np.array_equal(xr[::-1], base.x) and np.array_equal(yr[::-1], base.y) and np.array_equal(rr[::-1], base.rec)


def _edge(P, q, A, l, u, r):
    """three elements (test_gpu_lockstep_direct.py _edge's q) with the base's perturbation: SOLVED, certified, and against their own fresh handles at ATOL"""
    P, A = _csc(sp.triu(P)), _csc(A)
    n = len(q)
    rng = np.random.default_rng(5)
    Q = np.stack([q * (1.0 + 0.3 * b) + 0.1 * b * rng.standard_normal(n) * (q != 0) for b in range(3)])
    L, U = np.tile(l, (3, 1)), np.tile(u, (3, 1))
    Px, Ax = _perturb(P, A, 3)
    s = _handle(P, q, A, l, u)
    assert s._solver.hip_stats()['woodbury_rows'] == r
    x, y, rec = s._solver.hip_batch_solve_lockstep_direct(q=Q, l=L, u=U, Px=Px, Ax=Ax)
    assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all(), rec[:, REC_STATUS]
    assert s._solver.lockstep_direct_mat_last_record()['chunks'] == 1
    for b in range(3):
        Pb, Ab = _own(P, A, Px, Ax, b)
        _certify(Pb, Q[b], Ab, L[b], U[b], x[b], y[b], rec[b, REC_OBJ])
        xf, yf, rf = _fresh(Pb, Q[b], Ab, L[b], U[b])
        assert rf[REC_STATUS] == S.OSQP_SOLVED
        ex, ey = _close(x[b], xf), _close(y[b], yf)
        print('r = %d element %d: %d iterations (its own handle %d); |dx| %.2e |dy| %.2e' % (r, b, rec[b, REC_ITER], rf[REC_ITER], ex, ey))
        assert ex <= ATOL and ey <= ATOL, (r, b, ex, ey)


def test_one_dense_row():
    """r = 1: test_gpu_lockstep_direct.py test_one_dense_row's shape (n = 500)."""
    n = 500
    rng = np.random.default_rng(2)
    P = sp.diags(0.5 + rng.random(n), format='csc')
    budget = sp.csc_matrix((np.ones(200), (np.zeros(200, dtype=int), np.arange(0, 400, 2))), shape=(1, n))
    A = sp.vstack([budget, sp.identity(n)], format='csc')
    l, u = np.concatenate([[1.0], np.zeros(n)]), np.concatenate([[1.0], np.ones(n)])
    _edge(P, rng.standard_normal(n), A, l, u, 1)


def test_128_dense_rows():
    """r = 128, the LDS limit of the inversion: _factor_qp(400, 127, 0.7)."""
    P, q, A, l, u = shared._factor_qp(400, 127, 0.7)
    _edge(P, q, A, l, u, 128)


STOPPED = shared.STOPPED


def test_statuses_in_one_chunk_on_own_matrices(base):
    """A solved element, a primal-infeasible one (budget row with every upper bound 0) and one stopped by max_iter in one chunk, built as
    test_gpu_lockstep_direct.py Chunk builds them; the certificate is checked against the element's own A_b, and the two finished elements are
    bit-identical to a run without the long-running neighbour."""
    cst = dict(eps_abs=1e-7, eps_rel=1e-7, eps_prim_inf=1e-5, eps_dual_inf=1e-5)
    s = _handle(base.P, base.q, base.A, base.l, base.u, **cst)
    _, _, rec8 = s._solver.hip_batch_solve_lockstep_direct(**base.rows(slice(0, 8)))
    assert (rec8[:, REC_STATUS] == S.OSQP_SOLVED).all()
    it = rec8[:, REC_ITER]
    short, long_ = int(np.argmin(it)), int(np.argmax(it))
    cap = int(it[short]) + 25
    assert it[long_] > cap, it
    idx = [short, 1, long_]
    Q, L, U, Px, Ax = base.Q[idx], np.stack([base.L[short], base.l, base.L[long_]]), np.stack([base.U[short], base.u, base.U[long_]]), base.Px[idx], base.Ax[idx]
    U[1, base.K + 1:] = 0.0
    s = _handle(base.P, base.q, base.A, base.l, base.u, max_iter=cap, **cst)
    x, y, rec = s._solver.hip_batch_solve_lockstep_direct(q=Q, l=L, u=U, Px=Px, Ax=Ax)
    print('statuses', rec[:, REC_STATUS], 'iterations', rec[:, REC_ITER], 'max_iter', cap)
    assert list(rec[:2, REC_STATUS]) == [S.OSQP_SOLVED, S.OSQP_PRIMAL_INFEASIBLE] and int(rec[2, REC_STATUS]) in STOPPED and rec[2, REC_ITER] == cap
    assert rec[0, REC_ITER] < cap and rec[1, REC_ITER] < cap
    _, A1 = base.own(1)
    yc = y[1]                                                                          # certificate of primal infeasibility (_osqp.py:796-820), on A_b
    assert np.abs(A1.T @ yc).max() <= cst['eps_prim_inf'] * np.abs(yc).max()
    assert U[1] @ np.maximum(yc, 0) + L[1] @ np.minimum(yc, 0) < 0
    xf, yf, rf = s._solver.hip_batch_solve_lockstep_direct(q=Q[:2], l=L[:2], u=U[:2], Px=Px[:2], Ax=Ax[:2])      # without the long-running neighbour
    eq = lambda a, b: np.array_equal(a, b, equal_nan=True)
    assert eq(xf, x[:2]) and eq(yf, y[:2]) and eq(rf, rec[:2])


def test_declines(base, monkeypatch):
    """What the shared direct route declines (a banded handle, a lasso handle, two-entry short rows, a reordered handle) and a repeated (j, j) entry in the
    stored triangle of P: OSQP_FUNC_NOT_IMPLEMENTED, for the nbatch = 0 query of the device entry too; the new record stays all zeros."""
    na, k = base.NA, base.K

    def declined(solver, q, A):
        for call in (lambda: solver.hip_batch_solve_lockstep_direct(q=np.tile(q, (3, 1)), Ax=np.tile(_csc(A).data, (3, 1))),
                     lambda: solver.hip_batch_solve_lockstep_direct_device(0, None, None, None, None, None, None, Px_ptr=0, Ax_ptr=0)):
            with pytest.raises(ValueError) as e:
                call()
            assert e.value.code == NOT_IMPL
        assert all(v == 0 for v in solver.lockstep_direct_mat_last_record().values())

    Pb, qb, Ab, lb, ub = problems.banded_qp(400, window=40)
    Pl, ql, Al, ll, ul = problems.lasso_qp(nf=150, ns=200)
    pair = sp.diags([np.ones(na), -np.ones(na - 1)], [0, 1], shape=(na, na))          # x_i - x_{i+1}: two entries per short row
    A2 = sp.vstack([sp.csr_matrix(base.A)[:k + 1], sp.hstack([pair, sp.csc_matrix((na, k))])], format='csc')
    l2, u2 = np.concatenate([base.l[:k + 1], -np.ones(na)]), np.concatenate([base.u[:k + 1], np.ones(na)])
    for name, (P, q, A, l, u) in (('banded', (Pb, qb, Ab, lb, ub)), ('lasso', (Pl, ql, Al, ll, ul)), ('two-entry rows', (base.P, base.q, A2, l2, u2))):
        s = _handle(P, q, _csc(A), l, u, eps_abs=1e-6, eps_rel=1e-6)
        declined(s._solver, q, A)
    # a repeated (j, j) in the stored triangle of P, straight through the C ABI (the duplicates stay): the chunk's assembly has one writer per entry
    d = base.P.diagonal()
    Pdup = sp.csc_matrix((np.repeat(0.5 * d, 2), np.repeat(np.arange(base.n), 2), 2 * np.arange(base.n + 1)), shape=(base.n, base.n))
    assert Pdup.nnz == 2 * base.n
    ext = osqp_amd.interface._backend('hip')
    st = ext.OSQPSettings(); ext.osqp_set_default_settings(st)
    st.verbose = 0; st.eps_abs = st.eps_rel = 1e-7
    solver = ext.OSQPSolver(ext.CSC(Pdup), base.q, ext.CSC(base.A), base.l, base.u, base.m, base.n, st)
    declined(solver, base.q, base.A)
    monkeypatch.setenv('OSQP_HIP_REORDER', '2')
    s = _handle(base.P, base.q, base.A, base.l, base.u)
    assert s._solver.hip_stats()['reordered'] == 1 and s._solver.hip_stats()['woodbury_rows'] == 5
    declined(s._solver, base.q, base.A)


def test_the_handle_is_left_alone(base):
    """solve() and the shared direct call give bit-identical results before and after a call with per-problem matrices; and such a call after
    update(Ax=...) on the handle uses the UPDATED values for a side passed as None."""
    s = _handle(base.P, base.q, base.A, base.l, base.u)
    kw = dict(q=base.Q[:3], l=base.L[:3], u=base.U[:3])
    rho = s.settings.rho
    r0 = s.solve()
    s.update_settings(rho=rho)                                                        # (a solve leaves its adapted rho in the settings: test_gpu_lockstep_direct.py _single)
    d0 = s._solver.hip_batch_solve_lockstep_direct(**kw)
    s._solver.hip_batch_solve_lockstep_direct(Px=base.Px[:3], Ax=base.Ax[:3], **kw)
    d1 = s._solver.hip_batch_solve_lockstep_direct(**kw)
    r1 = s.solve()
    assert all(np.array_equal(a, b) for a, b in zip(d0, d1))
    assert np.array_equal(r0.x, r1.x) and np.array_equal(r0.y, r1.y) and r0.info.iter == r1.info.iter and r0.info.status_val == r1.info.status_val == S.OSQP_SOLVED
    s.update(Ax=base.Ax[1])                                                           # the handle now holds element 1's A
    x, y, rec = s._solver.hip_batch_solve_lockstep_direct(Px=base.Px[:3], **kw)      # A: the handle's CURRENT values for every element
    assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all()
    _, A1 = base.own(1)
    for b in range(3):
        Pb, _ = base.own(b)
        _certify(Pb, base.Q[b], A1, base.L[b], base.U[b], x[b], y[b], rec[b, REC_OBJ])
    xe, ye, re_ = s._solver.hip_batch_solve_lockstep_direct(Px=base.Px[:3], Ax=np.tile(base.Ax[1], (3, 1)), **kw)      # the same values given explicitly
    assert np.array_equal(x, xe) and np.array_equal(y, ye) and np.array_equal(rec, re_)


def test_device_pointers(base):
    """The device entry on torch tensors: x, y and rec bit-identical to the host entry's."""
    import torch
    sl = slice(58, 70)                                                                # the tail of the full chunk and the ragged one, as a batch of 12
    dev = torch.device('cuda')
    t = {k: torch.tensor(np.ascontiguousarray(v[sl]), dtype=torch.float64, device=dev) for k, v in base.kw.items()}
    nb = 12
    x = torch.empty((nb, base.n), dtype=torch.float64, device=dev); y = torch.empty((nb, base.m), dtype=torch.float64, device=dev)
    rec = torch.empty((nb, ext_hip.OSQPSolver.BATCH_REC), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    base.s._solver.hip_batch_solve_lockstep_direct_device(nb, t['q'].data_ptr(), t['l'].data_ptr(), t['u'].data_ptr(), x.data_ptr(), y.data_ptr(), rec.data_ptr(),
                                                          stream=torch.cuda.current_stream(dev).cuda_stream, Px_ptr=t['Px'].data_ptr(), Ax_ptr=t['Ax'].data_ptr())
    xh, yh, rh = base.s._solver.hip_batch_solve_lockstep_direct(**base.rows(sl))
    assert np.array_equal(x.cpu().numpy(), xh) and np.array_equal(y.cpu().numpy(), yh) and np.array_equal(rec.cpu().numpy(), rh)
    assert np.array_equal(xh, base.x[sl]) and np.array_equal(rh, base.rec[sl])       # (and, by independence, the base batch's)


def test_warm_start(base):
    sl = slice(60, 66)                                                                # the batch's own elements: their solutions are base.x / base.y
    x, y, rec = base.s._solver.hip_batch_solve_lockstep_direct(x0=base.x[sl], y0=base.y[sl], **base.rows(sl))
    assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all()
    assert (rec[:, REC_ITER] < base.rec[sl, REC_ITER]).all(), (rec[:, REC_ITER], base.rec[sl, REC_ITER])
    for b in range(6):
        assert _close(x[b], base.x[sl][b]) <= ATOL and _close(y[b], base.y[sl][b]) <= ATOL


@pytest.mark.parametrize('device', ['cpu', 'cuda'])
def test_torch_layer(base, device):
    """2-D P_val and A_val: large_batch='lockstep_direct' makes ONE call of the new entry and agrees with 'loop' at ATOL."""
    import torch
    from osqp_amd.nn.torch import OSQP as Layer
    nb = 3
    Pc, Ac = base.P, base.A                                                           # (P is diagonal: its full pattern is its upper triangle)
    pco, aco = Pc.tocoo(), Ac.tocoo()
    assert np.array_equal(sp.csc_matrix((np.arange(Ac.nnz), (aco.row, aco.col)), shape=Ac.shape).data, np.arange(Ac.nnz))      # A_val is in the CSC order
    mk = lambda **kw: Layer((pco.row, pco.col), Pc.shape, (aco.row, aco.col), Ac.shape, eps_rel=EPS, eps_abs=EPS, max_iter=200000, **kw)
    vals = [base.Px[:nb], base.Q[:nb], base.Ax[:nb], base.L[:nb], base.U[:nb]]
    direct, loop = mk(large_batch='lockstep_direct'), mk(large_batch='loop')
    ts = [torch.tensor(np.array(v), dtype=torch.float64, device=device) for v in vals]
    with torch.no_grad():
        x, xl = direct(*ts), loop(*ts)
    assert x.device == ts[1].device and x.shape == (nb, base.n)
    X, Xl = x.cpu().numpy(), xl.cpu().numpy()
    print('layer: direct with own matrices vs loop |dx| %.2e (relative)' % (np.abs(X - Xl).max() / (1 + np.abs(Xl).max())))
    assert np.abs(X - Xl).max() / (1 + np.abs(Xl).max()) <= ATOL
    assert direct.mat_lockstep_direct_launches == 1 and direct.setup_count == 1 and loop.setup_count == 1
    assert direct._solver._solver.lockstep_direct_mat_last_record()['chunks'] == 1
    assert loop.mat_lockstep_direct_launches == 0 and all(v == 0 for v in loop._solver._solver.lockstep_direct_mat_last_record().values())      # the loop layer still loops
