"""GPU tier: the lockstep route with PER-PROBLEM MATRICES (osqp_hip_batch_solve_lockstep_mat[_device]; osqp-python_amd/csrc/lockstep_hip.hip "matrices of
a chunk") -- a batch in which every element has its own values of P and A, at a size one workgroup's LDS does not hold.  Shape, settings and tolerance are
test_gpu_batch_lockstep.py's: banded_qp(400, window=40) (n = 400, m = 800, nnz(A) = 4000, 600 stored entries of triu P, 77 equality rows), B = 70 (one full
chunk and a ragged one of 6), eps = 1e-8 with check_termination = 25 and adaptive_rho_interval = 50, ATOL = 2e-6 relative to the solution's scale.

The batch (rng = default_rng(3), drawn in this order): Ax = A.data (1 + 0.1 N(0,1)) per element and entry; Px = triu P with its diagonal times
1 + 0.2 U(0,1) (the off-diagonals stay: every P_b is diagonally dominant); Q = q + 0.05 N(0,1); bounds feasible by construction around z_b = A_b xh for
a fixed xh: equality rows of the base l_b = u_b = z_b, the others z_b -+ s with s = 1 + U(0,1)^m.

The scaling bound (test 2, test 8): a problem's D, E, c against those of a fresh handle set up with the problem's data alone.  The rule and the operand
orders are the same; the one legitimate difference is the order in which the mean of P's column norms inside c is summed (the single-QP setup: a
workgroup's strided sum; here: ls_rows' strips through ls_put / ls_fold).  The bound is 64 x the worst relative deviation observed on the MI355X,
floored at 1e-14: SCALING_OBSERVED below.  Observed: 0 -- D, E and c equal the fresh handle's to the last bit for elements 0 and 5 and on the reordered
handle (on this shape max |q| decides c's factor in every pass, so the sum's order does not show), and the fresh handle's own lockstep solve returns the
element's x, y bit for bit with the same 350 / 250 iterations."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_amd
import problems
from osqp_amd import ext_hip
from oracle import Oracle, SOLVED
from util import record_deviation
from test_gpu_batch_lockstep import ST, ATOL, EPS, B, PICK, REC_STATUS, REC_ITER, REC_OBJ, _certify, _handle

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
S = osqp_amd.SolverStatus
NOT_IMPL = ext_hip.osqp_error_type.OSQP_FUNC_NOT_IMPLEMENTED
SCALING_OBSERVED = 0.0     # worst relative deviation of D, E, c from the single-handle reference seen on the GPU (tests 2 and 8)
SCALING_BOUND = max(64 * SCALING_OBSERVED, 1e-14)
assert SCALING_BOUND <= 1e-10          # (above that the rule is not the same rule: a bug, not a tolerance)


def _rel(a, b):
    return float(np.abs(a - b).max() / (1 + np.abs(b).max()))


class Base:
    def __init__(self):
        self.P, self.q, self.A, self.l, self.u = problems.banded_qp(400, window=40)
        self.n, self.m = len(self.q), len(self.l)
        self.Pu = sp.triu(self.P, format='csc'); self.Pu.sort_indices()
        A, Pu, n, m = self.A, self.Pu, self.n, self.m
        assert (n, m, A.nnz, Pu.nnz, int((self.l == self.u).sum())) == (400, 800, 4000, 600, 77)
        rng = np.random.default_rng(3)
        self.Ax = A.data * (1 + 0.1 * rng.standard_normal((B, A.nnz)))
        diag = np.repeat(np.arange(n), np.diff(Pu.indptr)) == Pu.indices
        self.Px = np.tile(Pu.data, (B, 1))
        self.Px[:, diag] *= 1 + 0.2 * rng.random((B, int(diag.sum())))
        self.Q = self.q + 0.05 * rng.standard_normal((B, n))
        xh = rng.standard_normal(n)
        s = 1 + rng.random(m)
        eq = self.l == self.u
        z0 = A @ xh                               # the same construction on the handle's own A (test 4, Px alone)
        self.l_own, self.u_own = np.where(eq, z0, z0 - s), np.where(eq, z0, z0 + s)
        Z = np.stack([self.A_of(b) @ xh for b in range(B)])
        self.L, self.U = np.where(eq, Z, Z - s), np.where(eq, Z, Z + s)
        self.s = _handle(self.P, self.q, self.A, self.l, self.u)
        self.x, self.y, self.rec = self.s._solver.hip_batch_solve_lockstep(q=self.Q, l=self.L, u=self.U, Px=self.Px, Ax=self.Ax)
        self.last = self.s._solver.lockstep_mat_last_record()
        self.last_shared = self.s._solver.lockstep_last_record()

    def A_of(self, b, Ax=None):
        return sp.csc_matrix(((self.Ax if Ax is None else Ax)[b], self.A.indices, self.A.indptr), shape=self.A.shape)

    def P_of(self, b, Px=None):              # the full symmetric P_b from its stored upper triangle
        U = sp.csc_matrix(((self.Px if Px is None else Px)[b], self.Pu.indices, self.Pu.indptr), shape=self.P.shape)
        Pb = (U + sp.triu(U, 1).T).tocsc(); Pb.sort_indices()
        return Pb


@pytest.fixture(scope='module')
def base():
    return Base()


def _oracle(P, q, A, l, u, **kw):
    st = dict(ST, eps_abs=1e-9, eps_rel=1e-9); st.update(kw)
    xo, yo, io = Oracle().setup(P, q, A, l, u, **st).solve()
    return xo, yo, io


def _against_oracle(tag, b, P, q, A, l, u, x, y, rec):
    xo, yo, io = _oracle(P, q, A, l, u)
    assert io.status_val == SOLVED
    ex, ey = _rel(x, xo), _rel(y, yo)
    record_deviation('lockstep_mat_vs_oracle', '%s element %d' % (tag, b), dx_rel=ex, dy_rel=ey, iters=int(rec[REC_ITER]), oracle_iters=io.iter, atol=ATOL)
    print('%s element %d: lockstep-mat %d iterations, oracle %d; |dx| %.2e |dy| %.2e (relative)' % (tag, b, rec[REC_ITER], io.iter, ex, ey))
    assert ex <= ATOL and ey <= ATOL, (tag, b, ex, ey)


def test_oracle_per_element(base):
    """1. hip_batch_solve declines the shape; the lockstep-mat call solves all 70, every element certified on the host against its own P_b, A_b, four of
    them against the oracle at eps 1e-9 on their own matrices."""
    with pytest.raises(ValueError) as e:
        base.s._solver.hip_batch_solve(q=base.Q, l=base.L, u=base.U, Px=base.Px, Ax=base.Ax)
    assert e.value.code == NOT_IMPL
    assert (base.rec[:, REC_STATUS] == S.OSQP_SOLVED).all(), base.rec[:, REC_STATUS]
    assert (base.rec[:, 8] == 0).all() and (base.rec[:, 9] == 0).all()              # no polish on this entry
    assert base.last['chunks'] == 2 and base.last['width'] == 64 and base.last['matrix_block_bytes'] > 0 and 0 < base.last['prepare_gpu_ms'] < base.last['gpu_ms']
    assert base.last_shared['chunks'] == 2 and base.last_shared['kernel_launches'] == base.last['kernel_launches']
    print('lockstep-mat B=70: %s' % base.last)
    for b in range(B):
        _certify(base.P_of(b), base.Q[b], base.A_of(b), base.L[b], base.U[b], base.x[b], base.y[b], base.rec[b, REC_OBJ])
    for b in PICK:
        _against_oracle('batch', b, base.P_of(b), base.Q[b], base.A_of(b), base.L[b], base.U[b], base.x[b], base.y[b], base.rec[b])


def _scaling_deviation(tag, got, ref):
    (D, E, c), (D0, E0, c0) = got, ref
    dev = max(float(np.abs(D / D0 - 1).max()), float(np.abs(E / E0 - 1).max()), abs(c / c0 - 1))
    record_deviation('lockstep_mat_scaling', tag, rel_dev=dev, bound=SCALING_BOUND)
    print('%s: scaling deviates from the single-handle reference by %.3e (relative; bound %.3e)' % (tag, dev, SCALING_BOUND))
    return dev


def test_scaling_is_the_elements_own(base):
    """2. D, E, c of elements 0 and 5 of a batch of 6 against a fresh handle set up with that element's data alone; that handle's shared lockstep solve
    agrees with the mat call's element.  Observed on the MI355X: relative deviation 0 for both elements (SCALING_OBSERVED; bound = 64 x that, floored at
    1e-14 = 1e-14); x, y of the element's own handle equal to the mat call's bit for bit, 350 / 350 and 250 / 250 iterations."""
    nb = 6
    x, y, rec = base.s._solver.hip_batch_solve_lockstep(q=base.Q[:nb], l=base.L[:nb], u=base.U[:nb], Px=base.Px[:nb], Ax=base.Ax[:nb])
    got = {b: base.s._solver.lockstep_mat_scaling(b) for b in (0, 5)}
    with pytest.raises(ValueError) as e:
        base.s._solver.lockstep_mat_scaling(nb)                                  # outside the last chunk
    assert e.value.code == ext_hip.osqp_error_type.OSQP_DATA_NOT_INITIALIZED
    devs = []
    for b in (0, 5):
        f = _handle(base.P_of(b), base.Q[b], base.A_of(b), base.L[b], base.U[b])
        devs.append(_scaling_deviation('element %d' % b, got[b], f._solver.hip_scaling()))
        x1, y1, r1 = f._solver.hip_batch_solve_lockstep(nbatch=1)
        ex, ey = _rel(x[b], x1[0]), _rel(y[b], y1[0])
        record_deviation('lockstep_mat_vs_own_handle', 'element %d' % b, dx_rel=ex, dy_rel=ey, iters=int(rec[b, REC_ITER]), own_iters=int(r1[0, REC_ITER]), atol=ATOL)
        print('element %d: mat call %d iterations, its own handle %d; |dx| %.2e |dy| %.2e' % (b, rec[b, REC_ITER], r1[0, REC_ITER], ex, ey))
        assert r1[0, REC_STATUS] == S.OSQP_SOLVED and ex <= ATOL and ey <= ATOL
    assert max(devs) <= SCALING_BOUND, devs


def test_independence(base):
    """3. A problem's x, y and record do not depend on what else is in the batch or where in it the problem sits; its matrices are part of the problem."""
    for b in PICK:
        x1, y1, r1 = base.s._solver.hip_batch_solve_lockstep(q=base.Q[b:b + 1], l=base.L[b:b + 1], u=base.U[b:b + 1], Px=base.Px[b:b + 1], Ax=base.Ax[b:b + 1])
        assert np.array_equal(x1[0], base.x[b]) and np.array_equal(y1[0], base.y[b]) and np.array_equal(r1[0], base.rec[b]), b
    rv = lambda a: a[::-1].copy()
    xr, yr, rr = base.s._solver.hip_batch_solve_lockstep(q=rv(base.Q), l=rv(base.L), u=rv(base.U), Px=rv(base.Px), Ax=rv(base.Ax))
    assert np.array_equal(xr[::-1], base.x) and np.array_equal(yr[::-1], base.y) and np.array_equal(rr[::-1], base.rec)


def test_one_side_only(base):
    """4. Ax alone and Px alone (the other side is the handle's own) against the oracle; tiles of the handle's own values agree with the shared route."""
    nb = 7
    sl = slice(0, nb)
    x, y, rec = base.s._solver.hip_batch_solve_lockstep(q=base.Q[sl], l=base.L[sl], u=base.U[sl], Ax=base.Ax[sl])
    assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all()
    for b in (0, 6):
        _against_oracle('Ax alone', b, base.P, base.Q[b], base.A_of(b), base.L[b], base.U[b], x[b], y[b], rec[b])
    # (every element's A is the handle's here: the recipe's bounds around A xh, feasible by the same construction)
    L0, U0 = np.tile(base.l_own, (nb, 1)), np.tile(base.u_own, (nb, 1))
    x, y, rec = base.s._solver.hip_batch_solve_lockstep(q=base.Q[sl], l=L0, u=U0, Px=base.Px[sl])
    assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all()
    for b in (0, 6):
        _against_oracle('Px alone', b, base.P_of(b), base.Q[b], base.A, L0[b], U0[b], x[b], y[b], rec[b])
    xs, ys, rs = base.s._solver.hip_batch_solve_lockstep(q=base.Q[sl], l=L0, u=U0)
    xt, yt, rt = base.s._solver.hip_batch_solve_lockstep(q=base.Q[sl], l=L0, u=U0, Px=np.tile(base.Pu.data, (nb, 1)), Ax=np.tile(base.A.data, (nb, 1)))
    assert np.array_equal(rt[:, REC_STATUS], rs[:, REC_STATUS]) and (rs[:, REC_STATUS] == S.OSQP_SOLVED).all()
    for b in range(nb):
        assert _rel(xt[b], xs[b]) <= ATOL and _rel(yt[b], ys[b]) <= ATOL, b


def test_statuses_in_one_chunk():
    """5. The [I; I] problem of test_gpu_batch_lockstep.py::test_statuses, every element with its own positive multiple of A's values and of its bounds
    (which keeps its status): solved, primal infeasible and dual infeasible in one chunk, each equal to the oracle's on the element's own matrices,
    with certificates that hold on the element's own A_b."""
    n = 420
    rng = np.random.default_rng(7)
    d = 0.5 + rng.random(n); d[0] = 0.0
    P = sp.diags(d, format='csc'); A = sp.vstack([sp.identity(n), sp.identity(n)], format='csc')
    q = rng.standard_normal(n)
    l = np.concatenate([-np.ones(n), -2 * np.ones(n)]); u = np.concatenate([np.ones(n), 2 * np.ones(n)])
    st = dict(eps_abs=1e-6, eps_rel=1e-6, eps_prim_inf=1e-5, eps_dual_inf=1e-5, max_iter=4000, check_termination=25, adaptive_rho_interval=50)
    Q, L, U = np.tile(q, (3, 1)), np.tile(l, (3, 1)), np.tile(u, (3, 1))
    i = 5
    L[1, i] = U[1, i] = 1.0; L[1, n + i] = U[1, n + i] = -1.0                   # x_i = 1 and x_i = -1
    Q[2, 0] = -1.0; L[2, 0] = L[2, n] = -np.inf; U[2, 0] = U[2, n] = np.inf     # x_0 free, zero curvature, negative cost
    f = np.array([1.0, 3.0, 0.5])
    Ax = f[:, None] * np.tile(A.data, (3, 1)); L, U = f[:, None] * L, f[:, None] * U
    s = osqp_amd.OSQP(algebra='hip'); s.setup(P, q, A, l, u, verbose=False, **st)
    x, y, rec = s._solver.hip_batch_solve_lockstep(q=Q, l=L, u=U, Ax=Ax)
    assert list(rec[:, REC_STATUS]) == [S.OSQP_SOLVED, S.OSQP_PRIMAL_INFEASIBLE, S.OSQP_DUAL_INFEASIBLE], rec[:, REC_STATUS]
    Ab = [sp.csc_matrix((Ax[b], A.indices, A.indptr), shape=A.shape) for b in range(3)]
    for b in range(3):
        lo, uo = np.maximum(L[b], -1e30), np.minimum(U[b], 1e30)
        xo, yo, io = Oracle().setup(P, Q[b], Ab[b], lo, uo, **st).solve()
        assert io.status_val == int(rec[b, REC_STATUS]), (b, io.status_val, rec[b])
    yc = y[1]                                                                   # certificate of primal infeasibility (_osqp.py:796-820)
    assert np.abs(Ab[1].T @ yc).max() <= st['eps_prim_inf'] * np.abs(yc).max()
    assert U[1] @ np.maximum(yc, 0) + L[1] @ np.minimum(yc, 0) < 0
    xc = x[2]                                                                   # certificate of dual infeasibility (:822-878)
    assert np.abs(P @ xc).max() <= st['eps_dual_inf'] * np.abs(xc).max() and Q[2] @ xc < 0
    fin_u, fin_l = U[2] < 1e20, L[2] > -1e20
    axc = Ab[2] @ xc
    assert (axc[fin_u] <= st['eps_dual_inf'] * np.abs(xc).max()).all() and (axc[fin_l] >= -st['eps_dual_inf'] * np.abs(xc).max()).all()


def test_warm_start(base):
    """6. From the cold solution every element terminates at the first check."""
    pk = list(PICK)
    x, y, rec = base.s._solver.hip_batch_solve_lockstep(q=base.Q[pk], l=base.L[pk], u=base.U[pk], Px=base.Px[pk], Ax=base.Ax[pk], x0=base.x[pk], y0=base.y[pk])
    assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all()
    assert (rec[:, REC_ITER] == ST['check_termination']).all(), rec[:, REC_ITER]
    for k, b in enumerate(pk):
        assert _rel(x[k], base.x[b]) <= ATOL, b


def test_device_pointers(base):
    """7. The device entry on torch tensors gives the host entry's bits."""
    import torch
    nb = 33
    dev = torch.device('cuda', 0)
    t = lambda a: torch.tensor(a[:nb], dtype=torch.float64, device=dev).contiguous()
    qd, ld, ud, pd, ad = t(base.Q), t(base.L), t(base.U), t(base.Px), t(base.Ax)
    x = torch.empty((nb, base.n), dtype=torch.float64, device=dev); y = torch.empty((nb, base.m), dtype=torch.float64, device=dev)
    rec = torch.empty((nb, 12), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    base.s._solver.hip_batch_solve_lockstep_device(0, None, None, None, None, None, None, Px_ptr=pd.data_ptr(), Ax_ptr=ad.data_ptr())      # the applicability query: no exception
    base.s._solver.hip_batch_solve_lockstep_device(nb, qd.data_ptr(), ld.data_ptr(), ud.data_ptr(), x.data_ptr(), y.data_ptr(), rec.data_ptr(), warm=False, stream=stream,
                                                   Px_ptr=pd.data_ptr(), Ax_ptr=ad.data_ptr())
    xh, yh, rh = base.s._solver.hip_batch_solve_lockstep(q=base.Q[:nb], l=base.L[:nb], u=base.U[:nb], Px=base.Px[:nb], Ax=base.Ax[:nb])
    assert np.array_equal(x.cpu().numpy(), xh) and np.array_equal(y.cpu().numpy(), yh) and np.array_equal(rec.cpu().numpy(), rh)
    assert np.array_equal(xh, base.x[:nb]) and np.array_equal(rh, base.rec[:nb])


def test_reordered_handle(base, monkeypatch):
    """8. A handle that works on a permuted copy: the caller's CSC positions go through the value maps."""
    nb = 5
    monkeypatch.setenv('OSQP_HIP_REORDER', '2')
    s = _handle(base.P, base.q, base.A, base.l, base.u)
    assert s._solver.hip_stats()['reordered'] == 1
    sl = slice(0, nb)
    x, y, rec = s._solver.hip_batch_solve_lockstep(q=base.Q[sl], l=base.L[sl], u=base.U[sl], Px=base.Px[sl], Ax=base.Ax[sl])
    sc_r = s._solver.lockstep_mat_scaling(0)
    x0, y0, rec0 = base.s._solver.hip_batch_solve_lockstep(q=base.Q[sl], l=base.L[sl], u=base.U[sl], Px=base.Px[sl], Ax=base.Ax[sl])
    sc_0 = base.s._solver.lockstep_mat_scaling(0)
    assert np.array_equal(rec[:, REC_STATUS], rec0[:, REC_STATUS]) and (rec[:, REC_STATUS] == S.OSQP_SOLVED).all()
    for b in range(nb):
        _certify(base.P_of(b), base.Q[b], base.A_of(b), base.L[b], base.U[b], x[b], y[b], rec[b, REC_OBJ])
        assert _rel(x[b], x0[b]) <= ATOL and _rel(y[b], y0[b]) <= ATOL, b           # (not bitwise: the permutation changes the order of the sums)
    assert _scaling_deviation('reordered element 0', sc_r, sc_0) <= SCALING_BOUND


def test_torch_layer(base):
    """9. 2-D P_val / A_val: large_batch='lockstep' makes ONE lockstep-mat call on one set-up handle; the default layer loops and agrees."""
    import torch
    from osqp_amd.nn.torch import OSQP as Layer
    nb = 12
    Pc = sp.csc_matrix(base.P); Pc.sort_indices()
    Ac = sp.csc_matrix(base.A); Ac.sort_indices()
    pco, aco = Pc.tocoo(), Ac.tocoo()
    mk = lambda **kw: Layer((pco.row, pco.col), Pc.shape, (aco.row, aco.col), Ac.shape, eps_rel=EPS, eps_abs=EPS, max_iter=200000, **kw)
    Pfull = np.stack([base.P_of(b).tocoo().data for b in range(nb)])              # (the pattern of every P_b is P's: same order of entries)
    assert all(np.array_equal(base.P_of(b).indices, Pc.indices) for b in (0, nb - 1)) and Pfull.shape == (nb, Pc.nnz)
    ts = [torch.tensor(np.array(v), dtype=torch.float64) for v in (Pfull, base.Q[:nb], base.Ax[:nb], base.L[:nb], base.U[:nb])]
    lock, default = mk(large_batch='lockstep'), mk()
    with torch.no_grad():
        X = lock(*ts).numpy()
        Xd = default(*ts).numpy()
    assert lock.mat_lockstep_launches == 1 and lock.setup_count == 1
    assert default.mat_lockstep_launches == 0
    assert lock._solver._solver.lockstep_mat_last_record()['chunks'] == 1 and default._solver._solver.lockstep_mat_last_record()['chunks'] == 0
    for b in (0, nb - 1):
        xo, yo, io = _oracle(base.P_of(b), base.Q[b], base.A_of(b), base.L[b], base.U[b], check_termination=25)
        assert io.status_val == SOLVED
        ex = _rel(X[b], xo)
        record_deviation('lockstep_mat_torch_vs_oracle', 'element %d' % b, dx_rel=ex, atol=ATOL)
        assert ex <= ATOL, (b, ex)
    for b in range(nb):
        assert _rel(X[b], Xd[b]) <= ATOL, b


def test_handle_is_untouched(base):
    """10. solve(), [mat call,] solve() on two handles: the handle's matrices, scaling, iterates and launch history are not touched."""
    out = []
    for call in (False, True):
        s = _handle(base.P, base.q, base.A, base.l, base.u, eps_abs=1e-6, eps_rel=1e-6)
        sc_a = s._solver.hip_scaling()
        ra = s.solve()
        if call:
            x, y, rec = s._solver.hip_batch_solve_lockstep(q=base.Q[:3], l=base.L[:3], u=base.U[:3], Px=base.Px[:3], Ax=base.Ax[:3])
            assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all()
            sc_b = s._solver.hip_scaling()
            assert np.array_equal(sc_a[0], sc_b[0]) and np.array_equal(sc_a[1], sc_b[1]) and sc_a[2] == sc_b[2]
        rb = s.solve()
        out.append((ra, rb))
    (a0, b0), (a1, b1) = out
    assert np.array_equal(a0.x, a1.x) and np.array_equal(a0.y, a1.y) and a0.info.iter == a1.info.iter
    assert np.array_equal(b0.x, b1.x) and np.array_equal(b0.y, b1.y) and b0.info.iter == b1.info.iter and b0.info.status_val == b1.info.status_val == S.OSQP_SOLVED
