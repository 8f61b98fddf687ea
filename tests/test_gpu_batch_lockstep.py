"""GPU tier: the lockstep batch route (osqp_hip_batch_solve_lockstep[_device]; osqp-python_amd/csrc/lockstep_hip.hip) -- a batch of QPs that share
P and A, at sizes one workgroup's LDS does not hold.  The base problem is banded_qp(400, window=40): m = 800, 10 n + 8 m = 10 400 doubles > 8192,
the smallest standard shape past the batch kernel's limit.  Batches are built as the torch test of test_gpu_adjoint_pcg.py builds them:
q + noise, l - delta_b, u + delta_b (widening keeps every element feasible).

Bounds.  Solutions of two eps = 1e-8 iterates of the same QP are compared at ATOL = 2e-6 relative to the solution's scale: the bound
test_gpu_baseline_configs.py (_tight) applies to the single handle against the oracle at that eps (its ATOL_1E6 = 2e-5 belongs to eps = 1e-6).
Certificates use that file's certify rule: residuals <= 1.01 (eps + eps scale), objective to 1e-6 relative."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_amd
import problems
from osqp_amd import ext_hip
from oracle import Oracle, SOLVED
from util import record_deviation

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
S = osqp_amd.SolverStatus
NOT_IMPL = ext_hip.osqp_error_type.OSQP_FUNC_NOT_IMPLEMENTED
EPS = 1e-8
ATOL = 2e-6
B = 70                     # one full chunk of 64 and a ragged one of 6
PICK = (0, 63, 64, 69)     # first / last lane of the full chunk, first / last of the ragged one
ST = dict(eps_abs=EPS, eps_rel=EPS, max_iter=50000, adaptive_rho_interval=50, check_termination=25)
REC_STATUS, REC_ITER, REC_OBJ, REC_PCG = 0, 1, 2, 7


def _batch(q, l, u, nb, seed=13):
    rng = np.random.default_rng(seed)
    return (np.stack([q + 0.05 * b * rng.standard_normal(len(q)) for b in range(nb)]), np.stack([l - 0.01 * b for b in range(nb)]),
            np.stack([u + 0.01 * b for b in range(nb)]))


def _handle(P, q, A, l, u, **kw):
    st = dict(ST); st.update(kw)
    s = osqp_amd.OSQP(algebra='hip')
    s.setup(P, q, A, l, u, verbose=False, **st)
    return s


def _certify(P, q, A, l, u, x, y, obj, eps=EPS):
    k = problems.kkt_certificate(P, q, A, l, u, x, y)
    ax = A @ x
    scale_p = max(np.abs(ax).max(), np.abs(np.clip(ax, l, u)).max())
    scale_d = max(np.abs(P @ x).max(), np.abs(A.T @ y).max(), np.abs(q).max())
    assert k['pri'] <= 1.01 * (eps + eps * scale_p), k
    assert k['dua'] <= 1.01 * (eps + eps * scale_d), k
    assert abs(k['obj'] - obj) <= 1e-6 * (1 + abs(k['obj']))


class Base:
    def __init__(self):
        self.P, self.q, self.A, self.l, self.u = problems.banded_qp(400, window=40)
        self.n, self.m = len(self.q), len(self.l)
        self.Q, self.L, self.U = _batch(self.q, self.l, self.u, B)
        self.s = _handle(self.P, self.q, self.A, self.l, self.u)
        self.x, self.y, self.rec = self.s._solver.hip_batch_solve_lockstep(q=self.Q, l=self.L, u=self.U)
        self.last = self.s._solver.lockstep_last_record()


@pytest.fixture(scope='module')
def base():
    return Base()


def test_the_limit_and_the_way_past_it(base):
    """hip_batch_solve declines this shape; the lockstep route solves B = 70 of it at eps 1e-8, every element certified on the host, four of them
    against the oracle at eps 1e-9."""
    with pytest.raises(ValueError) as e:
        base.s._solver.hip_batch_solve(q=base.Q, l=base.L, u=base.U)
    assert e.value.code == NOT_IMPL
    assert (base.rec[:, REC_STATUS] == S.OSQP_SOLVED).all(), base.rec[:, REC_STATUS]
    for b in range(B):
        _certify(base.P, base.Q[b], base.A, base.L[b], base.U[b], base.x[b], base.y[b], base.rec[b, REC_OBJ])
    for b in PICK:
        st = dict(ST, eps_abs=1e-9, eps_rel=1e-9)
        xo, yo, io = Oracle().setup(base.P, base.Q[b], base.A, base.L[b], base.U[b], **st).solve()
        assert io.status_val == SOLVED
        ex = np.abs(base.x[b] - xo).max() / (1 + np.abs(xo).max()); ey = np.abs(base.y[b] - yo).max() / (1 + np.abs(yo).max())
        record_deviation('lockstep_vs_oracle', 'banded n=400 element %d' % b, dx_rel=ex, dy_rel=ey, iters=int(base.rec[b, REC_ITER]), oracle_iters=io.iter, atol=ATOL)
        print('element %d: lockstep %d iterations, oracle %d; |dx| %.2e |dy| %.2e (relative)' % (b, base.rec[b, REC_ITER], io.iter, ex, ey))
        assert ex <= ATOL and ey <= ATOL


def test_independence(base):
    """A problem's x, y and record do not depend on what else is in the batch or where in it the problem sits."""
    assert base.last['chunks'] == 2 and base.last['width'] == 64
    for b in PICK:
        x1, y1, r1 = base.s._solver.hip_batch_solve_lockstep(q=base.Q[b:b + 1], l=base.L[b:b + 1], u=base.U[b:b + 1])
        assert np.array_equal(x1[0], base.x[b]) and np.array_equal(y1[0], base.y[b]) and np.array_equal(r1[0], base.rec[b]), b
    xr, yr, rr = base.s._solver.hip_batch_solve_lockstep(q=base.Q[::-1].copy(), l=base.L[::-1].copy(), u=base.U[::-1].copy())
    assert np.array_equal(xr[::-1], base.x) and np.array_equal(yr[::-1], base.y) and np.array_equal(rr[::-1], base.rec)


def test_freezing(base):
    """An element that terminates checks earlier than its chunk is frozen there: its bits and its PCG count are those of its solo solve."""
    nb, e = 5, 2
    Q, L, U = base.Q[:nb].copy(), base.L[:nb].copy(), base.U[:nb].copy()
    Q[e] = 0.0; L[e] = base.l - 1e3; U[e] = base.u + 1e3
    x, y, rec = base.s._solver.hip_batch_solve_lockstep(q=Q, l=L, u=U)
    assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all()
    assert rec[e, REC_ITER] < rec[:, REC_ITER].max(), rec[:, REC_ITER]
    x1, y1, r1 = base.s._solver.hip_batch_solve_lockstep(q=Q[e:e + 1], l=L[e:e + 1], u=U[e:e + 1])
    assert np.array_equal(x1[0], x[e]) and np.array_equal(y1[0], y[e]) and np.array_equal(r1[0], rec[e])
    assert r1[0, REC_PCG] == rec[e, REC_PCG]


def test_statuses():
    """A = [I; I], P = diag(d) with d_0 = 0: solved, primal infeasible and dual infeasible elements in one chunk, each with the status the oracle
    gives it alone and a certificate that holds on the host; max_iter = 25 leaves no element without a final status."""
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
    s = osqp_amd.OSQP(algebra='hip'); s.setup(P, q, A, l, u, verbose=False, **st)
    with pytest.raises(ValueError) as e:                                        # (10 n + 8 m + 16 = 10 936 doubles: past the batch kernel too)
        s._solver.hip_batch_solve(q=Q, l=L, u=U)
    assert e.value.code == NOT_IMPL
    x, y, rec = s._solver.hip_batch_solve_lockstep(q=Q, l=L, u=U)
    assert list(rec[:, REC_STATUS]) == [S.OSQP_SOLVED, S.OSQP_PRIMAL_INFEASIBLE, S.OSQP_DUAL_INFEASIBLE], rec[:, REC_STATUS]
    for b in range(3):
        lo, uo = np.maximum(L[b], -1e30), np.minimum(U[b], 1e30)
        xo, yo, io = Oracle().setup(P, Q[b], A, lo, uo, **st).solve()
        assert io.status_val == int(rec[b, REC_STATUS]), (b, io.status_val, rec[b])
    yc = y[1]                                                                   # certificate of primal infeasibility (_osqp.py:796-820)
    assert np.abs(A.T @ yc).max() <= st['eps_prim_inf'] * np.abs(yc).max()
    assert U[1] @ np.maximum(yc, 0) + L[1] @ np.minimum(yc, 0) < 0
    xc = x[2]                                                                   # certificate of dual infeasibility (:822-878)
    assert np.abs(P @ xc).max() <= st['eps_dual_inf'] * np.abs(xc).max() and Q[2] @ xc < 0
    fin_u, fin_l = U[2] < 1e20, L[2] > -1e20
    axc = A @ xc
    assert (axc[fin_u] <= st['eps_dual_inf'] * np.abs(xc).max()).all() and (axc[fin_l] >= -st['eps_dual_inf'] * np.abs(xc).max()).all()
    # max_iter = 25 at a tolerance nobody reaches by then
    st25 = dict(st, eps_abs=1e-10, eps_rel=1e-10, max_iter=25)
    s25 = osqp_amd.OSQP(algebra='hip'); s25.setup(P, q, A, l, u, verbose=False, **st25)
    Q25 = np.stack([q + 0.1 * b * rng.standard_normal(n) for b in range(3)])
    x, y, rec = s25._solver.hip_batch_solve_lockstep(q=Q25)
    allowed = {int(S.OSQP_MAX_ITER_REACHED), int(S.OSQP_SOLVED_INACCURATE), int(S.OSQP_PRIMAL_INFEASIBLE_INACCURATE), int(S.OSQP_DUAL_INFEASIBLE_INACCURATE)}
    for b in range(3):
        assert int(rec[b, REC_STATUS]) in allowed and rec[b, REC_ITER] == 25, rec[b]
        xo, yo, io = Oracle().setup(P, Q25[b], A, l, u, **st25).solve()
        assert io.status_val == int(rec[b, REC_STATUS]), (b, io.status_val, rec[b])


def test_warm_start(base):
    nb = 6
    sl = slice(60, 60 + nb)                                                      # (the batch's own elements: their solutions are base.x / base.y)
    x, y, rec = base.s._solver.hip_batch_solve_lockstep(q=base.Q[sl], l=base.L[sl], u=base.U[sl], x0=base.x[sl], y0=base.y[sl])
    assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all()
    assert (rec[:, REC_ITER] < base.rec[sl, REC_ITER]).all(), (rec[:, REC_ITER], base.rec[sl, REC_ITER])
    xa, ya, ra = base.s._solver.hip_batch_solve_lockstep(q=base.Q[sl], l=base.L[sl], u=base.U[sl], x0=base.x[sl])
    xb, yb, rb = base.s._solver.hip_batch_solve_lockstep(q=base.Q[sl], l=base.L[sl], u=base.U[sl], x0=base.x[sl], y0=np.zeros((nb, base.m)))
    assert np.array_equal(xa, xb) and np.array_equal(ya, yb) and np.array_equal(ra, rb)      # a missing y0 starts y from zero
    assert (ra[:, REC_STATUS] == S.OSQP_SOLVED).all()


def test_device_pointers(base):
    import torch
    dev = torch.device('cuda', 0)
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev).contiguous()
    qd, ld, ud = t(base.Q), t(base.L), t(base.U)
    x = torch.empty((B, base.n), dtype=torch.float64, device=dev); y = torch.empty((B, base.m), dtype=torch.float64, device=dev)
    rec = torch.empty((B, 12), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    base.s._solver.hip_batch_solve_lockstep_device(0, None, None, None, None, None, None)          # the applicability query: no exception
    base.s._solver.hip_batch_solve_lockstep_device(B, qd.data_ptr(), ld.data_ptr(), ud.data_ptr(), x.data_ptr(), y.data_ptr(), rec.data_ptr(), warm=False, stream=stream)
    assert np.array_equal(x.cpu().numpy(), base.x) and np.array_equal(y.cpu().numpy(), base.y) and np.array_equal(rec.cpu().numpy(), base.rec)


def test_reordered_handle(base, monkeypatch):
    nb = 5
    monkeypatch.setenv('OSQP_HIP_REORDER', '2')
    s = _handle(base.P, base.q, base.A, base.l, base.u)
    assert s._solver.hip_stats()['reordered'] == 1
    x, y, rec = s._solver.hip_batch_solve_lockstep(q=base.Q[:nb], l=base.L[:nb], u=base.U[:nb])
    assert np.array_equal(rec[:, REC_STATUS], base.rec[:nb, REC_STATUS])
    for b in range(nb):
        _certify(base.P, base.Q[b], base.A, base.L[b], base.U[b], x[b], y[b], rec[b, REC_OBJ])
        ex = np.abs(x[b] - base.x[b]).max() / (1 + np.abs(base.x[b]).max()); ey = np.abs(y[b] - base.y[b]).max() / (1 + np.abs(base.y[b]).max())
        assert ex <= ATOL and ey <= ATOL, (b, ex, ey)            # (not bitwise: the permutation changes the order of the sums)


def test_declines_on_a_woodbury_handle():
    P, q, A, l, u = problems.portfolio_qp(200, 10)
    st = dict(eps_abs=1e-6, eps_rel=1e-6, max_iter=20000)
    s0 = osqp_amd.OSQP(algebra='hip'); s0.setup(P, q, A, l, u, verbose=False, **st)
    s1 = osqp_amd.OSQP(algebra='hip'); s1.setup(P, q, A, l, u, verbose=False, **st)
    assert s1._solver.hip_stats()['woodbury_rows'] > 0
    with pytest.raises(ValueError) as e:
        s1._solver.hip_batch_solve_lockstep(q=np.tile(q, (3, 1)))
    assert e.value.code == NOT_IMPL
    r0, r1 = s0.solve(), s1.solve()                                # the declined call left no trace
    assert r1.info.status_val == S.OSQP_SOLVED and r1.info.iter == r0.info.iter
    assert np.array_equal(r0.x, r1.x) and np.array_equal(r0.y, r1.y)


def test_handle_state_is_untouched(base):
    """solve(), [lockstep call,] solve() on two handles: the route has its own workspace and touches neither the iterates nor the launch history."""
    out = []
    for call in (False, True):
        s = _handle(base.P, base.q, base.A, base.l, base.u, eps_abs=1e-6, eps_rel=1e-6)
        ra = s.solve()
        if call:
            s._solver.hip_batch_solve_lockstep(q=base.Q[:3], l=base.L[:3], u=base.U[:3])
        rb = s.solve()
        out.append((ra, rb))
    (a0, b0), (a1, b1) = out
    assert np.array_equal(a0.x, a1.x) and np.array_equal(a0.y, a1.y) and a0.info.iter == a1.info.iter
    assert np.array_equal(b0.x, b1.x) and np.array_equal(b0.y, b1.y) and b0.info.iter == b1.info.iter and b0.info.status_val == b1.info.status_val == S.OSQP_SOLVED


@pytest.mark.parametrize('device', ['cpu', 'cuda'])
def test_torch_layer(base, device):
    import torch
    from osqp_amd.nn.torch import OSQP as Layer
    nb = 3
    Pc, Ac = sp.csc_matrix(base.P), sp.csc_matrix(base.A)
    Pc.sort_indices(); Ac.sort_indices()
    pco, aco = Pc.tocoo(), Ac.tocoo()
    mk = lambda **kw: Layer((pco.row, pco.col), Pc.shape, (aco.row, aco.col), Ac.shape, eps_rel=EPS, eps_abs=EPS, max_iter=200000, **kw)
    vals = [Pc.data, base.Q[:nb], Ac.data, base.L[:nb], base.U[:nb]]
    lock, default = mk(large_batch='lockstep'), mk()
    ts = [torch.tensor(np.array(v), dtype=torch.float64, device=device, requires_grad=True) for v in vals]
    x = lock(*ts)
    with torch.no_grad():
        xd = default(*[t.detach() for t in ts])
    assert x.device == ts[1].device and x.shape == (nb, base.n)
    X, Xd = x.detach().cpu().numpy(), xd.cpu().numpy()
    assert np.abs(X - Xd).max() / (1 + np.abs(Xd).max()) <= ATOL
    assert lock._solver._solver.lockstep_last_record()['chunks'] == 1
    assert default._solver._solver.lockstep_last_record()['chunks'] == 0          # the default layer still loops
    before = lock.adjoint_launches
    (0.5 * (x ** 2).sum()).backward()
    assert lock.adjoint_launches == before + nb
    for t in ts:
        assert t.grad is not None and t.grad.shape == t.shape and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0
    with pytest.raises(ValueError):
        mk(large_batch='other')
