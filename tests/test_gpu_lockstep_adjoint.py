"""GPU tier: adjoint derivatives on the lockstep route (include/osqp_hip.h osqp_hip_batch_adjoint_lockstep; lockstep_hip.hip lockstep_adjoint_chunk) -- the
backward pass of a batch of QPs that share P and A at a size past the batch adjoint kernel.

The base batch is that of tests/test_gpu_batch_lockstep.py: banded_qp(400, window=40) (n = 400, m = 800), B = 70 = a full chunk and a ragged one of 6,
q / l / u as that file's _batch builds them, eps 1e-8; (x, y) come from ONE hip_batch_solve_lockstep call.  Input condition, asserted per element: every
inequality row keeps a class margin min(|(z - l) + y|, |(u - z) - y|) >= 1e-9.  Checks:
  * certificate (tests/adjoint_sparse_ref.certificate: K_a and g rebuilt on the host) below OSQP_HIP_ADJOINT_TOL for every element, with and without dy;
  * the sparse yardstick at elements 0, 63, 64, 69: |r - r_ref| / |r_ref| <= 10 (host residual) |g| / (sigma_min |r_ref|), the bound of
    tests/test_gpu_adjoint_pcg.py (a residual rho leaves at most rho |g| / sigma_min in r; 10 covers max-norm against 2-norm); dP / dA against the host
    formulas on the returned vectors to 1e-13 of max |value|;
  * independence (solo calls and the reversed batch give the same bits), the single-handle route within the two certified residuals' bounds added, the
    handle left alone (a twin that never made the call gives the same bits), a reordered handle, the statuses 0 / 2 / 3 in one chunk, the declines
    and queries, and the torch layer with large_batch='lockstep', large_backward='lockstep' (one engine call per backward)."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import adjoint_sparse_ref as ref
import osqp_amd
import problems
from osqp_amd import ext_hip
from util import record_deviation

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
S = osqp_amd.SolverStatus
NOT_IMPL = ext_hip.osqp_error_type.OSQP_FUNC_NOT_IMPLEMENTED
EPS = 1e-8
TOL = 1e-6                 # OSQP_HIP_ADJOINT_TOL
B = 70                     # one full chunk of 64 and a ragged one of 6
PICK = (0, 63, 64, 69)     # first / last lane of the full chunk, first / last of the ragged one
ST = dict(eps_abs=EPS, eps_rel=EPS, max_iter=50000, adaptive_rho_interval=50, check_termination=25)
KEYS = ('dP', 'dq', 'dA', 'dl', 'du', 'rec')


def _batch(q, l, u, nb, seed=13):      # (tests/test_gpu_batch_lockstep.py _batch)
    rng = np.random.default_rng(seed)
    return (np.stack([q + 0.05 * b * rng.standard_normal(len(q)) for b in range(nb)]), np.stack([l - 0.01 * b for b in range(nb)]),
            np.stack([u + 0.01 * b for b in range(nb)]))


def _handle(P, q, A, l, u, **kw):
    st = dict(ST); st.update(kw)
    s = osqp_amd.OSQP(algebra='hip')
    s.setup(P, q, A, l, u, verbose=False, **st)
    return s


def _margin(A, l, u, x, y):
    z = A @ x
    ineq = l != u
    return float(np.minimum(np.abs((z - l) + y), np.abs((u - z) - y))[ineq].min(initial=np.inf))


def _rvec(g, b, act):
    return np.concatenate([g['dq'][b], -(g['dl'][b] + g['du'][b])[act]])


class Base:
    def __init__(self):
        self.P, self.q, self.A, self.l, self.u = problems.banded_qp(400, window=40)
        self.P, self.A = sp.csc_matrix(self.P), sp.csc_matrix(self.A)
        self.n, self.m = len(self.q), len(self.l)
        self.Q, self.L, self.U = _batch(self.q, self.l, self.u, B)
        self.s = _handle(self.P, self.q, self.A, self.l, self.u)
        self.x, self.y, self.rec = self.s._solver.hip_batch_solve_lockstep(q=self.Q, l=self.L, u=self.U)
        assert (self.rec[:, 0] == S.OSQP_SOLVED).all()
        rng = np.random.default_rng(7)
        self.dx = self.x - 0.1 * rng.standard_normal((B, self.n))
        self.dy = rng.standard_normal((B, self.m))
        self.g = {wd: self.s._solver.hip_batch_adjoint_lockstep(self.x, self.y, self.dx, self.dy if wd else None, l=self.L, u=self.U) for wd in (False, True)}
        self.last = self.s._solver.lockstep_adjoint_last_record()
        self.cert = {}                       # (with_dy, b) -> (host residual, g, r, active rows): computed once, shared

    def certificate(self, wd, b):
        if (wd, b) not in self.cert:
            g = self.g[wd]
            self.cert[(wd, b)] = ref.certificate(self.P, self.A, self.L[b], self.U[b], self.x[b], self.y[b], self.dx[b], self.dy[b] if wd else None,
                                                 g['dq'][b], g['dl'][b], g['du'][b])
        return self.cert[(wd, b)]


@pytest.fixture(scope='module')
def base():
    return Base()


def test_certificate_every_element(base):
    """Every element, with and without dy: the host's certificate below the threshold, status 0, the active rows the host counts, the record's residual
    within a factor 10 of the host's; the batch adjoint kernel still declines this shape."""
    assert base.last['chunks'] == 2 and base.last['width'] == 64 and base.last['steps_max'] >= 4 and base.last['kernel_launches'] > 0, base.last
    for b in range(B):
        margin = _margin(base.A, base.L[b], base.U[b], base.x[b], base.y[b])
        assert margin >= 1e-9, (b, margin)
    worst = 0.0
    for wd in (False, True):
        rec = base.g[wd]['rec']
        for b in range(B):
            host_res, gv, rv, nact = base.certificate(wd, b)
            worst = max(worst, host_res)
            assert host_res < TOL, (wd, b, host_res)
            assert rec[b, 0] == 0 and rec[b, 1] == nact and rec[b, 3] >= 4, (wd, b, rec[b], nact)
            assert rec[b, 2] < TOL and rec[b, 2] <= 10 * host_res and host_res <= 10 * rec[b, 2], (wd, b, rec[b, 2], host_res)
    print('worst host residual %.3e; last record %s' % (worst, base.last))
    with pytest.raises(ValueError) as e:
        base.s._solver.hip_batch_adjoint(base.x, base.y, base.dx, l=base.L, u=base.U)
    assert e.value.code == NOT_IMPL


@pytest.mark.parametrize('with_dy', [False, True])
def test_yardstick(base, with_dy):
    g = base.g[with_dy]
    for b in PICK:
        host_res, gv, rv, nact = base.certificate(with_dy, b)
        y0 = ref.adjoint(base.P, base.A, base.L[b], base.U[b], base.x[b], base.y[b], base.dx[b], base.dy[b] if with_dy else None)
        r_ref = np.concatenate([y0['r_x'], y0['r_y'][y0['act']]])
        dev = float(np.linalg.norm(rv - r_ref) / np.linalg.norm(r_ref))
        bound = 10 * host_res * np.linalg.norm(gv) / (y0['sigma_min'] * np.linalg.norm(r_ref))
        record_deviation('test_gpu_lockstep_adjoint', 'banded n=400 element %d dy=%s' % (b, with_dy), r_rel_dev=dev, bound=float(bound), host_residual=host_res,
                         record_residual=float(g['rec'][b, 2]), active_rows=nact, steps=int(g['rec'][b, 3]), sigma_min=y0['sigma_min'])
        print('element %d dy=%s: |r - r_ref| / |r_ref| = %.3e (bound %.3e), sigma_min %.3e, steps %d' % (b, with_dy, dev, bound, y0['sigma_min'], g['rec'][b, 3]))
        assert dev <= bound, (b, dev, bound)
        dP, dA = ref.gradients(base.P, base.A, base.x[b], base.y[b], g['dq'][b], -(g['dl'][b] + g['du'][b]))
        for got, want in ((g['dP'][b], dP), (g['dA'][b], dA)):
            assert got.shape == want.shape
            assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), (b, np.abs(got - want).max() / np.abs(want).max())


def test_independence(base):
    """An element's outputs and record do not depend on what else is in the batch or where in it the element sits."""
    g = base.g[True]
    for b in PICK:
        sl = slice(b, b + 1)
        g1 = base.s._solver.hip_batch_adjoint_lockstep(base.x[sl], base.y[sl], base.dx[sl], base.dy[sl], l=base.L[sl], u=base.U[sl])
        for k in KEYS:
            assert np.array_equal(g1[k][0], g[k][b]), (b, k)
    r = lambda a: a[::-1].copy()
    gr = base.s._solver.hip_batch_adjoint_lockstep(r(base.x), r(base.y), r(base.dx), r(base.dy), l=r(base.L), u=r(base.U))
    for k in KEYS:
        assert np.array_equal(gr[k][::-1], g[k]), k


def _single(s, l, u, x, y, dx, dy):
    s.update(l=l, u=u)
    ext = s._solver
    st = ext.adjoint_derivative_compute_at(x, y, dx, dy)
    assert st == 0, (st, ext.adjoint_last_record())
    dq, dl, du = np.empty(len(x)), np.zeros(len(y)), np.zeros(len(y))
    assert ext.adjoint_derivative_get_vec(dq, dl, du) == 0
    return dict(dq=dq, dl=dl, du=du), ext.adjoint_last_record()


def _pair_bound(res_a, res_b, smin):
    """Both solve K_a r = g at the same (x, y), each to its own certified residual: r differs by at most (res_a + res_b) |g| / sigma_min (the yardstick's
    bound for each against the exact solution, added), with the factor 10 for max-norm against 2-norm (tests/test_gpu_adjoint_pcg.py test_reordered_handle)."""
    return 10 * (res_a[0] + res_b[0]) * np.linalg.norm(res_b[1]) / (smin * np.linalg.norm(res_b[2]))


def test_against_the_single_handle_route(base):
    for b in (0, 69):
        g1, rec1 = _single(base.s, base.L[b], base.U[b], base.x[b], base.y[b], base.dx[b], base.dy[b])
        res0 = base.certificate(True, b)
        res1 = ref.certificate(base.P, base.A, base.L[b], base.U[b], base.x[b], base.y[b], base.dx[b], base.dy[b], g1['dq'], g1['dl'], g1['du'])
        smin = ref.adjoint(base.P, base.A, base.L[b], base.U[b], base.x[b], base.y[b], base.dx[b], base.dy[b])['sigma_min']
        dev = float(np.linalg.norm(res0[2] - res1[2]) / np.linalg.norm(res1[2]))
        bound = _pair_bound(res0, res1, smin)
        record_deviation('test_gpu_lockstep_adjoint', 'element %d against the single-handle route' % b, r_rel_dev=dev, bound=float(bound), steps=int(base.g[True]['rec'][b, 3]),
                         single_steps=rec1['steps'])
        print('element %d: lockstep against single handle %.3e (bound %.3e); steps %d / %d' % (b, dev, bound, base.g[True]['rec'][b, 3], rec1['steps']))
        assert res0[3] == res1[3] == rec1['active_rows'] and dev <= bound, (dev, bound)
    base.s.update(l=base.l, u=base.u)


def test_handle_is_left_alone(base):
    """solve(), update(q), solve(), a warm start and a third solve with the lockstep adjoint called in between, against a twin that never calls it."""
    out = []
    q2 = base.Q[5]
    for call in (False, True):
        s = _handle(base.P, base.q, base.A, base.l, base.u, eps_abs=1e-6, eps_rel=1e-6)
        adj = (lambda: s._solver.hip_batch_adjoint_lockstep(base.x[:3], base.y[:3], base.dx[:3], base.dy[:3], l=base.L[:3], u=base.U[:3])) if call else (lambda: None)
        adj()
        ra = s.solve()
        adj()
        s.update(q=q2)
        rb = s.solve()
        adj()
        s.warm_start(x=ra.x, y=ra.y)
        adj()
        rc = s.solve()
        out.append((ra, rb, rc, s._solver.lockstep_last_record()))
    for a, b in zip(out[0][:3], out[1][:3]):
        assert a.info.status_val == b.info.status_val == S.OSQP_SOLVED and a.info.iter == b.info.iter
        assert np.array_equal(a.x, b.x) and np.array_equal(a.y, b.y)
    assert out[0][3] == out[1][3] and out[1][3]['chunks'] == 0                   # the forward route's record has not moved


def test_reordered_handle(base, monkeypatch):
    nb = 5
    monkeypatch.setenv('OSQP_HIP_REORDER', '2')
    s = _handle(base.P, base.q, base.A, base.l, base.u)
    assert s._solver.hip_stats()['reordered'] == 1
    sl = slice(0, nb)
    g = s._solver.hip_batch_adjoint_lockstep(base.x[sl], base.y[sl], base.dx[sl], base.dy[sl], l=base.L[sl], u=base.U[sl])
    for b in range(nb):
        res1 = ref.certificate(base.P, base.A, base.L[b], base.U[b], base.x[b], base.y[b], base.dx[b], base.dy[b], g['dq'][b], g['dl'][b], g['du'][b])
        res0 = base.certificate(True, b)
        assert res1[0] < TOL and g['rec'][b, 0] == 0 and g['rec'][b, 1] == res1[3] == res0[3], (b, res1[0], g['rec'][b])
        # the caller's numbering and CSC order: the host formulas at the caller's stored entries, from the returned vectors
        dP, dA = ref.gradients(base.P, base.A, base.x[b], base.y[b], g['dq'][b], -(g['dl'][b] + g['du'][b]))
        for got, want in ((g['dP'][b], dP), (g['dA'][b], dA)):
            assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), b
        smin = ref.adjoint(base.P, base.A, base.L[b], base.U[b], base.x[b], base.y[b], base.dx[b], base.dy[b])['sigma_min']
        dev = float(np.linalg.norm(res1[2] - res0[2]) / np.linalg.norm(res0[2]))
        bound = _pair_bound(res1, res0, smin)
        record_deviation('test_gpu_lockstep_adjoint', 'reordered against as numbered, element %d' % b, r_rel_dev=dev, bound=float(bound))
        assert dev <= bound, (b, dev, bound)


def test_statuses_in_one_chunk():
    """n = 420, P = diag(d), A = [I; I] (the caller supplies x, y: no forward solve): an ordinary box problem (status 0), every row an equality (840 active rows
    against 420 variables: status 2, no step), the same row of I stored twice as equalities with contradicting dy (status 3), another box problem; the
    two solved elements have the bits of their solo calls."""
    n = 420
    rng = np.random.default_rng(7)
    d = 0.5 + rng.random(n)
    P = sp.diags(d, format='csc'); A = sp.vstack([sp.identity(n), sp.identity(n)], format='csc')
    l = np.concatenate([-np.ones(n), -2 * np.ones(n)]); u = np.concatenate([np.ones(n), 2 * np.ones(n)])
    s = osqp_amd.OSQP(algebra='hip'); s.setup(P, rng.standard_normal(n), A, l, u, verbose=False, eps_abs=1e-6, eps_rel=1e-6)
    nb, m = 4, 2 * n
    L, U = np.tile(l, (nb, 1)), np.tile(u, (nb, 1))
    X, Y, DX, DY = np.zeros((nb, n)), np.zeros((nb, m)), rng.standard_normal((nb, n)), np.zeros((nb, m))
    for b in (0, 3):                                                            # the box problems' exact solutions: x = clip(-q / d, -1, 1), y from stationarity
        q = 2.0 * rng.standard_normal(n)
        X[b] = np.clip(-q / d, -1.0, 1.0)
        Y[b, :n] = np.where(np.abs(X[b]) == 1.0, -(d * X[b] + q), 0.0)
        DY[b] = rng.standard_normal(m)
        assert 0 < np.count_nonzero(Y[b]) < n and _margin(A, L[b], U[b], X[b], Y[b]) >= 1e-9
    X[1] = rng.standard_normal(n); L[1] = U[1] = np.concatenate([X[1], X[1]]); Y[1] = rng.standard_normal(m)      # every row an equality at a consistent b
    L[2] = -np.inf; U[2] = np.inf; L[2, [0, n]] = U[2, [0, n]] = 0.0; DY[2, 0], DY[2, n] = 1.0, -1.0          # x_0 = -1 and x_0 = +1
    g = s._solver.hip_batch_adjoint_lockstep(X, Y, DX, DY, l=L, u=U)
    rec = g['rec']
    print(rec)
    assert list(rec[:, 0]) == [0, 2, 3, 0], rec
    assert rec[1, 1] == 2 * n and rec[1, 3] == 0 and rec[2, 1] == 2 and rec[2, 3] > 0 and not (rec[2, 2] < TOL)
    for b in (0, 3):
        res = ref.certificate(P, A, L[b], U[b], X[b], Y[b], DX[b], DY[b], g['dq'][b], g['dl'][b], g['du'][b])
        assert res[0] < TOL and rec[b, 1] == res[3], (b, res[0], rec[b])
        sl = slice(b, b + 1)
        g1 = s._solver.hip_batch_adjoint_lockstep(X[sl], Y[sl], DX[sl], DY[sl], l=L[sl], u=U[sl])
        for k in KEYS:
            assert np.array_equal(g1[k][0], g[k][b]), (b, k)


def test_declines_and_queries(base):
    P, q, A, l, u = problems.portfolio_qp(200, 10)
    s1 = osqp_amd.OSQP(algebra='hip'); s1.setup(P, q, A, l, u, verbose=False, eps_abs=1e-6, eps_rel=1e-6, max_iter=20000)
    assert s1._solver.hip_stats()['woodbury_rows'] > 0
    n, m = len(q), len(l)
    with pytest.raises(ValueError) as e:
        s1._solver.hip_batch_adjoint_lockstep(np.zeros((3, n)), np.zeros((3, m)), np.ones((3, n)))
    assert e.value.code == NOT_IMPL
    with pytest.raises(ValueError) as e:
        s1._solver.hip_batch_adjoint_lockstep_device(0, None, None, None)
    assert e.value.code == NOT_IMPL
    base.s._solver.hip_batch_adjoint_lockstep_device(0, None, None, None)          # the applicability query on the base handle: no exception


def test_device_pointers(base):
    import torch
    dev = torch.device('cuda', 0)
    nb = 6
    t = lambda a: torch.tensor(a[64:64 + nb], dtype=torch.float64, device=dev).contiguous()
    xd, yd, gx, gy, ld, ud = t(base.x), t(base.y), t(base.dx), t(base.dy), t(base.L), t(base.U)
    ext = base.s._solver
    widths = dict(dP=ext.nnz_P, dq=base.n, dA=ext.nnz_A, dl=base.m, du=base.m, rec=4)
    out = {k: torch.empty((nb, w), dtype=torch.float64, device=dev) for k, w in widths.items()}
    ext.hip_batch_adjoint_lockstep_device(nb, xd.data_ptr(), yd.data_ptr(), gx.data_ptr(), gy.data_ptr(), ld.data_ptr(), ud.data_ptr(),
                                          out['dP'].data_ptr(), out['dq'].data_ptr(), out['dA'].data_ptr(), out['dl'].data_ptr(), out['du'].data_ptr(), out['rec'].data_ptr(),
                                          stream=torch.cuda.current_stream(dev).cuda_stream)
    for k in KEYS:
        assert np.array_equal(out[k].cpu().numpy(), base.g[True][k][64:64 + nb]), k


@pytest.mark.parametrize('device', ['cpu', 'cuda'])
def test_torch_layer(base, device):
    import torch
    from osqp_amd.nn.torch import OSQP as Layer
    with pytest.raises(ValueError):
        Layer(([0], [0]), (1, 1), ([0], [0]), (1, 1), large_backward='other')
    nb = 3
    Pc, Ac = sp.csc_matrix(base.P), sp.csc_matrix(base.A)
    Pc.sort_indices(); Ac.sort_indices()
    pco, aco = Pc.tocoo(), Ac.tocoo()
    mk = lambda **kw: Layer((pco.row, pco.col), Pc.shape, (aco.row, aco.col), Ac.shape, eps_rel=EPS, eps_abs=EPS, max_iter=200000, **kw)
    vals = [Pc.data, base.Q[:nb], Ac.data, base.L[:nb], base.U[:nb]]
    # (large_backward is a keyword of its own: large_batch='lockstep' alone keeps the per-element backward it has always had, see the last case)
    for mode, kw, calls in (('lockstep', dict(large_batch='lockstep', large_backward='lockstep'), 1), ('loop', dict(large_batch='loop'), nb),
                            ('lockstep forward only', dict(large_batch='lockstep'), nb)):
        layer = mk(**kw)
        ts = [torch.tensor(np.array(v), dtype=torch.float64, device=device, requires_grad=True) for v in vals]
        x = layer(*ts)
        before = layer.adjoint_launches
        (0.5 * (x ** 2).sum()).backward()
        assert layer.adjoint_launches == before + calls, (mode, layer.adjoint_launches - before)
        rec = torch.as_tensor(layer.last_adjoint_rec).cpu().numpy()
        assert rec.shape == (nb, 4) and (rec[:, 0] == 0).all(), rec
        for t in ts:
            assert t.grad is not None and t.grad.shape == t.shape and t.grad.device == t.device and bool(torch.isfinite(t.grad).all())
        if mode != 'lockstep':
            continue
        X, Y = x.detach().cpu().numpy(), torch.as_tensor(layer.last_dual).cpu().numpy()
        gP, dq, gA, dl, du = (t.grad.cpu().numpy() for t in ts)
        p_map = layer._p_map(len(Pc.data))
        sumP, sumA, scale = np.zeros(len(Pc.data)), np.zeros(len(Ac.data)), [0.0, 0.0]
        for b in range(nb):
            host_res, gv, rv, nact = ref.certificate(base.P, base.A, base.L[b], base.U[b], X[b], Y[b], X[b], None, dq[b], dl[b], du[b])
            assert host_res < TOL and rec[b, 1] == nact, (b, host_res, rec[b], nact)
            dP, dA = ref.gradients(base.P, base.A, X[b], Y[b], dq[b], -(dl[b] + du[b]))
            sumP += dP[p_map]; sumA += dA
            scale = [max(scale[0], np.abs(dP).max()), max(scale[1], np.abs(dA).max())]
        # every element's entries agree with the host formulas to 1e-13 of their largest (test_yardstick); the sum of nb of them to nb times that
        assert np.abs(gP - sumP).max() <= 1e-13 * nb * scale[0], np.abs(gP - sumP).max() / scale[0]
        assert np.abs(gA - sumA).max() <= 1e-13 * nb * scale[1], np.abs(gA - sumA).max() / scale[1]
