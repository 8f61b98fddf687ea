"""GPU tier: adjoint derivatives on the direct lockstep route (include/osqp_hip.h osqp_hip_batch_adjoint_lockstep_direct; lockstep_hip.hip
lockstep_direct_adjoint_chunk) -- the backward pass of a batch of QPs that share P and A on a Woodbury handle with a diagonal K0.

The base batch is that of tests/test_gpu_lockstep_direct.py: problems.portfolio_qp(600, 4) (n = 604, m = 605, r = 5), B = 70 = a full chunk and a ragged
one of 6, that file's Q / L / U and settings at eps 1e-8; (x, y) come from ONE hip_batch_solve_lockstep_direct call, dx = x - 0.1 noise and dy random from
default_rng(7).  Input condition, asserted per element: every inequality row keeps a class margin min(|(z - l) + y|, |(u - z) - y|) >= 1e-9.  Checks
(the tolerances are those of tests/test_gpu_lockstep_adjoint.py):
  * certificate (tests/adjoint_sparse_ref.certificate: K_a and g rebuilt on the host) below OSQP_HIP_ADJOINT_TOL for every element, with and without dy,
    one inversion of S per problem;
  * the sparse yardstick at elements 0, 63, 64, 69: |r - r_ref| / |r_ref| <= 10 (host residual) |g| / (sigma_min |r_ref|); dP / dA -- the dense rows'
    entries included -- against the host formulas on the returned vectors to 1e-13 of max |value|;
  * independence (solo calls and the reversed batch give the same bits), the handle left alone, r = 1 and r = 128, the declines at r = 129 and on a
    banded handle, the statuses 0 / 2 / 3 in one chunk, device pointers, and the torch layer with large_batch = large_backward = 'lockstep_direct'."""
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
ST = dict(eps_abs=EPS, eps_rel=EPS, max_iter=50000, adaptive_rho_interval=50, check_termination=25, warm_starting=False)      # (tests/test_gpu_lockstep_direct.py ST)
KEYS = ('dP', 'dq', 'dA', 'dl', 'du', 'rec')
NA, K = 600, 4


def _handle(P, q, A, l, u, **kw):
    st = dict(ST); st.update(kw)
    s = osqp_amd.OSQP(algebra='hip')
    s.setup(P, q, A, l, u, verbose=False, **st)
    return s


def _margin(A, l, u, x, y):
    z = A @ x
    ineq = l != u
    return float(np.minimum(np.abs((z - l) + y), np.abs((u - z) - y))[ineq].min(initial=np.inf))


def _factor_qp(na, k, density, seed=3):      # (tests/test_gpu_lockstep_direct.py _factor_qp)
    rng = np.random.default_rng(seed)
    F = sp.random(na, k, density=density, random_state=rng, data_rvs=rng.standard_normal, format='csc')
    D = sp.diags(rng.random(na) * np.sqrt(k))
    mu = rng.standard_normal(na)
    P = sp.block_diag([2.0 * D, 2.0 * sp.eye(k)], format='csc')
    q = np.concatenate([-mu, np.zeros(k)])
    A = sp.vstack([sp.hstack([F.T, -sp.eye(k)]), sp.hstack([sp.csc_matrix(np.ones((1, na))), sp.csc_matrix((1, k))]),
                   sp.hstack([sp.eye(na), sp.csc_matrix((na, k))])], format='csc')
    l = np.concatenate([np.zeros(k), [1.0], np.zeros(na)])
    u = np.concatenate([np.zeros(k), [1.0], np.ones(na)])
    return P, q, A, l, u


def _one_dense_row():                         # (tests/test_gpu_lockstep_direct.py test_one_dense_row)
    n = 500
    rng = np.random.default_rng(2)
    P = sp.diags(0.5 + rng.random(n), format='csc')
    budget = sp.csc_matrix((np.ones(200), (np.zeros(200, dtype=int), np.arange(0, 400, 2))), shape=(1, n))
    A = sp.vstack([budget, sp.identity(n)], format='csc')
    l, u = np.concatenate([[1.0], np.zeros(n)]), np.concatenate([[1.0], np.ones(n)])
    return P, rng.standard_normal(n), A, l, u


class Base:
    def __init__(self):
        self.P, self.q, self.A, self.l, self.u = problems.portfolio_qp(NA, K)
        self.P, self.A = sp.csc_matrix(self.P), sp.csc_matrix(self.A)
        self.n, self.m = len(self.q), len(self.l)
        rng = np.random.default_rng(17)                                                  # (tests/test_gpu_lockstep_direct.py Base)
        self.Q = np.stack([np.concatenate([-rng.standard_normal(NA) / (1.0 + 0.05 * b), np.zeros(K)]) for b in range(B)])
        self.L, self.U = np.tile(self.l, (B, 1)), np.tile(self.u, (B, 1))
        for b in (3, 63, 66):
            self.U[b, K + 1:] = 0.02 + 0.01 * rng.random(NA)
        self.s = _handle(self.P, self.q, self.A, self.l, self.u)
        ext = self.s._solver
        self.x, self.y, self.rec = ext.hip_batch_solve_lockstep_direct(q=self.Q, l=self.L, u=self.U)
        assert (self.rec[:, 0] == S.OSQP_SOLVED).all()
        self.fwd_last = ext.lockstep_direct_last_record()
        rng = np.random.default_rng(7)
        self.dx = self.x - 0.1 * rng.standard_normal((B, self.n))
        self.dy = rng.standard_normal((B, self.m))
        self.g, self.last = {}, {}
        for wd in (False, True):
            self.g[wd] = ext.hip_batch_adjoint_lockstep_direct(self.x, self.y, self.dx, self.dy if wd else None, l=self.L, u=self.U)
            self.last[wd] = ext.lockstep_direct_adjoint_last_record()
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
    """Every element, with and without dy: the host's certificate below the threshold, status 0, the active rows the host counts, at least
    1 + polish_refine_iter steps, the record's residual within a factor 10 of the host's; S inverted once per problem and never at a step; the forward
    route's record has not moved."""
    assert (base.n, base.m) == (604, 605) and base.s._solver.hip_stats()['woodbury_rows'] == 5
    min_steps = 1 + int(base.s.settings.polish_refine_iter)
    for b in range(B):
        margin = _margin(base.A, base.L[b], base.U[b], base.x[b], base.y[b])
        assert margin >= 1e-9, (b, margin)
    worst = 0.0
    for wd in (False, True):
        last, rec = base.last[wd], base.g[wd]['rec']
        assert last['chunks'] == 2 and last['width'] == 64 and last['inversions'] == B and last['kernel_launches'] > 0, last
        for b in range(B):
            host_res, gv, rv, nact = base.certificate(wd, b)
            worst = max(worst, host_res)
            print('dy=%s element %d: host residual %.3e, record residual %.3e, active rows %d, steps %d' % (wd, b, host_res, rec[b, 2], rec[b, 1], rec[b, 3]))
            assert host_res < TOL, (wd, b, host_res)
            assert rec[b, 0] == 0 and rec[b, 1] == nact and rec[b, 3] >= min_steps, (wd, b, rec[b], nact)
            assert rec[b, 2] < TOL and rec[b, 2] <= 10 * host_res and host_res <= 10 * rec[b, 2], (wd, b, rec[b, 2], host_res)
        assert last['steps_max'] == rec[:, 3].max()
        print('dy=%s: steps %d .. %d, record residual %.3e .. %.3e, last record %s' % (wd, rec[:, 3].min(), rec[:, 3].max(), rec[:, 2].min(), rec[:, 2].max(), last))
    print('worst host residual %.3e' % worst)
    assert base.s._solver.lockstep_direct_last_record() == base.fwd_last
    for route in (base.s._solver.hip_batch_adjoint, base.s._solver.hip_batch_adjoint_lockstep):      # the two other batch routes still decline this handle
        with pytest.raises(ValueError) as e:
            route(base.x, base.y, base.dx, l=base.L, u=base.U)
        assert e.value.code == NOT_IMPL


@pytest.mark.parametrize('with_dy', [False, True])
def test_yardstick(base, with_dy):
    g = base.g[with_dy]
    dense = np.diff(sp.csr_matrix(base.A).indptr) > 128
    assert int(dense.sum()) == 5
    in_dense = dense[sp.csc_matrix(base.A).tocoo().row]      # (tocoo of a CSC matrix keeps the CSC order: adjoint_sparse_ref.stored_entries)
    for b in PICK:
        host_res, gv, rv, nact = base.certificate(with_dy, b)
        y0 = ref.adjoint(base.P, base.A, base.L[b], base.U[b], base.x[b], base.y[b], base.dx[b], base.dy[b] if with_dy else None)
        r_ref = np.concatenate([y0['r_x'], y0['r_y'][y0['act']]])
        dev = float(np.linalg.norm(rv - r_ref) / np.linalg.norm(r_ref))
        bound = 10 * host_res * np.linalg.norm(gv) / (y0['sigma_min'] * np.linalg.norm(r_ref))
        record_deviation('test_gpu_lockstep_direct_adjoint', 'portfolio 600x4 element %d dy=%s' % (b, with_dy), r_rel_dev=dev, bound=float(bound), host_residual=host_res,
                         record_residual=float(g['rec'][b, 2]), active_rows=nact, steps=int(g['rec'][b, 3]), sigma_min=y0['sigma_min'])
        print('element %d dy=%s: |r - r_ref| / |r_ref| = %.3e (bound %.3e), sigma_min %.3e, steps %d' % (b, with_dy, dev, bound, y0['sigma_min'], g['rec'][b, 3]))
        assert dev <= bound, (b, dev, bound)
        dP, dA = ref.gradients(base.P, base.A, base.x[b], base.y[b], g['dq'][b], -(g['dl'][b] + g['du'][b]))
        for got, want in ((g['dP'][b], dP), (g['dA'][b], dA), (g['dA'][b][in_dense], dA[in_dense])):
            assert got.shape == want.shape and got.size > 0
            assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), (b, np.abs(got - want).max() / np.abs(want).max())


def test_independence(base):
    """An element's outputs and record do not depend on what else is in the batch or where in it the element sits."""
    g = base.g[True]
    call = base.s._solver.hip_batch_adjoint_lockstep_direct
    for b in PICK:
        sl = slice(b, b + 1)
        g1 = call(base.x[sl], base.y[sl], base.dx[sl], base.dy[sl], l=base.L[sl], u=base.U[sl])
        for k in KEYS:
            assert np.array_equal(g1[k][0], g[k][b]), (b, k)
    r = lambda a: a[::-1].copy()
    gr = call(r(base.x), r(base.y), r(base.dx), r(base.dy), l=r(base.L), u=r(base.U))
    for k in KEYS:
        assert np.array_equal(gr[k][::-1], g[k]), k


def test_handle_is_left_alone(base):
    """solve(), update(q), solve(), a warm start and a third solve with the direct lockstep adjoint called in between, against a twin that never calls it."""
    out = []
    q2 = base.Q[5]
    for call in (False, True):
        s = _handle(base.P, base.q, base.A, base.l, base.u, eps_abs=1e-6, eps_rel=1e-6, warm_starting=True)
        adj = (lambda: s._solver.hip_batch_adjoint_lockstep_direct(base.x[:3], base.y[:3], base.dx[:3], base.dy[:3], l=base.L[:3], u=base.U[:3])) if call else (lambda: None)
        adj()
        ra = s.solve()
        adj()
        s.update(q=q2)
        rb = s.solve()
        adj()
        s.warm_start(x=ra.x, y=ra.y)
        adj()
        rc = s.solve()
        out.append((ra, rb, rc, s._solver.lockstep_direct_last_record(), s._solver.lockstep_direct_adjoint_last_record()))
    for a, b in zip(out[0][:3], out[1][:3]):
        assert a.info.status_val == b.info.status_val == S.OSQP_SOLVED and a.info.iter == b.info.iter
        assert np.array_equal(a.x, b.x) and np.array_equal(a.y, b.y)
    assert out[0][3] == out[1][3] and out[1][3]['chunks'] == 0                   # the forward route's record has not moved
    assert out[0][4]['chunks'] == 0 and out[1][4]['chunks'] == 1 and out[1][4]['inversions'] == 3


def _edge(P, q, A, l, u, r):
    """Three elements as tests/test_gpu_lockstep_direct.py _edge builds them, solved by the forward route, then the backward: certificate and status."""
    P, A = sp.csc_matrix(P), sp.csc_matrix(A)
    n, m = len(q), len(l)
    rng = np.random.default_rng(5)
    Q = np.stack([q * (1.0 + 0.3 * b) + 0.1 * b * rng.standard_normal(n) * (q != 0) for b in range(3)])
    L, U = np.tile(l, (3, 1)), np.tile(u, (3, 1))
    s = _handle(P, q, A, l, u)
    assert s._solver.hip_stats()['woodbury_rows'] == r
    x, y, rec = s._solver.hip_batch_solve_lockstep_direct(q=Q, l=L, u=U)
    assert (rec[:, 0] == S.OSQP_SOLVED).all(), rec[:, 0]
    rng = np.random.default_rng(7)
    dx, dy = x - 0.1 * rng.standard_normal((3, n)), rng.standard_normal((3, m))
    g = s._solver.hip_batch_adjoint_lockstep_direct(x, y, dx, dy, l=L, u=U)
    last = s._solver.lockstep_direct_adjoint_last_record()
    assert last['chunks'] == 1 and last['inversions'] == 3, last
    for b in range(3):
        margin = _margin(A, L[b], U[b], x[b], y[b])
        assert margin >= 1e-9, (r, b, margin)
        host_res, gv, rv, nact = ref.certificate(P, A, L[b], U[b], x[b], y[b], dx[b], dy[b], g['dq'][b], g['dl'][b], g['du'][b])
        print('r = %d element %d: margin %.2e, active rows %d, host residual %.3e, record %s' % (r, b, margin, nact, host_res, g['rec'][b]))
        assert host_res < TOL and g['rec'][b, 0] == 0 and g['rec'][b, 1] == nact and nact < n, (r, b, host_res, g['rec'][b])


def test_one_dense_row():
    P, q, A, l, u = _one_dense_row()
    assert int((np.diff(sp.csr_matrix(A).indptr) > 128).sum()) == 1
    _edge(P, q, A, l, u, 1)


def test_128_dense_rows():
    P, q, A, l, u = _factor_qp(400, 127, 0.7)
    assert len(q) == 527 and int((np.diff(sp.csr_matrix(A).indptr) > 128).sum()) == 128
    _edge(P, q, A, l, u, 128)


def test_declines_and_queries(base):
    """r = 129 and a banded handle (no Woodbury rows): OSQP_FUNC_NOT_IMPLEMENTED on both entries, the nbatch == 0 query included; the base handle's
    query answers."""
    for data, rows in ((_factor_qp(400, 128, 0.7), None), (problems.banded_qp(400, window=40), 0)):
        P, q, A, l, u = data
        if rows is None:
            assert int((np.diff(sp.csr_matrix(A).indptr) > 128).sum()) == 129
        s = _handle(P, q, A, l, u, eps_abs=1e-6, eps_rel=1e-6)
        if rows is not None:
            assert s._solver.hip_stats()['woodbury_rows'] == rows
        n, m = len(q), len(l)
        for call in (lambda: s._solver.hip_batch_adjoint_lockstep_direct(np.zeros((3, n)), np.zeros((3, m)), np.ones((3, n))),
                     lambda: s._solver.hip_batch_adjoint_lockstep_direct_device(0, None, None, None)):
            with pytest.raises(ValueError) as e:
                call()
            assert e.value.code == NOT_IMPL
        assert s._solver.lockstep_direct_adjoint_last_record()['chunks'] == 0
    base.s._solver.hip_batch_adjoint_lockstep_direct_device(0, None, None, None)          # the applicability query on the base handle: no exception


def test_statuses_in_one_chunk():
    """n = 500, P diagonal, A = [budget over 200 columns; I; e_0'] (r = 1; the row of x_0 is stored twice, the second copy with bounds it never reaches in
    the solved elements): an element solved by the forward (status 0), every row an equality at a consistent point (n + 2 active rows against n
    variables: status 2, no step), only the two copies of the row of x_0 as equalities with contradicting dy (status 3), another solved element; the
    two solved elements have the bits of their solo calls."""
    n = 500
    rng = np.random.default_rng(2)
    P = sp.diags(0.5 + rng.random(n), format='csc')
    budget = sp.csc_matrix((np.ones(200), (np.zeros(200, dtype=int), np.arange(0, 400, 2))), shape=(1, n))
    e0 = sp.csc_matrix(([1.0], ([0], [0])), shape=(1, n))
    A = sp.vstack([budget, sp.identity(n), e0], format='csc')
    q = rng.standard_normal(n)
    l, u = np.concatenate([[1.0], np.zeros(n), [-10.0]]), np.concatenate([[1.0], np.ones(n), [10.0]])
    nb, m = 4, n + 2
    s = _handle(P, q, A, l, u)
    assert s._solver.hip_stats()['woodbury_rows'] == 1
    Q = np.stack([q, q, q, 1.3 * q + 0.1 * rng.standard_normal(n)])
    L, U = np.tile(l, (nb, 1)), np.tile(u, (nb, 1))
    xf, yf, recf = s._solver.hip_batch_solve_lockstep_direct(q=Q[[0, 3]], l=L[[0, 3]], u=U[[0, 3]])
    assert (recf[:, 0] == S.OSQP_SOLVED).all()
    X, Y, DX, DY = np.zeros((nb, n)), np.zeros((nb, m)), rng.standard_normal((nb, n)), np.zeros((nb, m))
    for k, b in enumerate((0, 3)):
        X[b], Y[b], DY[b] = xf[k], yf[k], rng.standard_normal(m)
        assert _margin(A, L[b], U[b], X[b], Y[b]) >= 1e-9
    X[1] = rng.standard_normal(n); L[1] = U[1] = A @ X[1]; Y[1] = rng.standard_normal(m)                          # every row an equality at a consistent point
    L[2] = -np.inf; U[2] = np.inf; L[2, [1, n + 1]] = U[2, [1, n + 1]] = 0.0; DY[2, 1], DY[2, n + 1] = 1.0, -1.0      # x_0 = -1 and x_0 = +1
    call = s._solver.hip_batch_adjoint_lockstep_direct
    g = call(X, Y, DX, DY, l=L, u=U)
    rec = g['rec']
    print(rec)
    assert list(rec[:, 0]) == [0, 2, 3, 0], rec
    assert rec[1, 1] == n + 2 and rec[1, 3] == 0 and rec[2, 1] == 2 and rec[2, 3] > 0 and not (rec[2, 2] < TOL)
    for b in (0, 3):
        res = ref.certificate(P, A, L[b], U[b], X[b], Y[b], DX[b], DY[b], g['dq'][b], g['dl'][b], g['du'][b])
        assert res[0] < TOL and rec[b, 1] == res[3], (b, res[0], rec[b])
        sl = slice(b, b + 1)
        g1 = call(X[sl], Y[sl], DX[sl], DY[sl], l=L[sl], u=U[sl])
        for k in KEYS:
            assert np.array_equal(g1[k][0], g[k][b]), (b, k)


def test_device_pointers(base):
    import torch
    dev = torch.device('cuda', 0)
    nb = 6
    t = lambda a: torch.tensor(a[64:64 + nb], dtype=torch.float64, device=dev).contiguous()
    xd, yd, gx, gy, ld, ud = t(base.x), t(base.y), t(base.dx), t(base.dy), t(base.L), t(base.U)
    ext = base.s._solver
    widths = dict(dP=ext.nnz_P, dq=base.n, dA=ext.nnz_A, dl=base.m, du=base.m, rec=4)
    out = {k: torch.empty((nb, w), dtype=torch.float64, device=dev) for k, w in widths.items()}
    ext.hip_batch_adjoint_lockstep_direct_device(nb, xd.data_ptr(), yd.data_ptr(), gx.data_ptr(), gy.data_ptr(), ld.data_ptr(), ud.data_ptr(),
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
    tensors = lambda: [torch.tensor(np.array(v), dtype=torch.float64, device=device, requires_grad=True) for v in vals]

    layer = mk(large_batch='lockstep_direct', large_backward='lockstep_direct')
    ts = tensors()
    x = layer(*ts)
    before = layer.adjoint_launches
    (0.5 * (x ** 2).sum()).backward()
    assert layer.adjoint_launches == before + 1, layer.adjoint_launches - before      # ONE engine call for the batch
    assert layer._solver._solver.lockstep_direct_adjoint_last_record()['chunks'] == 1
    rec = torch.as_tensor(layer.last_adjoint_rec).cpu().numpy()
    assert rec.shape == (nb, 4) and (rec[:, 0] == 0).all(), rec
    for t in ts:
        assert t.grad is not None and t.grad.shape == t.shape and t.grad.device == t.device and bool(torch.isfinite(t.grad).all())
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

    layer = mk(large_batch='lockstep_direct')                                        # the forward route alone: the backward it has always had
    x = layer(*tensors())
    with pytest.raises(NotImplementedError):
        (0.5 * (x ** 2).sum()).backward()
