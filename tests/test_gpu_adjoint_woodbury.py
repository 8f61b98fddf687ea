"""GPU tier: adjoint derivatives of a single QP whose linear solve runs the Woodbury-corrected preconditioner (OSQPHipStats::woodbury_rows > 0), the
PCG route of Engine::adjoint_compute_pcg with OSQPHipPolicy::adjoint_woodbury = 1.  Without the field such a handle answers
OSQP_FUNC_NOT_IMPLEMENTED (tested at the end); on the parent of this change set_policy(adjoint_woodbury=1) raises ValueError, so every case here fails.

Problems (eps 1e-8, the policy set right after setup): portfolio_qp(600, 4) and (2000, 20) -- the small form in direct mode; lasso_qp(300, 600) -- the
large form, column space, fused iteration; banded_qp(3000, window=30) with six dense rows, three of them inactive -- the small form as preconditioner
only (K0 not diagonal), rho_L = 1e-6 on the inactive dense rows.  Per problem, with and without dy, the checks of test_gpu_adjoint_pcg._check restated:
the mode through hip_stats(), the independent certificate below OSQP_HIP_ADJOINT_TOL, the record against it, the sparse yardstick within
10 (host residual) |g| / (sigma_min |r|), dP / dA against the host formulas to 1e-13.
Forms: the portfolio QP under OSQP_HIP_WOODBURY_FUSED 1 / 2 / 0 and OSQP_HIP_REORDER=2, the lasso under OSQP_HIP_WOODBURY_DUAL 1 / 0, each certified
and compared pairwise by the two-handle bound of test_gpu_adjoint_pcg.test_reordered_handle.
Finite differences through the engine (portfolio, eps 1e-10, H = 1e-5, rtol = atol = 5e-3), the state contract against a twin handle (bits of later
solves, the four Woodbury statistics, get_policy()), the same with the test hook that makes the inversion at the adjoint's rho report "inaccurate",
and the torch layer's woodbury_backward=True."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import adjoint_sparse_ref as ref
import osqp_amd
import problems
from util import record_deviation

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
ST = dict(eps_abs=1e-8, eps_rel=1e-8, max_iter=200000, verbose=False)
SOLVED = int(osqp_amd.SolverStatus.OSQP_SOLVED)
NI = int(osqp_amd.SolverError.OSQP_FUNC_NOT_IMPLEMENTED)
TOL = 1e-6          # OSQP_HIP_ADJOINT_TOL
H = 1e-5
WB_STATS = ('woodbury_rows', 'woodbury_direct', 'woodbury_factorisations', 'woodbury_cache_hits')


@pytest.fixture(autouse=True)
def _pcg_path(monkeypatch):
    monkeypatch.setenv('OSQP_HIP_SMALL_DIRECT', '0')
    monkeypatch.delenv('OSQP_HIP_ADJOINT_WOODBURY', raising=False)


def banded_dense_qp():
    """banded_qp(3000, window=30) + the six dense rows of test_gpu_woodbury.py, bounds dense @ x0 -/+ half: three tight rows, three loose ones."""
    P, q, A, l, u = problems.banded_qp(3000, window=30)
    rng = np.random.default_rng(1)
    dense = sp.random(6, 3000, density=0.3, random_state=rng, data_rvs=rng.standard_normal, format='csc')
    A2 = sp.vstack([A, dense], format='csc')
    x0 = 0.1 * rng.standard_normal(3000)
    half = np.array([1.0, 1.0, 1.0, 1e3, 1e3, 1e3])
    return P, q, A2, np.concatenate([l, dense @ x0 - half]), np.concatenate([u, dense @ x0 + half])


PROBLEMS = {
    'portfolio 600': (lambda: problems.portfolio_qp(600, 4), dict(woodbury_rows=5, woodbury_direct=2, woodbury_one_launch=1)),
    'portfolio 2000': (lambda: problems.portfolio_qp(2000, 20), dict(woodbury_rows=21, woodbury_direct=2, woodbury_one_launch=1)),
    'lasso 300x600': (lambda: problems.lasso_qp(300, 600), dict(woodbury_rows=600, woodbury_direct=1, woodbury_dual_cols=300, woodbury_fused_iteration=None)),
    'banded + dense rows': (banded_dense_qp, dict(woodbury_rows=6, woodbury_direct=0)),
}


def _setup(P, q, A, l, u, switch=1, **over):
    s = osqp_amd.OSQP(algebra='hip')
    s.setup(P, q, A, l, u, **dict(ST, **over))
    if switch is not None:
        s._solver.set_policy(adjoint_woodbury=switch)
    return s


def _margin(A, l, u, x, y):
    z = A @ x
    ineq = l != u
    return float(np.minimum(np.abs((z - l) + y), np.abs((u - z) - y))[ineq].min(initial=np.inf))


def _grads(s, dx, dy=None):
    s.adjoint_derivative_compute(dx=dx, dy=dy)
    dP, dA = s.adjoint_derivative_get_mat(as_dense=False)
    dq, dl, du = s.adjoint_derivative_get_vec()
    return dict(dP=dP.data.copy(), dA=dA.data.copy(), dq=dq, dl=dl, du=du)


def _mode(s, mode):
    st = s._solver.hip_stats()
    for k, v in mode.items():
        assert (st[k] > 0) if v is None else (st[k] == v), (k, st[k], v)
    return st


def _check(name, P, q, A, l, u, with_dy, mode, seed=7):
    """test_gpu_adjoint_pcg._check on a Woodbury handle: returns the handle, its solve, the incoming gradients and the results."""
    n, m = len(q), len(l)
    rng = np.random.default_rng(seed)
    s = _setup(P, q, A, l, u)
    _mode(s, {k: v for k, v in mode.items() if k == 'woodbury_rows'})
    r = s.solve()
    st = _mode(s, mode)                                        # (the large form decides its direct mode by the probe of a factorisation: after the solve)
    assert r.info.status_val == SOLVED and st['kernel_launches'] > 1, (r.info.status_val, st['kernel_launches'])
    x, y = r.x.copy(), r.y.copy()
    margin = _margin(A, l, u, x, y)
    assert margin >= 1e-9, margin
    dx = x - 0.1 * rng.standard_normal(n)
    dy = rng.standard_normal(m) if with_dy else None
    g = _grads(s, dx, dy)
    rec = s.adjoint_last_record()
    _mode(s, mode)                                             # the call leaves the mode as it found it
    host_res, gv, rv, nact = ref.certificate(P, A, l, u, x, y, dx, dy, g['dq'], g['dl'], g['du'])
    print('%s dy=%s: host residual %.3e, record %s, margin %.2e' % (name, with_dy, host_res, rec, margin))
    assert host_res < TOL, host_res
    assert rec['status'] == 0 and rec['steps'] > 0 and rec['active_rows'] == nact, (rec, nact)
    assert rec['residual'] < TOL and rec['residual'] <= 10 * host_res and host_res <= 10 * rec['residual'], (rec['residual'], host_res)
    y0 = ref.adjoint(P, A, l, u, x, y, dx, dy)
    r_ref = np.concatenate([y0['r_x'], y0['r_y'][y0['act']]])
    dev = float(np.linalg.norm(rv - r_ref) / np.linalg.norm(r_ref))
    bound = 10 * host_res * np.linalg.norm(gv) / (y0['sigma_min'] * np.linalg.norm(r_ref))
    record_deviation('test_gpu_adjoint_woodbury', '%s dy=%s' % (name, with_dy), r_rel_dev=dev, bound=float(bound), host_residual=host_res, record_residual=rec['residual'],
                     active_rows=nact, steps=rec['steps'], sigma_min=y0['sigma_min'], margin=margin, recurrence_s=rec['recurrence_s'], gradient_s=rec['gradient_s'])
    print('   |r - r_ref| / |r_ref| = %.3e (bound %.3e), sigma_min %.3e, steps %d' % (dev, bound, y0['sigma_min'], rec['steps']))
    assert dev <= bound, (dev, bound)
    dP, dA = ref.gradients(P, A, x, y, g['dq'], -(g['dl'] + g['du']))
    for got, want in ((g['dP'], dP), (g['dA'], dA)):
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), np.abs(got - want).max() / np.abs(want).max()
    return s, r, dx, dy, g


@pytest.mark.parametrize('with_dy', [False, True])
@pytest.mark.parametrize('name', list(PROBLEMS))
def test_problem(name, with_dy):
    make, mode = PROBLEMS[name]
    P, q, A, l, u = make()
    s, r, dx, dy, g = _check(name, P, q, A, l, u, with_dy, mode)
    if name == 'banded + dense rows':                          # the problem with inactive long rows: rho_L = 1e-6 there, S carries 1e6
        low, upp = ref.active_set(A, l, u, r.x, r.y)
        act = (low | upp)[-6:]
        assert act.any() and not act.all(), act


def _pairwise(tag, P, A, l, u, runs):
    """runs: name -> (solve, dx, dy, gradients).  Both handles of a pair solve K_a r = g, each to its own certified residual: r differs by at most
    (res_a + res_b) |g| / sigma_min, plus the 1e-8 / sigma_min the two solves' own (x, y) differ by -- the bound of test_gpu_adjoint_pcg.test_reordered_handle."""
    names = list(runs)
    cert = {k: ref.certificate(P, A, l, u, runs[k][0].x, runs[k][0].y, runs[k][1], runs[k][2], runs[k][3]['dq'], runs[k][3]['dl'], runs[k][3]['du']) for k in names}
    r0 = runs[names[0]]
    smin = ref.adjoint(P, A, l, u, r0[0].x, r0[0].y, r0[1], r0[2])['sigma_min']
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            ca, cb = cert[a], cert[b]
            dev = float(np.linalg.norm(ca[2] - cb[2]) / np.linalg.norm(cb[2]))
            bound = 10 * ((ca[0] + cb[0]) * np.linalg.norm(cb[1]) / (smin * np.linalg.norm(cb[2])) + 1e-8 / smin)
            record_deviation('test_gpu_adjoint_woodbury', '%s: %s against %s' % (tag, a, b), r_rel_dev=dev, bound=float(bound))
            print('%s: %s against %s: %.3e (bound %.3e)' % (tag, a, b, dev, bound))
            assert ca[3] == cb[3] and dev <= bound, (a, b, dev, bound)


def test_portfolio_forms(monkeypatch):
    """The small form's direct mode in one launch (k_wbz), two launches, five launches, and on a reordered handle."""
    P, q, A, l, u = problems.portfolio_qp(600, 4)
    forms = {'one launch': ({'OSQP_HIP_WOODBURY_FUSED': '1'}, dict(woodbury_rows=5, woodbury_direct=2, woodbury_one_launch=1)),
             'two launches': ({'OSQP_HIP_WOODBURY_FUSED': '2'}, dict(woodbury_rows=5, woodbury_direct=2, woodbury_one_launch=0)),
             'five launches': ({'OSQP_HIP_WOODBURY_FUSED': '0'}, dict(woodbury_rows=5, woodbury_direct=1, woodbury_one_launch=0)),
             'reordered': ({'OSQP_HIP_REORDER': '2'}, dict(woodbury_rows=5, reordered=1))}
    runs = {}
    dx = dy = None
    for form, (env, mode) in forms.items():
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            s, r, dx_, dy_, g = _check('portfolio 600, ' + form, P, q, A, l, u, True, mode)
        if dx is None:
            dx, dy = dx_, dy_
        else:                                                  # every form differentiates at the same incoming gradients
            g = _grads(s, dx, dy)
        runs[form] = (r, dx, dy, g)
    _pairwise('portfolio 600', P, A, l, u, runs)


def test_lasso_forms(monkeypatch):
    """The large form in column space (fused iteration) and in row space."""
    P, q, A, l, u = problems.lasso_qp(300, 600)
    forms = {'column space': ({'OSQP_HIP_WOODBURY_DUAL': '1'}, dict(woodbury_rows=600, woodbury_direct=1, woodbury_dual_cols=300, woodbury_fused_iteration=None)),
             'row space': ({'OSQP_HIP_WOODBURY_DUAL': '0'}, dict(woodbury_rows=600, woodbury_direct=1, woodbury_dual_cols=0, woodbury_fused_iteration=0))}
    runs = {}
    dx = dy = None
    for form, (env, mode) in forms.items():
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            s, r, dx_, dy_, g = _check('lasso 300x600, ' + form, P, q, A, l, u, True, mode)
        if dx is None:
            dx, dy = dx_, dy_
        else:
            g = _grads(s, dx, dy)
        runs[form] = (r, dx, dy, g)
    _pairwise('lasso 300x600', P, A, l, u, runs)


def test_finite_differences_through_the_engine():
    """Five coordinates each of q, l, u and five stored entries each of P and A, three of the A entries in a dense row.  The portfolio's solution
    holds a handful of assets; everywhere else the box row x_j >= 0 is active and q_j, P_jj and the column's entries of A move the solution only
    at second order.  So each draw is seeded and ordered: the coordinates at which the derivative is of first order first (q_j, P_jj and dense-row
    entries of A at a column with |x_j| > 1e-3; l_i / u_i on inequality rows active at that bound -- an equality row's bound cannot move alone),
    then the others, whose derivative is zero (no row is active at the upper bound x_j <= 1)."""
    na, k = 600, 4
    P, q, A, l, u = problems.portfolio_qp(na, k)
    n = len(q)
    Pt = sp.triu(P, format='csc')
    rng = np.random.default_rng(3)
    xt = 0.1 * rng.standard_normal(n)
    s = _setup(P, q, A, l, u, eps_abs=1e-10, eps_rel=1e-10)
    r = s.solve()
    st = s._solver.hip_stats()
    assert r.info.status_val == SOLVED and st['woodbury_rows'] == k + 1 and st['woodbury_direct'] == 2
    assert _margin(A, l, u, r.x, r.y) >= 1e-9
    g = _grads(s, r.x - xt)
    assert s.adjoint_last_record()['steps'] > 0
    f0 = 0.5 * np.sum((r.x - xt) ** 2)
    low, upp = ref.active_set(A, l, u, r.x, r.y)
    base = dict(q=q, l=l, u=u, Px=Pt.data, Ax=A.data)

    def loss(**kw):
        s.update(**kw)
        rr = s.solve()
        assert rr.info.status_val == SOLVED
        return 0.5 * np.sum((rr.x - xt) ** 2)
    (pr, pc), (ar, ac) = ref.stored_entries(P, A)
    ineq = l != u

    def first(prefer, pool, count):
        a, b = np.nonzero(prefer & pool)[0], np.nonzero(~prefer & pool)[0]
        return np.concatenate([rng.permutation(a), rng.permutation(b)])[:count]
    held = np.abs(r.x) > 1e-3
    assert held.sum() >= 3, held.sum()
    picks = dict(dq=first(held, np.ones(n, bool), 5), dl=first(low, ineq, 5), du=first(upp, ineq, 5), dP=first(held[pc] & (pr == pc), np.ones(len(pc), bool), 5),
                 dA=np.concatenate([first(held[ac], ar <= k, 3), first(held[ac], ar > k, 2)]))
    for key in picks:
        assert len(set(picks[key].tolist())) == 5, key
    assert (ar[picks['dA']] <= k).sum() >= 2
    for which, key in (('dq', 'q'), ('dl', 'l'), ('du', 'u'), ('dP', 'Px'), ('dA', 'Ax')):
        for e in picks[which]:
            v = base[key].copy(); v[e] += H
            fd = (loss(**{key: v}) - f0) / H
            got = g[which][e] * (2.0 if which == 'dP' and pr[e] != pc[e] else 1.0)
            print(which, int(e), 'fd %.6e adjoint %.6e' % (fd, got))
            np.testing.assert_allclose(got, fd, rtol=5e-3, atol=5e-3)
        s.update(**{key: base[key]})


def _same(s, twin, r, rt):
    assert r.info.iter == rt.info.iter and (r.x == rt.x).all() and (r.y == rt.y).all()
    a, b = s._solver.hip_stats(), twin._solver.hip_stats()
    assert [a[k] for k in WB_STATS] == [b[k] for k in WB_STATS], ([a[k] for k in WB_STATS], [b[k] for k in WB_STATS])
    assert s._solver.get_policy() == twin._solver.get_policy()


@pytest.mark.parametrize('name', ['portfolio 600', 'lasso 300x600'])
def test_state_is_left_as_it_was(name):
    """test_gpu_adjoint_pcg.test_state_is_left_as_it_was on a Woodbury handle, against a twin with the same policy that never computes adjoints."""
    make, mode = PROBLEMS[name]
    P, q, A, l, u = make()
    n, m = len(q), len(l)
    rng = np.random.default_rng(5)
    s, twin = _setup(P, q, A, l, u), _setup(P, q, A, l, u)
    with pytest.raises(ValueError):
        s.adjoint_derivative_compute(dx=np.zeros(n))             # before a solve
    r, rt = s.solve(), twin.solve()
    _same(s, twin, r, rt)
    _mode(s, mode)
    pol = s._solver.get_policy()
    dx, dy = r.x - 0.1 * rng.standard_normal(n), rng.standard_normal(m)
    g1 = _grads(s, dx, dy)
    assert s.adjoint_last_record()['steps'] > 0
    g2 = _grads(s, dx, dy)
    for k in g1:
        assert (g1[k] == g2[k]).all(), k
    assert s._solver.get_policy() == pol
    info = s._solver.info
    assert info.iter == r.info.iter and info.status_val == SOLVED
    assert (s._solver.solution.x == r.x).all() and (s._solver.solution.y == r.y).all()
    a, b = s._solver.hip_stats(), twin._solver.hip_stats()
    assert [a[k] for k in WB_STATS] == [b[k] for k in WB_STATS]
    r, rt = s.solve(), twin.solve()                              # warm-started from the solve's own iterates
    _same(s, twin, r, rt)
    _grads(s, dx)
    q2 = q + 0.01 * rng.standard_normal(n)
    s.update(q=q2); twin.update(q=q2)
    with pytest.raises(ValueError):
        s.adjoint_derivative_compute(dx=dx)                      # after an update
    r, rt = s.solve(), twin.solve()
    _same(s, twin, r, rt)
    _grads(s, dx)
    x0, y0 = 0.5 * r.x, 0.5 * r.y
    s.warm_start(x=x0, y=y0); twin.warm_start(x=x0, y=y0)
    r, rt = s.solve(), twin.solve()
    _same(s, twin, r, rt)
    _mode(s, mode)


def test_an_inaccurate_inversion_at_the_adjoints_rho_leaves_the_direct_mode_on():
    """debug_fail_refactor = 1: the next inversion of S -- the one at the adjoint's rho vector -- reports "inaccurate", which clears the direct mode for
    good in a solve.  The call runs the recurrence with the correction as preconditioner and returns a certified result (or status 3); the handle's
    direct mode is back afterwards, and the next solves give the twin's bits (a hook still pending would fail their first rho update instead)."""
    P, q, A, l, u = problems.portfolio_qp(600, 4)
    n, m = len(q), len(l)
    rng = np.random.default_rng(11)
    s, twin = _setup(P, q, A, l, u), _setup(P, q, A, l, u)
    r, rt = s.solve(), twin.solve()
    assert r.info.status_val == SOLVED and (r.x == rt.x).all()
    assert s._solver.hip_stats()['woodbury_direct'] == 2
    dx, dy = r.x - 0.1 * rng.standard_normal(n), rng.standard_normal(m)
    s._solver.set_policy(debug_fail_refactor=1)
    st = s._solver.adjoint_derivative_compute(dx, dy)
    rec = s.adjoint_last_record()
    print('inaccurate inversion: return %d, record %s' % (st, rec))
    assert rec['steps'] > 0 and rec['status'] in (0, 3), rec
    if rec['status'] == 0:
        assert st == 0
        dq, dl, du = s.adjoint_derivative_get_vec()
        host_res, gv, rv, nact = ref.certificate(P, A, l, u, r.x, r.y, dx, dy, dq, dl, du)
        assert host_res < TOL and rec['active_rows'] == nact, (host_res, rec)
    else:
        assert st == int(osqp_amd.SolverError.OSQP_LINSYS_SOLVER_INIT_ERROR) and not rec['residual'] < TOL
    a, b = s._solver.hip_stats(), twin._solver.hip_stats()
    assert a['woodbury_direct'] == 2 and [a[k] for k in WB_STATS] == [b[k] for k in WB_STATS]
    for _ in range(2):
        q2 = q + 0.01 * rng.standard_normal(n)
        s.update(q=q2); twin.update(q=q2)
        r, rt = s.solve(), twin.solve()
        assert r.info.status_val == SOLVED and r.info.iter == rt.info.iter and (r.x == rt.x).all() and (r.y == rt.y).all()
        a, b = s._solver.hip_stats(), twin._solver.hip_stats()
        assert a['woodbury_direct'] == 2 and [a[k] for k in WB_STATS] == [b[k] for k in WB_STATS]


def _layer_inputs(nb, device):
    import torch
    P, q, A, l, u = problems.portfolio_qp(600, 4)
    Pc, Ac = sp.csc_matrix(P), sp.csc_matrix(A)
    Pc.sort_indices(); Ac.sort_indices()
    pco, aco = Pc.tocoo(), Ac.tocoo()
    rng = np.random.default_rng(13)
    if nb == 1:
        vals = [Pc.data, q, Ac.data, l, u]
    else:                                                      # q per element; l, u as rows too (the same bounds), so that every element's dl, du come back
        vals = [Pc.data, np.stack([q + 0.05 * b * rng.standard_normal(len(q)) for b in range(nb)]), Ac.data, np.stack([l] * nb), np.stack([u] * nb)]
    ts = [torch.tensor(np.array(v), dtype=torch.float64, device=device, requires_grad=True) for v in vals]
    return (P, q, A, l, u), (pco, aco, Pc.shape, Ac.shape), vals, ts


@pytest.mark.parametrize('device', ['cpu', 'cuda'])
@pytest.mark.parametrize('nb', [1, 3])
def test_torch_layer_woodbury_backward(device, nb):
    """woodbury_backward=True: the 'loop' backward differentiates every element on the Woodbury handle (nb = 3: q per element), each held to the certificate."""
    import torch
    from osqp_amd.nn.torch import OSQP as Layer
    (P, q, A, l, u), (pco, aco, Pshape, Ashape), vals, ts = _layer_inputs(nb, device)
    n, m = len(q), len(l)
    layer = Layer((pco.row, pco.col), Pshape, (aco.row, aco.col), Ashape, eps_rel=1e-8, eps_abs=1e-8, max_iter=200000, woodbury_backward=True)
    xt = 0.1 * np.random.default_rng(17).standard_normal(n)
    xt_t = torch.tensor(xt, dtype=torch.float64, device=device)
    x = layer(*ts)
    assert x.grad_fn is not None and layer._solver._solver.hip_stats()['woodbury_rows'] == 5
    assert layer._solver._solver.get_policy()['adjoint_woodbury'] == 1
    before = layer.adjoint_launches
    (0.5 * ((x - xt_t) ** 2).sum()).backward()
    assert layer.adjoint_launches == before + nb
    assert int((torch.as_tensor(layer.last_adjoint_rec)[:, 0] != 0).sum()) == 0
    grads = [t.grad.detach().cpu().numpy() for t in ts]
    for t, gr in zip(ts, grads):
        assert gr.shape == tuple(t.shape) and t.grad.device == t.device
    X = x.detach().cpu().numpy().reshape(nb, n)
    Y = np.asarray(layer.last_dual).reshape(nb, m)
    for b in range(nb):
        dq, dl, du = (grads[k].reshape(nb, -1)[b] for k in (1, 3, 4))
        assert _margin(A, l, u, X[b], Y[b]) >= 1e-9
        host_res, gv, rv, nact = ref.certificate(P, A, l, u, X[b], Y[b], X[b] - xt, None, dq, dl, du)
        assert host_res < TOL and int(layer.last_adjoint_rec[b, 1]) == nact, (b, host_res, nact)


def test_torch_layer_default_raises_on_a_woodbury_handle():
    import torch
    from osqp_amd.nn.torch import OSQP as Layer
    (P, q, A, l, u), (pco, aco, Pshape, Ashape), vals, ts = _layer_inputs(1, 'cpu')
    layer = Layer((pco.row, pco.col), Pshape, (aco.row, aco.col), Ashape, eps_rel=1e-8, eps_abs=1e-8, max_iter=200000)
    x = layer(*ts)
    assert layer._solver._solver.get_policy()['adjoint_woodbury'] == 0
    with pytest.raises(NotImplementedError, match='backward is not available on this handle'):
        (0.5 * (x ** 2).sum()).backward()


def test_without_the_switch_the_handle_answers_not_implemented():
    """The pinned default (test_gpu_adjoint_pcg.test_woodbury_handle_answers_not_implemented), and the switch on a live handle in both directions."""
    P, q, A, l, u = problems.portfolio_qp(600, 4)
    s = _setup(P, q, A, l, u, switch=None)
    assert s._solver.get_policy()['adjoint_woodbury'] == 0 and s._solver.hip_stats()['woodbury_rows'] == 5
    r = s.solve()
    assert r.info.status_val == SOLVED
    assert s._solver.adjoint_derivative_compute(r.x, None) == NI
    with pytest.raises(NotImplementedError, match='adjoint_woodbury'):
        s.adjoint_derivative_compute(dx=r.x)
    dq, dl, du = np.zeros(len(q)), np.zeros(len(l)), np.zeros(len(l))
    assert s._solver.adjoint_derivative_get_vec(dq, dl, du) == NI
    s._solver.set_policy(adjoint_woodbury=1)
    assert s._solver.adjoint_derivative_compute(r.x, None) == 0
    assert s._solver.adjoint_derivative_get_vec(dq, dl, du) == 0 and np.abs(dq).max() > 0
    s._solver.set_policy(adjoint_woodbury=0)
    assert s._solver.adjoint_derivative_compute(r.x, None) == NI
