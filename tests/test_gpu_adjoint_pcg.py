"""GPU tier: adjoint derivatives of a single large QP on the PCG path (adjoint_hip.hip, Engine::adjoint_compute_pcg) -- every handle the batch
adjoint kernel does not hold.  On the parent of this change every case here ends in NotImplementedError.

What is asserted per problem (banded_qp at n = 2000 / 20000 / 100000, one unstructured n = 20000 case, one reordered handle; eps 1e-8):
  * the solve ran on the PCG path (kernel_launches > 1) and the input condition holds: with the handle's own (x, y), every inequality row keeps
    min(|(z - l) + y|, |(u - z) - y|) >= 1e-9, so that rounding does not decide a row's class;
  * an INDEPENDENT certificate: K_a and g rebuilt on the host from the caller's data, r_x = dq, r_y = -(dl + du):  max |g - K_a r| / max |g| <
    OSQP_HIP_ADJOINT_TOL (1e-6, the project's constant); the record's residual within a factor 10 of that value, its active-row count equal to
    the helper's;
  * against the sparse yardstick tests/adjoint_sparse_ref.py at the same (x, y): |r - r_ref| / |r_ref| <= 10 (host residual) |g| / (sigma_min |r|)
    (a residual rho leaves an error of at most rho |g| / sigma_min in r; the factor 10 covers max-norm against 2-norm), recorded with
    record_deviation;
  * the gradient kernels: dP, dA recomputed on the host from the returned dq, dl, du, x, y at the caller's stored entries agree to 1e-13 of
    max |value|;
  * finite differences through the engine at n = 2000 (five coordinates each of q, l, u, five stored entries each of P and A) to 5e-3, the
    tolerance of test_gpu_adjoint._fd_check;
  * state: two consecutive calls are bit-identical; a solve afterwards equals the bits of a twin handle that never computed adjoints, also after
    an update(q) and a warm start; before a solve and after an update the reference's ValueError stays.
  * the torch layer at n = 2000 (its forward runs one element after the other on the handle): an unbatched and a batched (nb = 3) backward on cpu
    and cuda tensors, every element held to the same certificate and yardstick bound, shared inputs to the batch sum, adjoint_launches to the
    number of elements differentiated.
Handles with a Woodbury-corrected preconditioner keep answering NotImplementedError (include/osqp_hip.h) -- tested below."""
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
TOL = 1e-6          # OSQP_HIP_ADJOINT_TOL
H = 1e-5


@pytest.fixture(autouse=True)
def _pcg_path(monkeypatch):
    monkeypatch.setenv('OSQP_HIP_SMALL_DIRECT', '0')      # (as tests/test_reorder.py: the n = 2000 problem must take the PCG path)


def _setup(P, q, A, l, u, **over):
    s = osqp_amd.OSQP(algebra='hip')
    s.setup(P, q, A, l, u, **dict(ST, **over))
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


def _check(name, P, q, A, l, u, with_dy, seed=7):
    n, m = len(q), len(l)
    rng = np.random.default_rng(seed)
    s = _setup(P, q, A, l, u)
    r = s.solve()
    st = s._solver.hip_stats()
    assert r.info.status_val == SOLVED and st['kernel_launches'] > 1, (r.info.status_val, st['kernel_launches'])
    x, y = r.x.copy(), r.y.copy()
    margin = _margin(A, l, u, x, y)
    assert margin >= 1e-9, margin
    dx = x - 0.1 * rng.standard_normal(n)
    dy = rng.standard_normal(m) if with_dy else None
    g = _grads(s, dx, dy)
    rec = s.adjoint_last_record()
    # independent certificate
    host_res, gv, rv, nact = ref.certificate(P, A, l, u, x, y, dx, dy, g['dq'], g['dl'], g['du'])
    print('%s dy=%s: host residual %.3e, record %s, margin %.2e' % (name, with_dy, host_res, rec, margin))
    assert host_res < TOL, host_res
    assert rec['status'] == 0 and rec['active_rows'] == nact, (rec, nact)
    assert rec['residual'] < TOL and rec['residual'] <= 10 * host_res and host_res <= 10 * rec['residual'], (rec['residual'], host_res)
    # the sparse yardstick at the same (x, y)
    y0 = ref.adjoint(P, A, l, u, x, y, dx, dy)
    r_ref = np.concatenate([y0['r_x'], y0['r_y'][y0['act']]])
    dev = float(np.linalg.norm(rv - r_ref) / np.linalg.norm(r_ref))
    bound = 10 * host_res * np.linalg.norm(gv) / (y0['sigma_min'] * np.linalg.norm(r_ref))
    record_deviation('test_gpu_adjoint_pcg', '%s dy=%s' % (name, with_dy), r_rel_dev=dev, bound=float(bound), host_residual=host_res, record_residual=rec['residual'],
                     active_rows=nact, steps=rec['steps'], sigma_min=y0['sigma_min'], margin=margin, recurrence_s=rec['recurrence_s'], gradient_s=rec['gradient_s'])
    print('   |r - r_ref| / |r_ref| = %.3e (bound %.3e), sigma_min %.3e, steps %d' % (dev, bound, y0['sigma_min'], rec['steps']))
    assert dev <= bound, (dev, bound)
    # gradient kernels: the formulas at the caller's stored entries, from the returned vectors
    dP, dA = ref.gradients(P, A, x, y, g['dq'], -(g['dl'] + g['du']))
    for got, want in ((g['dP'], dP), (g['dA'], dA)):
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), np.abs(got - want).max() / np.abs(want).max()
    return s, r, dx, dy, g


@pytest.mark.parametrize('with_dy', [False, True])
@pytest.mark.parametrize('n,window', [(2000, 40), (20000, 40), (100000, 200)])
def test_banded(n, window, with_dy):
    P, q, A, l, u = problems.banded_qp(n, window=window)
    _check('banded n=%d' % n, P, q, A, l, u, with_dy)


def test_unstructured():
    P, q, A, l, u = problems.banded_qp(20000, window=40, long_range=0.05)
    _check('long_range n=20000', P, q, A, l, u, True)


def test_reordered_handle(monkeypatch):
    monkeypatch.setenv('OSQP_HIP_REORDER', '2')
    P, q, A, l, u = problems.banded_qp(2000, window=40)
    s, r, dx, dy, g = _check('reordered n=2000', P, q, A, l, u, True)
    assert s._solver.hip_stats()['reordered'] == 1
    monkeypatch.setenv('OSQP_HIP_REORDER', '0')
    s0 = _setup(P, q, A, l, u)
    r0 = s0.solve()
    assert s0._solver.hip_stats()['reordered'] == 0 and r0.info.status_val == SOLVED
    g0 = _grads(s0, dx, dy)
    # Both handles solve K_a r = g, each to its own certified residual: r differs by at most (res + res0) |g| / sigma_min (the yardstick's bound
    # for each against the exact solution, added), here with the same factor 10 for max-norm against 2-norm.
    res1 = ref.certificate(P, A, l, u, r.x, r.y, dx, dy, g['dq'], g['dl'], g['du'])
    res0 = ref.certificate(P, A, l, u, r0.x, r0.y, dx, dy, g0['dq'], g0['dl'], g0['du'])
    smin = ref.adjoint(P, A, l, u, r.x, r.y, dx, dy)['sigma_min']
    dev = float(np.linalg.norm(res1[2] - res0[2]) / np.linalg.norm(res0[2]))
    # (the two handles' own (x, y) differ by the solves' accuracy, eps = 1e-8 relative: that enters g = -[x - x_target; dy] and the products alike)
    bound = 10 * ((res1[0] + res0[0]) * np.linalg.norm(res0[1]) / (smin * np.linalg.norm(res0[2])) + 1e-8 / smin)
    record_deviation('test_gpu_adjoint_pcg', 'reordered against as numbered', r_rel_dev=dev, bound=float(bound))
    print('reordered against as numbered: %.3e (bound %.3e)' % (dev, bound))
    assert res1[3] == res0[3] and dev <= bound, (dev, bound)


def test_finite_differences_through_the_engine():
    n = 2000
    P, q, A, l, u = problems.banded_qp(n, window=40)
    Pt = sp.triu(P, format='csc')
    rng = np.random.default_rng(3)
    xt = 0.1 * rng.standard_normal(n)
    # (eps 1e-10 here, tighter than the module's 1e-8: a forward difference over H = 1e-5 needs solves whose error is far below H)
    s = _setup(P, q, A, l, u, eps_abs=1e-10, eps_rel=1e-10)
    r = s.solve()
    assert r.info.status_val == SOLVED and s._solver.hip_stats()['kernel_launches'] > 1
    assert _margin(A, l, u, r.x, r.y) >= 1e-9
    g = _grads(s, r.x - xt)
    f0 = 0.5 * np.sum((r.x - xt) ** 2)
    low, upp = ref.active_set(A, l, u, r.x, r.y)
    base = dict(q=q, l=l, u=u, Px=Pt.data, Ax=A.data)

    def loss(**kw):
        s.update(**kw)
        rr = s.solve()
        assert rr.info.status_val == SOLVED
        return 0.5 * np.sum((rr.x - xt) ** 2)
    (pr, pc), _ = ref.stored_entries(P, A)
    ineq = l != u
    picks = dict(dq=rng.choice(n, 5, replace=False), dl=rng.choice(np.nonzero(low & ineq)[0], 5, replace=False), du=rng.choice(np.nonzero(upp & ineq)[0], 5, replace=False),
                 dP=rng.choice(len(Pt.data), 5, replace=False), dA=rng.choice(len(A.data), 5, replace=False))
    for which, key in (('dq', 'q'), ('dl', 'l'), ('du', 'u'), ('dP', 'Px'), ('dA', 'Ax')):
        for k in picks[which]:
            v = base[key].copy(); v[k] += H
            fd = (loss(**{key: v}) - f0) / H
            got = g[which][k] * (2.0 if which == 'dP' and pr[k] != pc[k] else 1.0)      # a stored off-diagonal entry stands for both triangles
            print(which, int(k), 'fd %.6e adjoint %.6e' % (fd, got))
            np.testing.assert_allclose(got, fd, rtol=5e-3, atol=5e-3)
        s.update(**{key: base[key]})


def test_state_is_left_as_it_was():
    P, q, A, l, u = problems.banded_qp(2000, window=40)
    rng = np.random.default_rng(5)
    s, twin = _setup(P, q, A, l, u), _setup(P, q, A, l, u)
    with pytest.raises(ValueError):
        s.adjoint_derivative_compute(dx=np.zeros(2000))          # before a solve
    r, rt = s.solve(), twin.solve()
    assert r.info.iter == rt.info.iter and (r.x == rt.x).all() and (r.y == rt.y).all()
    dx, dy = r.x - 0.1 * rng.standard_normal(2000), rng.standard_normal(4000)
    g1 = _grads(s, dx, dy)
    g2 = _grads(s, dx, dy)
    for k in g1:
        assert (g1[k] == g2[k]).all(), k
    info = s._solver.info
    assert info.iter == r.info.iter and info.status_val == SOLVED
    assert (s._solver.solution.x == r.x).all() and (s._solver.solution.y == r.y).all()
    r, rt = s.solve(), twin.solve()                              # warm-started from the solve's own iterates
    assert r.info.iter == rt.info.iter and (r.x == rt.x).all() and (r.y == rt.y).all()
    _grads(s, dx)
    q2 = q + 0.01 * rng.standard_normal(2000)
    s.update(q=q2); twin.update(q=q2)
    with pytest.raises(ValueError):
        s.adjoint_derivative_compute(dx=dx)                      # after an update
    r, rt = s.solve(), twin.solve()
    assert r.info.iter == rt.info.iter and (r.x == rt.x).all() and (r.y == rt.y).all()
    _grads(s, dx)
    x0, y0 = 0.5 * r.x, 0.5 * r.y
    s.warm_start(x=x0, y=y0); twin.warm_start(x=x0, y=y0)
    r, rt = s.solve(), twin.solve()
    assert r.info.iter == rt.info.iter and (r.x == rt.x).all() and (r.y == rt.y).all()


def test_woodbury_handle_answers_not_implemented():
    """The portfolio QP's dense rows switch the Woodbury-corrected preconditioner on (its forward runs the one-launch direct form): such a
    handle is outside both adjoint routes (include/osqp_hip.h)."""
    P, q, A, l, u = problems.portfolio_qp(2000, 20)
    s = _setup(P, q, A, l, u, eps_abs=1e-6, eps_rel=1e-6)
    assert s._solver.hip_stats()['woodbury_rows'] > 0
    r = s.solve()
    assert r.info.status_val == SOLVED
    assert s._solver.adjoint_derivative_compute(r.x, None) == int(osqp_amd.SolverError.OSQP_FUNC_NOT_IMPLEMENTED)
    with pytest.raises(NotImplementedError):
        s.adjoint_derivative_compute(dx=r.x)


@pytest.mark.parametrize('device', ['cpu', 'cuda'])
@pytest.mark.parametrize('nb', [1, 3])
def test_torch_layer_backward_outside_the_batch_kernel(device, nb):
    """nb = 1: every input 1-D.  nb = 3: q, l, u per element, P_val and A_val shared -- they receive the sum over the batch."""
    import torch
    from osqp_amd.nn.torch import OSQP as Layer
    n = 2000
    P, q, A, l, u = problems.banded_qp(n, window=40)
    m = len(l)
    Pc, Ac = sp.csc_matrix(P), sp.csc_matrix(A)
    Pc.sort_indices(); Ac.sort_indices()
    pco, aco = Pc.tocoo(), Ac.tocoo()
    layer = Layer((pco.row, pco.col), Pc.shape, (aco.row, aco.col), Ac.shape, eps_rel=1e-8, eps_abs=1e-8, max_iter=200000)
    rng = np.random.default_rng(13)
    xt = 0.1 * rng.standard_normal(n)
    if nb == 1:
        vals = [Pc.data, q, Ac.data, l, u]
    else:
        vals = [Pc.data, np.stack([q + 0.05 * b * rng.standard_normal(n) for b in range(nb)]), Ac.data,
                np.stack([l - 0.01 * b for b in range(nb)]), np.stack([u + 0.01 * b for b in range(nb)])]
    ts = [torch.tensor(np.array(v), dtype=torch.float64, device=device, requires_grad=True) for v in vals]
    xt_t = torch.tensor(xt, dtype=torch.float64, device=device)
    x = layer(*ts)
    assert x.grad_fn is not None
    before = layer.adjoint_launches
    (0.5 * ((x - xt_t) ** 2).sum()).backward()
    assert layer.adjoint_launches == before + nb                          # one single-handle adjoint per element
    assert int((torch.as_tensor(layer.last_adjoint_rec)[:, 0] != 0).sum()) == 0
    grads = [t.grad.detach().cpu().numpy() for t in ts]
    for t, gr in zip(ts, grads):
        assert gr.shape == tuple(t.shape) and t.grad.device == t.device
    X = x.detach().cpu().numpy().reshape(nb, n)
    Y = np.asarray(layer.last_dual).reshape(nb, m)
    dP_sum, dA_sum = np.zeros(Pc.nnz), np.zeros(Ac.nnz)
    for b in range(nb):
        qb, lb, ub = (vals[k][b] if nb > 1 else vals[k] for k in (1, 3, 4))
        dq, dl, du = (grads[k].reshape(nb, -1)[b] for k in (1, 3, 4))
        assert _margin(A, lb, ub, X[b], Y[b]) >= 1e-9
        dx = X[b] - xt
        host_res, gv, rv, nact = ref.certificate(P, A, lb, ub, X[b], Y[b], dx, None, dq, dl, du)
        assert host_res < TOL and int(layer.last_adjoint_rec[b, 1]) == nact, (host_res, nact)
        y0 = ref.adjoint(P, A, lb, ub, X[b], Y[b], dx)
        r_ref = np.concatenate([y0['r_x'], y0['r_y'][y0['act']]])
        dev = float(np.linalg.norm(rv - r_ref) / np.linalg.norm(r_ref))
        bound = 10 * host_res * np.linalg.norm(gv) / (y0['sigma_min'] * np.linalg.norm(r_ref))
        record_deviation('test_gpu_adjoint_pcg', 'torch %s nb=%d element %d' % (device, nb, b), r_rel_dev=dev, bound=float(bound), host_residual=host_res)
        assert dev <= bound, (dev, bound)
        ry = -(dl + du)
        dP_sum += 0.5 * (dq[pco.row] * X[b][pco.col] + dq[pco.col] * X[b][pco.row])      # every entry of the full pattern, either triangle the same value
        dA_sum += Y[b][aco.row] * dq[aco.col] + ry[aco.row] * X[b][aco.col]
    for got, want in ((grads[0], dP_sum), (grads[2], dA_sum)):             # shared inputs: the sum over the batch
        assert np.abs(got - want).max() <= 1e-13 * nb * np.abs(want).max()


def _forced_reorder_small(monkeypatch, P, q, A, l, u):
    """A small dense problem on the PCG route: a reordered handle is outside the batch kernel whatever its size.  The solve itself may run the
    small-problem direct kernel (the module's OSQP_HIP_SMALL_DIRECT=0 is lifted here)."""
    monkeypatch.delenv('OSQP_HIP_SMALL_DIRECT', raising=False)
    monkeypatch.setenv('OSQP_HIP_REORDER', '2')
    s = _setup(sp.csc_matrix(P), q, sp.csc_matrix(A), l, u, eps_abs=1e-9, eps_rel=1e-9)
    assert s._solver.hip_stats()['reordered'] == 1
    r = s.solve()
    assert r.info.status_val == SOLVED
    return s, r


def test_small_reordered_handle_takes_the_pcg_route(monkeypatch):
    from test_adjoint_reference_cpu import reference_problem
    import adjoint_ref
    P, q, A, l, u, xt = reference_problem(30, 30, 1)
    s, r = _forced_reorder_small(monkeypatch, P, q, A, l, u)
    dx = r.x - xt
    g = _grads(s, dx)
    rec = s.adjoint_last_record()
    host_res, gv, rv, nact = ref.certificate(sp.csc_matrix(P), sp.csc_matrix(A), l, u, r.x, r.y, dx, None, g['dq'], g['dl'], g['du'])
    assert rec['status'] == 0 and rec['steps'] > 0 and rec['active_rows'] == nact and host_res < TOL, (rec, host_res)
    d = adjoint_ref.adjoint(P, A, l, u, r.x, r.y, dx)
    sv = np.linalg.svd(d['K'], compute_uv=False).min()
    r_ref = np.concatenate([d['r_x'], d['r_y'][d['act']]])
    dev = np.linalg.norm(rv - r_ref) / np.linalg.norm(r_ref)
    assert dev <= 10 * host_res * np.linalg.norm(gv) / (sv * np.linalg.norm(r_ref)), dev


def test_singular_adjoint_systems_are_reported(monkeypatch):
    """Status 2: more active rows than variables (60 consistent equality rows, 50 variables).  Status 3: dependent active rows with an inconsistent
    right-hand side (an equality row stored twice, dy different on the two copies): the recurrence stalls above the threshold.  Both return
    OSQP_LINSYS_SOLVER_INIT_ERROR, raise with the record's residual in the message and leave no result."""
    rng = np.random.default_rng(21)
    n = 50
    L = rng.standard_normal((n, n))
    P = L @ L.T / n + 0.1 * np.eye(n)
    q = rng.standard_normal(n)
    x0 = rng.standard_normal(n)
    E = int(osqp_amd.SolverError.OSQP_LINSYS_SOLVER_INIT_ERROR)
    A2 = rng.standard_normal((60, n)); b2 = A2 @ x0
    A3 = rng.standard_normal((10, n)); A3 = np.vstack([A3, A3[:1]]); b3 = A3 @ x0
    dy3 = np.zeros(11); dy3[0], dy3[10] = 1.0, -1.0
    for A, b, dy, status in ((A2, b2, None, 2), (A3, b3, dy3, 3)):
        s, r = _forced_reorder_small(monkeypatch, P, q, A, b, b)
        assert s._solver.adjoint_derivative_compute(r.x, dy) == E
        rec = s.adjoint_last_record()
        assert rec['status'] == status and rec['active_rows'] == A.shape[0] and not rec['residual'] < TOL, rec
        with pytest.raises(ArithmeticError, match='residual'):
            s.adjoint_derivative_compute(dx=r.x, dy=dy)
        dq, dl, du = np.zeros(n), np.zeros(A.shape[0]), np.zeros(A.shape[0])
        assert s._solver.adjoint_derivative_get_vec(dq, dl, du) == int(osqp_amd.SolverError.OSQP_DATA_NOT_INITIALIZED)
        r2 = s.solve()                                            # the handle is left usable
        assert r2.info.status_val == SOLVED


def test_compute_at_a_kept_solution_equals_compute():
    """osqp_hip_adjoint_compute_at with the handle's own (x, y) gives the bits of osqp_adjoint_derivative_compute; also after an update of q (which
    the derivative does not depend on) has reset the status; x without y is a validation error."""
    P, q, A, l, u = problems.banded_qp(2000, window=40)
    rng = np.random.default_rng(9)
    s = _setup(P, q, A, l, u)
    r = s.solve()
    assert r.info.status_val == SOLVED
    x, y = r.x.copy(), r.y.copy()
    dx, dy = x - 0.1 * rng.standard_normal(2000), rng.standard_normal(4000)
    g = _grads(s, dx, dy)
    ext = s._solver

    def at():
        assert ext.adjoint_derivative_compute_at(x, y, dx, dy) == 0
        dP, dA = s.ext.CSC(s._derivative_cache['P'].copy()), s.ext.CSC(s._derivative_cache['A'].copy())
        dq, dl, du = np.empty(2000), np.zeros(4000), np.zeros(4000)
        assert ext.adjoint_derivative_get_mat(dP, dA) == 0 and ext.adjoint_derivative_get_vec(dq, dl, du) == 0
        return dict(dP=dP.x.copy(), dA=dA.x.copy(), dq=dq, dl=dl, du=du)
    g1 = at()
    s.update(q=q + 1.0)
    g2 = at()
    for k in g:
        assert (g[k] == g1[k]).all() and (g[k] == g2[k]).all(), k
    assert ext.adjoint_derivative_compute_at(x, None, dx, dy) == int(osqp_amd.SolverError.OSQP_DATA_VALIDATION_ERROR)
