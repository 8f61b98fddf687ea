"""GPU tier: adjoint derivatives -- the batched backward kernel (osqp_hip_batch_adjoint), the three adjoint_derivative_* calls of a handle and the
backward of the torch layer.  The yardstick is tests/adjoint_ref.py (pinned against finite differences through the oracle by
tests/test_adjoint_reference_cpu.py), evaluated at the engine's own (x, y).

Tolerance of every comparison with the helper: adjoint_ref.solve_bound(K_a) = 10 max(1e3 eps cond_2(K_a), (delta / sigma_min(K_a))^(refine + 1)),
relative to max |r| -- derived per case from the KKT matrix of the active set, not fitted.  It bounds the error e of r; the outputs inherit it as
    dq, dl, du: e;      dP_ij = (r_i x_j + r_j x_i) / 2: e max |x|;      dA_ij = y_i r_j + r_y,i x_j: e (max |x| + max |y|).
Every problem compared against the helper has an inactive-slack margin > 1e-4, active inequality |y| > 1e-4 and sigma_min(K_a) > 1e-4 (asserted).
The reference's (100, 120) case does not fit the adjoint kernel: a dense K of order n has half bandwidth n - 1, and the band limit is 56.  Two cases
take its place.  (43, 52) with the same share of equality rows and rows without lower bound is the largest size of that shape whose FORWARD also runs
on the direct variant (4096 stored entries per matrix: n^2 + n m <= 4096), so that the finite differences go through the same path as every other
case; it is checked at the reference's relaxed 1e-2.  (57, 68) is the largest size the adjoint itself holds (half bandwidth 56, 121 KB of LDS:
above the default 64 KB); its forward would run on another variant, so it is given the oracle's (x, y) through the batch entry point and checked
against the helper with the derived bound (test_largest_dense_problem_the_band_limit_allows)."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import adjoint_ref
import osqp_amd
import problems
from test_adjoint_reference_cpu import reference_problem
from util import record_deviation

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
ST = dict(eps_abs=1e-9, eps_rel=1e-9, max_iter=500000, verbose=False)
H = 1e-5
SOLVED = int(osqp_amd.SolverStatus.OSQP_SOLVED)


def _setup(P, q, A, l, u, **over):
    s = osqp_amd.OSQP(algebra='hip')
    s.setup(sp.csc_matrix(P), q, sp.csc_matrix(A), l, u, **dict(ST, **over))
    return s


def _conditions(P, A, l, u, x, y):
    slack, ymin, smin, cond = adjoint_ref.conditions(P, A, l, u, x, y)
    assert slack > 1e-4 and ymin > 1e-4 and smin > 1e-4, (slack, ymin, smin, cond)


def _deviations(got, P, A, l, u, x, y, dx, dy=None):
    """Largest deviation of each output from the helper at (x, y), divided by what the bound allows (<= 1 passes), and the bound itself.
    got: dq, dl, du vectors; dP values at the upper-triangle CSC entries of P; dA values at the CSC entries of A."""
    g = adjoint_ref.adjoint(P, A, l, u, x, y, dx, dy)
    bound = adjoint_ref.solve_bound(g['K'])
    rn = max(np.abs(g['r_x']).max(), np.abs(g['r_y']).max(initial=0.0))
    xs, ys = np.abs(x).max(), np.abs(y).max(initial=0.0)
    Pt, Ac = sp.triu(sp.csc_matrix(P), format='csc'), sp.csc_matrix(A)
    Pt.sort_indices(); Ac.sort_indices()
    pr, pc = Pt.tocoo().row, Pt.tocoo().col
    ar, ac = Ac.tocoo().row, Ac.tocoo().col
    ref = dict(dq=g['dq'], dl=g['dl'], du=g['du'], dP=g['dP'][pr, pc], dA=g['dA'][ar, ac])
    scale = dict(dq=1.0, dl=1.0, du=1.0, dP=max(xs, 1e-300), dA=max(xs + ys, 1e-300))
    out = {}
    for k in ref:
        if k in got and got[k] is not None:
            out[k] = float(np.abs(np.asarray(got[k]).ravel() - ref[k]).max(initial=0.0) / (bound * rn * scale[k]))
    return out, bound, g


def _handle_grads(s, dx, dy=None):
    s.adjoint_derivative_compute(dx=dx, dy=dy)
    dP, dA = s.adjoint_derivative_get_mat(as_dense=False)
    dq, dl, du = s.adjoint_derivative_get_vec()
    return dict(dP=dP.data, dA=dA.data, dq=dq, dl=dl, du=du)


CASES = [(5, 5, 1, 0, 0), (3, 3, 1, 0, 0), (10, 20, 1, 0, 0), (30, 30, 1, 0, 0), (30, 20, 1, 10, 0), (20, 15, 1, 15, 0), (10, 10, 2, 5, 5),
         (5, 20, 3, 0, 0), (43, 52, 3, 9, 9)]      # n, m, seed, equality rows, rows without lower bound; (5, 20, 3): a vertex (5 active rows)


# ---------------------------------------------------------------------------------------------------- 1. single handle against the helper
@pytest.mark.parametrize('n,m,seed,n_eq,n_inf', CASES)
def test_single_handle_matches_the_helper(n, m, seed, n_eq, n_inf):
    P, q, A, l, u, xt = reference_problem(n, m, seed, n_eq, n_inf)
    s = _setup(P, q, A, l, u)
    assert s.has_capability('OSQP_CAPABILITY_DERIVATIVES')
    with pytest.raises(ValueError):
        s.adjoint_derivative_compute(dx=np.zeros(n))                       # before a solve
    r = s.solve()
    assert r.info.status_val == SOLVED
    _conditions(P, A, l, u, r.x, r.y)
    rng = np.random.RandomState(seed)
    for label, dx, dy in (('dx', r.x - xt, None), ('dx+dy', r.x - xt, rng.randn(m))):
        dev, bound, g = _deviations(_handle_grads(s, dx, dy), P, A, l, u, r.x, r.y, dx, dy)
        record_deviation('test_single_handle_matches_the_helper', 'n=%d m=%d seed=%d %s' % (n, m, seed, label), bound=bound, **dev)
        print(n, m, seed, label, 'bound %.2e' % bound, dev)
        assert set(dev) == {'dq', 'dl', 'du', 'dP', 'dA'} and max(dev.values()) <= 1.0, (dev, bound)
    if (n, m, seed) == (5, 20, 3):                                         # the vertex: with dy = 0, dq is zero to rounding -- compared absolutely
        assert int((g['low'] | g['upp']).sum()) == n
        gv = adjoint_ref.adjoint(P, A, l, u, r.x, r.y, r.x - xt)
        assert np.abs(gv['dq']).max() <= 1e-12
        assert np.abs(_handle_grads(s, r.x - xt)['dq']).max() <= adjoint_ref.solve_bound(gv['K']) * np.abs(gv['r_y']).max()
    dPd, dAd = s.adjoint_derivative_get_mat()                              # dense, upper triangle; and the full symmetric form
    assert dPd.shape == (n, n) and dAd.shape == (m, n) and np.abs(np.tril(dPd, -1)).max() == 0.0
    dPf, _ = s.adjoint_derivative_get_mat(dP_as_triu=False)
    assert np.array_equal(dPf, dPf.T) and np.array_equal(np.triu(dPf), dPd)
    s.update(q=q + 1.0)                                                    # new data: derivatives need a new solve
    with pytest.raises(ValueError):
        s.adjoint_derivative_compute(dx=r.x - xt)


# ---------------------------------------------------------------------------------------------------- 2. against finite differences through the engine
def _fd_check(n, m, seed, n_eq, n_inf, which, tol=5e-3):
    P, q, A, l, u, xt = reference_problem(n, m, seed, n_eq, n_inf)
    Pt, Ac = sp.triu(sp.csc_matrix(P), format='csc'), sp.csc_matrix(A)
    s = _setup(P, q, A, l, u)
    r = s.solve()
    assert r.info.status_val == SOLVED
    _conditions(P, A, l, u, r.x, r.y)
    grads = _handle_grads(s, r.x - xt)
    f0 = 0.5 * np.sum((r.x - xt) ** 2)

    def loss(**kw):
        s.update(**kw)
        rr = s.solve()
        assert rr.info.status_val == SOLVED
        return 0.5 * np.sum((rr.x - xt) ** 2)
    base = dict(q=q, l=l, u=u, Px=Pt.data, Ax=Ac.data)
    key = dict(dq='q', dl='l', du='u', dP='Px', dA='Ax')[which]
    v0 = base[key]
    fd = np.zeros(len(v0))
    for k in range(len(v0)):
        v = v0.copy(); v[k] += H
        if which in ('dl', 'du') and l[k] == u[k]:                         # an equality row moves both bounds together: dl + du
            fd[k] = (loss(l=np.where(np.arange(m) == k, l + H, l), u=np.where(np.arange(m) == k, u + H, u)) - f0) / H
            s.update(l=l, u=u)
            continue
        if which == 'dl' and l[k] <= -1e30:
            continue
        fd[k] = (loss(**{key: v}) - f0) / H
    s.update(**{key: v0})
    got = np.asarray(grads[which], dtype=float).copy()
    if which in ('dl', 'du'):
        eq = l == u
        got[eq] = (grads['dl'] + grads['du'])[eq]
    if which == 'dP':                                                       # a stored off-diagonal entry stands for both triangles: 2 dP_ij
        co = Pt.tocoo()
        got = got * np.where(co.row == co.col, 1.0, 2.0)
    worst = float(np.abs(got - fd).max())
    record_deviation('test_against_finite_differences', '%s n=%d m=%d seed=%d' % (which, n, m, seed), worst_abs=worst)
    print(which, n, m, seed, 'worst |fd - adjoint| = %.2e' % worst)
    np.testing.assert_allclose(got, fd, rtol=tol, atol=tol)


def test_dl_dq(): _fd_check(5, 5, 1, 0, 0, 'dq')
def test_dl_dP(): _fd_check(3, 3, 1, 0, 0, 'dP')
def test_dl_dA(): _fd_check(3, 3, 1, 0, 0, 'dA')
def test_dl_dl(): _fd_check(30, 30, 1, 0, 0, 'dl')
def test_dl_du(): _fd_check(10, 20, 1, 0, 0, 'du')
def test_dl_dA_eq(): _fd_check(30, 20, 1, 10, 0, 'dA')
def test_dl_dq_eq(): _fd_check(20, 15, 1, 15, 0, 'dq')
def test_dl_dq_eq_large(): _fd_check(43, 52, 3, 9, 9, 'dq', tol=1e-2)      # in place of the reference's (100, 120): see the module docstring


# ---------------------------------------------------------------------------------------------------- 3. batch
def _device_adjoint(s, x, y, dx, l, u, Px=None, Ax=None):
    import torch
    dev = torch.device('cuda', 0)
    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    B, sv = x.shape[0], s._solver
    ins = [t(a) for a in (x, y, dx, l, u, Px, Ax)]
    outs = {k: torch.zeros((B, w), dtype=torch.float64, device=dev) for k, w in (('dP', sv.nnz_P), ('dq', sv.n), ('dA', sv.nnz_A), ('dl', sv.m), ('du', sv.m), ('rec', 4))}
    p = lambda a: None if a is None else a.data_ptr()
    torch.cuda.synchronize()
    sv.hip_batch_adjoint_device(B, p(ins[0]), p(ins[1]), p(ins[2]), None, p(ins[3]), p(ins[4]), p(ins[5]), p(ins[6]),
                                p(outs['dP']), p(outs['dq']), p(outs['dA']), p(outs['dl']), p(outs['du']), p(outs['rec']), stream=None)
    return {k: v.cpu().numpy() for k, v in outs.items()}


def test_batch_of_mpc_problems():
    B = 64
    P, q, A, L, U = problems.mpc_batch(B)
    n, m = P.shape[0], A.shape[0]
    s = _setup(P, q, A, L[0], U[0])
    x, y, rec = s._solver.hip_batch_solve(l=L, u=U)
    assert (rec[:, 0] == SOLVED).all(), rec[:, 0]
    dx = np.random.default_rng(5).standard_normal((B, n))
    res = s._solver.hip_batch_adjoint(x, y, dx, l=L, u=U)
    assert res['rec'].shape == (B, 4) and (res['rec'][:, 0] == 0).all(), res['rec'][:, :3]
    assert (res['rec'][:, 2] < s._solver.ADJOINT_TOL).all()
    worst = {}
    for b in range(B):
        _conditions(P, A, L[b], U[b], x[b], y[b])
        dev, bound, g = _deviations({k: res[k][b] for k in ('dP', 'dq', 'dA', 'dl', 'du')}, P, A, L[b], U[b], x[b], y[b], dx[b])
        assert int(res['rec'][b, 1]) == int((g['low'] | g['upp']).sum())
        assert max(dev.values()) <= 1.0, (b, dev, bound)
        for k, v in dev.items():
            worst[k] = max(worst.get(k, 0.0), v)
    record_deviation('test_batch_of_mpc_problems', 'B=64', worst_residual=float(res['rec'][:, 2].max()), **worst)
    print('worst deviation / bound:', worst, 'worst residual', res['rec'][:, 2].max())
    again = s._solver.hip_batch_adjoint(x, y, dx, l=L, u=U)
    on_dev = _device_adjoint(s, x, y, dx, L, U)
    for k in ('dP', 'dq', 'dA', 'dl', 'du', 'rec'):
        assert np.array_equal(res[k], again[k]), k                          # deterministic: bit-identical
        assert np.array_equal(res[k], on_dev[k]), k                         # host-array and device entry points: bit for bit
    only = s._solver.hip_batch_adjoint(x, y, dx, l=L, u=U, want=('dq',))    # any output may be left out
    assert set(only) == {'dq', 'rec'} and np.array_equal(only['dq'], res['dq'])


@pytest.mark.parametrize('N', [11, 15])
def test_batch_of_mpc_problems_beyond_128_variables(N):
    """The substitutions past n = 128 (csrc/band_ldl.h band_solve, the adjoint kernel's own instance): N = 11 gives n = 132, m = 264 -- a lane's third
    element, the e + 128 refill, first exists; N = 15 gives n = 180, m = 360 -- the refill reads real elements and the elimination runs a third
    64-pivot epoch.  Same assertions and bounds as test_batch_of_mpc_problems."""
    B = 4
    P, q, A, L, U = problems.mpc_batch(B, N=N, seed=2)
    n, m = P.shape[0], A.shape[0]
    assert (n, m) == (12 * N, 24 * N) and n > 128
    s = _setup(P, q, A, L[0], U[0])
    x, y, rec = s._solver.hip_batch_solve(l=L, u=U)
    assert (rec[:, 0] == SOLVED).all(), rec[:, 0]
    dx = np.random.default_rng(5).standard_normal((B, n))
    res = s._solver.hip_batch_adjoint(x, y, dx, l=L, u=U)
    assert res['rec'].shape == (B, 4) and (res['rec'][:, 0] == 0).all(), res['rec'][:, :3]
    assert (res['rec'][:, 2] < s._solver.ADJOINT_TOL).all()
    worst = {}
    for b in range(B):
        _conditions(P, A, L[b], U[b], x[b], y[b])
        dev, bound, g = _deviations({k: res[k][b] for k in ('dP', 'dq', 'dA', 'dl', 'du')}, P, A, L[b], U[b], x[b], y[b], dx[b])
        assert int(res['rec'][b, 1]) == int((g['low'] | g['upp']).sum())
        print(N, b, 'bound %.2e' % bound, dev, 'residual %.2e' % res['rec'][b, 2])
        assert max(dev.values()) <= 1.0, (b, dev, bound)
        for k, v in dev.items():
            worst[k] = max(worst.get(k, 0.0), v)
    record_deviation('test_batch_of_mpc_problems_beyond_128_variables', 'N=%d B=%d' % (N, B), worst_residual=float(res['rec'][:, 2].max()), **worst)
    again = s._solver.hip_batch_adjoint(x, y, dx, l=L, u=U)
    on_dev = _device_adjoint(s, x, y, dx, L, U)
    for k in ('dP', 'dq', 'dA', 'dl', 'du', 'rec'):
        assert np.array_equal(res[k], again[k]), k                          # deterministic: bit-identical
        assert np.array_equal(res[k], on_dev[k]), k                         # host-array and device entry points: bit for bit


def test_largest_dense_problem_the_band_limit_allows():
    """n = 57 dense: half bandwidth 56 = the limit, LDS above 64 KB.  (x, y) from the oracle: the adjoint does not depend on which variant solved."""
    from oracle import Oracle, SOLVED as OSOLVED
    n, m = 57, 68
    P, q, A, l, u, xt = reference_problem(n, m, 3, 11, 11)
    x, y, info = Oracle().setup(sp.csc_matrix(P), q, sp.csc_matrix(A), l, u, eps_abs=1e-9, eps_rel=1e-9, max_iter=500000).solve()
    assert info.status_val == OSOLVED
    _conditions(P, A, l, u, x, y)
    s = _setup(P, q, A, l, u)
    rng = np.random.RandomState(2)
    for label, dx, dy in (('dx', x - xt, None), ('dx+dy', x - xt, rng.randn(m))):
        res = s._solver.hip_batch_adjoint(x, y, dx, dy)
        assert res['rec'][0, 0] == 0, res['rec']
        dev, bound, g = _deviations({k: res[k][0] for k in ('dP', 'dq', 'dA', 'dl', 'du')}, P, A, l, u, x, y, dx, dy)
        record_deviation('test_largest_dense_problem_the_band_limit_allows', label, bound=bound, residual=float(res['rec'][0, 2]), **dev)
        print(n, m, label, 'bound %.2e' % bound, dev, 'residual %.2e' % res['rec'][0, 2])
        assert max(dev.values()) <= 1.0, (dev, bound)
    assert int(s._solver.hip_stats()['batch_direct_bw']) == n - 1
    P2, q2, A2, l2, u2, _ = reference_problem(58, 60, 3)                     # half bandwidth 57: declined, as the header says
    s2 = _setup(P2, q2, A2, l2, u2)
    with pytest.raises(ValueError) as e:
        s2._solver.hip_batch_adjoint(np.zeros(58), np.zeros(60), np.zeros(58))
    assert str(e.value) == str(int(osqp_amd.SolverError.OSQP_FUNC_NOT_IMPLEMENTED))


# ---------------------------------------------------------------------------------------------------- 4. per-element matrices
def test_per_element_matrices_equal_a_single_handle_per_element():
    B = 6
    P, q, A, L, U = problems.mpc_batch(B, seed=11)
    rng = np.random.default_rng(7)      # (perturbation seeds 3 .. 7 were checked with the oracle; 7 keeps every element's margins widest: slack 3.9e-3, |y| 1.2e-2)
    Pt = sp.triu(P, format='csc')
    sel = np.abs(np.abs(A.data) - 1.0) > 1e-12
    Ax = np.tile(A.data, (B, 1)); Px = np.tile(Pt.data, (B, 1))
    Ax[:, sel] *= 1 + 0.1 * rng.standard_normal((B, int(sel.sum())))
    Px *= 1 + 0.2 * rng.random((B, Pt.nnz))
    Q = 0.1 * rng.standard_normal((B, P.shape[0]))
    s = _setup(P, q, A, L[0], U[0])
    x, y, rec = s._solver.hip_batch_solve(q=Q, l=L, u=U, Px=Px, Ax=Ax)
    assert (rec[:, 0] == SOLVED).all(), rec[:, 0]
    dx = rng.standard_normal((B, P.shape[0]))
    res = s._solver.hip_batch_adjoint(x, y, dx, l=L, u=U, Px=Px, Ax=Ax)
    assert (res['rec'][:, 0] == 0).all(), res['rec'][:, :3]
    for i in range(B):
        Pi = sp.csc_matrix((Px[i], Pt.indices, Pt.indptr), shape=Pt.shape)
        Pi = (Pi + Pi.T - sp.diags(Pi.diagonal())).tocsc()
        Ai = sp.csc_matrix((Ax[i], A.indices, A.indptr), shape=A.shape)
        _conditions(Pi, Ai, L[i], U[i], x[i], y[i])
        got = {k: res[k][i] for k in ('dP', 'dq', 'dA', 'dl', 'du')}
        dev, bound, g = _deviations(got, Pi, Ai, L[i], U[i], x[i], y[i], dx[i])
        assert max(dev.values()) <= 1.0, (i, dev, bound)
        one = _setup(Pi, Q[i], Ai, L[i], U[i])
        r1 = one.solve()
        assert r1.info.status_val == SOLVED
        alone = _handle_grads(one, dx[i])
        # the two solves agree to the solver's tolerance, not to the bit: dP and dA carry x and y as factors, so their comparison allows
        # max |r| times the difference of the two solutions on top of the bound; dq, dl, du depend on (x, y) through the active set only
        rn = max(np.abs(g['r_x']).max(), np.abs(g['r_y']).max())
        dxy = max(np.abs(r1.x - x[i]).max(), np.abs(r1.y - y[i]).max())
        assert dxy < 1e-7, (i, dxy)                                         # the two routes solve to eps = 1e-9: a larger difference is a forward discrepancy
        xs, ys = np.abs(x[i]).max(), np.abs(y[i]).max()
        for k, sc, extra in (('dq', 1.0, 0.0), ('dl', 1.0, 0.0), ('du', 1.0, 0.0), ('dP', xs, rn * dxy), ('dA', xs + ys, 2 * rn * dxy)):
            d = np.abs(alone[k] - got[k]).max()
            assert d <= 2 * bound * rn * sc + extra, (i, k, d, bound, rn, dxy)
        record_deviation('test_per_element_matrices_equal_a_single_handle', 'element %d' % i, bound=bound, solutions_differ_by=float(dxy), **dev)


# ---------------------------------------------------------------------------------------------------- 5. torch layer
def _layer_problem(nb, batched, seed=1, n=10, m=20):
    """The reference-style (10, 20) problem; batched: every input 2-D, element b with its own (mildly different) data."""
    P, q, A, l, u, xt = reference_problem(n, m, seed)
    Pc, Ac = sp.csc_matrix(P), sp.csc_matrix(A)
    P_idx, A_idx = ((c.row, c.col) for c in (Pc.tocoo(), Ac.tocoo()))     # CSC order: the order of .data
    if not batched:
        return (P_idx, Pc.shape, A_idx, Ac.shape), [Pc.data.copy(), q, Ac.data.copy(), l, u], xt
    rng = np.random.RandomState(7)
    Pv = np.stack([Pc.data * (1 + 0.05 * b) for b in range(nb)])
    Av = np.stack([Ac.data * (1 + 0.01 * rng.randn(Ac.nnz) * (b > 0)) for b in range(nb)])
    qv = np.stack([q + 0.1 * b for b in range(nb)])
    lv = np.stack([l - 0.01 * b for b in range(nb)]); uv = np.stack([u + 0.01 * b for b in range(nb)])
    return (P_idx, Pc.shape, A_idx, Ac.shape), [Pv, qv, Av, lv, uv], xt


def _layer(struct):
    from osqp_amd.nn.torch import OSQP as Layer
    return Layer(*struct, eps_rel=1e-9, eps_abs=1e-9, max_iter=500000)


@pytest.mark.parametrize('device', ['cpu', 'cuda'])
@pytest.mark.parametrize('batched', [False, True])
def test_torch_layer_backward(device, batched):
    import torch
    nb = 3 if batched else 1
    struct, vals, xt = _layer_problem(nb, batched)
    (P_idx, P_shape, A_idx, A_shape) = struct
    n, m = P_shape[0], A_shape[0]
    layer = _layer(struct)
    ts = [torch.tensor(v, dtype=torch.float64, device=device, requires_grad=True) for v in vals]
    xt_t = torch.tensor(xt, dtype=torch.float64, device=device)
    x = layer(*ts)
    assert x.grad_fn is not None and x.requires_grad
    loss = 0.5 * ((x - xt_t) ** 2).sum()
    before = layer.adjoint_launches
    loss.backward()
    assert layer.adjoint_launches == before + 1                            # ONE adjoint launch per backward
    assert int((torch.as_tensor(layer.last_adjoint_rec)[:, 0] != 0).sum()) == 0
    grads = [t.grad.detach().cpu().numpy() for t in ts]
    for t, gr in zip(ts, grads):
        assert gr.shape == tuple(t.shape) and t.grad.device == t.device
    X = x.detach().cpu().numpy().reshape(nb, n)
    Y = np.asarray(torch.as_tensor(layer.last_dual).cpu()).reshape(nb, m)
    pr, pc, ar, ac = P_idx[0], P_idx[1], A_idx[0], A_idx[1]
    for b in range(nb):
        Pb = sp.csc_matrix((vals[0][b] if batched else vals[0], P_idx), shape=P_shape).toarray()
        Ab = sp.csc_matrix((vals[2][b] if batched else vals[2], A_idx), shape=A_shape).toarray()
        qb, lb, ub = (vals[k][b] if batched else vals[k] for k in (1, 3, 4))
        _conditions(Pb, Ab, lb, ub, X[b], Y[b])
        g = adjoint_ref.adjoint(Pb, Ab, lb, ub, X[b], Y[b], X[b] - xt)
        bound = adjoint_ref.solve_bound(g['K'])
        rn = max(np.abs(g['r_x']).max(), np.abs(g['r_y']).max()); xs, ys = np.abs(X[b]).max(), np.abs(Y[b]).max()
        ref = [g['dP'][pr, pc], g['dq'], g['dA'][ar, ac], g['dl'], g['du']]      # dP: every entry of the full pattern, either triangle the same value
        for name, gr, rf, sc in zip(('dP', 'dq', 'dA', 'dl', 'du'), grads, ref, (xs, 1.0, xs + ys, 1.0, 1.0)):
            d = np.abs((gr[b] if batched else gr) - rf).max()
            assert d <= bound * rn * sc, (device, batched, b, name, d, bound)
    # ... and against forward differences through the layer's own forward, at the reference's tolerance: dq of element 0 in full, and probes of
    # the other four inputs.  An entry of P_val moves with its mirror (the engine reads the upper triangle): the quotient is the sum of both gradients.
    base = [np.array(v, dtype=float) for v in vals]
    f0 = loss.item()

    def fd(changes):
        vs = [v.copy() for v in base]
        for which, k in changes:
            vs[which].reshape(nb, -1)[0, k] += H
        with torch.no_grad():
            xk = layer(*[torch.tensor(v, dtype=torch.float64, device=device) for v in vs])
        assert xk.grad_fn is None
        return (0.5 * ((xk - xt_t) ** 2).sum().item() - f0) / H
    el0 = [gr.reshape(nb, -1)[0] for gr in grads]
    np.testing.assert_allclose(el0[1], [fd([(1, k)]) for k in range(n)], rtol=5e-3, atol=5e-3)
    rng = np.random.RandomState(3)
    mirror = {(int(r_), int(c_)): k for k, (r_, c_) in enumerate(zip(pr, pc))}
    for k in rng.choice(len(pr), 6, replace=False):
        k2 = mirror[(int(pc[k]), int(pr[k]))]
        want = el0[0][k] if k2 == k else el0[0][k] + el0[0][k2]
        np.testing.assert_allclose(want, fd([(0, k)] if k2 == k else [(0, k), (0, k2)]), rtol=5e-3, atol=5e-3, err_msg='P_val[%d]' % k)
    for k in rng.choice(len(ar), 6, replace=False):
        np.testing.assert_allclose(el0[2][k], fd([(2, k)]), rtol=5e-3, atol=5e-3, err_msg='A_val[%d]' % k)
    for k in rng.choice(m, 5, replace=False):
        np.testing.assert_allclose(el0[3][k], fd([(3, k)]), rtol=5e-3, atol=5e-3, err_msg='l[%d]' % k)
        np.testing.assert_allclose(el0[4][k], fd([(4, k)]), rtol=5e-3, atol=5e-3, err_msg='u[%d]' % k)


@pytest.mark.parametrize('device', ['cpu', 'cuda'])
def test_torch_shared_inputs_get_the_sum_over_the_batch(device):
    import torch
    nb = 4
    struct, vals, xt = _layer_problem(1, False)
    n = struct[1][0]
    rng = np.random.RandomState(11)
    Q = np.stack([vals[1] + 0.05 * rng.randn(n) for _ in range(nb)])
    xt_t = torch.tensor(xt, dtype=torch.float64, device=device)
    mk = lambda v: torch.tensor(v, dtype=torch.float64, device=device, requires_grad=True)
    layer = _layer(struct)
    P_t, A_t, l_t, u_t, q_t = mk(vals[0]), mk(vals[2]), mk(vals[3]), mk(vals[4]), mk(Q)
    x = layer(P_t, q_t, A_t, l_t, u_t)
    (0.5 * ((x - xt_t) ** 2).sum()).backward()
    assert layer.adjoint_launches == 1 and tuple(q_t.grad.shape) == (nb, n) and tuple(P_t.grad.shape) == tuple(P_t.shape)
    sums = [np.zeros_like(vals[k]) for k in (0, 2, 3, 4)]
    scale = 0.0
    for b in range(nb):                                                     # every element alone, every input batched: its own gradients
        e = [mk(v[None]) for v in (vals[0], Q[b], vals[2], vals[3], vals[4])]
        xb = layer(*e)
        (0.5 * ((xb - xt_t) ** 2).sum()).backward()
        np.testing.assert_allclose(e[1].grad.cpu().numpy()[0], q_t.grad.cpu().numpy()[b], rtol=0, atol=1e-9 * (1 + np.abs(q_t.grad.cpu().numpy()).max()))
        for acc, k in zip(sums, (0, 2, 3, 4)):
            acc += e[k].grad.cpu().numpy()[0]
            scale = max(scale, np.abs(e[k].grad.cpu().numpy()).max())
    assert layer.adjoint_launches == 1 + nb
    for acc, t in zip(sums, (P_t, A_t, l_t, u_t)):
        np.testing.assert_allclose(t.grad.cpu().numpy(), acc, rtol=0, atol=1e-9 * nb * (1 + scale))


def test_torch_module_takes_an_optimiser_step():
    import torch
    struct, vals, xt = _layer_problem(1, False, seed=4)      # (seed 1 solves to a vertex: x would not move with q; seed 4 has 7 active rows for 10 variables)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.q = torch.nn.Parameter(torch.tensor(vals[1], dtype=torch.float64))
            self.qp = _layer(struct)

        def forward(self):
            t = lambda v: torch.tensor(v, dtype=torch.float64)
            return self.qp(t(vals[0]), self.q, t(vals[2]), t(vals[3]), t(vals[4]))
    net = Net()
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    xt_t = torch.tensor(xt, dtype=torch.float64)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = 0.5 * ((net() - xt_t) ** 2).sum()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert net.qp.adjoint_launches == 3 and net.qp.setup_count == 1
    assert not np.allclose(net.q.detach().numpy(), vals[1]) and losses[-1] < losses[0]
    with torch.no_grad():
        assert net().grad_fn is None


# ---------------------------------------------------------------------------------------------------- 6. a degenerate element
def test_degenerate_element_is_flagged_and_leaves_the_others_alone():
    """The (5, 20) vertex problem with one of its five active rows stored twice: six active rows for five variables in the element whose copy
    carries the row's bounds; in the other elements the copy is unbounded, i.e. never active."""
    n, m = 5, 20
    P, q, A, l, u, xt = reference_problem(n, m, 3)
    s0 = _setup(P, q, A, l, u)
    r0 = s0.solve()
    low, upp = adjoint_ref.active_set(A, l, u, r0.x, r0.y)
    k = int(np.nonzero(low | upp)[0][0])
    A2 = np.vstack([A, A[k]])
    free = lambda v, b: np.append(v, b)
    L = np.stack([free(l, -1e30), free(l, l[k]), free(l, -1e30)]); U = np.stack([free(u, 1e30), free(u, u[k]), free(u, 1e30)])
    Q = np.stack([q, q, 1.1 * q])
    s = _setup(P, q, A2, L[0], U[0])
    x, y, rec = s._solver.hip_batch_solve(q=Q, l=L, u=U)
    assert (rec[:, 0] == SOLVED).all(), rec[:, 0]
    dx = x - xt
    res = s._solver.hip_batch_adjoint(x, y, dx, l=L, u=U)
    print('adjoint records:', res['rec'])
    assert res['rec'][1, 0] != 0 and res['rec'][1, 1] > n, res['rec'][1]
    assert res['rec'][0, 0] == 0 and res['rec'][2, 0] == 0
    for kk in ('dP', 'dq', 'dA', 'dl', 'du'):
        assert np.isfinite(res[kk]).all(), kk
    keep = [0, 2]
    ref = s._solver.hip_batch_adjoint(x[keep], y[keep], dx[keep], l=L[keep], u=U[keep])
    for kk in ('dP', 'dq', 'dA', 'dl', 'du', 'rec'):
        assert np.array_equal(res[kk][keep], ref[kk]), kk                  # bit for bit
