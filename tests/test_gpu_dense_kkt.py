"""The dense KKT mode at the level of osqp_solve (include/osqp_hip.h osqp_hip_dense_kkt).

GPU tier: with the reference's literal rho rule the mode -- exact linear solves -- counts ADMM iterations and rho updates like the oracle's direct path;
the path taken (state 1, no PCG iteration, one factorisation per rho update, bit-identical repeats); on / off; updates; declines; refusal by the probe;
polish and adjoint derivatives on an enabled handle; a reordered handle.
CPU tier (the one test here that is not marked gpu): equal counts are a fair demand only where the oracle's own decisions are not borderline -- every
parity case must give the oracle the same iteration and rho-update counts at 0.9 eps and 1.1 eps as at eps.  The seeds below were chosen by that screen."""
import warnings

import numpy as np
import numpy.testing as npt
import pytest
import scipy.sparse as sp

import osqp_amd
import problems
from oracle import Oracle, SOLVED
from util import Fixture

gpu = pytest.mark.gpu
warnings.simplefilter('ignore')
EPS = 1e-6
ST = dict(eps_abs=EPS, eps_rel=EPS, max_iter=20000, adaptive_rho_interval=50, check_termination=25)
LITERAL = dict(rho_tol_exp=1.0, rho_persist=0, rho_window=0, rho_eq_factor=1e3)          # as tests/test_literal_rho_rule.py sets it
NOT_IMPLEMENTED = 10

PARITY = {
    'banded63': lambda: problems.banded_qp(63, window=16, seed=1),
    'banded64': lambda: problems.banded_qp(64, window=16, seed=64),
    'banded65': lambda: problems.banded_qp(65, window=16, seed=65),
    'banded130': lambda: problems.banded_qp(130, window=30, seed=2),
    'banded257': lambda: problems.banded_qp(257, window=40, seed=257),
    'random130': lambda: problems.random_qp(n=130, m=260, density=0.15, seed=1),
    'banded300': lambda: problems.banded_qp(300, window=40, seed=300),
}
_oracle_cache = {}


def oracle(name):
    """(x, y, info) of the oracle at eps, computed once per case and shared (nobody writes to it)."""
    if name not in _oracle_cache:
        P, q, A, l, u = PARITY[name]()
        x, y, info = Oracle().setup(P, q, A, l, u, **ST).solve()
        x.setflags(write=False); y.setflags(write=False)
        _oracle_cache[name] = (x, y, info)
    return _oracle_cache[name]


@pytest.mark.parametrize('name', list(PARITY))
def test_oracle_decisions_are_not_borderline_on_the_parity_cases(name):
    P, q, A, l, u = PARITY[name]()
    _, _, io = oracle(name)
    assert io.status_val == SOLVED
    for f in (0.9, 1.1):
        _, _, i2 = Oracle().setup(P, q, A, l, u, **dict(ST, eps_abs=f * EPS, eps_rel=f * EPS)).solve()
        assert (i2.status_val, i2.iter, i2.rho_updates) == (SOLVED, io.iter, io.rho_updates), (name, f, i2.iter, io.iter, i2.rho_updates, io.rho_updates)


def handle(P, q, A, l, u, on=True, literal=True, **over):
    m = osqp_amd.OSQP(algebra='hip'); m.setup(P, q, A, l, u, verbose=False, **dict(ST, **over))
    if literal:
        m._solver.set_policy(**LITERAL)
    if on:
        assert m._solver.hip_dense_kkt(True) == 0
        assert m._solver.hip_dense_kkt_record()['state'] == 1
    return m


def close(a, b, tol):
    return np.abs(a - b).max() <= tol * (1 + np.abs(b).max())


def assert_parity(r, name):
    xo, yo, io = oracle(name)
    assert r.info.status_val == 1 and io.status_val == SOLVED
    print('%s: iter %d (oracle %d), rho updates %d (%d), |dx| %.2e |dy| %.2e' % (name, r.info.iter, io.iter, r.info.rho_updates, io.rho_updates,
                                                                                 np.abs(r.x - xo).max() / (1 + np.abs(xo).max()), np.abs(r.y - yo).max() / (1 + np.abs(yo).max())))
    assert r.info.iter == io.iter and r.info.rho_updates == io.rho_updates, (r.info.iter, io.iter, r.info.rho_updates, io.rho_updates)
    npt.assert_allclose(r.x, xo, rtol=0, atol=1e-7 * (1 + np.abs(xo).max()))
    npt.assert_allclose(r.y, yo, rtol=0, atol=1e-7 * (1 + np.abs(yo).max()))
    assert abs(r.info.obj_val - io.obj_val) <= 1e-9 * (1 + abs(io.obj_val))


@gpu
@pytest.mark.parametrize('name', list(PARITY))
def test_oracle_parity_and_the_path_taken(name):
    P, q, A, l, u = PARITY[name]()
    m = handle(P, q, A, l, u, warm_starting=False)
    before = m._solver.hip_dense_kkt_record()['factorisations']
    r = m.solve()
    assert_parity(r, name)
    rec, st = m._solver.hip_dense_kkt_record(), m._solver.hip_stats()
    assert rec['state'] == 1 and rec['order'] == len(q)
    assert st['pcg_iters_total'] == 0 and st['kernel_launches'] >= 3 * r.info.iter
    assert rec['solve_factorisations'] == r.info.rho_updates and rec['factorisations'] == before + r.info.rho_updates
    assert rec['solve_factor_ms'] > 0 or r.info.rho_updates == 0
    # a second cold solve from the same rho: the same bits
    x1, y1, it1 = r.x.copy(), r.y.copy(), r.info.iter
    m.update_settings(rho=0.1)
    r2 = m.solve()
    assert r2.info.iter == it1 and np.array_equal(r2.x, x1) and np.array_equal(r2.y, y1)


@gpu
@pytest.mark.parametrize('name', ['banded65', 'banded300'])
def test_off_is_the_handle_that_was_never_enabled(name):
    P, q, A, l, u = PARITY[name]()
    a, twin = handle(P, q, A, l, u, warm_starting=False), handle(P, q, A, l, u, on=False, warm_starting=False)
    ra = a.solve()
    xa, ya = ra.x.copy(), ra.y.copy()
    rt0 = twin.solve()
    assert close(xa, rt0.x, 2e-5) and close(ya, rt0.y, 2e-5)                           # on against off: the eps-level bound
    assert a._solver.hip_dense_kkt(False) == 0
    assert all(v == 0 for v in a._solver.hip_dense_kkt_record().values())
    a.update_settings(rho=0.1); twin.update_settings(rho=0.1)
    rb, rt = a.solve(), twin.solve()
    assert rb.info.status_val == rt.info.status_val == 1 and rb.info.iter == rt.info.iter
    assert np.array_equal(rb.x, rt.x) and np.array_equal(rb.y, rt.y)


@gpu
def test_updates_refactorise():
    P, q, A, l, u = PARITY['banded257']()
    a, twin = handle(P, q, A, l, u), handle(P, q, A, l, u, on=False)
    rng = np.random.default_rng(4)
    q2 = q + 0.05 * rng.standard_normal(len(q))
    # feasible by construction: the first problem's solution satisfies 1.1 l <= (1.1 A) x <= 1.1 u, and the rows that become equalities sit at its values
    xo = oracle('banded257')[0]
    l2, u2 = 1.1 * l, 1.1 * u
    # (every 20th inequality row: with every 7th the duals are so badly determined that the oracle's own eps = 1e-6 and eps = 1e-9 solutions differ by 9e-4
    #  in y -- no two solvers can agree to 2e-5 there; with every 20th they differ by 4e-6)
    rows = np.nonzero(u > l)[0][::20]
    l2[rows] = u2[rows] = 1.1 * (A @ xo)[rows]                                         # inequality rows become equalities: other classes, other rho_i
    Pu = sp.triu(P, format='csc')
    steps = (lambda m: m.update(q=q2, l=l2, u=u2), lambda m: m.update(Px=1.1 * Pu.data, Ax=1.1 * A.data), lambda m: m.update_settings(rho=0.3))
    P2, A2 = 1.1 * P, 1.1 * A
    count = a._solver.hip_dense_kkt_record()['factorisations']
    for step in steps:
        step(a); step(twin)
        rec = a._solver.hip_dense_kkt_record()
        assert rec['factorisations'] == count + 1 and rec['state'] == 1, rec
        count += 1
    ra, rt = a.solve(), twin.solve()
    assert ra.info.status_val == rt.info.status_val == 1
    assert a._solver.hip_stats()['pcg_iters_total'] == 0
    assert close(ra.x, rt.x, 2e-5) and close(ra.y, rt.y, 2e-5)
    k = problems.kkt_certificate(P2, q2, A2, l2, u2, ra.x, ra.y)
    ax = A2 @ ra.x
    assert k['pri'] <= EPS + EPS * max(np.abs(ax).max(), np.abs(np.clip(ax, l2, u2)).max()), k
    assert k['dua'] <= EPS + EPS * max(np.abs(P2 @ ra.x).max(), np.abs(A2.T @ ra.y).max(), np.abs(q2).max()), k


@gpu
@pytest.mark.parametrize('gen', [problems.portfolio_qp, lambda: problems.banded_qp(osqp_amd._lib.DENSE_KKT_MAX_N + 1, window=40)])
def test_declines_leave_the_handle_untouched(gen):
    P, q, A, l, u = gen()
    a, twin = handle(P, q, A, l, u, on=False, literal=False), handle(P, q, A, l, u, on=False, literal=False)
    assert a._solver.hip_dense_kkt(True) == NOT_IMPLEMENTED
    assert all(v == 0 for v in a._solver.hip_dense_kkt_record().values())
    ra, rt = a.solve(), twin.solve()
    assert ra.info.status_val == rt.info.status_val == 1 and ra.info.iter == rt.info.iter
    assert np.array_equal(ra.x, rt.x) and np.array_equal(ra.y, rt.y)


@gpu
def test_an_indefinite_P_is_refused_by_the_factorisation():
    f = Fixture('non_convex')
    a = osqp_amd.OSQP(); a.setup(f.P, f.q, f.A, f.l, f.u, sigma=1e-6, verbose=False)
    twin = osqp_amd.OSQP(); twin.setup(f.P, f.q, f.A, f.l, f.u, sigma=1e-6, verbose=False)
    assert a._solver.hip_dense_kkt(True) == 0
    rec = a._solver.hip_dense_kkt_record()
    assert rec['state'] == 2 and (not rec['min_pivot'] > 0 or not rec['probe'] <= 1e-6), rec
    ra, rt = a.solve(), twin.solve()
    assert ra.info.status_val == rt.info.status_val                                     # (a rho update inside the solve may make K positive definite: the state follows rho)


@gpu
def test_polish_and_adjoint_run_on_the_pcg_path_and_the_mode_comes_back(monkeypatch):
    import adjoint_sparse_ref as aref
    P, q, A, l, u = problems.banded_qp(1000, window=40)                                # (beyond one workgroup: polish and adjoint take their PCG routes)
    # polish: the certificate of tests/test_gpu_polish.py::test_polish_on_the_pcg_path_matches_the_oracle
    m = handle(P, q, A, l, u, literal=False, polishing=True, eps_abs=1e-4, eps_rel=1e-4)
    r = m.solve()
    rec = m._solver.hip_dense_kkt_record()
    assert r.info.status_val == 1 and r.info.status_polish == 1 and rec['state'] == 1
    assert rec['solve_factorisations'] == r.info.rho_updates + 1                       # the inverse for the ADMM rho, re-formed behind the polish: counted
    k = problems.kkt_certificate(P, q, A, l, u, r.x, r.y)
    ax = A @ r.x
    scale_p = 1 + max(np.abs(ax).max(), np.abs(np.clip(ax, l, u)).max())
    scale_d = 1 + max(np.abs(P @ r.x).max(), np.abs(A.T @ r.y).max(), np.abs(q).max())
    assert k['pri'] <= 1e-9 * scale_p and k['dua'] <= 1e-9 * scale_d, k
    # adjoint derivatives: the independent certificate of tests/test_gpu_adjoint_pcg.py::_check
    s = handle(P, q, A, l, u, literal=False, eps_abs=1e-8, eps_rel=1e-8, max_iter=200000)
    r = s.solve()
    assert r.info.status_val == 1 and s._solver.hip_stats()['pcg_iters_total'] == 0
    count = s._solver.hip_dense_kkt_record()['factorisations']
    dx = r.x - 0.1 * np.random.default_rng(7).standard_normal(len(q))
    s.adjoint_derivative_compute(dx=dx)
    dq, dl, du = s.adjoint_derivative_get_vec()
    host_res, gv, rv, nact = aref.certificate(P, A, l, u, r.x, r.y, dx, None, dq, dl, du)
    arec = s.adjoint_last_record()
    assert host_res < 1e-6 and arec['status'] == 0 and arec['active_rows'] == nact, (host_res, arec)
    rec = s._solver.hip_dense_kkt_record()
    assert rec['state'] == 1 and rec['factorisations'] == count + 1


@gpu
def test_a_reordered_handle_is_served(monkeypatch):
    monkeypatch.setenv('OSQP_HIP_REORDER', '2')                                         # through the default policy, as tests/test_reorder.py does
    P, q, A, l, u = PARITY['banded130']()
    m = handle(P, q, A, l, u)
    assert m._solver.hip_stats()['reordered'] == 1
    r = m.solve()
    assert_parity(r, 'banded130')
    assert m._solver.hip_stats()['pcg_iters_total'] == 0 and m._solver.hip_dense_kkt_record()['state'] == 1
