"""CPU tier: pins the yardstick of the adjoint tests.  tests/adjoint_ref.py (the dense numpy statement of the adjoint derivatives) is compared
against forward differences through the ORACLE (eps_abs = eps_rel = 1e-9, h = 1e-5) at the tolerances of the reference's own derivative test
(rtol = atol = 5e-3), on problems from that test's generator (restated below): dq, dl, du, dA and dP, with and without equality rows and
infinite bounds.  The loss is the reference's 0.5 |x - x_true|^2, so dx = x - x_true and dy = 0.

Through the host simulator (no adjoint kernel) adjoint_derivative_compute answers "not implemented" cleanly."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import adjoint_ref
from oracle import Oracle, SOLVED

warnings.simplefilter('ignore')
OST = dict(eps_abs=1e-9, eps_rel=1e-9, max_iter=500000)
H, RTOL, ATOL = 1e-5, 5e-3, 5e-3
INF = 1e30


def reference_problem(n, m, seed, n_eq=0, n_inf=0):
    """The generator of the reference's derivative test (get_prob), then its equality / infinite-bound variants: the first n_eq rows become
    equalities (u = l), the next n_inf rows lose their lower bound."""
    rng = np.random.RandomState(seed)
    L = rng.randn(n, n - 1)
    P = L.dot(L.T) + 0.1 * np.eye(n)
    x_0 = rng.randn(n)
    s_0 = rng.rand(m)
    A = rng.randn(m, n)
    u = A.dot(x_0) + s_0
    l = A.dot(x_0) - s_0
    q = rng.randn(n)
    true_x = rng.randn(n)
    u[:n_eq] = l[:n_eq]
    l[n_eq:n_eq + n_inf] = -INF
    return P, q, A, l, u, true_x


def oracle_solve(P, q, A, l, u):
    x, y, info = Oracle().setup(sp.csc_matrix(P), q, sp.csc_matrix(A), l, u, **OST).solve()
    assert info.status_val == SOLVED
    return x, y


def check_conditions(P, A, l, u, x, y):
    slack, ymin, smin, cond = adjoint_ref.conditions(P, A, l, u, x, y)
    assert slack > 1e-4 and ymin > 1e-4 and smin > 1e-4, (slack, ymin, smin, cond)


CASES = [  # n, m, seed, equality rows, rows without lower bound
    (5, 5, 1, 0, 0), (10, 20, 1, 0, 0), (30, 20, 1, 10, 0), (20, 15, 1, 15, 0), (10, 10, 2, 5, 5),
]


@pytest.mark.parametrize('n,m,seed,n_eq,n_inf', CASES)
def test_helper_matches_forward_differences_through_the_oracle(n, m, seed, n_eq, n_inf):
    P, q, A, l, u, xt = reference_problem(n, m, seed, n_eq, n_inf)
    x, y = oracle_solve(P, q, A, l, u)
    check_conditions(P, A, l, u, x, y)
    g = adjoint_ref.adjoint(P, A, l, u, x, y, x - xt)
    f0 = 0.5 * np.sum((x - xt) ** 2)

    def loss(P=P, q=q, A=A, l=l, u=u):
        xs, _ = oracle_solve(P, q, A, l, u)
        return 0.5 * np.sum((xs - xt) ** 2)

    def unit(k, size):
        e = np.zeros(size); e[k] = H
        return e
    worst = {}

    def close(name, fd, got):
        worst[name] = float(np.abs(np.asarray(fd) - np.asarray(got)).max())
        np.testing.assert_allclose(got, fd, rtol=RTOL, atol=ATOL, err_msg=name)
    close('dq', [(loss(q=q + unit(k, n)) - f0) / H for k in range(n)], g['dq'])
    fin = np.nonzero(l > -INF)[0]
    close('dl', [(loss(l=l + unit(k, m)) - f0) / H if l[k] < u[k] else 0.0 for k in fin], [g['dl'][k] if l[k] < u[k] else 0.0 for k in fin])
    close('du', [(loss(u=u + unit(k, m)) - f0) / H if l[k] < u[k] else 0.0 for k in range(m)], [g['du'][k] if l[k] < u[k] else 0.0 for k in range(m)])
    # an equality row moves both bounds together: dl + du
    eq = np.nonzero(l == u)[0]
    if eq.size:
        close('dl+du (equality rows)', [(loss(l=l + unit(k, m), u=u + unit(k, m)) - f0) / H for k in eq], (g['dl'] + g['du'])[eq])
    rng = np.random.RandomState(0)
    ent = [(rng.randint(m), rng.randint(n)) for _ in range(min(12, m * n))]
    fdA = []
    for i, j in ent:
        A2 = A.copy(); A2[i, j] += H
        fdA.append((loss(A=A2) - f0) / H)
    close('dA', fdA, [g['dA'][i, j] for i, j in ent])
    # P: a stored upper-triangle entry and its mirror move together, so the difference quotient is dP_ij + dP_ji = 2 dP_ij off the diagonal
    ent = [(min(i, j), max(i, j)) for i, j in [(rng.randint(n), rng.randint(n)) for _ in range(min(12, n * n))]]
    fdP = []
    for i, j in ent:
        P2 = P.copy(); P2[i, j] += H
        if i != j:
            P2[j, i] += H
        fdP.append((loss(P=P2) - f0) / H)
    close('dP', fdP, [g['dP'][i, j] * (1.0 if i == j else 2.0) for i, j in ent])
    print('worst deviations from the finite differences:', worst)


def test_vertex_case_is_kept_and_compared_absolutely():
    """As many active rows as variables: x does not move with q, dq is zero to rounding -- compared absolutely."""
    P, q, A, l, u, xt = reference_problem(5, 20, 3)
    x, y = oracle_solve(P, q, A, l, u)
    low, upp = adjoint_ref.active_set(A, l, u, x, y)
    assert int((low | upp).sum()) == 5, int((low | upp).sum())
    check_conditions(P, A, l, u, x, y)
    g = adjoint_ref.adjoint(P, A, l, u, x, y, x - xt)
    assert np.abs(g['dq']).max() < 1e-12
    f0 = 0.5 * np.sum((x - xt) ** 2)
    for k in range(5):
        q2 = q.copy(); q2[k] += H
        x2, _ = oracle_solve(P, q2, A, l, u)
        assert abs((0.5 * np.sum((x2 - xt) ** 2) - f0) / H) < ATOL


def test_host_simulator_answers_not_implemented():
    from hostsim_util import hostsim
    with hostsim():
        import osqp_amd
        P, q, A, l, u, xt = reference_problem(5, 5, 1)
        s = osqp_amd.OSQP(algebra='hip')
        s.setup(sp.csc_matrix(P), q, sp.csc_matrix(A), l, u, eps_abs=1e-6, eps_rel=1e-6, verbose=False)
        with pytest.raises(ValueError):
            s.adjoint_derivative_compute(dx=np.zeros(5))              # before a solve
        r = s.solve()
        assert r.info.status_val == osqp_amd.SolverStatus.OSQP_SOLVED
        assert s._solver.adjoint_derivative_compute(r.x - xt, None) == int(osqp_amd.SolverError.OSQP_FUNC_NOT_IMPLEMENTED)
        with pytest.raises(NotImplementedError):
            s.adjoint_derivative_compute(dx=r.x - xt)
        dq = np.zeros(5); dl = np.zeros(5); du = np.zeros(5)
        assert s._solver.adjoint_derivative_get_vec(dq, dl, du) == int(osqp_amd.SolverError.OSQP_FUNC_NOT_IMPLEMENTED)
