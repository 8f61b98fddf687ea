"""CPU tier: tests/adjoint_sparse_ref.py (the sparse yardstick of the PCG path's adjoint tests) pinned to the dense tests/adjoint_ref.py on the
small reference cases -- r, dq, dl, du and dP / dA at the stored entries to 1e-10 relative -- and its sigma_min estimate to the SVD's."""
import numpy as np
import pytest
import scipy.sparse as sp

import adjoint_ref
import adjoint_sparse_ref
from test_adjoint_reference_cpu import CASES, oracle_solve, reference_problem

RTOL = 1e-10


@pytest.mark.parametrize('n,m,seed,n_eq,n_inf', CASES)
@pytest.mark.parametrize('with_dy', [False, True])
def test_sparse_helper_equals_the_dense_helper(n, m, seed, n_eq, n_inf, with_dy):
    P, q, A, l, u, xt = reference_problem(n, m, seed, n_eq, n_inf)
    x, y = oracle_solve(P, q, A, l, u)
    dx = x - xt
    dy = np.random.default_rng(seed).standard_normal(m) if with_dy else None
    d = adjoint_ref.adjoint(P, A, l, u, x, y, dx, dy)
    s = adjoint_sparse_ref.adjoint(sp.csc_matrix(P), sp.csc_matrix(A), l, u, x, y, dx, dy)
    assert (d['low'] == s['low']).all() and (d['upp'] == s['upp']).all()
    (pr, pc), (ar, ac) = adjoint_sparse_ref.stored_entries(P, A)
    for key, ref in (('r_x', d['r_x']), ('r_y', d['r_y']), ('dq', d['dq']), ('dl', d['dl']), ('du', d['du']), ('dP', d['dP'][pr, pc]), ('dA', d['dA'][ar, ac])):
        # relative to the output's own largest entry -- or, where the whole output is a rounding-level zero in both helpers (the vertex case:
        # n active rows pin r_x = 0), to the rounding of the right-hand side it was solved from
        scale = max(np.abs(ref).max(initial=0.0), 1e-300)
        floor = 1e3 * adjoint_ref.EPS * np.abs(dx).max() * max(1.0, np.abs(x).max() + np.abs(y).max())
        err = np.abs(s[key] - ref).max(initial=0.0)
        assert err <= RTOL * scale or err <= floor, (key, err / scale)
    assert s['residual'] < 1e-12
    sv = np.linalg.svd(d['K'], compute_uv=False).min()
    assert abs(s['sigma_min'] - sv) <= 1e-3 * sv, (s['sigma_min'], sv)
    res, g, r, nact = adjoint_sparse_ref.certificate(sp.csc_matrix(P), sp.csc_matrix(A), l, u, x, y, dx, dy, s['dq'], s['dl'], s['du'])
    assert res < 1e-12 and nact == len(d['act'])
