"""GPU tier: the F1 form's reads through one buffer resource over its arena (backend.h DevF1::va: the n-vectors, rho, the P arrays, A's row
pointers, the column pointers).  Large banded and mixed-column problems, graph replay against eager launches and a second handle: every solve
bit-identical; a rho update (rho lives in the arena) and a warm re-solve match a fresh handle of the two-kernel form."""
import os
import warnings

import numpy as np
import pytest

import osqp_amd
import problems

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')


def _solve(P, q, A, l, u, f1, graph=True, **kw):
    old = {k: os.environ.get(k) for k in ('OSQP_HIP_F1', 'OSQP_HIP_GRAPH')}
    os.environ['OSQP_HIP_F1'] = str(f1)
    os.environ['OSQP_HIP_GRAPH'] = '1' if graph else '0'
    try:
        st = dict(eps_abs=1e-6, eps_rel=1e-6, max_iter=20000, adaptive_rho_interval=50, check_termination=25, verbose=False)
        st.update(kw)
        m = osqp_amd.OSQP(); m.setup(P, q, A, l, u, **st)
        return m, m.solve(), m._solver.hip_stats()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _rel(a, b):
    return np.abs(a - b).max() / (1 + np.abs(b).max())


@pytest.mark.parametrize('n,window,frac', [(250000, 200, 0.0), (100000, 200, 0.02)])
def test_f1_arena_solves_are_bit_identical(n, window, frac):
    P, q, A, l, u = problems.banded_qp(n, window=window, long_range=frac) if frac else problems.banded_qp(n, window=window)
    _, ra, sa = _solve(P, q, A, l, u, 1)
    _, rb, _ = _solve(P, q, A, l, u, 1, graph=False)
    _, rc, _ = _solve(P, q, A, l, u, 1)
    assert int(sa['pcg_fused']) == 2 and 1 <= int(sa['f1_replicas']) <= 4, sa
    assert (sa['f1_far_columns'] > 0) == (frac > 0), sa
    assert ra.info.status_val == osqp_amd.SolverStatus.OSQP_SOLVED
    assert ra.info.iter == rb.info.iter == rc.info.iter
    assert np.array_equal(ra.x, rb.x) and np.array_equal(ra.y, rb.y)          # graph replay vs eager launches
    assert np.array_equal(ra.x, rc.x) and np.array_equal(ra.y, rc.y)          # a second handle


def test_f1_arena_rho_update_and_warm_resolve():
    n = 20000
    P, q, A, l, u = problems.banded_qp(n, window=40)
    m1, r1, s1 = _solve(P, q, A, l, u, 1, adaptive_rho=False)
    assert int(s1['pcg_fused']) == 2
    old = os.environ.get('OSQP_HIP_F1'); os.environ['OSQP_HIP_F1'] = '1'
    try:
        m1.update_settings(rho=0.5)
        rw = m1.solve()
    finally:
        if old is None:
            os.environ.pop('OSQP_HIP_F1', None)
        else:
            os.environ['OSQP_HIP_F1'] = old
    _, r0, s0 = _solve(P, q, A, l, u, 0, adaptive_rho=False, rho=0.5)
    assert int(s0['pcg_fused']) != 2
    assert rw.info.status_val == r0.info.status_val == osqp_amd.SolverStatus.OSQP_SOLVED
    assert _rel(rw.x, r0.x) < 1e-4 and _rel(rw.y, r0.y) < 1e-4
