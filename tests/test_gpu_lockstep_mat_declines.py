"""GPU tier: what the lockstep route with per-problem matrices declines (include/osqp_hip.h osqp_hip_batch_solve_lockstep_mat) -- a handle whose stored
upper triangle of P repeats a (j, j) entry (the single-handle assembly sums those with an atomic; the chunk's assembly has one writer per entry), and a
handle the shared lockstep route declines (a Woodbury-corrected preconditioner) -- answers OSQP_FUNC_NOT_IMPLEMENTED, for the query too, and leaves no
trace; the shared route still serves the first handle."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_amd
import problems
from osqp_amd import ext_hip

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
NOT_IMPL = ext_hip.osqp_error_type.OSQP_FUNC_NOT_IMPLEMENTED
S = osqp_amd.SolverStatus


def test_declines_a_repeated_diagonal_entry():
    n, m, nb = 6, 8, 3
    rng = np.random.default_rng(2)
    A = sp.random(m, n, density=0.5, random_state=rng, data_rvs=rng.standard_normal, format='csc')
    q = rng.standard_normal(n); l = -np.ones(m); u = np.ones(m)
    indptr, indices, data = [0], [], []
    for j in range(n):                                   # column j: (0, j) [j > 0], then the diagonal stored TWICE (tests/test_csc_duplicates.py)
        if j > 0:
            indices.append(0); data.append(0.1)
        indices += [j, j]; data += [0.7, 0.5]
        indptr.append(len(indices))
    Pdup = sp.csc_matrix((np.array(data), np.array(indices), np.array(indptr)), shape=(n, n))
    assert Pdup.nnz == 3 * n - 1
    ext = osqp_amd.interface._backend('hip')
    st = ext.OSQPSettings(); ext.osqp_set_default_settings(st)
    st.verbose = 0; st.eps_abs = st.eps_rel = 1e-7
    solver = ext.OSQPSolver(ext.CSC(Pdup), q, ext.CSC(A), l, u, m, n, st)          # straight through the C ABI: the duplicates stay
    Q = np.tile(q, (nb, 1))
    with pytest.raises(ValueError) as e:
        solver.hip_batch_solve_lockstep(q=Q, Ax=np.tile(A.data, (nb, 1)))
    assert e.value.code == NOT_IMPL
    with pytest.raises(ValueError) as e:
        solver.hip_batch_solve_lockstep_device(0, None, None, None, None, None, None, Px_ptr=0, Ax_ptr=0)
    assert e.value.code == NOT_IMPL
    assert all(v == 0 for v in solver.lockstep_mat_last_record().values())
    x, y, rec = solver.hip_batch_solve_lockstep(q=Q)                                # the shared route sums the entries at setup and serves the handle
    assert (rec[:, 0] == S.OSQP_SOLVED).all()


def test_declines_on_a_woodbury_handle():
    P, q, A, l, u = problems.portfolio_qp(200, 10)
    s = osqp_amd.OSQP(algebra='hip'); s.setup(P, q, A, l, u, verbose=False, eps_abs=1e-6, eps_rel=1e-6, max_iter=20000)
    assert s._solver.hip_stats()['woodbury_rows'] > 0
    with pytest.raises(ValueError) as e:
        s._solver.hip_batch_solve_lockstep(q=np.tile(q, (3, 1)), Ax=np.tile(sp.csc_matrix(A).data, (3, 1)))
    assert e.value.code == NOT_IMPL
    assert s.solve().info.status_val == S.OSQP_SOLVED
