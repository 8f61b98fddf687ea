"""GPU tier: the host staging that hip_batch_solve (one workgroup per QP) and hip_batch_solve_lockstep share (engine_api.cpp Engine::BatchStage) -- the
handle's own bounds standing in for an argument given as None, the l <= u validation of every member, and the lockstep route's row mapping on a
reordered handle.  A random QP with n = 12, m = 18 and B = 3: both routes take it, every call is a few milliseconds.  Everything is compared exactly:
the same kernels run on the same numbers."""
import ctypes
import warnings

import numpy as np
import pytest

import osqp_amd
import problems
from osqp_amd import _lib, ext_hip

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
INVALID = ext_hip.osqp_error_type.OSQP_DATA_VALIDATION_ERROR
N, M, B = 12, 18, 3
ST = dict(eps_abs=1e-6, eps_rel=1e-6, max_iter=4000, verbose=False)
ROUTES = {'workgroup': 'hip_batch_solve', 'lockstep': 'hip_batch_solve_lockstep'}
REC_TIME = 9                        # polish seconds: the one field of a record that is a time


def _problem():
    P, q, A, l, u = problems.random_qp(N, M, seed=4)
    rng = np.random.default_rng(11)
    Q = np.stack([q + 0.05 * b * rng.standard_normal(N) for b in range(B)])
    L = np.stack([l - 0.01 * b for b in range(B)])
    return (P, q, A, l, u), Q, L


def _handle(prob):
    s = osqp_amd.OSQP(algebra='hip')
    s.setup(*prob, **ST)
    return s


def _same(a, b):
    ra, rb = np.delete(a[2], REC_TIME, axis=1), np.delete(b[2], REC_TIME, axis=1)
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(ra, rb)


def _refused(call, **kw):
    with pytest.raises(ValueError) as e:
        call(**kw)
    return e.value.code


@pytest.mark.parametrize('route', list(ROUTES))
def test_own_bounds_and_validation(route):
    prob, Q, L = _problem()
    u = prob[4]
    s = _handle(prob)
    call = getattr(s._solver, ROUTES[route])
    only_l = call(q=Q, l=L)
    assert (only_l[2][:, 0] == osqp_amd.SolverStatus.OSQP_SOLVED).all(), only_l[2][:, 0]
    assert _same(only_l, call(q=Q, l=L, u=np.tile(u, (B, 1))))              # u = None is the handle's own u for every member
    bad = L.copy()
    bad[1, 7] = u[7] + 1.0                                                  # one row of one member: l > u
    assert _refused(call, q=Q, l=bad) == INVALID                             # ... against the handle's own u
    assert _refused(call, q=Q, l=bad, u=np.tile(u, (B, 1))) == INVALID       # ... against the u given
    assert _same(call(q=Q, l=L), getattr(_handle(prob)._solver, ROUTES[route])(q=Q, l=L))      # the refused calls left no trace


def test_lockstep_validates_in_the_callers_numbering_on_a_reordered_handle(monkeypatch):
    """The host copies of the handle's own bounds are kept in the engine's numbering; with only l given, row i of the caller is compared with the
    own u of row i, not with what sits at position i of the copies (the own u of row perm_rows[i]).  Two rows that the reordering moves: for row i,
    whose own u is the smaller of the two, an l between them must be refused; for row j, whose own u is the larger, an l between them must be
    accepted -- reading position i / j gets both wrong."""
    prob, Q, L = _problem()
    u = prob[4]
    monkeypatch.setenv('OSQP_HIP_REORDER', '2')
    s = _handle(prob)
    assert s._solver.hip_stats()['reordered'] == 1
    pc, pr = np.empty(N, np.int32), np.empty(M, np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    assert _lib.handle().osqp_hip_get_reordering(s._solver._p, pc.ctypes.data_as(ip), pr.ctypes.data_as(ip)) == 0
    up = [i for i in range(M) if pr[i] != i and u[i] < u[pr[i]]]            # position i holds a larger u than row i's own
    down = [i for i in range(M) if pr[i] != i and u[i] > u[pr[i]]]
    assert up and down, pr
    i, j = up[0], down[0]
    bad = L.copy()
    bad[2, i] = 0.5 * (u[i] + u[pr[i]])                                     # above row i's own u
    assert _refused(s._solver.hip_batch_solve_lockstep, q=Q, l=bad) == INVALID
    ok = L.copy()
    ok[2, j] = 0.5 * (u[j] + u[pr[j]])                                      # below row j's own u, above what position j holds
    x, y, rec = s._solver.hip_batch_solve_lockstep(q=Q, l=ok)
    assert rec.shape == (B, 12) and np.isfinite(x[:2]).all()
