"""GPU tier: the batch family's kernels decide with ONE text (osqp-python_amd/csrc/term_rules.h) -- the same batch of five small QPs, one per status class,
through every batch route gives the same statuses, and they are the oracle's.

The problems are test_gpu_batch_lockstep.py::test_statuses' construction (A = [I; I; ...], P = diag(d) with d_0 = 0) at n = 80 with a third block of
pentadiagonal rows, m = 240: nnz(A) = 554 is the smallest such pattern the spectral and wave forms take (batch_plan.cpp: 520 entries, m <= 256).
max_iter = 150, checks every 25 iterations, eps_abs = 1e-5, eps_rel = 0:
  0  the base problem (q, l, u)                         solved
  1  x_5 = 1 and x_5 = -1                               primal infeasible
  2  x_0 free, zero curvature, negative cost            dual infeasible
  3  150 (q, l, u)                                      solved inaccurate
  4  5000 (q, l, u)                                     max_iter reached
How 3 and 4 are drawn.  A batch element runs on the handle's equilibration, so ADMM on s (q, l, u) is s times ADMM on (q, l, u), iterate for iterate
(the rho estimate is a ratio); with eps_rel = 0 the tolerances do not scale, so s alone places a problem against them.  The base problem's
residuals at iteration 150 are 1.9e-7 (primal) and 1.6e-8 (dual) -- the oracle and every route, measured, equal to two digits -- and ten times
that per 25 iterations before: eps / 53 at the last check; 150 times that is 2.9 eps, the middle of the approximate pass's window (eps, 10 eps),
and 29 eps one check earlier; 5000 times is 95 eps.  Every threshold is a factor 2.9 away or more.
The oracle of an element is what the batch routes compute: a solver set up with the handle's (q, l, u) -- its scaling -- then update(q, l, u)
and a cold solve.  cg_tol_fraction = 1e-4 keeps the PCG routes' inner solves tight: this test is about the decisions, and with the default 0.15
the inexact solves alone move a PCG route's residuals at a given iteration by orders of magnitude.
The wave route: the spectral form is prepared for batches of 32 and more, so the handle first solves 32 copies of the base problem; the five then
run on k_batch_wave (batch_wave_split >= 0), which hands 1 and 2 -- other constraint classes -- to the banded kernel.

test_every_route_steps_alike: the same routes on four elements whose ROWS differ in class -- what osqp-python_amd/csrc/step_rules.h states once (row
class, rho of a row, equality weight, the clamp of the load rules, the z / y step on loose and equality rows); `_four` describes them."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_amd
from oracle import Oracle

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
S = osqp_amd.SolverStatus
N, MAX_ITER = 80, 150
ST = dict(eps_abs=1e-5, eps_rel=0.0, eps_prim_inf=1e-5, eps_dual_inf=1e-5, max_iter=MAX_ITER, check_termination=25, adaptive_rho_interval=50)
EXPECTED = [S.OSQP_SOLVED, S.OSQP_PRIMAL_INFEASIBLE, S.OSQP_DUAL_INFEASIBLE, S.OSQP_SOLVED_INACCURATE, S.OSQP_MAX_ITER_REACHED]


def _five():
    n = N
    rng = np.random.default_rng(7)
    d = 0.5 + rng.random(n); d[0] = 0.0
    T = sp.diags([rng.standard_normal(n - abs(k)) for k in (-2, -1, 0, 1, 2)], [-2, -1, 0, 1, 2], format='csc')
    P = sp.diags(d, format='csc'); A = sp.vstack([sp.identity(n), sp.identity(n), T], format='csc')
    q = rng.standard_normal(n)
    l = np.concatenate([-np.ones(n), -2 * np.ones(n), -1.5 * np.ones(n)]); u = -l
    Q, L, U = np.tile(q, (5, 1)), np.tile(l, (5, 1)), np.tile(u, (5, 1))
    L[1, 5] = U[1, 5] = 1.0; L[1, n + 5] = U[1, n + 5] = -1.0
    rows0 = A.tocsr()[:, 0].nonzero()[0]                               # every row that holds x_0
    Q[2, 0] = -1.0; L[2, rows0] = -1e30; U[2, rows0] = 1e30
    for b, scale in ((3, 150.0), (4, 5000.0)):
        Q[b] *= scale; L[b] *= scale; U[b] *= scale
    return P, q, A, l, u, Q, L, U


@pytest.fixture(scope='module')
def five():
    P, q, A, l, u, Q, L, U = _five()
    oracle = []
    for b in range(5):
        o = Oracle().setup(P, q, A, l, u, **ST)
        o.update(q=Q[b], l=L[b], u=U[b])
        oracle.append(o.solve()[2])
    return P, q, A, l, u, Q, L, U, [int(io.status_val) for io in oracle], [int(io.iter) for io in oracle]


def test_every_route_decides_like_the_oracle(five):
    P, q, A, l, u, Q, L, U, ostat, oiter = five
    assert ostat == [int(s) for s in EXPECTED], ostat                  # the draws are what the docstring says they are
    routes = (('generic', dict(batch_variant=5), False), ('direct', dict(batch_variant=1), False), ('wave', dict(batch_wave=1), False), ('lockstep', {}, True))
    res = {}
    for name, pol, lockstep in routes:
        s = osqp_amd.OSQP(algebra='hip'); s.setup(P, q, A, l, u, verbose=False, cg_tol_fraction=1e-4, **ST)
        if pol:
            s._solver.set_policy(**pol)
        if name == 'wave':
            s._solver.hip_batch_solve(q=np.tile(Q[0], (32, 1)), l=np.tile(L[0], (32, 1)), u=np.tile(U[0], (32, 1)))
        res[name] = (s._solver.hip_batch_solve_lockstep if lockstep else s._solver.hip_batch_solve)(q=Q, l=L, u=U)
        if name == 'wave':
            assert s._solver.hip_stats()['batch_wave_split'] >= 0      # k_batch_wave ran
        print(name, res[name][2][:, :2].tolist())
    for name, (x, y, rec) in res.items():
        assert [int(v) for v in rec[:, 0]] == ostat, (name, rec[:, 0], ostat)
        nx, ny = np.isnan(x), np.isnan(y)                              # certificates: dy in y and NaN in x (primal), dx in x and NaN in y (dual)
        assert nx[1].all() and not ny[1].any() and ny[2].all() and not nx[2].any(), name
        assert not nx[[0, 3, 4]].any() and not ny[[0, 3, 4]].any(), name
        assert np.isnan(rec).sum() == 0 and rec[1, 2] == 1e30 and rec[2, 2] == -1e30, (name, rec[:, 2])
        assert (rec[[3, 4], 1] == MAX_ITER).all(), (name, rec[:, 1])
    # the two PCG routes stop the problems that run to max_iter at the same iteration
    assert np.array_equal(res['generic'][2][[3, 4], 1], res['lockstep'][2][[3, 4], 1])


def _four():
    """_five's pattern and base problem; four elements, all solvable, whose rows differ in class (_osqp.py:505-522):
      a  the base problem                                                          240 inequality rows
      b  block one as equalities x = v, |v| <= 0.5 (inside the other blocks'       80 equality rows, 160 loose rows: no inequality row, so the
         bounds); blocks two and three loose (+-1e30)                               equality weight is the reference's 1e3; rho = 1e-6 on the loose rows
      c  every fourth row of block one an equality x_j = v_j, the rest as a        20 equality rows among 220 inequality rows: the mixed weight
      d  as a, with bounds that do not bind given beyond +-OSQP_INFTY (1e35):      the clamp; block two's lower and block three's upper bounds on
         block two below, block three above on every other row                      those rows become loose on ONE side -- still inequality rows
    Settings: ST with max_iter = 500 (ST4) -- under ST's 150 the base problem stops at 125 and c ends OSQP_SOLVED_INACCURATE; 500 puts every
    element's end in the first half.  Oracle, cold, with ST4: a 125, b 50, c 225, d 125 iterations, all OSQP_SOLVED; warm-started from that result: 25 each.
    (The warm oracle runs with c_core_warm_start: the batch routes scale a warm y by c Einv, as the C core does, the pure-Python reference by Einv
    alone -- without the flag the oracle's warm run repeats its cold one.)"""
    P, q, A, l, u, Q, L, U = _five()
    n = N
    Q, L, U = Q[:4].copy(), L[:4].copy(), U[:4].copy()
    Q[:] = q; L[:] = l; U[:] = u
    v = 0.5 * np.cos(np.arange(n))
    L[1, :n] = U[1, :n] = v; L[1, n:] = -1e30; U[1, n:] = 1e30
    L[2, 0:n:4] = U[2, 0:n:4] = v[0:n:4]
    L[3, n:2 * n:2] = -1e35; U[3, 2 * n::2] = 1e35
    return P, q, A, l, u, Q, L, U


ST4 = dict(ST, max_iter=500)


def test_every_route_steps_alike():
    P, q, A, l, u, Q, L, U = _four()
    cold, warm = [], []
    for b in range(4):
        for start in (cold, warm):
            o = Oracle().setup(P, q, A, l, u, c_core_warm_start=1, **ST4)
            o.update(q=Q[b], l=L[b], u=U[b])
            if start is warm:
                o.warm_start(x=cold[b][0], y=cold[b][1])
            start.append(o.solve())
    for tag, ref in (('cold', cold), ('warm', warm)):
        assert [int(r[2].status_val) for r in ref] == [int(S.OSQP_SOLVED)] * 4, tag
        assert max(int(r[2].iter) for r in ref) <= ST4['max_iter'] // 2, [int(r[2].iter) for r in ref]      # well before max_iter
    routes = (('generic', dict(batch_variant=5), False), ('direct', dict(batch_variant=1), False), ('wave', dict(batch_wave=1), False), ('lockstep', {}, True))
    res = {}
    for name, pol, lockstep in routes:
        s = osqp_amd.OSQP(algebra='hip'); s.setup(P, q, A, l, u, verbose=False, cg_tol_fraction=1e-4, **ST4)
        if pol:
            s._solver.set_policy(**pol)
        if name == 'wave':
            s._solver.hip_batch_solve(q=np.tile(Q[0], (32, 1)), l=np.tile(L[0], (32, 1)), u=np.tile(U[0], (32, 1)))
        solve = s._solver.hip_batch_solve_lockstep if lockstep else s._solver.hip_batch_solve
        c = solve(q=Q, l=L, u=U)
        if name == 'wave':
            assert s._solver.hip_stats()['batch_wave_split'] >= 0      # k_batch_wave ran (it hands b and c -- other classes than the handle's -- to the banded kernel)
        res[name] = (c, solve(q=Q, l=L, u=U, x0=c[0], y0=c[1]))
    for name, runs in res.items():
        # direct / wave: the oracle's algorithm -- its iteration counts, x and y to 1e-7 (test_gpu_batch_wave.py:67-68, test_gpu_batch.py:40-41).  The PCG
        # routes: 2e-4, test_gpu_batch.py:200's bound for a PCG variant's x against the oracle with the same settings (no test there compares such a
        # route's y with the oracle: the same number)
        exact = name in ('direct', 'wave')
        tol = 1e-7 if exact else 2e-4
        for tag, (x, y, rec), ref in (('cold', runs[0], cold), ('warm', runs[1], warm)):
            it = [int(r[2].iter) for r in ref]
            ex = [np.abs(x[b] - ref[b][0]).max() / (1 + np.abs(ref[b][0]).max()) for b in range(4)]
            ey = [np.abs(y[b] - ref[b][1]).max() / (1 + np.abs(ref[b][1]).max()) for b in range(4)]
            print(name, tag, 'iterations', rec[:, 1].tolist(), 'oracle', it, '|dx|', ['%.1e' % e for e in ex], '|dy|', ['%.1e' % e for e in ey])
            assert (rec[:, 0] == int(S.OSQP_SOLVED)).all(), (name, tag, rec[:, 0])
            if exact:
                assert [int(v) for v in rec[:, 1]] == it, (name, tag, rec[:, 1], it)
            assert max(ex) <= tol and max(ey) <= tol, (name, tag, ex, ey)
    # the two PCG routes stop every element at the same iteration, cold and warm
    for k in (0, 1):
        assert np.array_equal(res['generic'][k][2][:, 1], res['lockstep'][k][2][:, 1])
