"""The approximate-termination branch: when max_iter is reached the reference repeats its termination test with
every tolerance multiplied by 10 and reports *_INACCURATE statuses (/root/reference/src/osqppurepy/_osqp.py:1018-1022 the x10,
:1053-1075 the three outcomes, :1264-1266 the call at max_iter; status names bindings.cpp.in:350-360).

For each of the three outcomes the ORACLE is scanned over max_iter = 1, 2, ... (check_termination = 1) for the window of iteration
limits at which it reports the inaccurate status -- residuals / certificate between eps and 10 eps -- and the engine is run with the
limit in the middle of that window: same status as the oracle, through the host simulator (CPU tier), the one-launch direct path
('hip'), the multi-kernel PCG engine ('hip-pcg') and the batch kernel (GPU tier)."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_amd
import oracle as O
import problems
from backend_param import BACKENDS, engine
from oracle import Oracle

warnings.simplefilter('ignore')
S = osqp_amd.SolverStatus


def _solved_case():
    P, q, A, l, u = problems.random_qp()                      # BASELINE configs[0]
    return (P, q, A, l, u), dict(eps_abs=1e-5, eps_rel=1e-5, eps_prim_inf=1e-4, eps_dual_inf=1e-4), O.SOLVED_INACCURATE, O.SOLVED


def _primal_infeasible_case():
    n, m = 20, 30                                             # box on x + sum(x) >= 3n: infeasible, certificate converges gradually
    rng = np.random.default_rng(3)
    M = sp.random(n, n, 0.3, random_state=1, format='csc')
    P = (M @ M.T + 1e-2 * sp.eye(n)).tocsc()
    q = rng.standard_normal(n)
    A = sp.vstack([sp.random(m - n - 1, n, 0.4, random_state=2), sp.eye(n), sp.csr_matrix(np.ones((1, n)))]).tocsc()
    l = np.r_[-np.ones(m - n - 1), -np.ones(n), 3.0 * n]
    u = np.r_[np.ones(m - n - 1), np.ones(n), 4.0 * n]
    return (P, q, A, l, u), dict(eps_abs=1e-9, eps_rel=1e-9, eps_prim_inf=1e-4, eps_dual_inf=1e-4), O.PRIMAL_INFEASIBLE_INACCURATE, O.PRIMAL_INFEASIBLE


def _dual_infeasible_case():
    n, m = 20, 30                                             # three variables without curvature, one-sided rows: unbounded below
    rng = np.random.default_rng(2)
    P = sp.diags(np.r_[np.ones(n - 3), np.zeros(3)]).tocsc()
    A = sp.vstack([sp.random(m - 5, n, 0.4, random_state=7), sp.eye(n, format='csr')[:5]]).tocsc()
    l = -np.ones(m)
    u = np.full(m, 1e30)
    q = rng.standard_normal(n)
    return (P, q, A, l, u), dict(eps_abs=1e-9, eps_rel=1e-9, eps_prim_inf=1e-4, eps_dual_inf=1e-4), O.DUAL_INFEASIBLE_INACCURATE, O.DUAL_INFEASIBLE


CASES = {'solved': _solved_case, 'primal_infeasible': _primal_infeasible_case, 'dual_infeasible': _dual_infeasible_case}
_window_cache = {}


def oracle_window(name):
    """(problem, settings, inaccurate status, [K_first, K_last]): the iteration limits at which the oracle ends in the inaccurate status."""
    if name not in _window_cache:
        prob, stg, inacc, exact = (CASES.get(name) or GAP_CASES[name])()
        win = []
        for K in range(1, 600):
            _, _, info = Oracle().setup(*prob, max_iter=K, check_termination=1, adaptive_rho=0, **stg).solve()
            if info.status_val == inacc:
                win.append(K)
            elif info.status_val == exact:
                break
        assert len(win) >= 5 and win == list(range(win[0], win[-1] + 1)), (name, win)
        _window_cache[name] = (prob, stg, inacc, win)
    return _window_cache[name]


def test_oracle_reports_every_inaccurate_status():
    """the checker itself: each window exists, is contiguous, and ends where the exact status begins"""
    for name in CASES:
        _, _, inacc, win = oracle_window(name)
        assert inacc in (O.SOLVED_INACCURATE, O.PRIMAL_INFEASIBLE_INACCURATE, O.DUAL_INFEASIBLE_INACCURATE)
        assert win[0] > 1


@pytest.mark.parametrize('backend', BACKENDS)
@pytest.mark.parametrize('name', list(CASES))
def test_inaccurate_status_at_max_iter(backend, name):
    prob, stg, inacc, win = oracle_window(name)
    K = (win[0] + win[-1]) // 2
    with engine(backend):
        m = osqp_amd.OSQP(algebra='hip')
        m.setup(*prob, max_iter=K, check_termination=1, adaptive_rho=False, verbose=False, cg_max_iter=200, cg_tol_fraction=0.01, **stg)
        r = m.solve()
        assert r.info.status_val == inacc, (name, backend, K, win[0], win[-1], r.info.status, r.info.iter)   # (the enums agree: bindings.cpp.in:349-361)
        assert r.info.iter == K
        if name == 'solved':
            assert np.isfinite(r.info.obj_val) and np.all(np.isfinite(r.x))
        elif name == 'primal_infeasible':
            assert r.info.obj_val == np.inf or r.info.obj_val >= 1e30
            assert np.all(np.isfinite(r.prim_inf_cert))
        else:
            assert r.info.obj_val == -np.inf or r.info.obj_val <= -1e30
            assert np.all(np.isfinite(r.dual_inf_cert))
        # one iteration past the window's end the exact status takes over (same handle: update_settings)
        m.update_settings(max_iter=win[-1] + 40)
        m.warm_start(x=np.zeros(len(prob[1])), y=np.zeros(len(prob[3])))
        r2 = m.solve()
        assert r2.info.status_val == inacc - 1, (name, backend, r2.info.status)


def _gap_decides_case():
    """random_qp(20, 30, seed=3) at the tolerances of 'solved': its duality gap converges behind its residuals.  In the first twelve limits of the
    oracle's window (169..180 of 169..217) both residual tests pass at 10 eps while |duality_gap| is still above 10 eps_abs + 10 eps_rel max(|obj_val|,
    |dual_obj_val|).  On 'solved' itself the gap leads the residuals by a factor of three to five wherever the residuals pass, at every ratio of
    eps_abs to eps_rel tried (1e-5 : 0 .. 1e-7 : 1e-4) and at rho = 1: no tolerance makes the gap test decide there."""
    P, q, A, l, u = problems.random_qp(20, 30, seed=3)
    return (P, q, A, l, u), dict(eps_abs=1e-5, eps_rel=1e-5, eps_prim_inf=1e-4, eps_dual_inf=1e-4), O.SOLVED_INACCURATE, O.SOLVED


GAP_CASES = {'solved': CASES['solved'], 'gap_decides': _gap_decides_case}


@pytest.mark.parametrize('name', list(GAP_CASES))
def test_dual_gap_in_the_approximate_pass(name):
    """check_dualgap = True on the host simulator, eps_abs = eps_rel = 1e-5: at max_iter = K the status is SOLVED_INACCURATE exactly when both residual
    tests pass at 10 eps AND |duality_gap| < 10 eps_abs + 10 eps_rel max(|obj_val|, |dual_obj_val|), else MAX_ITER_REACHED -- for every K of the
    oracle's window and the five below it.  The gap test is judged from the reported info fields.  The residual tests need normalisations that info
    does not carry (||A x||, ||z||, ...): they are judged by the same solve with check_dualgap = False, which stops at the same point (same iter,
    prim_res, dual_res, obj_val: asserted) and ends SOLVED_INACCURATE exactly when the two of them pass.
    'solved': both statuses occur (asserted), MAX_ITER_REACHED through the residuals below the window; the gap test passes at every K.
    'gap_decides': residuals pass with the gap passing AND residuals pass with the gap failing both occur (asserted): there the gap term alone
    turns SOLVED_INACCURATE into MAX_ITER_REACHED, which neither dropping it nor any other factor than 10 on its tolerances survives unnoticed
    (the gap crosses the threshold inside the window, so x1 and x100 move the crossing)."""
    prob, stg, inacc, win = oracle_window(name)
    assert inacc == O.SOLVED_INACCURATE
    kw = dict(check_termination=1, adaptive_rho=False, verbose=False, cg_max_iter=200, cg_tol_fraction=0.01, **stg)
    seen, combos = set(), {}
    with engine('hostsim'):
        with_gap, without = osqp_amd.OSQP(algebra='hip'), osqp_amd.OSQP(algebra='hip')
        with_gap.setup(*prob, max_iter=win[-1], check_dualgap=True, **kw)
        without.setup(*prob, max_iter=win[-1], check_dualgap=False, **kw)
        for K in range(win[0] - 5, win[-1] + 1):
            out = []
            for m in (with_gap, without):
                m.update_settings(max_iter=K)
                m.warm_start(x=np.zeros(len(prob[1])), y=np.zeros(len(prob[3])))
                out.append(m.solve().info)
            g, r = out
            assert g.iter == r.iter == K and g.prim_res == r.prim_res and g.dual_res == r.dual_res and g.obj_val == r.obj_val, (K, g.iter, r.iter)
            assert r.status_val in (O.SOLVED_INACCURATE, O.MAX_ITER_REACHED), (K, r.status)
            residuals_pass = r.status_val == O.SOLVED_INACCURATE
            gap_pass = abs(g.duality_gap) < 10 * stg['eps_abs'] + 10 * stg['eps_rel'] * max(abs(g.obj_val), abs(g.dual_obj_val))
            assert g.duality_gap == g.obj_val - g.dual_obj_val
            want = O.SOLVED_INACCURATE if residuals_pass and gap_pass else O.MAX_ITER_REACHED
            assert g.status_val == want, (K, g.status, residuals_pass, gap_pass, g.duality_gap)
            seen.add(g.status_val)
            combos.setdefault((residuals_pass, gap_pass), []).append(K)
    print(name, {k: (v[0], v[-1]) for k, v in combos.items()})
    assert seen == {O.SOLVED_INACCURATE, O.MAX_ITER_REACHED}, seen
    if name == 'gap_decides':
        assert (True, True) in combos and (True, False) in combos, combos
        # the gap crosses its threshold strictly inside the window: limits with the residuals passing lie on both sides of the crossing
        assert min(combos[(True, True)]) > min(combos[(True, False)]) >= win[0]


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CASES))
def test_inaccurate_status_in_the_batch_kernel(name):
    """the batch kernel carries its own copy of the x10 pass (batch_hip.hip): every member of a batch ends like the oracle"""
    prob, stg, inacc, win = oracle_window(name)
    P, q, A, l, u = prob
    K = (win[0] + win[-1]) // 2
    m = osqp_amd.OSQP(algebra='hip')
    m.setup(P, q, A, l, u, max_iter=K, check_termination=1, adaptive_rho=False, verbose=False, **stg)
    B = 6
    x, y, rec = m._solver.hip_batch_solve(q=np.tile(q, (B, 1)), nbatch=B)
    assert np.all(rec[:, 0] == inacc), rec[:, 0]
    assert np.all(rec[:, 1] == K)
