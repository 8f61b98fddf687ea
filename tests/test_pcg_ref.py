"""CPU tier of the kernel-level tests of the PCG forms (tests/pcg_ref.py: reference, bound, judge; tests/test_gpu_pcg_kernels.py is the GPU tier).
The reference is guarded on its own -- against a dense long-double solve of K x = rhs and against oracle.py's first iterate --; the judge runs through
the REAL entry osqp_hip_test_admm on the host simulator (three-kernel form on plain loops) with every run of the GPU tier; the fp64 twin stays below 1/8
of every bound at every shape the GPU tier uses; twelve planted mistakes in a numpy stand-in are each rejected at those shapes; and the host side of the
entry runs as a stand-alone program under the host sanitizers (tests/hostsim/admm_entry_probe.cpp)."""
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import hostsim_build
import pcg_ref as R
from hostsim_util import hostsim

warnings.simplefilter('ignore')
L = np.longdouble
SIGMA, ALPHA = 1e-6, 1.6


# ------------------------------------------------------------------------------------------------------------------------------ guards on the reference
def _guard_problem():
    import problems
    P, q, A, l, u = problems.random_qp(40, 70)
    l, u = R.with_free_rows(l, u)
    eq = np.arange(70) % 10 == 6
    u[eq] = l[eq]                                             # equality rows too: all three row classes
    return P, q, A, l, u


def _reference_rho(l, u, rho=0.1):
    """the reference's rho rule (_osqp.py:505-522): 1e-6 on free rows, 1e3 rho on equality rows, rho elsewhere"""
    free = np.isinf(l) & np.isinf(u)
    return np.where(free, 1e-6, np.where(u - l < 1e-4, 1e3 * rho, rho))


def test_reference_pcg_equals_a_dense_long_double_solve():
    """With a large cap the reference's x~ is the solution of K x = rhs.  The issue asks for 1e-25 relative; np.longdouble on x86 carries 64 bits
    (eps = 1.08e-19), where no solve of either kind can hold 1e-25: the guard is 1e-25 where the format carries it (eps <= 1e-30), otherwise
    256 eps cond_2(K) -- what a backward-stable solve of K loses -- which is 6e-15 or better here: nine orders below anything the fp64 kernels resolve."""
    P, q, A, l, u = _guard_problem()
    s = R.Scaled(P, q, A, l, u, np.ones(40), np.ones(70), 1.0, SIGMA, ALPHA, 0.9)
    rho = _reference_rho(l, u)
    start = R.starts(s, 3)
    r = R.admm(s, rho, start, 1, 400, 0.0, 0.0, L, 'host')
    x, z, y, xt = (np.asarray(a, dtype=L) for a in start)
    rhs = L(SIGMA) * x - np.asarray(s.q, dtype=L) + np.asarray(s.A.todense(), dtype=L).T @ (np.asarray(rho, dtype=L) * z - y)
    K = R.dense_K(s, rho)
    want = R.dense_solve_L(K, rhs)
    eps = float(np.finfo(L).eps)
    cond = float(np.linalg.cond(np.asarray(K, dtype=np.float64)))
    bound = 1e-25 if eps <= 1e-30 else 256 * eps * cond
    err = float(np.abs(r['xt'] - want).max() / np.abs(want).max())
    print('dense guard: relative error %.3e, bound %.3e (eps %.3e, cond %.3e), PCG iterations %d' % (err, bound, eps, cond, r['used'][0]))
    assert bound <= 1e-13 and err <= bound, (err, bound)
    assert float(np.abs(K @ want - rhs).max() / np.abs(rhs).max()) <= 64 * eps              # the dense solve itself


@pytest.mark.parametrize('scaling', [0, 10])
def test_one_reference_iteration_equals_the_oracle_after_one_iteration(scaling):
    """oracle.py solves its linear system exactly (LDL' of the KKT matrix); the reference with a PCG run to convergence is then the same iterate:
    x, y after max_iter = 1 from a cold start, to fp64 accuracy (1e-9 relative: cond(K) 1e3 times the oracle's fp64 factorisation error)."""
    from oracle import Oracle
    P, q, A, l, u = _guard_problem()
    o = Oracle().setup(P, q, A, l, u, scaling=scaling, max_iter=1, check_termination=0, adaptive_rho=0, warm_start=0, rho=0.1, sigma=SIGMA, alpha=ALPHA)
    xo, yo, info = o.solve()
    D, E, c = o.scaling()
    s = R.Scaled(P, q, A, l, u, D, E, c, SIGMA, ALPHA, 0.9)
    rho = _reference_rho(s.l, s.u)
    zero = (np.zeros(s.n), np.zeros(s.m), np.zeros(s.m), np.zeros(s.n))
    r = R.admm(s, rho, zero, 1, 600, 0.0, 1e-17, L, 'host')
    assert r['done'][0]
    x = D * np.asarray(r['x'], dtype=np.float64)
    y = E * np.asarray(r['y'], dtype=np.float64) / c
    assert info.iter == 1 and np.isfinite(xo).all()
    ex, ey = np.abs(x - xo).max() / np.abs(xo).max(), np.abs(y - yo).max() / np.abs(yo).max()
    print('oracle guard (scaling %d): |dx| %.3e |dy| %.3e' % (scaling, ex, ey))
    assert ex <= 1e-9 and ey <= 1e-9, (ex, ey)


# ------------------------------------------------------------------------------------------------------------------------------ the judge through the real entry
_states = {}


def state_of(name, which='base'):
    """The runs of a case's state with the host simulator's scaling and rho (cached: the reference is computed once)."""
    key = (name, which)
    if key not in _states:
        P, q, A, l, u = R.problem(name)
        with hostsim():
            import osqp_amd
            m = osqp_amd.OSQP(algebra='hip')
            m.setup(P, q, A if A.shape[0] else None, l if A.shape[0] else None, u if A.shape[0] else None, **R.SETTINGS)
            sv = m._solver
            if which == 'rho':
                m.update_settings(rho=R.RHO_UPDATE)
            if which == 'mat':
                Px, pi, Ax, ai, P, A = R.updated_matrices(P, A)
                m.update(Px=Px, Px_idx=pi, Ax=Ax, Ax_idx=ai)
            s = R.scaled_of(sv, P, q, A, l, u, SIGMA, ALPHA)
            st, out = sv.hip_test_admm(*R.starts(s, R.SEED), 1, 0)
            assert st == 0 and out['form'] == 0
            _states[key] = (R.StateRuns(s, out['rho'], R.SEED), m)
    return _states[key]


@pytest.mark.parametrize('name', R.HOSTSIM_CASES + ('unconstrained_50',))
def test_judge_through_the_entry_on_the_host_simulator(name):
    worst = R.Worst()
    with hostsim():
        state, m = state_of(name)
        assert m._solver.hip_test_admm(*state.start, 1, 1)[1]['form'] == 0
        for run in state.all_runs('host'):
            run.check_twin()
        R.check_state(m._solver.hip_test_admm, state, 'host', worst, '%s, host simulator' % name, form=0)
        for which in ('rho', 'mat'):
            if name == 'unconstrained_50' and which == 'rho':
                continue
            st2, m2 = state_of(name, which)
            R.check_state(m2._solver.hip_test_admm, st2, 'host', worst, '%s after %s update, host simulator' % (name, which), form=0, pairs=((3, 3),), stop=False, repeat=False)
    print('%s: worst ratio to the bound %s' % (name, {k: round(v, 4) for k, v in worst.items()}))


def test_entry_validates_before_it_runs_and_leaves_a_cold_start_possible():
    P, q, A, l, u = R.problem('random_50x100')
    with hostsim():
        import osqp_amd
        state, m = state_of('random_50x100')
        sv = m._solver
        ok = lambda **kw: sv.hip_test_admm(*state.start, **kw)
        for bad in (dict(iters=0), dict(iters=9), dict(cap=-1), dict(cap=17), dict(tol_rel=-1.0), dict(tol_abs=np.nan), dict(tol_abs=np.inf),
                    dict(lens=dict(n_len=49)), dict(lens=dict(m_len=101)), dict(cap=2, lens=dict(hist_len=5))):
            st, out = ok(**bad)
            assert st == R.VALIDATION and all(np.isnan(out[k]).all() for k in R.N_OUT + R.M_OUT), bad
        # a solve after the entry cold-starts (warm_starting = 0) and equals a fresh handle's bit for bit
        ok(iters=3, cap=4)
        r1 = m.solve()
        f = osqp_amd.OSQP(algebra='hip'); f.setup(P, q, A, l, u, **R.SETTINGS)
        r2 = f.solve()
        assert r1.info.iter == r2.info.iter and np.array_equal(r1.x, r2.x) and np.array_equal(r1.y, r2.y)


# ------------------------------------------------------------------------------------------------------------------------------ planted mistakes
def _gpu_shapes():
    return tuple(R.CASES)                                      # every shape of tests/test_gpu_pcg_kernels.py


@pytest.mark.parametrize('name', R.HOSTSIM_CASES)
def test_standin_without_a_mistake_passes(name):
    state, _ = state_of(name)
    for fam in ('host', 'slot'):
        R.check_state(R.Standin(state.s, state.rho, fam), state, fam, R.Worst(), '%s stand-in' % name, repeat=False)


@pytest.mark.parametrize('plant', R.PLANTS)
def test_judge_rejects_a_planted_mistake_at_every_shape_of_the_gpu_tier(plant):
    """What the GPU tier's green run is worth: each stand-in differs from a correct one in one place, and the judge refuses it in both families of
    forms at every shape (a shape without constraints has no A' to drop a column from)."""
    for name in _gpu_shapes():
        state, _ = state_of(name)
        if state.s.m == 0 and plant in ('far_column_dropped', 't0_stale', 'y_without_old_z'):
            continue
        for fam in ('host', 'slot'):
            with pytest.raises(AssertionError, match='against the tolerance'):
                R.check_state(R.Standin(state.s, state.rho, fam, plant=plant), state, fam, R.Worst(), '%s stand-in with %s' % (name, plant), repeat=False)


def test_fp64_twin_stays_below_an_eighth_of_every_bound_at_every_shape():
    for name in _gpu_shapes():
        state, _ = state_of(name)
        for fam in ('host', 'slot'):
            for run in state.all_runs(fam):
                run.check_twin()
                # the unit stays small against the signal.  The stop-rule runs start 1e6 ||rhs|| away from the solution and cancel that again: two more
                # orders on their vectors; their ||r_0|| and gamma / alpha belong to PCGs that start (nearly) converged -- what is left of a cancellation
                # has no digits to hold to, and the judge's bound for them follows the twin's own loss
                keys = list(run.e64) if run.tol_abs == 0.0 else [k for k in run.e64 if k in R.N_OUT + R.M_OUT]
                assert max(run.e64[k] for k in keys) <= (1e-9 if run.tol_abs == 0.0 else 1e-7), (name, run.label(), run.e64)


# ------------------------------------------------------------------------------------------------------------------------------ the entry's host side under the sanitizers
def test_admm_entry_probe_is_clean_under_the_host_sanitizers(tmp_path):
    """tests/hostsim/admm_entry_probe.cpp: a stand-alone program (own main) over the product's host driver and the host simulator, compiled with
    -fsanitize=address,undefined: every validation branch, the permuted POKE / PEEK copies and the run itself."""
    cxx = shutil.which('g++')
    assert cxx, 'g++ is needed to build the probe'
    exe = str(tmp_path / 'admm_entry_probe')
    src = [os.path.join(hostsim_build.ROOT, 'tests', 'hostsim', 'admm_entry_probe.cpp')] + hostsim_build.SRCS
    subprocess.check_call([cxx, '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-o', exe] + src)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'admm_entry_probe OK' in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
