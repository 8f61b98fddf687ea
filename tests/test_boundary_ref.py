"""CPU tier of the kernel-level tests of the chunk boundary (tests/boundary_ref.py: reference, bounds, batteries; tests/test_gpu_boundary_kernels.py is the
GPU tier).  The mode 0 battery runs through the REAL entry osqp_hip_test_boundary on the host simulator -- tests/hostsim/backend_host.cpp states the same
quantities on plain loops, independently of the reference --; a numpy stand-in without a mistake passes the batteries at every shape of the GPU tier and
with each of nine planted mistakes is rejected at every one of them; the fp64 twin stays below 1/8 of every bound; the inputs of the device-driven
scenarios put the two sides of every comparison that decides them a factor 2 apart; the entry validates before it runs, leaves a cold start possible, and
its host side runs as a stand-alone program under the host sanitizers (tests/hostsim/boundary_entry_probe.cpp)."""
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import boundary_ref as B
import hostsim_build
import pcg_ref as R
from hostsim_util import hostsim

warnings.simplefilter('ignore')
SIGMA, ALPHA = 1e-6, 1.6
GPU_SHAPES = ('random_50x100', 'banded_1537x2999', 'lasso_60x300', 'unstructured_3000', 'unconstrained_50', 'f1_D2', 'kform_333')      # tests/test_gpu_boundary_kernels.py's
_data = {}


def sim_handle(name, **over):
    P, q, A, l, u = R.problem(name)
    import osqp_amd
    m = osqp_amd.OSQP(algebra='hip')
    none = A.shape[0] == 0
    m.setup(P, q, None if none else A, None if none else l, None if none else u, **{**R.SETTINGS, **over})
    return m


def data_of(name, scaling=10):
    """the scaled problem of a shape with the host simulator's scaling (cached)"""
    key = (name, scaling)
    if key not in _data:
        with hostsim():
            m = sim_handle(name, scaling=scaling)
            _data[key] = (B.data_of(m._solver, *R.problem(name), SIGMA, ALPHA), m)
    return _data[key]


def test_names_are_the_engines_order():
    with hostsim():
        _, m = data_of('random_50x100')
        assert tuple(m._solver.hip_res_names()) == B.NAMES


@pytest.mark.parametrize('name,scaling', [(nm, 10) for nm in R.HOSTSIM_CASES + ('unconstrained_50',)] + [('random_50x100', 0)])
def test_mode0_battery_through_the_entry_on_the_host_simulator(name, scaling):
    worst = R.Worst()
    with hostsim():
        d, m = data_of(name, scaling)
        sv = m._solver
        spmv = lambda v: sv.hip_test_spmv(1, v)
        calls = B.check_mode0(sv.hip_test_boundary, spmv, d, worst, '%s scaling %d, host simulator' % (name, scaling))
    print('%s scaling %d: %d calls, worst ratio to the bound %s' % (name, scaling, calls, {k: round(v, 4) for k, v in worst.items()}))


def test_entry_validates_before_it_runs_and_leaves_a_cold_start_possible():
    P, q, A, l, u = R.problem('random_50x100')
    with hostsim():
        d, m = data_of('random_50x100')
        sv = m._solver
        vec = B.draw(d, 5)
        for bad in (dict(mode=2), dict(mode=-1), dict(need=4), dict(need=-1), dict(unscaled=2), dict(keep=2), dict(thr=-1.0), dict(thr=np.nan), dict(thr=np.inf),
                    dict(lens=dict(n_len=49)), dict(lens=dict(m_len=101)), dict(lens=dict(res_len=27)), dict(lens=dict(res_len=29)),
                    dict(mode=1, groups=0), dict(mode=1, groups=3), dict(mode=1, at_check=2), dict(mode=1, chunk_done=-1), dict(mode=1, status_in=3), dict(mode=1, iter=-1)):
            st, out = B.call(sv.hip_test_boundary, vec, **bad)
            assert st == B.VALIDATION and np.isnan(out['res_vec']).all() and all(np.isnan(out[k]).all() for k in ('rho', 'v', 'xg', 'Minv')), bad
        st, out = B.call(sv.hip_test_boundary, vec, mode=1, iter=50)          # the device-driven group does not exist on the host simulator
        assert st == B.NOT_IMPLEMENTED and np.isnan(out['res_vec']).all()
        # a solve after the entry cold-starts (warm_starting = 0) and equals a fresh handle's bit for bit
        st, out = B.call(sv.hip_test_boundary, vec, need=3, thr=0.5)
        assert st == 0
        r1 = m.solve()
        r2 = sim_handle('random_50x100').solve()
        assert r1.info.iter == r2.info.iter and np.array_equal(r1.x, r2.x) and np.array_equal(r1.y, r2.y)


# ------------------------------------------------------------------------------------------------------------------------------ stand-in and planted mistakes
def _battery(d, plant, where):
    """everything the GPU tier asks of a handle, asked of the stand-in"""
    sd = B.Standin(d, plant)
    B.check_mode0(sd, sd.spmv, d, R.Worst(), where)


def _rho_battery(d, plant, where):
    if d.m == 0:
        return
    vec = B.draw(d, 7)
    rho_old = B.rho_vector(d, 0.1, np.full(d.m, 1.0), 0.1)                     # (equality weight 10)
    sd = B.Standin(d, plant, rho=rho_old, rho_bar=0.1)
    B.check_rho_change(sd.rho_change(vec, 0.37), d, vec, 0.37, rho_old, 0.1, True, R.Worst(), where)


@pytest.mark.parametrize('name', GPU_SHAPES)
def test_standin_without_a_mistake_passes_and_the_twin_stays_below_an_eighth(name):
    d, _ = data_of(name)
    _battery(d, None, '%s stand-in' % name)                                    # (check_mode0 asserts the twin's eighth on its dense draw)
    _rho_battery(d, None, '%s stand-in' % name)
    for seed in (11, 12, 13):
        vec = B.draw(d, seed)
        B.Ref(d, vec, B.L, 3, 0.75, 1).check_twin(B.Ref(d, vec, np.float64, 3, 0.75, 1))


@pytest.mark.parametrize('plant', B.PLANTS)
def test_a_planted_mistake_is_rejected_at_every_shape_of_the_gpu_tier(plant):
    for name in GPU_SHAPES:
        d, _ = data_of(name)
        if d.m == 0 and plant in ('support_l_u_swapped', 'v_from_old_rho', 'ztg_not_reset'):
            continue                                                           # (no row to swap bounds on, no rho vector)
        with pytest.raises(AssertionError, match='against the tolerance'):
            if plant in ('v_from_old_rho', 'ztg_not_reset'):
                _rho_battery(d, plant, '%s stand-in with %s' % (name, plant))
            else:
                _battery(d, plant, '%s stand-in with %s' % (name, plant))


# ------------------------------------------------------------------------------------------------------------------------------ the inputs of the device-driven scenarios
LOOSE = dict(eps_abs=1e-3, eps_rel=1e-3)


@pytest.mark.parametrize('name', GPU_SHAPES)
def test_scenario_inputs_decide_every_comparison_by_a_factor_two(name):
    """What tests/test_gpu_boundary_kernels.py pokes in mode 1, judged by the reference's reading of the rules (boundary_ref.Rules): converged iterates pass
    every residual test with a factor 2 to spare, the far point fails them by as much and asks for a rho update no rounding can undo, the certificates hold
    (or, spoiled, fail) by a factor 2, the NaN point is NON_CVX."""
    with hostsim():
        d, m = data_of(name)
        sol = sim_handle(name).solve()                          # (whatever its status: scenario_expectation judges the point)
    tight = dict(scaling=10, **{k: R.SETTINGS[k] for k in LOOSE})
    if np.isfinite(sol.x).all():                                # (lasso_60x300 with a tenth of its rows freed is unbounded: no converged point to poke)
        vec, _ = B.scenario(d, 'c', sol=(sol.x, sol.y if d.m else None))
        B.scenario_expectation(d, 'c', vec, dict(scaling=10, **LOOSE), 0.1)
    else:
        assert name == 'lasso_60x300'
    for which in ('d', 'h'):
        vec, _ = B.scenario(d, which)
        B.scenario_expectation(d, which, vec, dict(scaling=10, **LOOSE), 0.1)
    if d.m == 0:
        return
    P, q, A, l, u, j0 = B.variant_problem(*R.problem(name))
    with hostsim():
        import osqp_amd
        mv = osqp_amd.OSQP(algebra='hip'); mv.setup(P, q, A, l, u, **R.SETTINGS)
        dv = B.data_of(mv._solver, P, q, A, l, u, SIGMA, ALPHA)
    for which in ('e', 'e2', 'f'):
        vec, _ = B.scenario(dv, which, j0=j0)
        ref, ru = B.scenario_expectation(dv, which, vec, tight, 0.1)
        assert (ru.need == B.NEED_DINF) == (which == 'f')


# ------------------------------------------------------------------------------------------------------------------------------ the entry's host side under the sanitizers
def test_boundary_entry_probe_is_clean_under_the_host_sanitizers(tmp_path):
    """tests/hostsim/boundary_entry_probe.cpp: a stand-alone program (own main) over the product's host driver and the host simulator, compiled with
    -fsanitize=address,undefined: every validation branch, the permuted POKE / PEEK copies and mode 0 itself."""
    cxx = shutil.which('g++')
    assert cxx, 'g++ is needed to build the probe'
    exe = str(tmp_path / 'boundary_entry_probe')
    src = [os.path.join(hostsim_build.ROOT, 'tests', 'hostsim', 'boundary_entry_probe.cpp')] + hostsim_build.SRCS
    subprocess.check_call([cxx, '-O1', '-g', '-std=c++17', '-Wall', '-Wextra', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-o', exe] + src)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'boundary_entry_probe OK' in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
