"""GPU tier, kernel level: the CHUNK BOUNDARY of a single-QP solve (osqp-python_amd/csrc/backend_hip.hip) -- the residual kernels k_res_m / k_res_n and
their two-level fold put_partial -> k_res_final, the second stage of the infeasibility tests k_inf_primal / k_inf_dual_p / k_inf_dual_a, what follows a rho
change (k_set_rho, k_init_guess, k_precond, k_kf_values) and the device-driven group ctl_group, whose kernels decide for themselves whether to act and whose
k_decide runs the rules of csrc/policy.h -- against the long-double reference of tests/boundary_ref.py (reference, derived bounds, batteries;
tests/test_boundary_ref.py proves them on the CPU and shows nine planted mistakes rejected).  The diagnostic entry osqp_hip_test_boundary pokes seven scaled
vectors into a set-up handle, runs the boundary (mode 0: the host-synchronous launches; mode 1: the group as a device-driven solve enqueues it) and peeks
the residual block, the vectors a rho change writes and the state block, the latter next to the HOST's compilation of the same rules.

Mode 0, every shape: a dense seeded draw within the bounds (a repeat and an eager handle bit-identical), one-hot dy / dx at the first row, the last row and
the longest row with EXACT expectations, one entry of z / x scaled by 2^40, a NaN in x / y at the first and the last position, and the violation count
with both scalings.  Mode 1, forms 2, 3, 4: the scenarios of boundary_ref.check_mode1 (chunk unfinished; finished between checks; converged; a rho update,
once and with a second group that must change nothing, then osqp_hip_test_admm at the new rho judged by tests/pcg_ref.py; the solve already over; NaN) on
the shape's own problem, and the certificate scenarios of check_certificates (primal certificate, the same spoiled, dual certificate) on
boundary_ref.variant_problem of it (lasso_60x300 with a tenth of its rows freed is unbounded: it has no converged point and runs every scenario but that one).  Every case asserts the form it landed on; in every scenario the device's state block equals the host's field by field."""
import ctypes
import warnings

import numpy as np
import pytest

import boundary_ref as B
import osqp_amd
import pcg_ref as R
import util

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
SIGMA, ALPHA, RHO = 1e-6, 1.6, 0.1
LOOSE = dict(eps_abs=1e-3, eps_rel=1e-3)

BASE = dict(woodbury=0, small_direct=0, reorder=0, window=1, graph=1, kform=0)
FORM_POLICY = {0: dict(pcg_fused=0, slots=0, f1=0), 2: dict(pcg_fused=1, slots=1, f1=0), 3: dict(pcg_fused=1, slots=1, f1=1), 4: dict(pcg_fused=1, slots=1, f1=0, kform=1)}
VARIANT = {'': {}, 'window0': dict(window=0), 'reorder2': dict(reorder=2), 'graph0': dict(graph=0)}
# (shape, form, variant, scaling)
MODE0 = [('random_50x100', 2, '', 10), ('random_50x100', 2, '', 0), ('banded_1537x2999', 2, '', 10), ('banded_1537x2999', 2, 'window0', 10), ('lasso_60x300', 2, '', 10),
         ('unstructured_3000', 2, '', 10), ('unconstrained_50', 2, '', 10), ('f1_D2', 3, '', 10), ('f1_D2', 3, 'reorder2', 10), ('kform_333', 4, '', 10)]
MODE1 = [('random_50x100', 2, '', 10), ('random_50x100', 2, '', 0), ('banded_1537x2999', 2, '', 10), ('banded_1537x2999', 2, 'graph0', 10), ('lasso_60x300', 2, '', 10),
         ('unstructured_3000', 2, '', 10), ('unconstrained_50', 2, '', 10), ('f1_D2', 3, '', 10), ('f1_D2', 3, 'reorder2', 10), ('kform_333', 4, '', 10)]
CERT = [c for c in MODE1 if c[0] != 'unconstrained_50' and c[3] == 10]
_handles, _variants = {}, {}


def case_id(c):
    return '%s-form%d%s-scaling%d' % (c[0], c[1], '-' + c[2] if c[2] else '', c[3])


def setup_handle(prob, form, variant, scaling):
    """a fresh handle: the form's policy as the thread's default while osqp_setup runs"""
    from osqp_amd import _lib
    h = _lib.handle()
    P, q, A, l, u = prob
    pol = _lib.PolicyStruct()
    h.osqp_hip_default_policy(ctypes.byref(pol))
    for k, v in {**BASE, **FORM_POLICY[form], **VARIANT[variant]}.items():
        setattr(pol, k, v)
    h.osqp_hip_set_default_policy(ctypes.byref(pol))
    try:
        m = osqp_amd.OSQP(algebra='hip')
        none = A.shape[0] == 0
        m.setup(P, q, None if none else A, None if none else l, None if none else u, **{**R.SETTINGS, 'scaling': scaling})
    finally:
        h.osqp_hip_set_default_policy(None)
    return m


def handle_of(case):
    """(handle, data) of a case, built once per module"""
    if case not in _handles:
        shape, form, variant, scaling = case
        m = setup_handle(R.problem(shape), form, variant, scaling)
        _handles[case] = (m, B.data_of(m._solver, *R.problem(shape), SIGMA, ALPHA))
    return _handles[case]


def variant_of(case):
    if case not in _variants:
        shape, form, variant, scaling = case
        P, q, A, l, u, j0 = B.variant_problem(*R.problem(shape))
        m = setup_handle((P, q, A, l, u), form, variant, scaling)
        _variants[case] = (m, B.data_of(m._solver, P, q, A, l, u, SIGMA, ALPHA), j0)
    return _variants[case]


def entry_of(m, form, where):
    sv = m._solver

    def entry(*a, **kw):
        st, out = sv.hip_test_boundary(*a, **kw)
        if st == 0:
            assert out['form'] == form, 'the handle runs the %s form, not the %s form (%s)' % (R.FORM_NAME.get(out['form']), R.FORM_NAME[form], where)
        return st, out
    return entry


def report(test, case, worst):
    print('%s: worst ratio to the bound %s' % (case_id(case), {k: round(v, 4) for k, v in sorted(worst.items())}))
    util.record_deviation(test, case_id(case), **{k: float(v) for k, v in worst.items()})


@pytest.mark.parametrize('case', MODE0, ids=case_id)
def test_mode0_residuals_fold_and_second_stage_against_the_long_double_reference(case):
    m, d = handle_of(case)
    where = case_id(case)
    sv = m._solver
    assert tuple(sv.hip_res_names()) == B.NAMES
    other = None
    if case == ('banded_1537x2999', 2, '', 10):
        other = entry_of(handle_of(('banded_1537x2999', 2, 'graph0', 10))[0], 2, where + ' graph0')
    worst = R.Worst()
    calls = B.check_mode0(entry_of(m, case[1], where), lambda v: sv.hip_test_spmv(1, v), d, worst, where, other=other)
    assert calls >= 6
    report('boundary_mode0', case, worst)


@pytest.mark.parametrize('case', MODE1, ids=case_id)
def test_mode1_device_driven_group_equals_the_host_rules_and_the_reference(case):
    shape, form, variant, scaling = case
    m, d = handle_of(case)
    where = case_id(case)
    sv = m._solver
    entry = entry_of(m, form, where)
    sol = setup_handle(R.problem(shape), form, variant, scaling).solve()      # (whatever its status: check_mode1 judges the point by the reference before it is poked)
    m.update_settings(**LOOSE)
    settings = dict(scaling=scaling, **LOOSE)
    worst = R.Worst()
    try:
        point = (sol.x, sol.y if d.m else None) if np.isfinite(sol.x).all() else None      # (lasso_60x300 with a tenth of its rows freed is unbounded: no scenario c)
        assert point is not None or shape == 'lasso_60x300'
        vec, kw, out_d = B.check_mode1(entry, d, settings, RHO, True, worst, where, sol=point, tight_factor=sv.get_policy()['rho_window_tol'])
        if d.m:
            # keep = 1: the handle adopts the new rho; the PCG forms run at it (k_precond / k_kf_values with cond = 1 gave them Minv and K)
            st, out = B.call(entry, vec, keep=1, **kw)
            assert st == 0 and np.array_equal(out['rho'], out_d['rho'])
            s = R.scaled_of(sv, *R.problem(shape), SIGMA, ALPHA)
            state = R.StateRuns(s, out['rho'], R.SEED)
            w2 = R.Worst()
            R.check_state(sv.hip_test_admm, state, R.FORM_FAMILY[form], w2, where + ' after the group\'s rho update', form=form, pairs=((3, 3),), stop=False, repeat=False)
            worst.update({'admm.' + k: v for k, v in w2.items()})
    finally:
        m.update_settings(rho=RHO, **{k: R.SETTINGS[k] for k in LOOSE})
    report('boundary_mode1', case, worst)


@pytest.mark.parametrize('case', CERT, ids=case_id)
def test_mode1_infeasibility_certificates(case):
    shape, form, variant, scaling = case
    m, d, j0 = variant_of(case)
    where = case_id(case) + ' variant'
    worst = R.Worst()
    B.check_certificates(entry_of(m, form, where), d, dict(scaling=scaling, **{k: R.SETTINGS[k] for k in LOOSE}), RHO, j0, worst, where)
    report('boundary_certificates', case, worst)


@pytest.mark.parametrize('case', [('banded_1537x2999', 2, '', 10), ('f1_D2', 3, '', 10)], ids=case_id)
def test_a_solve_after_the_entry_is_the_solve_of_a_fresh_handle(case):
    """keep = 0: the group's rho update is taken back; with warm_starting = 0 the next osqp_solve is a fresh handle's bit for bit."""
    shape, form, variant, scaling = case
    m = setup_handle(R.problem(shape), form, variant, scaling)
    d = handle_of(case)[1]
    vec, kw = B.scenario(d, 'd')
    st, out = B.call(m._solver.hip_test_boundary, vec, **kw)
    assert st == 0 and out['form'] == form and out['dev']['rho_flag'] == 1
    r1 = m.solve()
    r2 = setup_handle(R.problem(shape), form, variant, scaling).solve()
    assert r1.info.status_val == r2.info.status_val and r1.info.iter == r2.info.iter and r1.info.rho_updates == r2.info.rho_updates
    assert np.array_equal(r1.x, r2.x) and np.array_equal(r1.y, r2.y)


def test_entry_refuses_what_it_cannot_run():
    import problems
    m0 = setup_handle(R.problem('random_50x100'), 0, '', 10)                  # no slot form: mode 0 runs, mode 1 does not exist
    d = handle_of(('random_50x100', 2, '', 10))[1]
    vec = B.draw(d, 3)
    st, out = B.call(m0._solver.hip_test_boundary, vec, need=3, thr=0.5)
    assert st == 0 and out['form'] == 0
    B.judge(out, st, B.Ref(d, vec, B.L, 3, 0.5, 0), R.Worst(), 'random_50x100 form 0')
    st, out = B.call(m0._solver.hip_test_boundary, vec, mode=1, iter=50)
    assert st == B.NOT_IMPLEMENTED and np.isnan(out['res_vec']).all()
    P, q, A, l, u = problems.portfolio_qp(200, 10)
    mw = osqp_amd.OSQP(algebra='hip'); mw.setup(P, q, A, l, u, verbose=False)
    if int(mw._solver.hip_stats()['woodbury_rows']) > 0:
        z = [np.zeros(len(q))] * 3 + [np.zeros(len(l))] * 4
        st, out = mw._solver.hip_test_boundary(*z, mode=1, iter=50)
        assert st == B.NOT_IMPLEMENTED and np.isnan(out['res_vec']).all()
    m2 = handle_of(('random_50x100', 2, '', 10))[0]
    for bad in (dict(mode=2), dict(need=4), dict(thr=-1.0), dict(lens=dict(n_len=51)), dict(lens=dict(res_len=27)), dict(mode=1, groups=3), dict(mode=1, status_in=3)):
        st, out = B.call(m2._solver.hip_test_boundary, vec, **bad)
        assert st == B.VALIDATION and np.isnan(out['res_vec']).all() and np.isnan(out['rho']).all(), bad
