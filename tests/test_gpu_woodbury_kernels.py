"""GPU tier, kernel level: the Woodbury correction of osqp-python_amd/csrc/woodbury_hip.hip and the direct modes of wbdirect_hip.hip against
np.longdouble references (tests/wb_ref.py: cases, references, tolerances and where each comes from; tests/test_wb_ref.py proves that machinery on a
numpy stand-in and shows that it notices seven kinds of planted mistake).

APPLY tier: the diagnostic entry osqp_hip_test_woodbury runs wb_factor and wb_apply unchanged on a handle of the test and returns u = M^-1 r, x~,
1 / D0, S or T, its inverse, the rho vector and the PCG's partial results -- for the small form (r = 1 ... 128 long rows, n = 129 ... 257 on the edges of
k_wb_S's slices and unroll, K0 diagonal and not), the device-factorised row-space form (r = 129 ... 257 and 1030, where k_wb_gemv's unrolled loop
runs) and the column-space form (cd = 130, 131, 200 and 1540, where the even path of k_wbd_gemv reaches its main loop), as set up, after
update_settings(rho) and after update(Ax).  ITERATION tier: the direct modes that never call wb_apply after k = 1, 2, 3 ADMM iterations against the
textbook iteration in long double.

Every check is  err <= 64 max(e64, n 2^-53) scale  with e64 the error of a plain fp64 numpy evaluation against the same long-double reference.
Worst ratios to that tolerance measured on an MI355X: WORST below -- a record, asserted nowhere (the assertion is ratio <= 1);
every test prints its own.  No kernel bug was found: the kernels are as accurate as the fp64 numpy evaluation of the same formulas (every ratio is
below 0.13, i.e. 8 e64)."""
import numpy as np
import pytest

import wb_ref as R
from util import record_deviation

pytestmark = pytest.mark.gpu

# worst error / tolerance per quantity on an MI355X (apply tier: all cases of a form; iteration tier: all cases and both rho values of a form)
WORST = {
    'small': dict(Dinv0=1.1e-3, S=5.6e-4, Sinv=1.4e-2, u=2.1e-2, gamma=1.6e-2, xs=2.1e-2),
    'row': dict(Dinv0=1.6e-4, S=7.7e-4, Sinv=1.9e-2, u=2.7e-3, gamma=8.0e-4, xs=2.2e-3),
    'col': dict(Dinv0=6.3e-5, T=5.0e-4, Sinv=4.3e-3, u=1.4e-3, gamma=1.3e-3, xs=9.4e-4),
    'iterations': {'unfused': dict(x=0.039, y=0.13), 'two-launch': dict(x=0.029, y=0.10), 'one-launch': dict(x=0.017, y=0.0016), 'slots': dict(x=0.029, y=0.10),
                   'row-space': dict(x=0.013, y=0.0096), 'column-space-unfused': dict(x=0.055, y=0.041), 'column-space-fused-csr': dict(x=0.032, y=0.023),
                   'column-space-thin': dict(x=0.059, y=0.040), 'dense-block': dict(x=0.019, y=0.0065)},
}


def _big(c):
    return c.get('cd', 0) > 1000 or c['r'] > 1000


def _report(test, case, w):
    record_deviation(test, case, **{k + '_ratio': v for k, v in w.items()})
    print(case, {k: '%.2e' % v for k, v in w.items()}, 'e64', {k: '%.1e' % v for k, v in w.e64.items()})


@pytest.mark.parametrize('c', R.small_cases(), ids=R.case_id)
def test_small_form(c):
    """k_wb_diag, k_wb_S, k_wb_invert, k_wb_gather; k_wb_p1 / p2 / p3 with both parities and with and without the direct mode's x~ update"""
    _report('test_small_form', R.case_id(c), R.check_apply(R.Product(c), c))


@pytest.mark.parametrize('c', R.row_cases(), ids=R.case_id)
def test_device_factorised_row_space_form(c):
    """k_wb_fillW, the GEMM, k_wb_adddiag, the inverse, k_wb_symm, the two checks; k_wb_p1, k_wb_gemv, k_wb_p3.  (The r = 1030 case: as set up only --
    its references take seconds.)"""
    _report('test_device_factorised_row_space_form', R.case_id(c), R.check_apply(R.Product(c), c, updates=not _big(c)))


@pytest.mark.parametrize('c', R.col_cases(), ids=R.case_id)
def test_column_space_form(c):
    """k_wbd_gather, k_wbd_weights, k_wbd_fillW, k_wbd_adddiag; k_wbd_beta, k_wbd_g, k_wbd_gemv (odd and even cd), k_wbd_t, k_wbd_fin.  (The cd = 1540
    case: as set up only.)"""
    _report('test_column_space_form', R.case_id(c), R.check_apply(R.Product(c), c, updates=not _big(c)))


ENTRY_CASES = [R.small_cases()[10], R.row_cases()[1], R.col_cases()[1]]


@pytest.mark.parametrize('c', ENTRY_CASES, ids=R.case_id)
def test_entry_rejects_wrong_lengths_and_flags_and_repeats_bit_for_bit(c):
    h = R.Product(c)
    R.check_rejections(h, c)
    R.check_repeatable(h, c)


def test_entry_is_not_implemented_without_a_correction():
    import scipy.sparse as sp
    import osqp_amd
    m = osqp_amd.OSQP(algebra='hip')
    m.setup(sp.identity(4, format='csc'), np.ones(4), sp.identity(4, format='csc'), -np.ones(4), np.ones(4), verbose=False)
    st, out = m._solver.hip_test_woodbury(np.ones(4), order=1)
    assert st == R.NOT_IMPLEMENTED and all(np.isnan(out[k]).all() for k in ('u', 'xs', 'dinv0', 'S', 'Sinv', 'rho'))


@pytest.mark.parametrize('c', ENTRY_CASES + [R.small_cases()[11]], ids=R.case_id)
def test_a_solve_after_the_entry_is_the_solve_without_it(c):
    """The entry saves and restores the residual, u, x~, the flags and the partial slots, and a re-factorisation recomputes what the handle holds: x, y
    and the iteration count of a solve are bit-identical with and without calls in front of it and between two solves."""
    rhs = R.right_hand_sides(c)
    got = []
    for calls in (False, True):
        h = R.Product(c, max_iter=24, adaptive_rho=True, adaptive_rho_interval=10)        # (rho updates where the estimate asks for one; no termination check before the last iteration: the iterate comes back whatever the problem's status would be)
        if calls:
            for k, (refactor, parity, direct) in enumerate(((1, 0, 0), (0, 1, 1), (1, 1, 0))):
                assert h.test(rhs[k], np.sin(np.arange(len(rhs[k]))) if direct else None, refactor=refactor, parity=parity, direct=direct)[0] == 0
        r1 = h.model.solve()
        if calls:
            assert h.test(rhs[3], rhs[0], refactor=1, parity=0, direct=1)[0] == 0
        r2 = h.model.solve()
        assert r1.info.iter == r2.info.iter == 24, (r1.info.status, r1.info.iter, r2.info.status, r2.info.iter)
        info = [v for r in (r1, r2) for v in (r.info.status_val, r.info.rho_updates, r.info.prim_res, r.info.dual_res, r.info.rho_estimate)]
        assert np.isfinite(info).all()
        got.append((info, np.array(r1.x), np.array(r1.y), np.array(r2.x), np.array(r2.y)))
    # (the last iteration's check may find the case infeasible -- the row-space one is -- and x, y then come back as NaN: the residuals of that check and
    #  the rho estimate, which are functions of the iterates, are compared in every bit as well)
    assert np.array_equal(R.bits(got[0][0]), R.bits(got[1][0])), (got[0][0], got[1][0])
    for a, b in zip(got[0][1:], got[1][1:]):
        assert np.array_equal(R.bits(a), R.bits(b))
    assert c['form'] == 'row' or all(np.isfinite(a).all() for a in got[0][1:])


@pytest.mark.parametrize('form', list(R.SMALL_FORMS))
def test_direct_mode_iterations_of_the_small_form(form):
    """unfused (KB, wb_apply, KA), two launches (k_wbx_x / _y), one launch (k_wbz), the slot form: r and n on the edges of the 64-column workgroups and of
    the row pairs, n = 5185 with 82 workgroups (partials folded in two batches), a column with two one-entry rows; then after update_settings(rho)."""
    environment, expect = R.SMALL_FORMS[form]
    w = R.Worst()
    for c in R.iter_cases():
        R.check_iteration_form(R.ProductIterations(c, environment, expect), c, w, form)
    _report('test_direct_mode_iterations_of_the_small_form', form, w)


@pytest.mark.parametrize('job', R.large_iter_cases(), ids=lambda j: j[0])
def test_direct_mode_iterations_of_the_device_factorised_forms(job):
    """row-space direct (wb_apply); column space unfused (wb_apply), fused on CSR passes (k_wbf_r / beta / g / t / x / s), with one thread per short row
    (k_wbf_rb / s2), and with the dense block held dense (k_wbf_gd / gr / td)"""
    name, c, environment, expect = job
    w = R.check_iteration_form(R.ProductIterations(c, environment, expect), c, R.Worst(), name)
    _report('test_direct_mode_iterations_of_the_device_factorised_forms', name, w)
