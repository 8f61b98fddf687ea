"""GPU tier, kernel level: the banded LDL' factor and the wave-0 substitutions of osqp-python_amd/csrc/band_ldl.h -- the linear solver of every small
single QP, of every batch on the workgroup kernels and of the batched backward -- on test matrices through the diagnostic entry osqp_hip_test_band
(k_test_band<64, false>, <256, false>, <256, true>: the three forms the product runs), against np.longdouble references (tests/band_ref.py: cases,
bounds and where each bound comes from).  The whole solves of test_gpu_small_direct.py / test_gpu_adjoint.py reach this code with narrow bands, or with
the widest band only where no lane takes a second element; here every n sits on a block edge (multiples of 8) or a lane-wrap edge (64, 128, 192) with
bands up to the limit 56, where the first pivot that touches element e + 64 sits in the block right after the one that finishes e.
tests/test_band_ref.py proves this file's machinery on plain loops and shows that it notices five kinds of subtly wrong result.

The last test reaches what the entry cannot: the batch kernel's own assembly of the band and the register-resident n <= 128 form of the substitutions
(k_batch_admm, N128), by a one-iteration probe whose result is -K^-1 q.

Worst ratios to the bounds measured on an MI355X (all n, bw and classes): factor 0.28 and solve 0.42 of the bound on each of the
three instantiations (their results are bit-identical), GUARD 0.26, the probe 1.5e-4 in both variants."""
import numpy as np
import pytest
import scipy.sparse as sp

import band_ref as R
from util import record_deviation

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def solver():
    import osqp_amd
    m = osqp_amd.OSQP(algebra='hip')
    m.setup(sp.identity(4, format='csc'), np.ones(4), sp.identity(4, format='csc'), -np.ones(4), np.ones(4), verbose=False)
    yield m._solver


@pytest.mark.parametrize('n', R.SIZES)
def test_factor_substitutions_padding_and_bit_identity(solver, n):
    worst = {}
    for bw in R.bws_for(n):
        for cls in R.classes_for(n, bw):
            for inst, (wf, ws) in R.check_case(solver, cls, n, bw).items():
                f, s = worst.get(inst, (0.0, 0.0))
                worst[inst] = (max(f, wf), max(s, ws))
    for (threads, guard), (wf, ws) in worst.items():
        record_deviation('test_factor_substitutions_padding_and_bit_identity', 'n=%d threads=%d guard=%d' % (n, threads, guard), factor_ratio=wf, solve_ratio=ws)
        print(n, threads, guard, 'factor %.3f solve %.3f of the bound' % (wf, ws))


@pytest.mark.parametrize('n', R.SIZES)
def test_guard_replaces_a_pivot_by_its_magnitude_or_one_and_reports_it(solver, n):
    worst = 0.0
    for bw in R.guard_bws(n):
        for cstar in R.guard_points(n):
            for kind in R.GUARD_KINDS:
                worst = max(worst, R.check_guard(solver, n, bw, cstar, kind))
    record_deviation('test_guard_replaces_a_pivot_by_its_magnitude_or_one_and_reports_it', 'n=%d' % n, factor_ratio=worst)
    print(n, 'factor %.3f of the bound' % worst)


def test_entry_rejects_what_could_leave_the_band(solver):
    R.check_rejections(solver)


def _probe(variant, monkeypatch):
    import osqp_amd
    monkeypatch.setenv('OSQP_HIP_BATCH_VARIANT', variant)
    xs, stats = [], []
    for n, seed, per_row in R.PROBE_CASES:
        P, A, Q = R.probe_problem(n, seed, per_row)
        m = osqp_amd.OSQP(algebra='hip')
        m.setup(P, Q[0], A, -1e3 * np.ones(n), 1e3 * np.ones(n), **R.PROBE_SETTINGS)
        x, y, rec = m._solver.hip_batch_solve(q=Q)
        assert (rec[:, 1] == 1).all() and (rec[:, 7] == 0).all(), rec[:, [0, 1, 7]]           # one iteration, no PCG: a direct variant ran
        st = m._solver.hip_stats()
        stats.append((n, int(st['batch_direct_bw']), A.nnz, int(st['nnzB'])))
        xs.append(x)
    return xs, stats


def test_one_iteration_probe_of_the_batch_kernels_band_and_the_n128_form(monkeypatch):
    """After exactly one iteration from a cold start (alpha = 1, no bound in reach) the iterate is x = -K^-1 q, K = P + sigma I + rho A'A: (i) both
    variants within the backward-error bound of band_ref.probe_bound_ratio; (ii) band_solve on 64 threads and the register-resident form on 256 agree
    in every bit -- the claim of the comment at k_batch_admm's N128 form."""
    x64, stats = _probe('direct', monkeypatch)
    x256, stats256 = _probe('direct256', monkeypatch)
    assert stats == stats256
    R.probe_conditions(stats)
    for (n, seed, per_row), (_, bw, _, _), a, b in zip(R.PROBE_CASES, stats, x64, x256):
        P, A, Q = R.probe_problem(n, seed, per_row)
        for i in range(Q.shape[0]):
            r64, r256 = R.probe_bound_ratio(P, A, Q[i], a[i], bw), R.probe_bound_ratio(P, A, Q[i], b[i], bw)
            differ = np.flatnonzero(R.bits(a[i]) != R.bits(b[i]))
            record_deviation('test_one_iteration_probe_of_the_batch_kernels_band_and_the_n128_form', 'n=%d bw=%d q%d' % (n, bw, i), direct_ratio=r64, direct256_ratio=r256,
                             elements_that_differ=int(differ.size))
            print(n, bw, i, 'direct %.3e direct256 %.3e of the bound; %d elements differ' % (r64, r256, differ.size), differ[:8])
            assert r64 <= 1.0 and r256 <= 1.0, (n, bw, r64, r256)
            assert differ.size == 0, (n, bw, differ, a[i][differ], b[i][differ])
