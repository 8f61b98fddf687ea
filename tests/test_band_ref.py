"""CPU tier of the band kernel tests: every case and check of tests/test_gpu_band_kernels.py (tests/band_ref.py: cases, references, bounds) on the host
simulator's textbook loops (tests/hostsim/backend_host.cpp test_band), and the proof that the checks notice a result that is subtly wrong: five kinds of
mistake, planted into copies of a correct result or into a plain-double run of the kernel's order of operations, each have to fail."""
import numpy as np
import pytest
import scipy.sparse as sp

import band_ref as R
from hostsim_util import hostsim


@pytest.fixture(scope='module')
def solver():
    with hostsim():
        import osqp_amd
        m = osqp_amd.OSQP(algebra='hip')
        m.setup(sp.identity(4, format='csc'), np.ones(4), sp.identity(4, format='csc'), -np.ones(4), np.ones(4), verbose=False)
        yield m._solver


@pytest.mark.parametrize('n', R.SIZES)
def test_factor_and_substitutions_on_plain_loops(solver, n):
    for bw in R.bws_for(n):
        for cls in R.classes_for(n, bw):
            for wf, ws in R.check_case(solver, cls, n, bw).values():
                assert wf <= 1.0 and ws <= 1.0


@pytest.mark.parametrize('n', R.SIZES)
def test_guard_rule_on_plain_loops(solver, n):
    for bw in R.guard_bws(n):
        for cstar in R.guard_points(n):
            for kind in R.GUARD_KINDS:
                R.check_guard(solver, n, bw, cstar, kind)


def test_rejections_on_plain_loops(solver):
    R.check_rejections(solver)


def test_kkt_class_is_ill_conditioned_and_guard_class_keeps_its_pivots():
    for n, bw in ((65, 31), (200, 56)):
        ev = np.linalg.eigvalsh(R.dense_matrix('kkt', n, bw))
        assert ev[0] > 0 and 1e7 <= ev[-1] / ev[0] <= 1e10, ev[-1] / ev[0]
        ev = np.linalg.eigvalsh(R.dense_matrix('guard', n, bw))
        assert 0.25 < ev[0] and ev[-1] < 1.5


SABOTAGE_SHAPES = [(73, 9), (65, 56), (137, 31)]


def _checks(out, c, perm, rhs):
    R.check_padding(out)
    R.check_factor(out, c['Kd'])
    R.check_solve(out, perm, rhs)


@pytest.mark.parametrize('cls', ['dd', 'kkt'])
@pytest.mark.parametrize('n,bw', SABOTAGE_SHAPES)
def test_checks_notice_a_subtly_wrong_result(solver, n, bw, cls):
    """What the GPU tier's green run is worth: each of these differs from a correct result in one place."""
    c = R.case(cls, n, bw)
    perm, rhs = c['perms'][1], c['rhs'][:3]
    # the emulation itself passes, as do the plain loops
    _checks(R.emulate(n, bw, c['band'], perm, rhs), c, perm, rhs)
    good = R.call(solver, n, bw, c['band'], perm, rhs)
    _checks(good, c, perm, rhs)
    # one trailing update dropped at the band's edge (k = bw), early and late in the matrix
    # (at a step c and a column c + a where the dropped product L[c + bw][c] L[c + a][c] is not a structural zero of the kkt class)
    Ld, _ = R.factor_of(good)
    steps = [(s, a) for s in range(n - bw) for a in range(1, bw) if Ld[bw, s] != 0 and Ld[a, s] != 0]
    assert steps, 'no step of this case has a product at the band edge'
    for step in (steps[0], steps[-1]):
        with pytest.raises(AssertionError, match='factor bound missed|not finite'):
            R.check_factor(R.emulate(n, bw, c['band'], perm, rhs, drop_update=step), c['Kd'])
    # kmax off by one in the last bw columns
    with pytest.raises(AssertionError, match='factor bound missed|not finite'):
        R.check_factor(R.emulate(n, bw, c['band'], perm, rhs, short_kmax=True), c['Kd'])
    # one padding slot not zero: behind a column, in front of column 0, a diagonal slot, the slack
    W = R.band_stride(bw)
    for cell in (R.FRONT + 5 * W + bw + 1, R.FRONT - 1, R.FRONT + 7 * W, R.band_doubles(n, bw) - 1, R.FRONT + (n - 1) * W + 1):
        bad = good.copy()
        bad.image[cell] = 1e-300
        with pytest.raises(AssertionError, match='outside the factor'):
            R.check_padding(bad)
    # the last element of a substitution left unfinished: the forward pass (emulation), and on the copy the backward pass's last element with a term, one term short
    with pytest.raises(AssertionError, match='solve bound missed'):
        e = R.emulate(n, bw, c['band'], perm, rhs, unfinished=True)
        R.check_factor(e, c['Kd'])
        R.check_solve(e, perm, rhs)
    bad = good.copy()
    X = bad.solutions()
    i, k = next((i, k) for i in range(n) for k in range(1, bw + 1) if Ld[k, i] != 0)          # (the first column of L^ with an entry, its first entry)
    X[:, perm[i]] += float(Ld[k, i]) * X[:, perm[i + k]]
    with pytest.raises(AssertionError, match='solve bound missed'):
        R.check_solve(bad, perm, rhs)
    # x and perm mixed up: out[k] instead of out[perm[k]]
    bad = good.copy()
    bad.solutions()[:] = good.solutions()[:, perm]
    with pytest.raises(AssertionError, match='solve bound missed'):
        R.check_solve(bad, perm, rhs)
    with pytest.raises(AssertionError, match='solve bound missed'):
        R.check_solve(R.emulate(n, bw, c['band'], perm, rhs, mix_perm=True), perm, rhs)
    # an x cell not written, a sentinel overwritten
    for cell in (n - 1, 3 * n + 2):
        bad = good.copy()
        bad.x[cell] = R.SENTINEL if cell < 3 * n else 0.0
        with pytest.raises(AssertionError, match='x cell was not written|sentinel'):
            R.check_padding(bad)


def test_probe_seeds_meet_their_conditions_on_the_symbolic_analysis():
    """The band widths of the one-iteration probe's problems (tests/test_gpu_band_kernels.py), from the host simulator's symbolic analysis."""
    stats = []
    with hostsim():
        import osqp_amd
        for n, seed, per_row in R.PROBE_CASES:
            P, A, Q = R.probe_problem(n, seed, per_row)
            m = osqp_amd.OSQP(algebra='hip')
            m.setup(P, Q[0], A, -1e3 * np.ones(n), 1e3 * np.ones(n), **R.PROBE_SETTINGS)
            with pytest.raises(ValueError):                                 # (no batch kernel in the simulator; the symbolic analysis has run)
                m._solver.hip_batch_solve(q=Q)
            stats.append((n, int(m._solver.hip_stats()['batch_direct_bw']), A.nnz, A.nnz + n))
    R.probe_conditions(stats)
