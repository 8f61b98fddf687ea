"""CPU tier of the Woodbury kernel tests: every case and check of tests/test_gpu_woodbury_kernels.py (tests/wb_ref.py: cases, long-double references,
tolerances) on a numpy stand-in that evaluates the three forms of M^-1 in plain fp64, with the conditions the tolerance rests on asserted for every
case (e64 <= 1e-12; in the iteration tier rows that clamp low, high and stay free at every iteration, no projected value within 1e-6 of a bound,
cond_2(K) <= 1e7) -- and the proof that the checks notice a result that is subtly wrong: seven planted mistakes each have to fail."""
import numpy as np
import pytest
import scipy.sparse as sp

import wb_ref as R
from hostsim_util import hostsim

ALPHA = 1.6


def _big(c):
    return c.get('cd', 0) > 1000 or c['r'] > 1000


@pytest.mark.parametrize('c', R.small_cases() + R.row_cases() + R.col_cases(), ids=R.case_id)
def test_apply_cases_meet_their_conditions_and_pass_on_the_standin(c):
    w = R.check_apply(R.Standin(c), c, updates=not _big(c))
    assert set(w) >= {'Dinv0', 'u', 'gamma', 'xs', 'Sinv'} and max(w.e64.values()) <= R.E64_MAX


def test_case_lists_cover_every_edge_the_kernels_have():
    assert {r for r, n in R.SMALL_PAIRS} == set(R.SMALL_R) and {n for r, n in R.SMALL_PAIRS} == set(R.SMALL_N) and len(set(R.SMALL_PAIRS)) == 20
    assert {r for r, n in R.ITER_PAIRS} == set(R.ITER_R) and {n for r, n in R.ITER_PAIRS} == set(R.ITER_N)
    for c in R.small_cases() + R.row_cases() + R.col_cases() + R.iter_cases():
        p, s = R.problem(c), R.structure(R.problem(c)['A'], c['form'])
        cnt = np.diff(sp.csr_matrix(p['A']).indptr)
        assert len(s['long']) == c['r'] and cnt[s['long']].min() > R.LONG
        assert (p['l'][s['long']] == p['u'][s['long']]).any()                          # an equality row among the long rows
        if c['form'] == 'small':
            assert c['r'] <= R.SMALL_MAX
            if c['n'] > R.LONG + 1:
                assert (s['kind'] == 0).any()                                          # a column no long row touches
            if not c['k0diag']:
                short = cnt[s['short']]
                assert short.min() >= 2 and short.max() <= 5 and (p['P'] - sp.diags(p['P'].diagonal())).nnz > 0
        if c['form'] == 'row':
            assert c['r'] > R.SMALL_MAX and 0 < (s['kind'] != 0).sum() < p['n']
        if c['form'] == 'col':
            assert s['order'] == c['cd'] and 4 * c['cd'] <= 3 * c['r'] and (s['kind'] == 0).any() and (s['kind'] == 2).sum() == c['r'] * c['singles']
    assert {(r['n'] - 3) % 2 for r in R.row_cases()} == {0, 1}                         # both parities of the touched-column count
    assert any(c['r'] > 768 for c in R.row_cases()) and any(c['cd'] > 1536 and c['cd'] % 2 == 0 for c in R.col_cases()) and any(c['cd'] % 2 for c in R.col_cases())
    blk = R.large_iter_cases()[-1][1]
    s = R.structure(R.problem(blk)['A'], 'col')
    AL = sp.csr_matrix(R.problem(blk)['A'])[s['long']][:, s['dcol']]
    assert blk['cd'] == 512 and blk['r'] == 700 and 2 * AL.nnz >= 512 * 700               # the dense block at least half full
    big = R.iter_cases()[-1]
    assert (big['n'] + 63) // 64 == 82 and big['r'] == 3
    two = sp.csr_matrix(R.problem(R.iter_cases()[0])['A'])
    assert (np.bincount(two.indices[np.repeat(np.diff(two.indptr) == 1, np.diff(two.indptr))]) >= 2).any()      # a column with two one-entry rows


PLANT_CASES = {
    'S_drops_last_column': dict(form='small', r=7, n=137, k0diag=True, seed=104, scaling=0),
    'rho_for_its_inverse': dict(form='small', r=64, n=136, k0diag=True, seed=109, scaling=0),
    'singleton_dropped_from_sigma': R.col_cases()[1],
    'untouched_column_zero': dict(form='small', r=2, n=161, k0diag=False, seed=119, scaling=0),
    'xs_overwritten': R.row_cases()[0],
    'S_row_swapped_in_idx': dict(form='small', r=63, n=161, k0diag=True, seed=108, scaling=0),
}


@pytest.mark.parametrize('plant', R.Standin.PLANTS)
def test_checks_notice_a_planted_mistake_in_the_apply_tier(plant):
    """What the GPU tier's green run is worth: each stand-in differs from a correct one in one place."""
    c = PLANT_CASES[plant]
    R.check_apply(R.Standin(c), c, updates=False)                                       # (the same case passes without the mistake)
    with pytest.raises(AssertionError, match='against the tolerance'):
        R.check_apply(R.Standin(c, plant=plant), c, updates=False)


class _StandinIterations:
    def __init__(self, c, plant=None):
        self.h, self.c, self.plant, self.alpha = R.Standin(c, alpha=ALPHA), c, plant, ALPHA

    def rho(self):
        return self.h.rho_vec()

    def __call__(self, k, x0, y0):
        return R.admm_reference(self.c, self.h.A, self.h.rho_vec(), self.h.sigma, ALPHA, self.h.scaling(), k, x0, y0, np.float64, plant=self.plant)[:2]


@pytest.mark.parametrize('c', R.iter_cases() + [t[1] for t in R.large_iter_cases()[:3]] + [R.large_iter_cases()[4][1]], ids=R.case_id)
def test_iteration_cases_meet_their_conditions_and_pass_on_the_standin(c):
    w = R.check_iteration_form(_StandinIterations(c), c, R.Worst(), 'stand-in')
    assert max(w.e64.values()) <= R.E64_MAX


@pytest.mark.parametrize('c', [R.iter_cases()[2], R.large_iter_cases()[1][1]], ids=R.case_id)
def test_checks_notice_a_clamped_row_updated_with_the_wrong_bound(c):
    with pytest.raises(AssertionError, match='against the tolerance'):
        R.check_iteration_form(_StandinIterations(c, plant='wrong_bound'), c, R.Worst(), 'stand-in')


def test_the_host_simulator_has_no_woodbury_correction():
    """The simulator does not define be::test_woodbury and sets no correction up: the entry answers OSQP_FUNC_NOT_IMPLEMENTED and writes nothing."""
    c = R.small_cases()[0]
    p = R.problem(c)
    with hostsim():
        import osqp_amd
        m = osqp_amd.OSQP(algebra='hip')
        m.setup(p['P'], p['q'], p['A'], p['l'], p['u'], **R.settings(c))
        st, out = m._solver.hip_test_woodbury(np.ones(p['n']), order=1)
    assert st == R.NOT_IMPLEMENTED
    assert all(np.isnan(out[k]).all() for k in ('u', 'xs', 'dinv0', 'S', 'Sinv', 'rho')) and (out['idx'] == -1).all()
