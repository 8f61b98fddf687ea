"""CPU tier: tests/direct_polish_ref.py -- the fp64 restatement of polish on the direct lockstep route -- against the oracle's polish.

The oracle solves each QP at eps = 1e-6 (the settings of tests/test_gpu_lockstep_direct_polish.py) and polishes it (delta = 1e-6, polish_refine_iter = 3);
the restatement is given the same ADMM point and must sit within 1e-8 relative of the oracle's polished x and y after every step count a handle with
polish_refine_iter = 3 .. 8 would take at least (1 + 3 .. 1 + 8).  Shapes: the four the GPU tier runs -- portfolio_qp(600, 4) elements PICK of that
tier's batch, portfolio_qp(256, 1), test_one_dense_row's QP and _factor_qp(400, 127, 0.7) with _edge's three elements each.

The two planted mistakes of direct_polish_ref.py must fail that check.  'free_y' fails on every shape.  'dense_rho' concerns an INACTIVE dense row, and
in all four shapes every dense row is an equality (the factor rows, the budget): there it changes nothing, so it is shown on a fifth QP --
test_one_dense_row's with the budget row widened to [0, 1000], which ends inactive."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import problems
import test_gpu_lockstep_direct as shared
from direct_polish_ref import direct_polish
from oracle import Oracle, SOLVED

warnings.simplefilter('ignore')
ST = dict(eps_abs=1e-6, eps_rel=1e-6, max_iter=50000, adaptive_rho_interval=50, check_termination=25)
STEPS = range(1 + 3, 1 + 8 + 1)
TOL = 1e-8


def _rel(a, b):
    return np.abs(a - b).max() / (1 + np.abs(b).max())


def one_dense_row_qp():
    """test_gpu_lockstep_direct.py::test_one_dense_row's QP"""
    n = 500
    rng = np.random.default_rng(2)
    P = sp.diags(0.5 + rng.random(n), format='csc')
    budget = sp.csc_matrix((np.ones(200), (np.zeros(200, dtype=int), np.arange(0, 400, 2))), shape=(1, n))
    A = sp.vstack([budget, sp.identity(n)], format='csc')
    l, u = np.concatenate([[1.0], np.zeros(n)]), np.concatenate([[1.0], np.ones(n)])
    return P, rng.standard_normal(n), A, l, u


def edge_batch(q, l, u):
    """test_gpu_lockstep_direct.py::_edge's three elements"""
    rng = np.random.default_rng(5)
    Q = np.stack([q * (1.0 + 0.3 * b) + 0.1 * b * rng.standard_normal(len(q)) * (q != 0) for b in range(3)])
    return Q, np.tile(l, (3, 1)), np.tile(u, (3, 1))


def base_batch():
    """test_gpu_lockstep_direct.py::Base's Q, L, U (without its handle)"""
    P, q, A, l, u = problems.portfolio_qp(600, 4)
    rng = np.random.default_rng(17)
    Q = np.stack([np.concatenate([-rng.standard_normal(600) / (1.0 + 0.05 * b), np.zeros(4)]) for b in range(shared.B)])
    L, U = np.tile(l, (shared.B, 1)), np.tile(u, (shared.B, 1))
    for b in (3, 63, 66):
        U[b, 5:] = 0.02 + 0.01 * rng.random(600)
    return P, A, Q, L, U


def _cases():
    P, A, Q, L, U = base_batch()
    for b in shared.PICK:
        yield 'portfolio 600x4 element %d' % b, (P, Q[b], A, L[b], U[b])
    yield 'portfolio 256x1', problems.portfolio_qp(256, 1)
    for name, (P, q, A, l, u) in (('one dense row', one_dense_row_qp()), ('128 dense rows', shared._factor_qp(400, 127, 0.7))):
        Q, L, U = edge_batch(q, l, u)
        for b in range(3):
            yield '%s element %d' % (name, b), (P, Q[b], A, L[b], U[b])


class Polished:
    """the oracle's ADMM point and its polish, once per QP"""
    def __init__(self, data):
        self.data = data
        o = Oracle().setup(*data, **ST)
        self.x, self.y, io = o.solve()
        assert io.status_val == SOLVED
        self.xp, self.yp, self.info, self.status = o.polish(delta=1e-6, polish_refine_iter=3)

    def worst(self, mistake=None):
        """the restatement's largest relative distance from the oracle's polish over STEPS: (x, y)"""
        dev = [direct_polish(*self.data, self.x, self.y, steps, mistake=mistake) for steps in STEPS]
        return max(_rel(x, self.xp) for x, _ in dev), max(_rel(y, self.yp) for _, y in dev)


@pytest.fixture(scope='module')
def polished():
    return {name: Polished(data) for name, data in _cases()}


def test_the_restatement_reaches_the_oracles_polish(polished):
    for name, p in polished.items():
        ex, ey = p.worst()
        print('%-32s oracle polish %d (%.1e / %.1e); restatement |dx| %.2e |dy| %.2e' % (name, p.status, p.info.pri_res, p.info.dua_res, ex, ey))
        assert p.status == 1, name
        assert ex <= TOL and ey <= TOL, (name, ex, ey)


def test_free_rows_not_freed_is_seen(polished):
    for name, p in polished.items():
        ex, ey = p.worst('free_y')
        print('%-32s free_y: |dx| %.2e |dy| %.2e' % (name, ex, ey))
        assert not (ex <= TOL and ey <= TOL), name


def test_inactive_dense_row_at_rho_bar_is_seen(polished):
    """every dense row of the four shapes is an equality: the mistake is vacuous there (asserted), and seen on a QP whose dense row ends inactive"""
    for name, p in polished.items():
        assert p.worst('dense_rho') == p.worst(), name
    P, q, A, l, u = one_dense_row_qp()
    l[0], u[0] = 0.0, 1000.0
    p = Polished((P, q, A, l, u))
    z0 = (A @ p.xp)[0]
    assert p.status == 1 and l[0] < z0 < u[0] and p.yp[0] == 0.0                      # the dense row is inactive at the polished point
    good, bad = p.worst(), p.worst('dense_rho')
    print('inactive dense row: restatement |dx| %.2e |dy| %.2e; with the dense row at rho_bar |dx| %.2e |dy| %.2e' % (good + bad))
    assert good[0] <= TOL and good[1] <= TOL, good
    assert not (bad[0] <= TOL and bad[1] <= TOL), bad
