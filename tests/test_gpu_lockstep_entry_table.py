"""GPU tier: what the sixteen lockstep entry points share -- the code each device entry answers on a handle of its own route and on a handle of the other
route, WHICH of the nine last-call records a call moves (and that every other record stays exactly as it was, timings included), and when
lockstep_mat_scaling answers.

Handles: the PCG route's is problems.banded_qp(40, window=8) with polishing; the direct route's is problems.portfolio_qp(256, 1) (n = 257, m = 258, r = 2:
the budget row and the one factor row, which holds 128 + 1 entries) -- the smallest portfolio_qp(assets, 1) the direct route accepts: every dense row needs
more than kLongRow = 128 entries, (130, 1) and (200, 1) are declined.  Every call is B = 2 (one ragged chunk) with max_iter at its default."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_amd
import problems
from osqp_amd import ext_hip

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
E = ext_hip.osqp_error_type
B = 2
GETTERS = dict(solve='lockstep_last_record', polish='lockstep_polish_last_record', mat='lockstep_mat_last_record', direct='lockstep_direct_last_record',
               direct_mat='lockstep_direct_mat_last_record', adjoint='lockstep_adjoint_last_record', mat_adjoint='lockstep_mat_adjoint_last_record',
               direct_adjoint='lockstep_direct_adjoint_last_record', direct_mat_adjoint='lockstep_direct_mat_adjoint_last_record')


class Handle:
    def __init__(self, data, **settings):
        P, self.q, A, self.l, self.u = data
        self.P, self.A = sp.csc_matrix(sp.triu(P)), sp.csc_matrix(A)
        self.P.sort_indices(); self.A.sort_indices()
        self.s = osqp_amd.OSQP(algebra='hip')
        self.s.setup(self.P, self.q, self.A, self.l, self.u, verbose=False, **settings)
        self.solver = self.s._solver
        rng = np.random.default_rng(3)                      # per-element values as tests/test_gpu_lockstep_direct_mat.py draws them
        self.Ax = self.A.data * (1.0 + 0.1 * rng.standard_normal((B, self.A.nnz)))
        self.Px = self.P.data * (1.0 + 0.2 * rng.random((B, self.P.nnz)))
        self.Q = np.stack([self.q * (1.0 + 0.05 * b) for b in range(B)])

    def records(self):
        return {k: getattr(self.solver, g)() for k, g in GETTERS.items()}

    def step(self, call, moves):
        """one call; exactly the records in `moves` differ from what they were, every other one is what it was"""
        before = self.records()
        out = call()
        after = self.records()
        assert {k for k in GETTERS if after[k] != before[k]} == set(moves), (moves, before, after)
        return out, after


@pytest.fixture(scope='module')
def pcg():
    return Handle(problems.banded_qp(40, window=8), polishing=True)


@pytest.fixture(scope='module')
def direct():
    return Handle(problems.portfolio_qp(256, 1))


def test_codes_of_the_device_entries(pcg, direct):
    """own route: the query succeeds, x NULL is a validation error; the other route's entries decline.  No kernel runs."""
    import torch
    solve = dict(pcg='hip_batch_solve_lockstep_device', direct='hip_batch_solve_lockstep_direct_device')
    adjoint = dict(pcg='hip_batch_adjoint_lockstep_device', direct='hip_batch_adjoint_lockstep_direct_device')
    for own, other, h in (('pcg', 'direct', pcg), ('direct', 'pcg', direct)):
        before = h.records()
        buf = {k: torch.zeros(w, dtype=torch.float64, device='cuda') for k, w in dict(y=len(h.l), rec=h.solver.BATCH_REC, dx=len(h.q), Px=h.P.nnz, Ax=h.A.nnz).items()}
        for mat in (dict(), dict(Px_ptr=buf['Px'].data_ptr(), Ax_ptr=buf['Ax'].data_ptr())):
            getattr(h.solver, solve[own])(0, None, None, None, None, None, None, **mat)                  # no exception: OSQP_NO_ERROR
            getattr(h.solver, adjoint[own])(0, None, None, None, **mat)
            for call in (lambda: getattr(h.solver, solve[own])(1, None, None, None, None, buf['y'].data_ptr(), buf['rec'].data_ptr(), **mat),
                         lambda: getattr(h.solver, adjoint[own])(1, None, buf['y'].data_ptr(), buf['dx'].data_ptr(), **mat)):
                with pytest.raises(ValueError) as e:
                    call()
                assert e.value.code == E.OSQP_DATA_VALIDATION_ERROR
            for call in (lambda: getattr(h.solver, solve[other])(0, None, None, None, None, None, None, **mat),
                         lambda: getattr(h.solver, adjoint[other])(0, None, None, None, **mat)):
                with pytest.raises(ValueError) as e:
                    call()
                assert e.value.code == E.OSQP_FUNC_NOT_IMPLEMENTED
        assert h.records() == before                        # nothing ran: no record moved


def test_records_a_call_moves_on_the_pcg_route(pcg):
    s, L, U = pcg.solver, np.tile(pcg.l, (B, 1)), np.tile(pcg.u, (B, 1))
    (x, y, rec), after = pcg.step(lambda: s.hip_batch_solve_lockstep(q=pcg.Q, l=L, u=U), {'solve', 'polish'})
    assert after['solve']['chunks'] == 1 and after['solve']['reserved'] == 0 and after['polish']['workspace_bytes'] > 0
    (xm, ym, recm), after = pcg.step(lambda: s.hip_batch_solve_lockstep(q=pcg.Q, l=L, u=U, Px=pcg.Px, Ax=pcg.Ax), {'solve', 'polish', 'mat'})
    assert after['solve']['reserved'] == 0 and after['mat']['chunks'] == 1
    D, Ev, c = s.lockstep_mat_scaling(0)                    # the block holds the forward's last chunk
    assert D.shape == (len(pcg.q),) and Ev.shape == (len(pcg.l),) and c > 0
    dx = np.ones_like(x)
    pcg.step(lambda: s.hip_batch_adjoint_lockstep(x, y, dx, l=L, u=U), {'adjoint'})
    s.lockstep_mat_scaling(0)                               # (the shared adjoint does not touch the matrix block)
    pcg.step(lambda: s.hip_batch_adjoint_lockstep(xm, ym, dx, l=L, u=U, Px=pcg.Px, Ax=pcg.Ax), {'adjoint', 'mat_adjoint'})
    with pytest.raises(ValueError) as e:                    # ... the one with per-problem matrices overwrites it
        s.lockstep_mat_scaling(0)
    assert e.value.code == E.OSQP_DATA_NOT_INITIALIZED


def test_records_a_call_moves_on_the_direct_route(direct):
    s = direct.solver
    zero = lambda after: all(v == 0 for v in after['polish'].values())
    (x, y, rec), after = direct.step(lambda: s.hip_batch_solve_lockstep_direct(q=direct.Q), {'direct'})
    assert after['direct']['chunks'] == 1 and after['direct']['seconds'] > 0 and zero(after)
    (xm, ym, recm), after = direct.step(lambda: s.hip_batch_solve_lockstep_direct(q=direct.Q, Px=direct.Px, Ax=direct.Ax), {'direct', 'direct_mat'})
    assert after['direct']['seconds'] > 0 and after['direct_mat']['chunks'] == 1 and zero(after)
    dx = np.ones_like(x)
    _, after = direct.step(lambda: s.hip_batch_adjoint_lockstep_direct(x, y, dx), {'direct_adjoint'})
    assert zero(after)
    _, after = direct.step(lambda: s.hip_batch_adjoint_lockstep_direct(xm, ym, dx, Px=direct.Px, Ax=direct.Ax), {'direct_adjoint', 'direct_mat_adjoint'})
    assert zero(after)
