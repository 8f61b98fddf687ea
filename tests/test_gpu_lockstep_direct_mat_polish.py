"""GPU tier: polish on the direct lockstep route with PER-PROBLEM MATRICES (settings.polishing with osqp_hip_batch_solve_lockstep_direct_mat[_device];
lockstep_hip.hip lockstep_direct_chunk with mat_ws, "polish"): element b is polished on its own P_b, A_b under its own scaling, as a polishing handle set up
with that element's data alone would polish it.

The base is that of test_gpu_lockstep_direct_mat.py (portfolio_qp(600, 4), B = 70, _perturb with default_rng(3)) at eps = 1e-6, check_termination = 25,
adaptive_rho_interval = 50, warm_starting off.  Bounds: those of test_gpu_lockstep_direct_polish.py -- the certificate at 64 * 2^-52 * rho_bar (1 + scale) on
the element's OWN matrices, x and y at 1e-8 and the objective at 1e-9 relative against the oracle's polish on them.  The oracle accepts polish on all 70
elements on their own matrices (checked on the CPU)."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_amd
import problems
import test_gpu_lockstep_direct_mat as mat
import test_gpu_lockstep_direct_polish as pol
from util import record_deviation

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
S = osqp_amd.SolverStatus
B, PICK = pol.B, pol.PICK
REC_STATUS, REC_POLISH, NOT_TIME = pol.REC_STATUS, pol.REC_POLISH, pol.NOT_TIME
_handle, _rel = pol._handle, pol._rel


class Base:
    def __init__(self):
        P, A, self.Q, _, _ = pol.ref.base_batch()
        _, self.q, _, self.l, self.u = problems.portfolio_qp(600, 4)
        self.P, self.A = mat._csc(sp.triu(P)), mat._csc(A)
        self.n, self.m = len(self.q), len(self.l)
        self.L, self.U = np.tile(self.l, (B, 1)), np.tile(self.u, (B, 1))             # (test_gpu_lockstep_direct_mat.py's Base: the handle's bounds)
        self.Px, self.Ax = mat._perturb(self.P, self.A, B)
        self.kw = dict(q=self.Q, l=self.L, u=self.U, Px=self.Px, Ax=self.Ax)
        self.sp = _handle(self.P, self.q, self.A, self.l, self.u, polishing=True)
        self.s0 = _handle(self.P, self.q, self.A, self.l, self.u)
        self.x, self.y, self.rec = self.sp._solver.hip_batch_solve_lockstep_direct(**self.kw)
        self.last, self.plast = self.sp._solver.lockstep_direct_mat_last_record(), self.sp._solver.lockstep_polish_last_record()
        self.x0, self.y0, self.rec0 = self.s0._solver.hip_batch_solve_lockstep_direct(**self.kw)
        self.last0, self.plast0 = self.s0._solver.lockstep_direct_mat_last_record(), self.s0._solver.lockstep_polish_last_record()

    def own(self, b):
        return mat._own(self.P, self.A, self.Px, self.Ax, b)

    def rows(self, idx):
        return dict(q=self.Q[idx], l=self.L[idx], u=self.U[idx], Px=self.Px[idx], Ax=self.Ax[idx])


@pytest.fixture(scope='module')
def base():
    return Base()


def test_polished_and_certified(base):
    """All 70 SOLVED and polished (the route used to write status_polish = 0), each certified on ITS matrices, four against the oracle's polish on them."""
    assert (base.rec[:, REC_STATUS] == S.OSQP_SOLVED).all(), base.rec[:, REC_STATUS]
    print('status_polish:', base.rec[:, REC_POLISH].astype(int).tolist(), base.plast)
    assert (base.rec[:, REC_POLISH] == 1).all(), base.rec[:, REC_POLISH]
    assert base.plast['attempted'] == B and base.plast['pcg_iters'] == 0 and base.plast['steps_max'] >= 4, base.plast
    worst = {}
    for b in range(B):
        Pb, Ab = base.own(b)
        fig = pol.certify(Pb, base.Q[b], Ab, base.L[b], base.U[b], base.x[b], base.y[b], base.rec[b])
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print('worst certificate figures over the batch (relative):', worst)
    record_deviation('lockstep_direct_mat_polish_vs_oracle', 'portfolio 600x4 certificate, worst of %d' % B, bound=pol.CERT, **worst)
    for b in PICK:
        Pb, Ab = base.own(b)
        pol.against_oracle('lockstep_direct_mat_polish_vs_oracle', 'portfolio 600x4 own matrices element %d' % b, Pb, base.Q[b], Ab, base.L[b], base.U[b], base.x[b], base.y[b], base.rec[b])
    print('worst ratio to each bound:', {k: '%.2e' % v for k, v in pol.WORST.items()})
    record_deviation('lockstep_direct_mat_polish_vs_oracle', 'worst ratio to each bound', **pol.WORST)


def test_the_elements_own_handle(base):
    """Elements 0 and 5 of a batch of 6 against a FRESH polishing handle set up with that element's data (the shared direct call, nbatch = 1) at 1e-8."""
    x, y, rec = base.sp._solver.hip_batch_solve_lockstep_direct(**base.rows(slice(0, 6)))
    assert (rec[:, REC_POLISH] == 1).all()
    for b in (0, 5):
        Pb, Ab = base.own(b)
        s = _handle(Pb, base.Q[b], Ab, base.L[b], base.U[b], polishing=True)
        xf, yf, rf = s._solver.hip_batch_solve_lockstep_direct(nbatch=1)
        assert rf[0, REC_STATUS] == S.OSQP_SOLVED and rf[0, REC_POLISH] == 1
        ex, ey = _rel(x[b], xf[0]), _rel(y[b], yf[0])
        bits = bool(np.array_equal(x[b], xf[0]) and np.array_equal(y[b], yf[0]))
        record_deviation('lockstep_direct_mat_polish_vs_own_handle', 'portfolio 600x4 element %d' % b, dx_rel=ex, dy_rel=ey, bits_equal=int(bits), atol=1e-8)
        print('element %d against its own polishing handle: |dx| %.2e |dy| %.2e (relative); bits equal: %s' % (b, ex, ey, bits))
        assert ex <= 1e-8 and ey <= 1e-8, (b, ex, ey)


def test_own_values_tiled(base):
    """Px, Ax = the handle's own values repeated: against the shared polished call on the same q, l, u at 1e-8; bit equality reported."""
    nb = 6
    kw = dict(q=base.Q[:nb], l=base.L[:nb], u=base.U[:nb])
    xs, ys, rs = base.sp._solver.hip_batch_solve_lockstep_direct(**kw)
    xm, ym, rm = base.sp._solver.hip_batch_solve_lockstep_direct(Px=np.tile(base.P.data, (nb, 1)), Ax=np.tile(base.A.data, (nb, 1)), **kw)
    assert (rs[:, REC_POLISH] == 1).all() and (rm[:, REC_POLISH] == 1).all()
    print('bits equal:', np.array_equal(xs, xm) and np.array_equal(ys, ym))
    for b in range(nb):
        ex, ey = _rel(xm[b], xs[b]), _rel(ym[b], ys[b])
        assert ex <= 1e-8 and ey <= 1e-8, (b, ex, ey)


def test_independence(base):
    solve = base.sp._solver.hip_batch_solve_lockstep_direct
    for b in PICK:
        x1, y1, r1 = solve(**base.rows(slice(b, b + 1)))
        assert np.array_equal(x1[0], base.x[b]) and np.array_equal(y1[0], base.y[b]) and np.array_equal(r1[0, NOT_TIME], base.rec[b, NOT_TIME]), b
    xr, yr, rr = solve(**{k: v[::-1].copy() for k, v in base.kw.items()})
    assert np.array_equal(xr[::-1], base.x) and np.array_equal(yr[::-1], base.y) and np.array_equal(rr[::-1][:, NOT_TIME], base.rec[:, NOT_TIME])


def test_off_means_off(base):
    """The ADMM part is the never-polishing handle's; with polishing switched off the polishing handle returns that handle's bits and launch count; the
    never-polishing handle's polish record is untouched (all zero)."""
    assert np.array_equal(base.rec[:, pol.ADMM_FIELDS], base.rec0[:, pol.ADMM_FIELDS])
    for k in ('admm_iters_max', 'factorisations', 'matrix_block_bytes'):
        assert base.last[k] == base.last0[k], (k, base.last, base.last0)
    assert all(v == 0 for v in base.plast0.values()), base.plast0
    assert (base.rec0[:, REC_POLISH] == 0).all() and (base.rec0[:, pol.REC_POLISH_TIME] == 0).all()
    try:
        base.sp.update_settings(polishing=False)
        x, y, rec = base.sp._solver.hip_batch_solve_lockstep_direct(**base.kw)
        last, plast = base.sp._solver.lockstep_direct_mat_last_record(), base.sp._solver.lockstep_polish_last_record()
    finally:
        base.sp.update_settings(polishing=True)
    assert np.array_equal(x, base.x0) and np.array_equal(y, base.y0) and np.array_equal(rec, base.rec0)
    assert last['kernel_launches'] == base.last0['kernel_launches'] and plast['attempted'] == 0, (last, base.last0, plast)
