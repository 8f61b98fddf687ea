"""GPU tier: polish on the lockstep batch route (settings.polishing with osqp_hip_batch_solve_lockstep[_device]; lockstep_hip.hip "polish of a chunk").
Every problem of a chunk that ends SOLVED is polished on block vectors by the recurrence Engine::polish runs on the PCG path; the others are left alone.

The base is banded_qp(400, window=40), m = 800, and the batch of test_gpu_batch_lockstep.py (seed 13): B = 70 -- one full chunk and a ragged one of 6.

Bounds.  They are those of test_gpu_polish.py::test_polish_on_the_pcg_path_matches_the_oracle, the single handle's polish on the PCG path: same recurrence,
same delta_eff, same inner tolerance.  A polished point is certified on the host at 1e-9 x (1 + scale) in both KKT residuals, the record's objective to
1e-9 relative of the certificate's; against the oracle's polish (delta = 1e-6, three refinement steps) x and y to 1e-8, the objective to 1e-9 relative;
a polish with delta = 1e-2 and eight refinement steps lands within 1e-7 of the default one."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_amd
import problems
from oracle import Oracle, SOLVED
from util import record_deviation

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
S = osqp_amd.SolverStatus
EPS = 1e-6
B = 70
PICK = (0, 63, 64, 69)
ST = dict(eps_abs=EPS, eps_rel=EPS, max_iter=50000, adaptive_rho_interval=50, check_termination=25)
REC_STATUS, REC_ITER, REC_OBJ, REC_PRI, REC_DUA, REC_POLISH, REC_POLISH_TIME = 0, 1, 2, 3, 4, 8, 9
ADMM_FIELDS = [0, 1, 5, 6, 7, 10]                  # status, iter, rho, rho_updates, pcg_iters, rho_estimate
NOT_TIME = [f for f in range(12) if f != REC_POLISH_TIME]


def _batch(q, l, u, nb, seed=13):
    rng = np.random.default_rng(seed)
    return (np.stack([q + 0.05 * b * rng.standard_normal(len(q)) for b in range(nb)]), np.stack([l - 0.01 * b for b in range(nb)]),
            np.stack([u + 0.01 * b for b in range(nb)]))


def _handle(P, q, A, l, u, **kw):
    st = dict(ST); st.update(kw)
    s = osqp_amd.OSQP(algebra='hip')
    s.setup(P, q, A, l, u, verbose=False, **st)
    return s


def _rel(a, b):
    return np.abs(a - b).max() / (1 + np.abs(b).max())


def _certify(P, q, A, l, u, x, y, rec):
    """test_polish_on_the_pcg_path_matches_the_oracle's certificate of a polished point; returns the figures"""
    k = problems.kkt_certificate(P, q, A, l, u, x, y)
    ax = A @ x
    scale_p = 1 + max(np.abs(ax).max(initial=0.0), np.abs(np.clip(ax, l, u)).max(initial=0.0))        # (initial: m = 0 has no rows)
    scale_d = 1 + max(np.abs(P @ x).max(), np.abs(A.T @ y).max(), np.abs(q).max())
    fig = dict(pri=k['pri'] / scale_p, dua=k['dua'] / scale_d, rec_pri=rec[REC_PRI] / scale_p, rec_dua=rec[REC_DUA] / scale_d,
               obj=abs(k['obj'] - rec[REC_OBJ]) / (1 + abs(k['obj'])))
    assert k['pri'] <= 1e-9 * scale_p and k['dua'] <= 1e-9 * scale_d, k
    assert rec[REC_PRI] <= 1e-9 * scale_p and rec[REC_DUA] <= 1e-9 * scale_d, rec
    assert abs(k['obj'] - rec[REC_OBJ]) <= 1e-9 * (1 + abs(k['obj'])), (k, rec)
    return fig


class Base:
    def __init__(self):
        self.P, self.q, self.A, self.l, self.u = problems.banded_qp(400, window=40)
        self.n, self.m = len(self.q), len(self.l)
        self.Q, self.L, self.U = _batch(self.q, self.l, self.u, B)
        self.sp = _handle(self.P, self.q, self.A, self.l, self.u, polishing=True)        # the polishing handle
        self.s0 = _handle(self.P, self.q, self.A, self.l, self.u)                        # the never-polishing one
        self.zero = self.sp._solver.lockstep_polish_last_record()
        self.x, self.y, self.rec = self.sp._solver.hip_batch_solve_lockstep(q=self.Q, l=self.L, u=self.U)
        self.last, self.plast = self.sp._solver.lockstep_last_record(), self.sp._solver.lockstep_polish_last_record()
        self.x0, self.y0, self.rec0 = self.s0._solver.hip_batch_solve_lockstep(q=self.Q, l=self.L, u=self.U)
        self.last0, self.plast0 = self.s0._solver.lockstep_last_record(), self.s0._solver.lockstep_polish_last_record()


@pytest.fixture(scope='module')
def base():
    return Base()


def test_polished_and_certified(base):
    """Every element of the batch is SOLVED and polished (status_polish = 1; the route used to write 0), every one is certified on the host, and four of
    them agree with the oracle's polish."""
    assert (base.rec[:, REC_STATUS] == S.OSQP_SOLVED).all(), base.rec[:, REC_STATUS]
    print('status_polish:', base.rec[:, REC_POLISH].astype(int).tolist(), base.plast)
    assert (base.rec[:, REC_POLISH] == 1).all(), base.rec[:, REC_POLISH]
    worst = {}
    for b in range(B):
        fig = _certify(base.P, base.Q[b], base.A, base.L[b], base.U[b], base.x[b], base.y[b], base.rec[b])
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print('worst certificate figures over the batch (relative):', worst)
    record_deviation('lockstep_polish_vs_oracle', 'banded n=400 certificate, worst of %d' % B, bound=1e-9, **worst)
    for b in PICK:
        o = Oracle().setup(base.P, base.Q[b], base.A, base.L[b], base.U[b], **ST)
        xo, yo, io = o.solve()
        assert io.status_val == SOLVED
        xp, yp, ip, sp_ = o.polish(delta=1e-6, polish_refine_iter=3)
        ex, ey, eo = _rel(base.x[b], xp), _rel(base.y[b], yp), abs(base.rec[b, REC_OBJ] - ip.obj_val) / (1 + abs(ip.obj_val))
        record_deviation('lockstep_polish_vs_oracle', 'banded n=400 element %d' % b, dx_rel=ex, dy_rel=ey, dobj_rel=eo, oracle_polish=int(sp_),
                         oracle_pri=ip.pri_res, oracle_dua=ip.dua_res, atol=1e-8)
        print('element %d: |dx| %.2e |dy| %.2e |dobj| %.2e (relative); oracle polish %d, residuals %.1e / %.1e' % (b, ex, ey, eo, sp_, ip.pri_res, ip.dua_res))
        assert sp_ == 1
        assert ex <= 1e-8 and ey <= 1e-8, (b, ex, ey)
        assert eo <= 1e-9, (b, eo)


def test_rejection_is_exact(base):
    """q = 0 inside bounds widened by 1e3: the ADMM point is x = y = 0 with both residuals exactly 0 at the first check, and no polished point improves on
    zero -- the element comes back rejected with its ADMM bits; its neighbours are polished."""
    nb, e = 5, 2
    Q, L, U = base.Q[:nb].copy(), base.L[:nb].copy(), base.U[:nb].copy()
    Q[e] = 0.0; L[e] = base.l - 1e3; U[e] = base.u + 1e3
    x, y, rec = base.sp._solver.hip_batch_solve_lockstep(q=Q, l=L, u=U)
    x0, y0, rec0 = base.s0._solver.hip_batch_solve_lockstep(q=Q, l=L, u=U)
    print('rejected element:', rec[e], 'unpolished:', rec0[e])
    assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all()
    assert rec0[e, REC_PRI] == 0.0 and rec0[e, REC_DUA] == 0.0 and rec0[e, REC_ITER] == 25
    assert rec[e, REC_POLISH] == -1
    assert np.array_equal(x[e], x0[e]) and np.array_equal(y[e], y0[e])
    f = [0, 1, 2, 3, 4, 5, 6, 7, 10]
    assert np.array_equal(rec[e, f], rec0[e, f]), (rec[e], rec0[e])
    others = [b for b in range(nb) if b != e]
    assert (rec[others, REC_POLISH] == 1).all(), rec[:, REC_POLISH]
    p = base.sp._solver.lockstep_polish_last_record()
    assert (p['attempted'], p['accepted'], p['rejected']) == (5, 4, 1), p


def test_admm_part_unchanged_and_off_means_off(base):
    assert np.array_equal(base.rec[:, ADMM_FIELDS], base.rec0[:, ADMM_FIELDS])
    assert (base.rec0[:, REC_POLISH] == 0).all() and (base.rec0[:, REC_POLISH_TIME] == 0).all()
    assert base.last['admm_iters_max'] == base.last0['admm_iters_max'] and base.last['pcg_iters'] == base.last0['pcg_iters'], (base.last, base.last0)
    assert base.last['workspace_bytes'] == base.last0['workspace_bytes']
    assert all(v == 0 for v in base.zero.values()) and all(v == 0 for v in base.plast0.values()), (base.zero, base.plast0)
    try:
        base.sp.update_settings(polishing=False)
        x, y, rec = base.sp._solver.hip_batch_solve_lockstep(q=base.Q, l=base.L, u=base.U)
        last, plast = base.sp._solver.lockstep_last_record(), base.sp._solver.lockstep_polish_last_record()
    finally:
        base.sp.update_settings(polishing=True)
    assert (rec[:, REC_POLISH] == 0).all()
    assert np.array_equal(x, base.x0) and np.array_equal(y, base.y0) and np.array_equal(rec, base.rec0)
    assert last['kernel_launches'] == base.last0['kernel_launches'] and plast['attempted'] == 0 and plast['kernel_launches'] == 0, (last, base.last0, plast)


def test_independence(base):
    """A problem's polished x, y and record (but for the chunk's polish seconds) do not depend on what else is in the batch or where in it the problem sits."""
    p = base.plast
    print(p)
    assert p['attempted'] == B and p['accepted'] + p['rejected'] == B and p['steps_max'] >= 1 + 3, p      # (polish_refine_iter = 3, the default)
    assert p['pcg_iters'] > 0 and p['kernel_launches'] > 0 and p['workspace_bytes'] >= 8 * 64 * (base.n + 4 * base.m)
    assert (base.rec[:, REC_POLISH_TIME] > 0).all()
    for b in PICK:
        x1, y1, r1 = base.sp._solver.hip_batch_solve_lockstep(q=base.Q[b:b + 1], l=base.L[b:b + 1], u=base.U[b:b + 1])
        assert np.array_equal(x1[0], base.x[b]) and np.array_equal(y1[0], base.y[b]) and np.array_equal(r1[0, NOT_TIME], base.rec[b, NOT_TIME]), b
    xr, yr, rr = base.sp._solver.hip_batch_solve_lockstep(q=base.Q[::-1].copy(), l=base.L[::-1].copy(), u=base.U[::-1].copy())
    assert np.array_equal(xr[::-1], base.x) and np.array_equal(yr[::-1], base.y) and np.array_equal(rr[::-1][:, NOT_TIME], base.rec[:, NOT_TIME])


def test_mixed_statuses():
    """test_gpu_batch_lockstep.py::test_statuses' batch -- a solved, a primal infeasible and a dual infeasible element in one chunk -- with polishing: only
    the solved element is polished, the other two keep their certificates bit for bit."""
    n = 420
    rng = np.random.default_rng(7)
    d = 0.5 + rng.random(n); d[0] = 0.0
    P = sp.diags(d, format='csc'); A = sp.vstack([sp.identity(n), sp.identity(n)], format='csc')
    q = rng.standard_normal(n)
    l = np.concatenate([-np.ones(n), -2 * np.ones(n)]); u = np.concatenate([np.ones(n), 2 * np.ones(n)])
    st = dict(eps_abs=1e-6, eps_rel=1e-6, eps_prim_inf=1e-5, eps_dual_inf=1e-5, max_iter=4000, check_termination=25, adaptive_rho_interval=50)
    Q, L, U = np.tile(q, (3, 1)), np.tile(l, (3, 1)), np.tile(u, (3, 1))
    i = 5
    L[1, i] = U[1, i] = 1.0; L[1, n + i] = U[1, n + i] = -1.0
    Q[2, 0] = -1.0; L[2, 0] = L[2, n] = -np.inf; U[2, 0] = U[2, n] = np.inf
    out = []
    for pol in (True, False):
        s = osqp_amd.OSQP(algebra='hip'); s.setup(P, q, A, l, u, verbose=False, polishing=pol, **st)
        out.append(s._solver.hip_batch_solve_lockstep(q=Q, l=L, u=U) + (s._solver.lockstep_polish_last_record(),))
    (x, y, rec, p), (x0, y0, rec0, _) = out
    print('status_polish:', rec[:, REC_POLISH], p)
    assert list(rec[:, REC_STATUS]) == [S.OSQP_SOLVED, S.OSQP_PRIMAL_INFEASIBLE, S.OSQP_DUAL_INFEASIBLE], rec[:, REC_STATUS]
    assert p['attempted'] == 1
    assert rec[0, REC_POLISH] in (1, -1)
    if rec[0, REC_POLISH] == 1:
        _certify(P, Q[0], A, L[0], U[0], x[0], y[0], rec[0])
    for b in (1, 2):
        assert rec[b, REC_POLISH] == 0
        assert np.array_equal(x[b], x0[b], equal_nan=True) and np.array_equal(y[b], y0[b], equal_nan=True) and np.array_equal(rec[b], rec0[b], equal_nan=True), b


def test_delta_and_refine_iter_are_honoured(base):
    """A larger delta_eff contracts less per step, more steps repair it: the same fixed point."""
    nb = 5
    s = _handle(base.P, base.q, base.A, base.l, base.u, polishing=True, delta=1e-2, polish_refine_iter=8)
    x, y, rec = s._solver.hip_batch_solve_lockstep(q=base.Q[:nb], l=base.L[:nb], u=base.U[:nb])
    p = s._solver.lockstep_polish_last_record()
    print(p, [(_rel(x[b], base.x[b]), _rel(y[b], base.y[b])) for b in range(nb)])
    assert (rec[:, REC_POLISH] == 1).all(), rec[:, REC_POLISH]
    assert p['steps_max'] >= 9, p
    for b in range(nb):
        assert _rel(x[b], base.x[b]) < 1e-7 and _rel(y[b], base.y[b]) < 1e-7, b


def test_reordered_handle(base, monkeypatch):
    nb = 5
    monkeypatch.setenv('OSQP_HIP_REORDER', '2')
    s = _handle(base.P, base.q, base.A, base.l, base.u, polishing=True)
    assert s._solver.hip_stats()['reordered'] == 1
    x, y, rec = s._solver.hip_batch_solve_lockstep(q=base.Q[:nb], l=base.L[:nb], u=base.U[:nb])
    print([(_rel(x[b], base.x[b]), _rel(y[b], base.y[b])) for b in range(nb)])
    assert (rec[:, REC_POLISH] == 1).all(), rec[:, REC_POLISH]
    for b in range(nb):
        assert _rel(x[b], base.x[b]) <= 1e-8 and _rel(y[b], base.y[b]) <= 1e-8, b      # (not bitwise: the permutation changes the order of the sums)


def test_device_pointers(base):
    import torch
    dev = torch.device('cuda', 0)
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev).contiguous()
    qd, ld, ud = t(base.Q), t(base.L), t(base.U)
    x = torch.empty((B, base.n), dtype=torch.float64, device=dev); y = torch.empty((B, base.m), dtype=torch.float64, device=dev)
    rec = torch.empty((B, 12), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    base.sp._solver.hip_batch_solve_lockstep_device(B, qd.data_ptr(), ld.data_ptr(), ud.data_ptr(), x.data_ptr(), y.data_ptr(), rec.data_ptr(), warm=False, stream=stream)
    assert np.array_equal(x.cpu().numpy(), base.x) and np.array_equal(y.cpu().numpy(), base.y)
    assert np.array_equal(rec.cpu().numpy()[:, NOT_TIME], base.rec[:, NOT_TIME])


def test_no_constraint_rows():
    """m = 0: the recurrence solves P x = -q.  Three elements of a tridiagonal, strictly diagonally dominant P at n = 900; the polished x is certified as above
    (no primal residual, the dual one at 1e-9 relative)."""
    n = 900
    rng = np.random.default_rng(3)
    d = 1.0 + rng.random(n)
    off = 0.3 * rng.standard_normal(n - 1)
    P = sp.diags([off, d + 1.0, off], [-1, 0, 1], format='csc')
    A = sp.csc_matrix((0, n)); l = np.zeros(0); u = np.zeros(0)
    q = rng.standard_normal(n)
    Q = np.stack([q + 0.1 * b * rng.standard_normal(n) for b in range(3)])
    s = osqp_amd.OSQP(algebra='hip')
    s.setup(P, q, A, l, u, verbose=False, polishing=True, eps_abs=EPS, eps_rel=EPS, max_iter=4000, check_termination=25)
    x, y, rec = s._solver.hip_batch_solve_lockstep(q=Q)
    p = s._solver.lockstep_polish_last_record()
    print(rec[:, [0, 1, 3, 4, 8]], p)
    assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all() and (rec[:, REC_POLISH] == 1).all(), rec
    assert p['attempted'] == 3 and p['steps_max'] >= 4
    for b in range(3):
        _certify(P, Q[b], A, l, u, x[b], y[b], rec[b])
