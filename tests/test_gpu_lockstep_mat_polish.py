"""GPU tier: polish on the lockstep route with PER-PROBLEM MATRICES (settings.polishing with osqp_hip_batch_solve_lockstep_mat[_device];
lockstep_hip.hip "polish of a chunk" on the chunk's own matrix block).  Every problem of a chunk that ends SOLVED is polished on its own P_b, A_b under its
own D_b, E_b, c_b by the recurrence Engine::polish runs on the PCG path; the others are left alone.

The batch is test_gpu_lockstep_mat.py's own Base: banded_qp(400, window=40), n = 400, m = 800, B = 70 (one full chunk and a ragged one of 6),
default_rng(3) in its draw order, that file's ST (eps 1e-8, check_termination = 25, adaptive_rho_interval = 50) -- on two handles, its own (which never
polishes) and one set up with polishing=True.  eps is 1e-8 and not the shared polish test's 1e-6 because on this batch the oracle's polished points have
an active inequality multiplier as small as 4.5e-6 and a smallest inactive slack of 1.0e-4: an ADMM point at 1e-6 would guess the active set with almost
no margin, at 1e-8 the margin is more than two orders of magnitude.

Bounds.  They are test_gpu_lockstep_polish.py's -- the same recurrence, the same delta_eff, the same inner tolerance: a polished point is certified on
the host at 1e-9 x (1 + scale) in both KKT residuals and the record's objective to 1e-9 relative (its _certify, imported); against the oracle's polish
(delta = 1e-6, three refinement steps) on the element's own matrices x and y to 1e-8.  Two routes that are each within 1e-8 of the same oracle point
are within 2e-8 of each other (tests 5 and 10)."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_amd
from oracle import Oracle, SOLVED
from util import record_deviation
from test_gpu_batch_lockstep import ST, ATOL, EPS, B, PICK, _handle
from test_gpu_lockstep_mat import Base as MatBase
from test_gpu_lockstep_polish import ADMM_FIELDS, NOT_TIME, REC_STATUS, REC_ITER, REC_OBJ, REC_POLISH, REC_POLISH_TIME, _certify

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
S = osqp_amd.SolverStatus
assert EPS == 1e-8 and ST['check_termination'] == 25 and ST['adaptive_rho_interval'] == 50


def _rel(a, b):
    return float(np.abs(a - b).max() / (1 + np.abs(b).max()))


class Base(MatBase):
    """test_gpu_lockstep_mat.py's batch; s / x / y / rec are the never-polishing handle's, sp / xp / yp / recp the polishing one's"""
    def __init__(self):
        super().__init__()
        self.plast0 = self.s._solver.lockstep_polish_last_record()
        self.sp = _handle(self.P, self.q, self.A, self.l, self.u, polishing=True)
        self.xp, self.yp, self.recp = self.sp._solver.hip_batch_solve_lockstep(q=self.Q, l=self.L, u=self.U, Px=self.Px, Ax=self.Ax)
        self.mlast, self.plast = self.sp._solver.lockstep_mat_last_record(), self.sp._solver.lockstep_polish_last_record()
        self._opol = {}

    def oracle_polish(self, key, P, q, A, l, u):
        """the oracle's ADMM solve at ST and its polish of that point; computed once per key"""
        if key not in self._opol:
            o = Oracle().setup(P, q, A, l, u, **ST)
            xo, yo, io = o.solve()
            assert io.status_val == SOLVED
            xq, yq, iq, sq = o.polish(delta=1e-6, polish_refine_iter=3)
            assert sq == 1
            self._opol[key] = (xq, yq, iq)
        return self._opol[key]

    def elem(self, b):
        return self.P_of(b), self.Q[b], self.A_of(b), self.L[b], self.U[b]


@pytest.fixture(scope='module')
def base():
    return Base()


def _against_polish(base, tag, b, prob, x, y, rec):
    xq, yq, iq = base.oracle_polish((tag, b), *prob)
    ex, ey, eo = _rel(x, xq), _rel(y, yq), abs(rec[REC_OBJ] - iq.obj_val) / (1 + abs(iq.obj_val))
    record_deviation('lockstep_mat_polish_vs_oracle', '%s element %d' % (tag, b), dx_rel=ex, dy_rel=ey, dobj_rel=eo, oracle_pri=iq.pri_res, oracle_dua=iq.dua_res, atol=1e-8)
    print('%s element %d: |dx| %.2e |dy| %.2e |dobj| %.2e (relative); oracle polish residuals %.1e / %.1e' % (tag, b, ex, ey, eo, iq.pri_res, iq.dua_res))
    assert ex <= 1e-8 and ey <= 1e-8, (tag, b, ex, ey)
    assert eo <= 1e-9, (tag, b, eo)


def test_polished_and_certified(base):
    """1. All 70 are SOLVED and polished (status_polish = 1; this entry used to pass polish off and write 0), every one is certified on the host against its
    own P_b, A_b, four of them agree with the oracle's polish on their own matrices."""
    assert (base.recp[:, REC_STATUS] == S.OSQP_SOLVED).all(), base.recp[:, REC_STATUS]
    print('status_polish:', base.recp[:, REC_POLISH].astype(int).tolist(), base.plast)
    assert (base.recp[:, REC_POLISH] == 1).all(), base.recp[:, REC_POLISH]
    worst = {}
    for b in range(B):
        fig = _certify(*base.elem(b), base.xp[b], base.yp[b], base.recp[b])
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print('worst certificate figures over the batch (relative):', worst)
    record_deviation('lockstep_mat_polish_vs_oracle', 'banded n=400 certificate, worst of %d' % B, bound=1e-9, **worst)
    for b in PICK:
        _against_polish(base, 'batch', b, base.elem(b), base.xp[b], base.yp[b], base.recp[b])
    assert (base.recp[:, REC_POLISH_TIME] > 0).all()
    p = base.plast
    assert p['attempted'] == B and p['accepted'] == B and p['rejected'] == 0, p
    assert p['steps_max'] >= 1 + 3 and p['pcg_iters'] > 0 and p['kernel_launches'] > 0, p                # (polish_refine_iter = 3, the default)
    assert p['workspace_bytes'] >= 8 * 64 * (base.n + 4 * base.m), p


def test_admm_part_unchanged_and_off_means_off(base):
    """2. Polish leaves the ADMM part's record fields and statistics alone; with polishing switched off the polishing handle returns the never-polishing
    one's bits with the same launches and a zero polish record."""
    assert np.array_equal(base.recp[:, ADMM_FIELDS], base.rec[:, ADMM_FIELDS])
    assert (base.rec[:, REC_POLISH] == 0).all() and (base.rec[:, REC_POLISH_TIME] == 0).all()
    assert base.mlast['kernel_launches'] == base.last['kernel_launches'] and base.mlast['pcg_iters'] == base.last['pcg_iters'], (base.mlast, base.last)
    assert base.mlast['admm_iters_max'] == base.last['admm_iters_max'] and base.mlast['matrix_block_bytes'] == base.last['matrix_block_bytes']
    assert all(v == 0 for v in base.plast0.values()), base.plast0
    try:
        base.sp.update_settings(polishing=False)
        x, y, rec = base.sp._solver.hip_batch_solve_lockstep(q=base.Q, l=base.L, u=base.U, Px=base.Px, Ax=base.Ax)
        last, plast = base.sp._solver.lockstep_mat_last_record(), base.sp._solver.lockstep_polish_last_record()
    finally:
        base.sp.update_settings(polishing=True)
    assert (rec[:, REC_POLISH] == 0).all()
    assert np.array_equal(x, base.x) and np.array_equal(y, base.y) and np.array_equal(rec, base.rec)
    assert last['kernel_launches'] == base.last['kernel_launches'], (last, base.last)
    assert all(v == 0 for v in plast.values()), plast


def test_rejection_is_exact(base):
    """3. test_gpu_lockstep_polish.py::test_rejection_is_exact with per-element matrices: q = 0 inside bounds widened by 1e3 -- the ADMM point is
    x = y = 0 with both residuals exactly 0 at the first check and no polished point improves on zero.  The element comes back rejected with its ADMM
    bits; its four neighbours are polished."""
    nb, e = 5, 2
    Q, L, U = base.Q[:nb].copy(), base.L[:nb].copy(), base.U[:nb].copy()
    Q[e] = 0.0; L[e] = base.l - 1e3; U[e] = base.u + 1e3
    kw = dict(q=Q, l=L, u=U, Px=base.Px[:nb], Ax=base.Ax[:nb])
    x, y, rec = base.sp._solver.hip_batch_solve_lockstep(**kw)
    p = base.sp._solver.lockstep_polish_last_record()
    x0, y0, rec0 = base.s._solver.hip_batch_solve_lockstep(**kw)
    print('rejected element:', rec[e], 'unpolished:', rec0[e])
    assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all()
    assert rec[e, REC_POLISH] == -1
    assert np.array_equal(x[e], x0[e]) and np.array_equal(y[e], y0[e])
    f = [0, 1, 2, 3, 4, 5, 6, 7, 10]
    assert np.array_equal(rec[e, f], rec0[e, f]), (rec[e], rec0[e])
    others = [b for b in range(nb) if b != e]
    assert (rec[others, REC_POLISH] == 1).all(), rec[:, REC_POLISH]
    assert (p['attempted'], p['accepted'], p['rejected']) == (5, 4, 1), p


def test_independence(base):
    """4. A problem's polished x, y and record (but for the chunk's polish seconds) do not depend on what else is in the batch or where in it the problem
    sits; its matrices are part of the problem."""
    for b in PICK:
        x1, y1, r1 = base.sp._solver.hip_batch_solve_lockstep(q=base.Q[b:b + 1], l=base.L[b:b + 1], u=base.U[b:b + 1], Px=base.Px[b:b + 1], Ax=base.Ax[b:b + 1])
        assert np.array_equal(x1[0], base.xp[b]) and np.array_equal(y1[0], base.yp[b]) and np.array_equal(r1[0, NOT_TIME], base.recp[b, NOT_TIME]), b
    rv = lambda a: a[::-1].copy()
    xr, yr, rr = base.sp._solver.hip_batch_solve_lockstep(q=rv(base.Q), l=rv(base.L), u=rv(base.U), Px=rv(base.Px), Ax=rv(base.Ax))
    assert np.array_equal(xr[::-1], base.xp) and np.array_equal(yr[::-1], base.yp) and np.array_equal(rr[::-1][:, NOT_TIME], base.recp[:, NOT_TIME])


def test_its_own_handle(base):
    """5. Elements 0 and 5 against a fresh polishing handle set up with that element's data alone, through its shared lockstep solve: the same polish
    status, x and y within 2e-8 relative (each is within 1e-8 of the same oracle point); the observed deviation is recorded.  Observed on the MI355X:
    0 -- the polished x, y equal the own handle's bit for bit for both elements, as the unpolished forward did (recorded, not required)."""
    for b in (0, 5):
        f = _handle(*base.elem(b), polishing=True)
        x1, y1, r1 = f._solver.hip_batch_solve_lockstep(nbatch=1)
        ex, ey = _rel(base.xp[b], x1[0]), _rel(base.yp[b], y1[0])
        bits = bool(np.array_equal(base.xp[b], x1[0]) and np.array_equal(base.yp[b], y1[0]))
        record_deviation('lockstep_mat_polish_vs_own_handle', 'element %d' % b, dx_rel=ex, dy_rel=ey, bit_identical=int(bits), iters=int(base.recp[b, REC_ITER]),
                         own_iters=int(r1[0, REC_ITER]), bound=2e-8)
        print('element %d: mat call %d iterations, its own handle %d; polished |dx| %.2e |dy| %.2e; bit-identical: %s' % (b, base.recp[b, REC_ITER], r1[0, REC_ITER], ex, ey, bits))
        assert r1[0, REC_STATUS] == S.OSQP_SOLVED and r1[0, REC_POLISH] == base.recp[b, REC_POLISH] == 1
        assert ex <= 2e-8 and ey <= 2e-8, (b, ex, ey)


def test_one_side_only(base):
    """6. Ax alone and Px alone (the other side is the handle's own), with test_gpu_lockstep_mat.py::test_one_side_only's bounds: all seven polished,
    elements 0 and 6 against the oracle's polish."""
    nb = 7
    sl = slice(0, nb)
    x, y, rec = base.sp._solver.hip_batch_solve_lockstep(q=base.Q[sl], l=base.L[sl], u=base.U[sl], Ax=base.Ax[sl])
    assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all() and (rec[:, REC_POLISH] == 1).all(), rec[:, [REC_STATUS, REC_POLISH]]
    for b in (0, 6):
        _against_polish(base, 'Ax alone', b, (base.P, base.Q[b], base.A_of(b), base.L[b], base.U[b]), x[b], y[b], rec[b])
    L0, U0 = np.tile(base.l_own, (nb, 1)), np.tile(base.u_own, (nb, 1))
    x, y, rec = base.sp._solver.hip_batch_solve_lockstep(q=base.Q[sl], l=L0, u=U0, Px=base.Px[sl])
    assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all() and (rec[:, REC_POLISH] == 1).all(), rec[:, [REC_STATUS, REC_POLISH]]
    for b in (0, 6):
        _against_polish(base, 'Px alone', b, (base.P_of(b), base.Q[b], base.A, L0[b], U0[b]), x[b], y[b], rec[b])


def test_statuses_in_one_chunk():
    """7. test_gpu_lockstep_mat.py::test_statuses_in_one_chunk's three elements -- solved, primal infeasible, dual infeasible, each with its own multiple
    of A's values -- on a polishing and a non-polishing handle: only the solved one is polished, the other two keep x, y and record bit for bit."""
    n = 420
    rng = np.random.default_rng(7)
    d = 0.5 + rng.random(n); d[0] = 0.0
    P = sp.diags(d, format='csc'); A = sp.vstack([sp.identity(n), sp.identity(n)], format='csc')
    q = rng.standard_normal(n)
    l = np.concatenate([-np.ones(n), -2 * np.ones(n)]); u = np.concatenate([np.ones(n), 2 * np.ones(n)])
    st = dict(eps_abs=1e-6, eps_rel=1e-6, eps_prim_inf=1e-5, eps_dual_inf=1e-5, max_iter=4000, check_termination=25, adaptive_rho_interval=50)
    Q, L, U = np.tile(q, (3, 1)), np.tile(l, (3, 1)), np.tile(u, (3, 1))
    i = 5
    L[1, i] = U[1, i] = 1.0; L[1, n + i] = U[1, n + i] = -1.0                   # x_i = 1 and x_i = -1
    Q[2, 0] = -1.0; L[2, 0] = L[2, n] = -np.inf; U[2, 0] = U[2, n] = np.inf     # x_0 free, zero curvature, negative cost
    f = np.array([1.0, 3.0, 0.5])
    Ax = f[:, None] * np.tile(A.data, (3, 1)); L, U = f[:, None] * L, f[:, None] * U
    out = []
    for pol in (True, False):
        s = osqp_amd.OSQP(algebra='hip'); s.setup(P, q, A, l, u, verbose=False, polishing=pol, **st)
        out.append(s._solver.hip_batch_solve_lockstep(q=Q, l=L, u=U, Ax=Ax) + (s._solver.lockstep_polish_last_record(),))
    (x, y, rec, p), (x0, y0, rec0, _) = out
    print('status_polish:', rec[:, REC_POLISH], p)
    assert list(rec[:, REC_STATUS]) == [S.OSQP_SOLVED, S.OSQP_PRIMAL_INFEASIBLE, S.OSQP_DUAL_INFEASIBLE], rec[:, REC_STATUS]
    assert p['attempted'] == 1, p
    assert rec[0, REC_POLISH] in (1, -1)
    if rec[0, REC_POLISH] == 1:
        A0 = sp.csc_matrix((Ax[0], A.indices, A.indptr), shape=A.shape)
        _certify(P, Q[0], A0, L[0], U[0], x[0], y[0], rec[0])
    for b in (1, 2):
        assert rec[b, REC_POLISH] == 0
        assert np.array_equal(x[b], x0[b], equal_nan=True) and np.array_equal(y[b], y0[b], equal_nan=True) and np.array_equal(rec[b], rec0[b], equal_nan=True), b


def test_no_constraint_rows():
    """8. m = 0: the recurrence solves P_b x = -q_b.  The tridiagonal, strictly diagonally dominant P at n = 900 of
    test_gpu_lockstep_polish.py::test_no_constraint_rows on three elements, each with its own factors on the diagonal (Px only)."""
    n = 900
    rng = np.random.default_rng(3)
    d = 1.0 + rng.random(n)
    off = 0.3 * rng.standard_normal(n - 1)
    P = sp.diags([off, d + 1.0, off], [-1, 0, 1], format='csc')
    A = sp.csc_matrix((0, n)); l = np.zeros(0); u = np.zeros(0)
    q = rng.standard_normal(n)
    Q = np.stack([q + 0.1 * b * rng.standard_normal(n) for b in range(3)])
    Pu = sp.triu(P, format='csc'); Pu.sort_indices()
    diag = np.repeat(np.arange(n), np.diff(Pu.indptr)) == Pu.indices
    Px = np.tile(Pu.data, (3, 1))
    Px[:, diag] *= 1 + 0.2 * rng.random((3, n))                                  # (every P_b stays strictly diagonally dominant)
    s = osqp_amd.OSQP(algebra='hip')
    s.setup(P, q, A, l, u, verbose=False, polishing=True, eps_abs=1e-6, eps_rel=1e-6, max_iter=4000, check_termination=25)
    x, y, rec = s._solver.hip_batch_solve_lockstep(q=Q, Px=Px)
    p = s._solver.lockstep_polish_last_record()
    print(rec[:, [0, 1, 3, 4, 8]], p)
    assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all() and (rec[:, REC_POLISH] == 1).all(), rec
    assert p['attempted'] == 3 and p['steps_max'] >= 4, p
    for b in range(3):
        U_ = sp.csc_matrix((Px[b], Pu.indices, Pu.indptr), shape=P.shape)
        Pb = (U_ + sp.triu(U_, 1).T).tocsc()
        g = np.abs(Pb @ x[b] + Q[b]).max()
        scale = 1 + max(np.abs(Pb @ x[b]).max(), np.abs(Q[b]).max())
        print('element %d: max |P_b x + q_b| = %.2e (relative %.2e)' % (b, g, g / scale))
        assert g <= 1e-9 * scale, (b, g, scale)
        _certify(Pb, Q[b], A, l, u, x[b], y[b], rec[b])


def test_device_pointers(base):
    """9. The device entry on torch tensors gives the host entry's bits in every field but the polish seconds."""
    import torch
    nb = 33
    dev = torch.device('cuda', 0)
    t = lambda a: torch.tensor(a[:nb], dtype=torch.float64, device=dev).contiguous()
    qd, ld, ud, pd, ad = t(base.Q), t(base.L), t(base.U), t(base.Px), t(base.Ax)
    x = torch.empty((nb, base.n), dtype=torch.float64, device=dev); y = torch.empty((nb, base.m), dtype=torch.float64, device=dev)
    rec = torch.empty((nb, 12), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    base.sp._solver.hip_batch_solve_lockstep_device(nb, qd.data_ptr(), ld.data_ptr(), ud.data_ptr(), x.data_ptr(), y.data_ptr(), rec.data_ptr(), warm=False, stream=stream,
                                                    Px_ptr=pd.data_ptr(), Ax_ptr=ad.data_ptr())
    p = base.sp._solver.lockstep_polish_last_record()
    assert p['attempted'] == nb and p['accepted'] == nb and p['workspace_bytes'] > 0, p
    r = rec.cpu().numpy()
    assert np.array_equal(x.cpu().numpy(), base.xp[:nb]) and np.array_equal(y.cpu().numpy(), base.yp[:nb])
    assert np.array_equal(r[:, NOT_TIME], base.recp[:nb][:, NOT_TIME]) and (r[:, REC_POLISH_TIME] > 0).all()


def test_reordered_handle(base, monkeypatch):
    """10. A handle that works on a permuted copy: five elements polished and certified, within 2e-8 of the unreordered handle's polished points (each is
    within 1e-8 of the same oracle point; not bitwise: the permutation changes the order of the sums)."""
    nb = 5
    monkeypatch.setenv('OSQP_HIP_REORDER', '2')
    s = _handle(base.P, base.q, base.A, base.l, base.u, polishing=True)
    assert s._solver.hip_stats()['reordered'] == 1
    sl = slice(0, nb)
    x, y, rec = s._solver.hip_batch_solve_lockstep(q=base.Q[sl], l=base.L[sl], u=base.U[sl], Px=base.Px[sl], Ax=base.Ax[sl])
    assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all() and (rec[:, REC_POLISH] == 1).all(), rec[:, [REC_STATUS, REC_POLISH]]
    for b in range(nb):
        _certify(*base.elem(b), x[b], y[b], rec[b])
        ex, ey = _rel(x[b], base.xp[b]), _rel(y[b], base.yp[b])
        record_deviation('lockstep_mat_polish_reordered', 'element %d' % b, dx_rel=ex, dy_rel=ey, bound=2e-8)
        assert ex <= 2e-8 and ey <= 2e-8, (b, ex, ey)


def test_handle_is_untouched(base):
    """11. solve(), [polishing mat call,] solve() on two handles: the handle's matrices, scaling, iterates and launch history are not touched."""
    out = []
    for call in (False, True):
        s = _handle(base.P, base.q, base.A, base.l, base.u, eps_abs=1e-6, eps_rel=1e-6, polishing=True)
        sc_a = s._solver.hip_scaling()
        ra = s.solve()
        if call:
            x, y, rec = s._solver.hip_batch_solve_lockstep(q=base.Q[:3], l=base.L[:3], u=base.U[:3], Px=base.Px[:3], Ax=base.Ax[:3])
            assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all() and (rec[:, REC_POLISH] != 0).all(), rec[:, [REC_STATUS, REC_POLISH]]
            sc_b = s._solver.hip_scaling()
            assert np.array_equal(sc_a[0], sc_b[0]) and np.array_equal(sc_a[1], sc_b[1]) and sc_a[2] == sc_b[2]
        rb = s.solve()
        out.append((ra, rb))
    (a0, b0), (a1, b1) = out
    assert np.array_equal(a0.x, a1.x) and np.array_equal(a0.y, a1.y) and a0.info.iter == a1.info.iter
    assert np.array_equal(b0.x, b1.x) and np.array_equal(b0.y, b1.y) and b0.info.iter == b1.info.iter and b0.info.status_val == b1.info.status_val == S.OSQP_SOLVED
    assert b0.info.status_polish == b1.info.status_polish


def test_torch_layer(base):
    """12. 2-D P_val / A_val with inputs requiring grad: polishing=True with large_batch='lockstep' / large_backward='lockstep' makes ONE forward call that
    polishes all twelve and ONE backward call; a layer built without the keyword does not polish and agrees within the unpolished tolerance."""
    import torch
    from osqp_amd.nn.torch import OSQP as Layer
    nb = 12
    Pc = sp.csc_matrix(base.P); Pc.sort_indices()
    Ac = sp.csc_matrix(base.A); Ac.sort_indices()
    pco, aco = Pc.tocoo(), Ac.tocoo()
    mk = lambda **kw: Layer((pco.row, pco.col), Pc.shape, (aco.row, aco.col), Ac.shape, eps_rel=EPS, eps_abs=EPS, max_iter=200000, large_batch='lockstep', large_backward='lockstep', **kw)
    Pfull = np.stack([base.P_of(b).tocoo().data for b in range(nb)])              # (the pattern of every P_b is P's: same order of entries)
    assert all(np.array_equal(base.P_of(b).indices, Pc.indices) for b in (0, nb - 1)) and Pfull.shape == (nb, Pc.nnz)
    vals = (Pfull, base.Q[:nb], base.Ax[:nb], base.L[:nb], base.U[:nb])
    lock, plain = mk(polishing=True), mk()
    ts = [torch.tensor(np.array(v), dtype=torch.float64, requires_grad=True) for v in vals]
    x = lock(*ts)
    X = x.detach().numpy()
    assert lock.mat_lockstep_launches == 1 and lock.setup_count == 1
    p = lock._solver._solver.lockstep_polish_last_record()
    assert p['attempted'] == nb and p['accepted'] == nb, p
    assert (lock.last_rec[:, REC_POLISH] == 1).all(), lock.last_rec[:, REC_POLISH]
    for b in (0, nb - 1):
        xq, yq, iq = base.oracle_polish(('batch', b), *base.elem(b))
        ex = _rel(X[b], xq)
        record_deviation('lockstep_mat_polish_torch_vs_oracle', 'element %d' % b, dx_rel=ex, atol=1e-8)
        assert ex <= 1e-8, (b, ex)
    (0.5 * (x ** 2).sum()).backward()
    assert lock.mat_lockstep_adjoint_launches == 1
    arec = torch.as_tensor(lock.last_adjoint_rec).cpu().numpy()
    assert arec.shape == (nb, 4) and (arec[:, 0] == 0).all(), arec
    with torch.no_grad():
        X0 = plain(*[t.detach() for t in ts]).numpy()
    assert plain.mat_lockstep_launches == 1 and (plain.last_rec[:, REC_POLISH] == 0).all(), plain.last_rec[:, REC_POLISH]
    assert all(v == 0 for v in plain._solver._solver.lockstep_polish_last_record().values())
    for b in range(nb):
        assert _rel(X[b], X0[b]) <= ATOL, b
