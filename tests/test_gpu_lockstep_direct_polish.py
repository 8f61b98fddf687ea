"""GPU tier: polish on the DIRECT lockstep route (settings.polishing with osqp_hip_batch_solve_lockstep_direct[_device]; lockstep_hip.hip
lockstep_direct_chunk, "polish").  Every problem of a chunk that ends SOLVED is polished by the recurrence of "polish of a chunk" with the Woodbury solve
in place of the PCG; the others are left alone.  tests/direct_polish_ref.py restates the recurrence on the CPU.

The base is that of test_gpu_lockstep_direct.py -- portfolio_qp(600, 4), n = 604, m = 605, r = 5, B = 70 (one full chunk and a ragged one of 6), the same
Q / L / U draw -- at eps = 1e-6, check_termination = 25, adaptive_rho_interval = 50, warm_starting off, on a polishing and a never-polishing handle.

Bounds.  A polished point is certified on the host: both KKT residuals <= 64 * 2^-52 * rho_bar * (1 + scale) = 1.42e-8 (1 + scale) with rho_bar = 1 / delta =
1e6 and the scales of test_gpu_lockstep_polish.py::_certify.  The recurrence's y step, y += rho_bar (z~ - z), multiplies the rounding error of z~ by
rho_bar: that is the floor of the dual residual in fp64 (the CPU restatement itself sits at 0.6 - 1e-9 relative), and 64 is the project's kernel-tier
margin.  The record's objective to 1e-9 relative of the certificate's.  Against the oracle's polish (delta = 1e-6, three refinement steps): x and y to
1e-8, the objective to 1e-9 relative -- the PCG route's bounds.  The oracle accepts polish on all 70 elements of this batch (checked on the CPU)."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_amd
import problems
import test_direct_polish_ref as ref
import test_gpu_lockstep_direct as shared
from oracle import Oracle, SOLVED
from util import record_deviation

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
S = osqp_amd.SolverStatus
EPS = 1e-6
B, PICK = shared.B, shared.PICK
ST = dict(eps_abs=EPS, eps_rel=EPS, max_iter=50000, adaptive_rho_interval=50, check_termination=25, warm_starting=False)
ORACLE_ST = {k: v for k, v in ST.items() if k != 'warm_starting'}
REC_STATUS, REC_ITER, REC_OBJ, REC_PRI, REC_DUA, REC_POLISH, REC_POLISH_TIME = 0, 1, 2, 3, 4, 8, 9
ADMM_FIELDS = [0, 1, 5, 6, 7, 10]                  # status, iter, rho, rho_updates, pcg_iters, rho_estimate
NOT_TIME = [f for f in range(12) if f != REC_POLISH_TIME]
RHO_BAR = 1e6                                      # 1 / delta
CERT = 64 * 2.0 ** -52 * RHO_BAR                   # 1.42e-8
WORST = {}                                         # the worst ratio to each bound seen in this session (printed by the tests that add to it)


def _handle(P, q, A, l, u, **kw):
    st = dict(ST); st.update(kw)
    s = osqp_amd.OSQP(algebra='hip')
    s.setup(P, q, A, l, u, verbose=False, **st)
    return s


def _rel(a, b):
    return np.abs(a - b).max() / (1 + np.abs(b).max())


def _ratio(name, value, bound):
    WORST[name] = max(WORST.get(name, 0.0), value / bound)


def certify(P, q, A, l, u, x, y, rec):
    """the certificate of a polished point at CERT (1 + scale); returns the figures relative to (1 + scale)"""
    k = problems.kkt_certificate(P, q, A, l, u, x, y)
    ax = A @ x
    scale_p = 1 + max(np.abs(ax).max(), np.abs(np.clip(ax, l, u)).max())
    scale_d = 1 + max(np.abs(P @ x).max(), np.abs(A.T @ y).max(), np.abs(q).max())
    fig = dict(pri=k['pri'] / scale_p, dua=k['dua'] / scale_d, rec_pri=rec[REC_PRI] / scale_p, rec_dua=rec[REC_DUA] / scale_d,
               obj=abs(k['obj'] - rec[REC_OBJ]) / (1 + abs(k['obj'])))
    _ratio('certificate pri', fig['pri'], CERT); _ratio('certificate dua', fig['dua'], CERT); _ratio('certificate obj', fig['obj'], 1e-9)
    assert k['pri'] <= CERT * scale_p and k['dua'] <= CERT * scale_d, (k, fig)
    assert abs(k['obj'] - rec[REC_OBJ]) <= 1e-9 * (1 + abs(k['obj'])), (k, rec)
    return fig


def against_oracle(test, case, P, q, A, l, u, x, y, rec):
    """x, y, objective against the oracle's polish of the same QP (delta = 1e-6, three refinement steps)"""
    o = Oracle().setup(P, q, A, l, u, **ORACLE_ST)
    _, _, io = o.solve()
    assert io.status_val == SOLVED
    xp, yp, ip, sp_ = o.polish(delta=1e-6, polish_refine_iter=3)
    ex, ey, eo = _rel(x, xp), _rel(y, yp), abs(rec[REC_OBJ] - ip.obj_val) / (1 + abs(ip.obj_val))
    record_deviation(test, case, dx_rel=ex, dy_rel=ey, dobj_rel=eo, oracle_polish=int(sp_), oracle_pri=ip.pri_res, oracle_dua=ip.dua_res, atol=1e-8)
    print('%s: |dx| %.2e |dy| %.2e |dobj| %.2e (relative); oracle polish %d, residuals %.1e / %.1e' % (case, ex, ey, eo, sp_, ip.pri_res, ip.dua_res))
    _ratio('oracle dx', ex, 1e-8); _ratio('oracle dy', ey, 1e-8); _ratio('oracle obj', eo, 1e-9)
    assert sp_ == 1
    assert ex <= 1e-8 and ey <= 1e-8, (case, ex, ey)
    assert eo <= 1e-9, (case, eo)


class Base:
    def __init__(self):
        self.P, self.A, self.Q, self.L, self.U = ref.base_batch()
        _, self.q, _, self.l, self.u = problems.portfolio_qp(600, 4)
        self.n, self.m = len(self.q), len(self.l)
        self.kw = dict(q=self.Q, l=self.L, u=self.U)
        self.sp = _handle(self.P, self.q, self.A, self.l, self.u, polishing=True)        # the polishing handle
        self.s0 = _handle(self.P, self.q, self.A, self.l, self.u)                        # the never-polishing one
        self.zero = self.sp._solver.lockstep_polish_last_record()
        self.x, self.y, self.rec = self.sp._solver.hip_batch_solve_lockstep_direct(**self.kw)
        self.last, self.plast = self.sp._solver.lockstep_direct_last_record(), self.sp._solver.lockstep_polish_last_record()
        self.x0, self.y0, self.rec0 = self.s0._solver.hip_batch_solve_lockstep_direct(**self.kw)
        self.last0, self.plast0 = self.s0._solver.lockstep_direct_last_record(), self.s0._solver.lockstep_polish_last_record()


@pytest.fixture(scope='module')
def base():
    return Base()


def test_polished_and_certified(base):
    """Every element of the batch is SOLVED and polished (status_polish = 1; the route used to write 0), every one is certified on the host, and four of
    them agree with the oracle's polish."""
    assert (base.n, base.m) == (604, 605) and base.sp._solver.hip_stats()['woodbury_rows'] == 5
    assert (base.rec[:, REC_STATUS] == S.OSQP_SOLVED).all(), base.rec[:, REC_STATUS]
    print('status_polish:', base.rec[:, REC_POLISH].astype(int).tolist(), base.plast)
    assert (base.rec[:, REC_POLISH] == 1).all(), base.rec[:, REC_POLISH]
    worst = {}
    for b in range(B):
        fig = certify(base.P, base.Q[b], base.A, base.L[b], base.U[b], base.x[b], base.y[b], base.rec[b])
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print('worst certificate figures over the batch (relative):', worst)
    record_deviation('lockstep_direct_polish_vs_oracle', 'portfolio 600x4 certificate, worst of %d' % B, bound=CERT, **worst)
    for b in PICK:
        against_oracle('lockstep_direct_polish_vs_oracle', 'portfolio 600x4 element %d' % b, base.P, base.Q[b], base.A, base.L[b], base.U[b], base.x[b], base.y[b], base.rec[b])
    print('worst ratio to each bound:', {k: '%.2e' % v for k, v in WORST.items()})
    record_deviation('lockstep_direct_polish_vs_oracle', 'worst ratio to each bound', **WORST)


def test_rejection_is_exact(base):
    """q = 0 inside bounds widened by 1e3: the ADMM point has both residuals exactly 0 at the first check, and no polished point improves on that -- the
    element comes back rejected with its ADMM bits; its neighbours are polished."""
    nb, e = 5, 2
    Q, L, U = base.Q[:nb].copy(), base.L[:nb].copy(), base.U[:nb].copy()
    Q[e] = 0.0; L[e] = base.l - 1e3; U[e] = base.u + 1e3
    x, y, rec = base.sp._solver.hip_batch_solve_lockstep_direct(q=Q, l=L, u=U)
    p = base.sp._solver.lockstep_polish_last_record()
    x0, y0, rec0 = base.s0._solver.hip_batch_solve_lockstep_direct(q=Q, l=L, u=U)
    print('rejected element:', rec[e], 'unpolished:', rec0[e])
    assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all()
    assert rec0[e, REC_PRI] == 0.0 and rec0[e, REC_DUA] == 0.0 and rec0[e, REC_ITER] == 25
    assert rec[e, REC_POLISH] == -1
    assert np.array_equal(x[e], x0[e]) and np.array_equal(y[e], y0[e])
    f = [0, 1, 2, 3, 4, 5, 6, 7, 10]
    assert np.array_equal(rec[e, f], rec0[e, f]), (rec[e], rec0[e])
    others = [b for b in range(nb) if b != e]
    assert (rec[others, REC_POLISH] == 1).all(), rec[:, REC_POLISH]
    assert (p['attempted'], p['accepted'], p['rejected']) == (5, 4, 1), p


def test_admm_part_unchanged_and_off_means_off(base):
    assert np.array_equal(base.rec[:, ADMM_FIELDS], base.rec0[:, ADMM_FIELDS])
    assert (base.rec0[:, REC_POLISH] == 0).all() and (base.rec0[:, REC_POLISH_TIME] == 0).all()
    for k in ('admm_iters_max', 'factorisations', 'workspace_bytes'):
        assert base.last[k] == base.last0[k], (k, base.last, base.last0)
    assert all(v == 0 for v in base.zero.values()) and all(v == 0 for v in base.plast0.values()), (base.zero, base.plast0)
    try:
        base.sp.update_settings(polishing=False)
        x, y, rec = base.sp._solver.hip_batch_solve_lockstep_direct(**base.kw)
        last, plast = base.sp._solver.lockstep_direct_last_record(), base.sp._solver.lockstep_polish_last_record()
    finally:
        base.sp.update_settings(polishing=True)
    assert (rec[:, REC_POLISH] == 0).all()
    assert np.array_equal(x, base.x0) and np.array_equal(y, base.y0) and np.array_equal(rec, base.rec0)
    assert last['kernel_launches'] == base.last0['kernel_launches'] and plast['attempted'] == 0 and plast['kernel_launches'] == 0, (last, base.last0, plast)


def test_independence(base):
    """A problem's polished x, y and record (but for the chunk's polish seconds) do not depend on what else is in the batch or where in it the problem
    sits.  S is inverted once per attempted problem for polish: the direct record's `factorisations` is the total less `attempted`, and it equals the
    never-polishing handle's."""
    p = base.plast
    print(p, base.last)
    assert p['attempted'] == B and p['accepted'] + p['rejected'] == B and p['steps_max'] >= 1 + 3, p      # (polish_refine_iter = 3, the default)
    assert p['pcg_iters'] == 0 and p['kernel_launches'] > 0 and p['gpu_ms'] > 0 and p['workspace_bytes'] >= 8 * 64 * (base.n + 4 * base.m), p
    assert base.last['factorisations'] == base.last0['factorisations'] == B + base.rec0[:, 6].sum(), (base.last, base.last0)
    assert (base.rec[:, REC_POLISH_TIME] > 0).all()
    solve = base.sp._solver.hip_batch_solve_lockstep_direct
    for b in PICK:
        x1, y1, r1 = solve(q=base.Q[b:b + 1], l=base.L[b:b + 1], u=base.U[b:b + 1])
        assert np.array_equal(x1[0], base.x[b]) and np.array_equal(y1[0], base.y[b]) and np.array_equal(r1[0, NOT_TIME], base.rec[b, NOT_TIME]), b
    xr, yr, rr = solve(q=base.Q[::-1].copy(), l=base.L[::-1].copy(), u=base.U[::-1].copy())
    assert np.array_equal(xr[::-1], base.x) and np.array_equal(yr[::-1], base.y) and np.array_equal(rr[::-1][:, NOT_TIME], base.rec[:, NOT_TIME])


class Shared:
    """test_gpu_lockstep_direct.py's Chunk reads P, q, A, l, u, Q, L, U and K of its base"""
    K = 4

    def __init__(self, base):
        for k in ('P', 'q', 'A', 'l', 'u', 'Q', 'L', 'U'):
            setattr(self, k, getattr(base, k))


def test_mixed_statuses(base, monkeypatch):
    """test_gpu_lockstep_direct.py's Chunk -- a solved, a primal infeasible and a stopped element in one chunk -- on a polishing and on a plain handle: only
    the solved element is polished, the other two keep their outputs bit for bit, NaNs included."""
    plain = shared.Chunk(Shared(base))
    monkeypatch.setattr(shared.Chunk, 'ST', dict(shared.Chunk.ST, polishing=True))
    pol = shared.Chunk(Shared(base))
    p = pol.s._solver.lockstep_polish_last_record()
    rec, rec0 = pol.rec, plain.rec
    print('statuses', rec[:, REC_STATUS], 'status_polish', rec[:, REC_POLISH], p)
    assert pol.cap == plain.cap
    assert list(rec[:2, REC_STATUS]) == [S.OSQP_SOLVED, S.OSQP_PRIMAL_INFEASIBLE] and int(rec[2, REC_STATUS]) in shared.STOPPED
    assert p['attempted'] == 1 and rec[0, REC_POLISH] in (1, -1)
    assert np.array_equal(rec[0, ADMM_FIELDS], rec0[0, ADMM_FIELDS])
    for b in (1, 2):
        assert rec[b, REC_POLISH] == 0
        eq = lambda a, c: np.array_equal(a, c, equal_nan=True)
        assert eq(pol.x[b], plain.x[b]) and eq(pol.y[b], plain.y[b]) and eq(rec[b], rec0[b]), b


def test_delta_and_refine_iter_are_honoured(base):
    """A larger delta_eff contracts less per step, more steps repair it: the same fixed point.  (On the CPU the oracle accepts delta = 1e-4 with eight
    refinement steps on this QP and lands on the default polish to 1e-15; it rejects delta = 1e-2, which is therefore not asked for.)"""
    nb = 5
    s = _handle(base.P, base.q, base.A, base.l, base.u, polishing=True, delta=1e-4, polish_refine_iter=8)
    x, y, rec = s._solver.hip_batch_solve_lockstep_direct(q=base.Q[:nb], l=base.L[:nb], u=base.U[:nb])
    p = s._solver.lockstep_polish_last_record()
    print(p, [(_rel(x[b], base.x[b]), _rel(y[b], base.y[b])) for b in range(nb)])
    assert (rec[:, REC_POLISH] == 1).all(), rec[:, REC_POLISH]
    assert p['steps_max'] >= 9, p
    for b in range(nb):
        assert _rel(x[b], base.x[b]) < 1e-7 and _rel(y[b], base.y[b]) < 1e-7, b


def _edge(name, P, q, A, l, u, r):
    """test_gpu_lockstep_direct.py::_edge's three elements on a polishing handle: polished, certified, within 1e-8 of the oracle's polish"""
    Q, L, U = ref.edge_batch(q, l, u)
    s = _handle(P, q, A, l, u, polishing=True)
    assert s._solver.hip_stats()['woodbury_rows'] == r
    x, y, rec = s._solver.hip_batch_solve_lockstep_direct(q=Q, l=L, u=U)
    print(s._solver.lockstep_polish_last_record())
    assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all() and (rec[:, REC_POLISH] == 1).all(), rec[:, [REC_STATUS, REC_POLISH]]
    for b in range(3):
        fig = certify(P, Q[b], A, L[b], U[b], x[b], y[b], rec[b])
        record_deviation('lockstep_direct_polish_vs_oracle', '%s certificate element %d' % (name, b), bound=CERT, **fig)
        against_oracle('lockstep_direct_polish_vs_oracle', '%s element %d' % (name, b), P, Q[b], A, L[b], U[b], x[b], y[b], rec[b])
    print('worst ratio to each bound so far:', {k: '%.2e' % v for k, v in WORST.items()})


def test_one_dense_row():
    _edge('one dense row', *ref.one_dense_row_qp(), 1)


def test_128_dense_rows():
    """r = 128: k_lw_inv holds S_b in 129 KB of LDS, here under polish's rho_bar"""
    _edge('128 dense rows', *shared._factor_qp(400, 127, 0.7), 128)


def test_device_pointers(base):
    import torch
    dev = torch.device('cuda', 0)
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev).contiguous()
    qd, ld, ud = t(base.Q), t(base.L), t(base.U)
    x = torch.empty((B, base.n), dtype=torch.float64, device=dev); y = torch.empty((B, base.m), dtype=torch.float64, device=dev)
    rec = torch.empty((B, 12), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    base.sp._solver.hip_batch_solve_lockstep_direct_device(B, qd.data_ptr(), ld.data_ptr(), ud.data_ptr(), x.data_ptr(), y.data_ptr(), rec.data_ptr(), warm=False, stream=stream)
    assert np.array_equal(x.cpu().numpy(), base.x) and np.array_equal(y.cpu().numpy(), base.y)
    assert np.array_equal(rec.cpu().numpy()[:, NOT_TIME], base.rec[:, NOT_TIME])


def _prod2_child(out):
    """Runs in a child process of the test below (OSQP_HIP_LS_POL_PROD2 is read once per process): the base batch, shared and with per-problem matrices"""
    import test_gpu_lockstep_direct_mat as mat
    P, A, Q, L, U = ref.base_batch()
    P, A = mat._csc(sp.triu(P)), mat._csc(A)
    _, q, _, l, u = problems.portfolio_qp(600, 4)
    s = _handle(P, q, A, l, u, polishing=True)
    x, y, rec = s._solver.hip_batch_solve_lockstep_direct(q=Q, l=L, u=U)
    Px, Ax = mat._perturb(P, A, B)
    xm, ym, recm = s._solver.hip_batch_solve_lockstep_direct(q=Q, l=L, u=U, Px=Px, Ax=Ax)
    np.savez(out, x=x, y=y, rec=rec, xm=xm, ym=ym, recm=recm, launches=s._solver.lockstep_polish_last_record()['kernel_launches'])


def test_prod2_bits(tmp_path):
    """The recurrence's dense rows by one two-operand product (k_lw_prod2 / k_lwm_prod2, the default) and by two k_lw_prod launches
    (OSQP_HIP_LS_POL_PROD2=0): x, y and the records but for the polish seconds are bit-equal, with shared and with per-problem matrices; the fused form
    saves one launch per step."""
    res = []
    for flag in ('0', '1'):
        out = str(tmp_path / ('prod2_%s.npz' % flag))
        env = dict(os.environ, OSQP_HIP_LS_POL_PROD2=flag, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
        r = subprocess.run([sys.executable, '-c', 'import sys, test_gpu_lockstep_direct_polish as t; t._prod2_child(sys.argv[1])', out], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        res.append(np.load(out))
    two, one = res
    assert (one['rec'][:, REC_POLISH] == 1).all() and (one['recm'][:, REC_POLISH] == 1).all()
    for k in ('x', 'y', 'xm', 'ym'):
        assert np.array_equal(two[k], one[k]), k
    for k in ('rec', 'recm'):
        assert np.array_equal(two[k][:, NOT_TIME], one[k][:, NOT_TIME]), k
    print('polish launches: two products %d, one fused %d' % (two['launches'], one['launches']))
    assert one['launches'] < two['launches']


def test_records_moved():
    """On a polishing portfolio_qp(256, 1) handle (n = 257, r = 2: the smallest the route accepts), B = 2: the shared call moves exactly {direct, polish},
    the call with per-problem matrices {direct, direct_mat, polish}; the two direct adjoint calls move no polish record."""
    import test_gpu_lockstep_entry_table as table
    h = table.Handle(problems.portfolio_qp(256, 1), polishing=True, **ST)
    s = h.solver
    (x, y, rec), after = h.step(lambda: s.hip_batch_solve_lockstep_direct(q=h.Q), {'direct', 'polish'})
    assert after['polish']['attempted'] == 2 and after['polish']['workspace_bytes'] > 0 and after['polish']['pcg_iters'] == 0, after['polish']
    assert (rec[:, REC_POLISH] != 0).all()
    (xm, ym, recm), after = h.step(lambda: s.hip_batch_solve_lockstep_direct(q=h.Q, Px=h.Px, Ax=h.Ax), {'direct', 'direct_mat', 'polish'})
    assert after['polish']['attempted'] == 2 and (recm[:, REC_POLISH] != 0).all()
    dx = np.ones_like(x)
    h.step(lambda: s.hip_batch_adjoint_lockstep_direct(x, y, dx), {'direct_adjoint'})
    h.step(lambda: s.hip_batch_adjoint_lockstep_direct(xm, ym, dx, Px=h.Px, Ax=h.Ax), {'direct_adjoint', 'direct_mat_adjoint'})


def test_torch_layer():
    """Layer(large_batch='lockstep_direct', polishing=True), three elements, with 1-D and with 2-D P_val / A_val: ONE call of the entry, every element
    polished, and the layer with large_batch='loop' (the handle's own polish per element) agrees at 1e-8.  The shape is portfolio_qp(460, 1) (n = 461,
    r = 2), just past the batch kernel (10 n + 8 m + 16 > 8192 doubles): portfolio_qp(256, 1) fits one workgroup's LDS, so the layer's route table hands
    it to hip_batch_solve and never reaches this entry."""
    import torch
    from osqp_amd.nn.torch import OSQP as Layer
    import test_gpu_lockstep_direct_mat as mat
    nb = 3
    P, q, A, l, u = problems.portfolio_qp(460, 1)
    assert 10 * len(q) + 8 * len(l) + 16 > 8192
    Pc, Ac = mat._csc(sp.triu(P)), mat._csc(A)
    pco, aco = Pc.tocoo(), Ac.tocoo()
    mk = lambda **kw: Layer((pco.row, pco.col), Pc.shape, (aco.row, aco.col), Ac.shape, eps_rel=EPS, eps_abs=EPS, max_iter=50000, polishing=True, **kw)
    Q = np.stack([q * (1.0 + 0.05 * b) for b in range(nb)])
    Px, Ax = mat._perturb(Pc, Ac, nb)
    for name, pv, av in (('1-D', Pc.data, Ac.data), ('2-D', Px, Ax)):
        direct, loop = mk(large_batch='lockstep_direct'), mk(large_batch='loop')
        ts = [torch.tensor(np.array(v), dtype=torch.float64) for v in (pv, Q, av, np.tile(l, (nb, 1)), np.tile(u, (nb, 1)))]
        with torch.no_grad():
            x, xl = direct(*ts), loop(*ts)
        ext = direct._solver._solver
        print(name, ext.lockstep_direct_last_record(), ext.lockstep_polish_last_record())
        assert direct.setup_count == 1 and direct.mat_lockstep_direct_launches == (1 if pv.ndim == 2 else 0)
        assert ext.lockstep_direct_last_record()['chunks'] == 1 and ext.lockstep_polish_last_record()['attempted'] == nb
        assert (direct.last_rec[:, REC_POLISH] == 1).all(), direct.last_rec[:, REC_POLISH]
        assert loop._solver._solver.lockstep_direct_last_record()['chunks'] == 0
        e = _rel(x.numpy(), xl.numpy())
        print('%s values: direct layer against the loop layer |dx| %.2e' % (name, e))
        assert e <= 1e-8, (name, e)
