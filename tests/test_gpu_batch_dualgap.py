"""GPU tier: settings.check_dualgap on the batch routes -- osqp_hip_batch_solve (every batch_variant of k_batch_admm), osqp_hip_batch_solve_lockstep and
osqp_hip_batch_solve_lockstep_direct, with shared and with per-problem matrices, and the torch layer on top.  With the setting a problem ends SOLVED
(SOLVED_INACCURATE at max_iter) only if, besides the residual tests, |gap| < eps_abs + eps_rel max(|obj|, |dual_obj|) (x 10 on the approximate pass), and the
record's column 11 carries the gap of the point the record describes; without it every route is what it was (column 11 = 0).

Routes and problems: hip_batch_solve and hip_batch_solve_lockstep on problems.random_qp(20, 30, seed=3), hip_batch_solve_lockstep_direct on
problems.portfolio_qp(60, 3) where its handle takes that route, else on portfolio_qp(600, 4); batches of 70 (a full chunk and a ragged one) built as
tests/test_gpu_batch_lockstep.py and tests/test_gpu_lockstep_direct.py build theirs.

Bounds.  Column 11 against the gap recomputed in np.longdouble from the returned unscaled x, y (tests/gap_ref.py gap_host): (n + m + r) 2^-53 S with S the
sum of the absolute values of every term and r = 16 roundings per term for scaling and unscaling, counted at gap_ref.ROUNDINGS_SCALING.  The comparison
with the single handle uses tests/test_gpu_lockstep_direct.py's ATOL.

Measured on the MI355X (worst fraction of the column-11 bound; a record, not a tolerance; DESIGN.md section 6 "Duality gap on the batch routes"):
hip_batch_solve 0.017 .. 0.020 over the variants, lockstep 0.023, direct 0.0012; with P_b = s_b P 0.019 / 0.018 / 0.0037.  Element 0 of the random_qp batch
stops at 218 iterations without and 231 with the setting; the direct route and the single handle took equal iteration counts on all 70 elements."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import gap_ref as G
import osqp_amd
import problems
from util import record_deviation

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
S = osqp_amd.SolverStatus
B = 70
PICK = (0, 63, 64, 69)
EPS = 1e-5
WIN = dict(eps_abs=EPS, eps_rel=EPS, check_termination=1, adaptive_rho=False, max_iter=20000, warm_starting=False)      # the window test's settings
ROUTES = ['batch-v%d' % v for v in range(6)] + ['lockstep', 'direct']      # batch_variant 0 (automatic: the spectral workgroup form where it applies) and 1 .. 5
SOLVED, INACC, MAXIT = int(S.OSQP_SOLVED), int(S.OSQP_SOLVED_INACCURATE), int(S.OSQP_MAX_ITER_REACHED)


def _full(P):
    U = sp.triu(sp.csc_matrix(P), format='csc')
    return (U + sp.triu(U, 1).T).tocsc()


def _batch(q, l, u, nb, seed=13):          # (tests/test_gpu_batch_lockstep.py _batch)
    rng = np.random.default_rng(seed)
    return (np.stack([q + 0.05 * b * rng.standard_normal(len(q)) for b in range(nb)]), np.stack([l - 0.01 * b for b in range(nb)]), np.stack([u + 0.01 * b for b in range(nb)]))


def _portfolio_batch(na, k):               # (tests/test_gpu_lockstep_direct.py Base)
    P, q, A, l, u = problems.portfolio_qp(na, k)
    rng = np.random.default_rng(17)
    Q = np.stack([np.concatenate([-rng.standard_normal(na) / (1.0 + 0.05 * b), np.zeros(k)]) for b in range(B)])
    L, U = np.tile(l, (B, 1)), np.tile(u, (B, 1))
    for b in (3, 63, 66):
        U[b, k + 1:] = (0.02 + 0.01 * rng.random(na)) * (600.0 / na)          # (scaled with 1 / na: the budget row, sum = 1, stays feasible at either size)
    return P, q, A, l, u, Q, L, U


class Route:
    """a handle, its batch and the entry that solves it; solve(**settings) updates the handle's settings first"""
    def __init__(self, name, **st):
        self.name = name
        if name == 'direct':
            for na, k in ((60, 3), (600, 4)):
                self.P, self.q, self.A, self.l, self.u, self.Q, self.L, self.U = _portfolio_batch(na, k)
                self.s = self._handle(st)
                try:
                    self.s._solver.hip_batch_solve_lockstep_direct_device(0, None, None, None, None, None, None)      # the applicability query
                    break
                except ValueError:
                    continue
            self.shape = (na, k)
            self.entry = self.s._solver.hip_batch_solve_lockstep_direct
        else:
            self.P, self.q, self.A, self.l, self.u = problems.random_qp(20, 30, seed=3)
            self.Q, self.L, self.U = _batch(self.q, self.l, self.u, B)
            self.s = self._handle(st)
            if name.startswith('batch-v'):
                self.s._solver.set_policy(batch_variant=int(name[-1]))
                self.entry = self.s._solver.hip_batch_solve
            else:
                self.entry = self.s._solver.hip_batch_solve_lockstep
        self.Pf = _full(self.P)
        self.n, self.m = len(self.q), len(self.l)
        self.cache = {}

    def _handle(self, st):
        s = osqp_amd.OSQP(algebra='hip')
        s.setup(self.P, self.q, self.A, self.l, self.u, verbose=False, **dict(WIN, **st))
        return s

    def solve(self, rows=slice(None), Px=None, **st):
        self.s.update_settings(**dict(dict(check_dualgap=False, polishing=False, max_iter=WIN['max_iter'], eps_abs=EPS, eps_rel=EPS), **st))
        return self.entry(q=self.Q[rows], l=self.L[rows], u=self.U[rows], **({'Px': Px} if Px is not None else {}))

    def full(self, gap):
        """the whole batch at the window settings, to the end, with / without the setting (computed once)"""
        if gap not in self.cache:
            self.cache[gap] = self.solve(check_dualgap=bool(gap))
        return self.cache[gap]


_routes = {}


def route(name):
    if name not in _routes:
        _routes[name] = Route(name)
    return _routes[name]


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _gap_fraction(R, b, x, y, gap, P=None):
    ref, mag = G.gap_host(R.Pf if P is None else P, R.Q[b], R.A, R.L[b], R.U[b], x, y)
    return float(abs(np.longdouble(gap) - ref)) / G.gap_bound(R.n, R.m, mag)


# ---------------------------------------------------------------------------------------------------------------- 3: the window
@pytest.mark.parametrize('name', ROUTES)
def test_window_between_the_two_stopping_points(name):
    """max_iter = K for K from three iterations below an element's stopping point without the setting up to its stopping point with it (every K where
    that window is short, its ends and a stride through its middle otherwise: the direct route's is about a thousand iterations wide), the whole batch
    under both settings.  Every element at every K: the element with the setting never stops earlier; where both stop at the same iteration, x, y and
    columns 1 - 10 are bit-equal and its status is SOLVED exactly when the other's is and its own column 11 passes the test (SOLVED_INACCURATE: the
    other's is SOLVED or SOLVED_INACCURATE and column 11 passes at 10 x), else MAX_ITER_REACHED; where it goes on alone, its status is backed by its
    own column 11.  "Residuals pass, gap fails" must occur."""
    R = route(name)
    (x0, y0, r0), (x1, y1, r1) = R.full(0), R.full(1)
    assert (r0[:, 0] == SOLVED).all() and (r1[:, 0] == SOLVED).all(), (r0[:, 0], r1[:, 0])
    K0, K1 = r0[:, 1].astype(int), r1[:, 1].astype(int)
    assert (K1 >= K0).all() and (K1 > K0).any(), (K0, K1)
    print(name, 'iterations without / with check_dualgap:', list(zip(K0, K1)))
    late = np.nonzero(K1 > K0)[0]
    b = int(late[np.argmin(K1[late])])                      # the element whose window ends first: no chunk runs past it
    lo, hi = int(K0[b]) - 3, int(K1[b])
    Ks = list(range(lo, hi + 1)) if hi - lo <= 24 else sorted(set(list(range(lo, lo + 6)) + list(range(hi - 2, hi + 1)) + [int(v) for v in np.linspace(lo + 6, hi - 3, 4)]))
    held = same = 0
    for K in Ks:
        xa, ya, ra = R.solve(check_dualgap=False, max_iter=K)
        xb, yb, rb = R.solve(check_dualgap=True, max_iter=K)
        assert (ra[:, 11] == 0).all()
        for e in range(B):
            sa, sb, ia, ib = int(ra[e, 0]), int(rb[e, 0]), int(ra[e, 1]), int(rb[e, 1])
            assert ib >= ia and sa in (SOLVED, INACC, MAXIT) and sb in (SOLVED, INACC, MAXIT), (K, e, sa, sb, ia, ib)
            ok1, ok10 = G.gap_passes(rb[e, 2], rb[e, 11], EPS, EPS), G.gap_passes(rb[e, 2], rb[e, 11], EPS, EPS, True)
            if ib == ia:
                same += 1
                assert _bits(xa[e], xb[e]) and _bits(ya[e], yb[e]) and _bits(ra[e, 1:11], rb[e, 1:11]), (K, e)
                want = SOLVED if (sa == SOLVED and ok1) else (INACC if (ib == K and sa in (SOLVED, INACC) and ok10) else MAXIT)
                assert sb == want, (K, e, sa, sb, want, rb[e, 2], rb[e, 11])
                held += sa == SOLVED and sb != SOLVED
            else:
                assert sa == SOLVED and (ib == K or sb == SOLVED), (K, e, sa, sb, ia, ib)
                assert (sb != SOLVED or ok1) and (sb != INACC or ok10), (K, e, sb, rb[e, 2], rb[e, 11])
    print(name, 'K =', Ks, ': elements compared at the same iteration', same, ', residuals passed and the gap held the element', held)
    assert held > 0 and same > held


# ---------------------------------------------------------------------------------------------------------------- 4: column 11 against the host
@pytest.mark.parametrize('name', ROUTES)
def test_column_eleven_is_the_gap_of_the_returned_point(name):
    R = route(name)
    x, y, rec = R.full(1)
    fr = [_gap_fraction(R, b, x[b], y[b], rec[b, 11]) for b in range(B)]
    print(name, 'column 11 against the host: worst fraction of the bound %.3g' % max(fr))
    record_deviation('batch_dualgap', name, gap_fraction=max(fr))
    assert max(fr) <= 1.0, fr
    for b in range(B):
        assert rec[b, 11] != 0 and G.gap_passes(rec[b, 2], rec[b, 11], EPS, EPS)


@pytest.mark.parametrize('name', ['batch-v0', 'lockstep', 'direct'])
def test_column_eleven_with_per_problem_matrices(name):
    """P_b = s_b P, s_b over 1e-2 .. 1e2: the elements' cost scales c differ by orders of magnitude -- a kernel that took the handle's cinv would miss the
    bound by as much.  The handle's own settings but adaptive rho on and eps 1e-6 (the scaled problems are far from the handle's rho)."""
    R = Route(name, adaptive_rho=True, check_termination=25, eps_abs=1e-6, eps_rel=1e-6, check_dualgap=True)
    sb = np.logspace(-2, 2, B)
    Px = sb[:, None] * sp.triu(sp.csc_matrix(R.P), format='csc').data[None, :]
    x, y, rec = R.entry(q=R.Q, l=R.L, u=R.U, Px=Px)
    assert np.isin(rec[:, 0], (SOLVED, MAXIT)).all() and (rec[:, 0] == SOLVED).sum() >= B // 2, rec[:, 0]
    fr = [_gap_fraction(R, b, x[b], y[b], rec[b, 11], P=sb[b] * R.Pf) for b in range(B)]
    print(name, 'per-problem matrices, column 11 against the host: worst fraction of the bound %.3g' % max(fr), 'statuses', np.unique(rec[:, 0], return_counts=True))
    record_deviation('batch_dualgap', name + '-mat', gap_fraction=max(fr))
    assert max(fr) <= 1.0, fr
    assert all(G.gap_passes(rec[b, 2], rec[b, 11], 1e-6, 1e-6) for b in range(B) if rec[b, 0] == SOLVED)


# ---------------------------------------------------------------------------------------------------------------- 5: only the stopping decision changes
@pytest.mark.parametrize('name', ROUTES)
def test_the_iterates_are_those_of_a_solve_that_is_simply_told_to_stop_there(name):
    R = route(name)
    x, y, rec = R.full(1)
    K0 = R.full(0)[2][:, 1]
    picks = sorted(set(PICK) | {int(np.argmax(rec[:, 1] - K0))})
    for b in picks:
        K = int(rec[b, 1])
        xe, ye, re = R.solve(rows=slice(b, b + 1), check_dualgap=False, eps_abs=1e-12, eps_rel=1e-12, max_iter=K)
        assert int(re[0, 1]) == K and int(re[0, 0]) == MAXIT and re[0, 11] == 0
        assert _bits(xe[0], x[b]) and _bits(ye[0], y[b]), b


# ---------------------------------------------------------------------------------------------------------------- 6: flag off
@pytest.mark.parametrize('name', ROUTES)
def test_without_the_setting_column_eleven_is_zero(name):
    assert (route(name).full(0)[2][:, 11] == 0).all()


def test_control_shape_takes_the_same_path_and_one_more_launch_per_check():
    """problems.banded_qp(400, window=40) at tests/test_gpu_batch_lockstep.py's settings: the gap never decides -- equal iteration counts, x, y and columns
    0 - 10 bit-equal; the ADMM part's kernel launches differ by one k_ls_supp per termination check of every chunk (a chunk checks every 25 iterations
    until its slowest problem ends)."""
    from test_gpu_batch_lockstep import ST, _batch as lb
    P, q, A, l, u = problems.banded_qp(400, window=40)
    Q, L, U = lb(q, l, u, B)
    s = osqp_amd.OSQP(algebra='hip'); s.setup(P, q, A, l, u, verbose=False, **ST)
    x0, y0, r0 = s._solver.hip_batch_solve_lockstep(q=Q, l=L, u=U)
    last0 = s._solver.lockstep_last_record()
    s.update_settings(check_dualgap=True)
    x1, y1, r1 = s._solver.hip_batch_solve_lockstep(q=Q, l=L, u=U)
    last1 = s._solver.lockstep_last_record()
    assert (r0[:, 0] == SOLVED).all() and _bits(x0, x1) and _bits(y0, y1) and _bits(r0[:, :11], r1[:, :11])
    assert (r0[:, 11] == 0).all() and (r1[:, 11] != 0).all()
    checks = sum(int(r0[c:c + 64, 1].max()) // ST['check_termination'] for c in range(0, B, 64))
    assert last1['kernel_launches'] - last0['kernel_launches'] == checks, (last0, last1, checks)
    s.update_settings(check_dualgap=False)
    x2, y2, r2 = s._solver.hip_batch_solve_lockstep(q=Q, l=L, u=U)
    assert _bits(r2, r0) and s._solver.lockstep_last_record()['kernel_launches'] == last0['kernel_launches']


def test_a_large_batch_with_the_setting_stays_off_the_wave_kernel():
    nb = 2048
    P, q, A, L, U = problems.mpc_batch(nb)
    s = osqp_amd.OSQP(); s.setup(P, q, A, L[0], U[0], eps_abs=1e-6, eps_rel=1e-6, verbose=False, max_iter=4000)
    x0, y0, r0 = s._solver.hip_batch_solve(l=L, u=U)
    assert s._solver.hip_stats()['batch_wave_split'] >= 0 and (r0[:, 11] == 0).all()
    s.update_settings(check_dualgap=True)
    x1, y1, r1 = s._solver.hip_batch_solve(l=L, u=U)
    assert s._solver.hip_stats()['batch_wave_split'] == -1
    assert (r1[:, 0] == SOLVED).all() and (r1[:, 11] != 0).all() and all(G.gap_passes(r1[b, 2], r1[b, 11], 1e-6, 1e-6) for b in range(nb))
    s.update_settings(check_dualgap=False)
    s._solver.hip_batch_solve(l=L, u=U)
    assert s._solver.hip_stats()['batch_wave_split'] >= 0


# ---------------------------------------------------------------------------------------------------------------- 7: the direct route against the single handle
def test_direct_route_against_the_single_handle_with_the_setting():
    """tests/test_gpu_lockstep_direct.py's shape, settings, batch and _single loop with check_dualgap on both sides.  Both sides round the gap differently: an
    element whose gap sits on the threshold at a check may differ by one check -- at most 2 of 70, each printed with both gaps, each still passing the test."""
    import test_gpu_lockstep_direct as D
    base = D.Base.__new__(D.Base)
    base.P, base.q, base.A, base.l, base.u = problems.portfolio_qp(D.Base.NA, D.Base.K)
    rng = np.random.default_rng(17)
    base.Q = np.stack([np.concatenate([-rng.standard_normal(D.Base.NA) / (1.0 + 0.05 * b), np.zeros(D.Base.K)]) for b in range(B)])
    base.L, base.U = np.tile(base.l, (B, 1)), np.tile(base.u, (B, 1))
    for b in (3, 63, 66):
        base.U[b, D.Base.K + 1:] = 0.02 + 0.01 * rng.random(D.Base.NA)
    s = D._handle(base.P, base.q, base.A, base.l, base.u, check_dualgap=True)
    x, y, rec = s._solver.hip_batch_solve_lockstep_direct(q=base.Q, l=base.L, u=base.U)
    s.update_settings(check_dualgap=False)
    r0 = s._solver.hip_batch_solve_lockstep_direct(q=base.Q, l=base.L, u=base.U)[2]
    assert (rec[:, 1] >= r0[:, 1]).all() and (rec[:, 1] > r0[:, 1]).any(), (rec[:, 1], r0[:, 1])
    single = D._single(D._handle(base.P, base.q, base.A, base.l, base.u, check_dualgap=True), base.Q, base.L, base.U)
    excused = []
    for b, r in enumerate(single):
        assert r.info.status_val == rec[b, 0] == SOLVED, b
        assert D._close(x[b], r.x) <= D.ATOL and D._close(y[b], r.y) <= D.ATOL, b
        if int(r.info.iter) != int(rec[b, 1]):
            print('element %d: %d iterations (single handle %d); gaps %.17g / %.17g' % (b, rec[b, 1], r.info.iter, rec[b, 11], r.info.duality_gap))
            assert abs(int(r.info.iter) - int(rec[b, 1])) == D.ST['check_termination'] and G.gap_passes(rec[b, 2], rec[b, 11], D.EPS, D.EPS)
            assert G.gap_passes(r.info.obj_val, r.info.duality_gap, D.EPS, D.EPS)
            excused.append(b)
    assert len(excused) <= 2, excused


# ---------------------------------------------------------------------------------------------------------------- 8: independence and polish
@pytest.mark.parametrize('name', ROUTES)
def test_independence_with_the_setting(name):
    R = route(name)
    x, y, rec = R.full(1)
    for b in PICK:
        x1, y1, r1 = R.solve(rows=slice(b, b + 1), check_dualgap=True)
        assert _bits(x1[0], x[b]) and _bits(y1[0], y[b]) and _bits(r1[0], rec[b]), b
    xr, yr, rr = R.solve(rows=slice(None, None, -1), check_dualgap=True)
    assert _bits(xr[::-1], x) and _bits(yr[::-1], y) and _bits(rr[::-1], rec)


@pytest.mark.parametrize('name', ['batch-v1', 'batch-v2', 'lockstep', 'direct'])
def test_polish_carries_the_polished_points_gap(name):
    """polishing with the setting: an accepted element's column 11 is the gap of the polished x, y (the bound of test 4 at that point), a rejected or
    unattempted element's is its ADMM gap, bit for bit that of the unpolished call."""
    R = route(name)
    x, y, rec = R.full(1)
    xp, yp, rp = R.solve(check_dualgap=True, polishing=True)
    acc, rej = np.nonzero(rp[:, 8] == 1)[0], np.nonzero(rp[:, 8] != 1)[0]
    print(name, 'polish accepted', len(acc), 'rejected / not attempted', len(rej))
    assert len(acc) > 0
    fr = [_gap_fraction(R, b, xp[b], yp[b], rp[b, 11]) for b in acc]
    record_deviation('batch_dualgap', name + '-polish', gap_fraction=max(fr))
    assert max(fr) <= 1.0, fr
    for b in rej:
        assert _bits(rp[b, 11], rec[b, 11]) and _bits(xp[b], x[b]) and _bits(yp[b], y[b]), b
    assert any(not _bits(rp[b, 11], rec[b, 11]) for b in acc)              # (the polished point is another point: so is its gap)


# ---------------------------------------------------------------------------------------------------------------- 9: the torch layer
def test_torch_layer_hands_the_setting_to_the_handle():
    import torch
    from osqp_amd.nn.torch import OSQP as OSQPLayer
    P, q, A, l, u = problems.random_qp(20, 30, seed=3)
    Q, L, U = _batch(q, l, u, 8)
    Pc, Ac = sp.coo_matrix(_full(P)), sp.coo_matrix(A)
    t = lambda a: torch.tensor(np.ascontiguousarray(a))
    for gap in (False, True):
        layer = OSQPLayer((Pc.row, Pc.col), Pc.shape, (Ac.row, Ac.col), Ac.shape, eps_abs=EPS, eps_rel=EPS, **({'check_dualgap': True} if gap else {}))
        layer(t(Pc.data), t(Q), t(Ac.data), t(L), t(U))                                     # shared matrices: the batch kernel
        assert bool(layer._solver.settings.check_dualgap) == gap
        rec = np.asarray(layer.last_rec)
        assert ((rec[:, 11] != 0).all() and all(G.gap_passes(r[2], r[11], EPS, EPS) for r in rec if r[0] == SOLVED)) if gap else (rec[:, 11] == 0).all()
        Pv = t(np.linspace(0.8, 1.25, 8)[:, None] * Pc.data[None, :])
        layer(Pv, t(Q), t(Ac.data), t(L), t(U))                                             # per-element P_val: the batch kernel with per-problem matrices
        rec = np.asarray(layer.last_rec)
        assert layer.mat_batch_launches == 1
        assert ((rec[:, 11] != 0).all() and all(G.gap_passes(r[2], r[11], EPS, EPS) for r in rec if r[0] == SOLVED)) if gap else (rec[:, 11] == 0).all()
