"""GPU tier: the direct lockstep route (osqp_hip_batch_solve_lockstep_direct[_device]; osqp-python_amd/csrc/lockstep_hip.hip "lockstep DIRECT") -- a batch of
QPs that share P and A on a Woodbury-corrected handle whose K0 is diagonal: r dense rows next to one-entry rows, P diagonal (the factor-model
portfolio QP).  Every shape is past the batch kernel (10 n + 8 m + 16 > 8192 doubles), hip_batch_solve and hip_batch_solve_lockstep both decline it.

Bounds.  Solutions of two eps = 1e-8 iterates of the same QP are compared at ATOL = 2e-6 relative to the solution's scale, the yardstick of
test_gpu_batch_lockstep.py; certificates use that file's rule: residuals <= 1.01 (eps + eps scale), objective to 1e-6 relative."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_amd
import problems
from osqp_amd import ext_hip
from oracle import Oracle, SOLVED
from util import record_deviation

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
S = osqp_amd.SolverStatus
NOT_IMPL = ext_hip.osqp_error_type.OSQP_FUNC_NOT_IMPLEMENTED
EPS = 1e-8
ATOL = 2e-6
B = 70                     # one full chunk of 64 and a ragged one of 6
PICK = (0, 63, 64, 69)     # first / last lane of the full chunk, first / last of the ragged one
ST = dict(eps_abs=EPS, eps_rel=EPS, max_iter=50000, adaptive_rho_interval=50, check_termination=25, warm_starting=False)
REC_STATUS, REC_ITER, REC_OBJ, REC_RHO, REC_RHOUPD, REC_PCG = 0, 1, 2, 5, 6, 7


def _handle(P, q, A, l, u, **kw):
    st = dict(ST); st.update(kw)
    s = osqp_amd.OSQP(algebra='hip')
    s.setup(P, q, A, l, u, verbose=False, **st)
    return s


def _certify(P, q, A, l, u, x, y, obj, eps=EPS):      # (tests/test_gpu_batch_lockstep.py _certify)
    k = problems.kkt_certificate(P, q, A, l, u, x, y)
    ax = A @ x
    scale_p = max(np.abs(ax).max(), np.abs(np.clip(ax, l, u)).max())
    scale_d = max(np.abs(P @ x).max(), np.abs(A.T @ y).max(), np.abs(q).max())
    assert k['pri'] <= 1.01 * (eps + eps * scale_p), k
    assert k['dua'] <= 1.01 * (eps + eps * scale_d), k
    assert abs(k['obj'] - obj) <= 1e-6 * (1 + abs(k['obj']))


def _past_both(s, n, m, r, **kw):
    """The shape is past the batch kernel, both existing batch routes decline the handle, and it has the intended number of dense rows."""
    assert 10 * n + 8 * m + 16 > 8192
    assert s._solver.hip_stats()['woodbury_rows'] == r
    for route in (s._solver.hip_batch_solve, s._solver.hip_batch_solve_lockstep):
        with pytest.raises(ValueError) as e:
            route(**kw)
        assert e.value.code == NOT_IMPL


def _single(s, Q, L, U):
    """update(q, l, u) + solve() per element on the single handle, every element under the handle's settings: cold (warm_starting is off) and from the rho
    of setup.  A solve leaves its adapted rho in the handle's settings (as the reference does, _osqp.py:923-930) and the next solve of a plain loop would
    start from it: a different setting per element, set by the order of the loop.  A batch element starts from the settings whatever else the batch holds
    (test_independence), so the loop is given them back before every element."""
    out, rho = [], s.settings.rho
    for b in range(len(Q)):
        s.update_settings(rho=rho)
        s.update(q=Q[b], l=L[b], u=U[b])
        out.append(s.solve())
    return out


def _close(x, xr):
    return np.abs(x - xr).max() / (1 + np.abs(xr).max())


def _factor_qp(na, k, density, seed=3):
    """problems.portfolio_qp with the density of F as an argument (rows of F' with more than 128 entries need it at small na)."""
    rng = np.random.default_rng(seed)
    F = sp.random(na, k, density=density, random_state=rng, data_rvs=rng.standard_normal, format='csc')
    D = sp.diags(rng.random(na) * np.sqrt(k))
    mu = rng.standard_normal(na)
    P = sp.block_diag([2.0 * D, 2.0 * sp.eye(k)], format='csc')
    q = np.concatenate([-mu, np.zeros(k)])
    A = sp.vstack([sp.hstack([F.T, -sp.eye(k)]), sp.hstack([sp.csc_matrix(np.ones((1, na))), sp.csc_matrix((1, k))]),
                   sp.hstack([sp.eye(na), sp.csc_matrix((na, k))])], format='csc')
    l = np.concatenate([np.zeros(k), [1.0], np.zeros(na)])
    u = np.concatenate([np.zeros(k), [1.0], np.ones(na)])
    return P, q, A, l, u


class Base:
    NA, K = 600, 4

    def __init__(self):
        self.P, self.q, self.A, self.l, self.u = problems.portfolio_qp(self.NA, self.K)
        self.n, self.m = len(self.q), len(self.l)
        rng = np.random.default_rng(17)
        self.Q = np.stack([np.concatenate([-rng.standard_normal(self.NA) / (1.0 + 0.05 * b), np.zeros(self.K)]) for b in range(B)])      # mu redrawn, gamma swept
        self.L, self.U = np.tile(self.l, (B, 1)), np.tile(self.u, (B, 1))
        for b in (3, 63, 66):
            self.U[b, self.K + 1:] = 0.02 + 0.01 * rng.random(self.NA)                # per-element box upper bounds (sum >= 12: the budget stays feasible)
        self.s = _handle(self.P, self.q, self.A, self.l, self.u)
        self.x, self.y, self.rec = self.s._solver.hip_batch_solve_lockstep_direct(q=self.Q, l=self.L, u=self.U)
        self.last = self.s._solver.lockstep_direct_last_record()


@pytest.fixture(scope='module')
def base():
    return Base()


def test_the_route(base):
    """portfolio_qp(600, 4): n = 604, m = 605, r = 5; B = 70 at eps 1e-8: every element certified on the host, four of them held to the oracle at
    eps 1e-9."""
    assert (base.n, base.m) == (604, 605)
    assert int((np.diff(sp.csr_matrix(base.A).indptr) > 128).sum()) == 5              # the rows of F' (about 300 entries each) and the budget row
    _past_both(base.s, base.n, base.m, 5, q=base.Q, l=base.L, u=base.U)
    base.s._solver.hip_batch_solve_lockstep_direct_device(0, None, None, None, None, None, None)      # the applicability query: no exception
    assert (base.rec[:, REC_STATUS] == S.OSQP_SOLVED).all(), base.rec[:, REC_STATUS]
    assert (base.rec[:, REC_PCG] == 0).all()
    assert base.last['chunks'] == 2 and base.last['width'] == 64 and base.last['admm_iters_max'] == base.rec[:, REC_ITER].max()
    for b in range(B):
        _certify(base.P, base.Q[b], base.A, base.L[b], base.U[b], base.x[b], base.y[b], base.rec[b, REC_OBJ])
    for b in PICK:
        st = dict(ST, eps_abs=1e-9, eps_rel=1e-9); st.pop('warm_starting')
        xo, yo, io = Oracle().setup(base.P, base.Q[b], base.A, base.L[b], base.U[b], **st).solve()
        assert io.status_val == SOLVED
        ex, ey = _close(base.x[b], xo), _close(base.y[b], yo)
        record_deviation('lockstep_direct_vs_oracle', 'portfolio 600x4 element %d' % b, dx_rel=ex, dy_rel=ey, iters=int(base.rec[b, REC_ITER]), oracle_iters=io.iter, atol=ATOL)
        print('element %d: direct lockstep %d iterations, oracle %d; |dx| %.2e |dy| %.2e (relative)' % (b, base.rec[b, REC_ITER], io.iter, ex, ey))
        assert ex <= ATOL and ey <= ATOL


def test_every_element_against_the_single_handle(base):
    """Every element's x, y against update(q, l, u) + solve() on a single handle, both at eps 1e-8, at ATOL = 2e-6.  The route adapts rho by the rule of
    the handle's own solve (term_rules.h single_rho_rule), so from the same settings the two take the same path: the deviations are rounding."""
    single = _single(_handle(base.P, base.q, base.A, base.l, base.u), base.Q, base.L, base.U)
    dev = []
    for b, r in enumerate(single):
        assert r.info.status_val == S.OSQP_SOLVED
        dev.append((_close(base.x[b], r.x), _close(base.y[b], r.y)))
        if b in PICK:
            record_deviation('lockstep_direct_vs_single', 'portfolio 600x4 element %d' % b, dx_rel=dev[-1][0], dy_rel=dev[-1][1], iters=int(base.rec[b, REC_ITER]), single_iters=int(r.info.iter), atol=ATOL)
    print('same iteration count as the single handle: %d of %d elements' % (sum(int(r.info.iter) == int(base.rec[b, REC_ITER]) for b, r in enumerate(single)), B))
    assert [int(r.info.iter) for r in single] == [int(i) for i in base.rec[:, REC_ITER]]      # the same rho rule from the same rho: the same path
    dev = np.array(dev)
    print('deviation from the single handle: worst |dx| %.2e |dy| %.2e (relative); over ATOL: %s' % (dev[:, 0].max(), dev[:, 1].max(), np.nonzero((dev > ATOL).any(axis=1))[0]))
    assert (dev <= ATOL).all(), (np.nonzero((dev > ATOL).any(axis=1))[0], dev.max(axis=0))


def test_independence(base):
    """A problem alone, at lane 0, at lane 63 and in the ragged chunk, among different neighbours: x, y and record are bit-identical."""
    solve = base.s._solver.hip_batch_solve_lockstep_direct
    for b in PICK:
        x1, y1, r1 = solve(q=base.Q[b:b + 1], l=base.L[b:b + 1], u=base.U[b:b + 1])
        assert np.array_equal(x1[0], base.x[b]) and np.array_equal(y1[0], base.y[b]) and np.array_equal(r1[0], base.rec[b]), b
    xr, yr, rr = solve(q=base.Q[::-1].copy(), l=base.L[::-1].copy(), u=base.U[::-1].copy())      # lane 0 <-> the ragged chunk's last, other neighbours
    assert np.array_equal(xr[::-1], base.x) and np.array_equal(yr[::-1], base.y) and np.array_equal(rr[::-1], base.rec)


def _edge(P, q, A, l, u, r):
    n, m = len(q), len(l)
    rng = np.random.default_rng(5)
    Q = np.stack([q * (1.0 + 0.3 * b) + 0.1 * b * rng.standard_normal(n) * (q != 0) for b in range(3)])
    L, U = np.tile(l, (3, 1)), np.tile(u, (3, 1))
    s = _handle(P, q, A, l, u)
    _past_both(s, n, m, r, q=Q, l=L, u=U)
    x, y, rec = s._solver.hip_batch_solve_lockstep_direct(q=Q, l=L, u=U)
    assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all(), rec[:, REC_STATUS]
    for b, res in enumerate(_single(_handle(P, q, A, l, u), Q, L, U)):
        _certify(P, Q[b], A, L[b], U[b], x[b], y[b], rec[b, REC_OBJ])
        assert res.info.status_val == S.OSQP_SOLVED
        ex, ey = _close(x[b], res.x), _close(y[b], res.y)
        print('r = %d element %d: %d iterations (single handle %d); |dx| %.2e |dy| %.2e' % (r, b, rec[b, REC_ITER], res.info.iter, ex, ey))
        assert ex <= ATOL and ey <= ATOL, (r, b, ex, ey)


def test_one_dense_row():
    """r = 1: diagonal P, box rows and one budget row over 200 of the 500 columns."""
    n = 500
    rng = np.random.default_rng(2)
    P = sp.diags(0.5 + rng.random(n), format='csc')
    budget = sp.csc_matrix((np.ones(200), (np.zeros(200, dtype=int), np.arange(0, 400, 2))), shape=(1, n))
    A = sp.vstack([budget, sp.identity(n)], format='csc')
    assert int((np.diff(sp.csr_matrix(A).indptr) > 128).sum()) == 1
    l, u = np.concatenate([[1.0], np.zeros(n)]), np.concatenate([[1.0], np.ones(n)])
    _edge(P, rng.standard_normal(n), A, l, u, 1)


def test_128_dense_rows_and_the_decline_at_129():
    """r = 128, the LDS and padding limit: na = 400, k = 127 with F at density 0.7 (every row of F' counted here); k = 128 gives r = 129: declined."""
    P, q, A, l, u = _factor_qp(400, 127, 0.7)
    counts = np.diff(sp.csr_matrix(A).indptr)
    assert (counts[:128] > 128).all() and (counts[128:] == 1).all(), counts[:128].min()
    _edge(P, q, A, l, u, 128)
    P, q, A, l, u = _factor_qp(400, 128, 0.7)
    assert int((np.diff(sp.csr_matrix(A).indptr) > 128).sum()) == 129
    s = _handle(P, q, A, l, u)
    for call in (lambda: s._solver.hip_batch_solve_lockstep_direct(q=np.tile(q, (3, 1))), lambda: s._solver.hip_batch_solve_lockstep_direct_device(0, None, None, None, None, None, None)):
        with pytest.raises(ValueError) as e:
            call()
        assert e.value.code == NOT_IMPL


class Chunk:
    """One chunk with a solved element, a primal-infeasible one (budget = 1 with every upper bound 0) and one stopped by max_iter: of eight of the
    base's elements the one that needs fewest iterations at eps 1e-7 is the solved one, the one that needs most is stopped 25 iterations after it."""
    ST = dict(eps_abs=1e-7, eps_rel=1e-7, eps_prim_inf=1e-5, eps_dual_inf=1e-5)

    def __init__(self, base):
        s = _handle(base.P, base.q, base.A, base.l, base.u, **self.ST)
        _, _, rec = s._solver.hip_batch_solve_lockstep_direct(q=base.Q[:8], l=base.L[:8], u=base.U[:8])
        assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all()
        it = rec[:, REC_ITER]
        short, long_ = int(np.argmin(it)), int(np.argmax(it))
        self.cap = int(it[short]) + 25
        assert it[long_] > self.cap, it
        self.Q = np.stack([base.Q[short], base.Q[1], base.Q[long_]])
        self.L, self.U = np.stack([base.L[short], base.l, base.L[long_]]), np.stack([base.U[short], base.u, base.U[long_]])
        self.U[1, base.K + 1:] = 0.0
        self.s = _handle(base.P, base.q, base.A, base.l, base.u, max_iter=self.cap, **self.ST)
        self.x, self.y, self.rec = self.s._solver.hip_batch_solve_lockstep_direct(q=self.Q, l=self.L, u=self.U)
        self.single = _single(_handle(base.P, base.q, base.A, base.l, base.u, max_iter=self.cap, **self.ST), self.Q, self.L, self.U)


@pytest.fixture(scope='module')
def chunk(base):
    return Chunk(base)


STOPPED = {int(S.OSQP_MAX_ITER_REACHED), int(S.OSQP_SOLVED_INACCURATE), int(S.OSQP_PRIMAL_INFEASIBLE_INACCURATE), int(S.OSQP_DUAL_INFEASIBLE_INACCURATE)}


def test_statuses_in_one_chunk(base, chunk):
    """The three statuses in one chunk, the infeasibility certificate checked on the host, and the finished elements frozen: their outputs equal those
    of a run without the long-running neighbour."""
    rec, y = chunk.rec, chunk.y
    print('statuses', rec[:, REC_STATUS], 'iterations', rec[:, REC_ITER], 'max_iter', chunk.cap)
    assert list(rec[:2, REC_STATUS]) == [S.OSQP_SOLVED, S.OSQP_PRIMAL_INFEASIBLE] and int(rec[2, REC_STATUS]) in STOPPED and rec[2, REC_ITER] == chunk.cap
    assert rec[0, REC_ITER] < chunk.cap and rec[1, REC_ITER] < chunk.cap
    yc = y[1]                                                                         # certificate of primal infeasibility (_osqp.py:796-820)
    assert np.abs(base.A.T @ yc).max() <= Chunk.ST['eps_prim_inf'] * np.abs(yc).max()
    assert chunk.U[1] @ np.maximum(yc, 0) + chunk.L[1] @ np.minimum(yc, 0) < 0
    xf, yf, rf = chunk.s._solver.hip_batch_solve_lockstep_direct(q=chunk.Q[:2], l=chunk.L[:2], u=chunk.U[:2])      # without the long-running neighbour
    eq = lambda a, b: np.array_equal(a, b, equal_nan=True)                            # (an infeasible element's x is NaN in both runs)
    assert eq(xf, chunk.x[:2]) and eq(yf, chunk.y[:2]) and eq(rf, rec[:2])


def test_statuses_against_the_single_handle(chunk):
    """Status, iteration count and certificate per element against the single handle under the same settings (_single: rho included).  The certificate
    is compared normalised at ATOL: both are the dy of the iteration that detected infeasibility."""
    rec = chunk.rec
    for b, r in enumerate(chunk.single):
        print('element %d: status %d / %d, iterations %d / %d (direct lockstep / single handle)' % (b, rec[b, REC_STATUS], r.info.status_val, rec[b, REC_ITER], r.info.iter))
    c0, c1 = chunk.y[1], chunk.single[1].prim_inf_cert
    print('certificates: normalised difference %.2e' % np.abs(c0 / np.abs(c0).max() - c1 / np.abs(c1).max()).max())
    for b, r in enumerate(chunk.single):
        assert r.info.status_val == int(rec[b, REC_STATUS]) and r.info.iter == int(rec[b, REC_ITER]), (b, r.info.status_val, r.info.iter, rec[b, :2])
    assert np.abs(c0 / np.abs(c0).max() - c1 / np.abs(c1).max()).max() <= ATOL


RHO_BATCH = []


def _rho_batch(base):
    if not RHO_BATCH:
        nb = 70
        # (no larger scales: at q x 100 the whole budget sits on one asset, x_i = u_i = 1 with the budget row active, the multipliers of those two
        #  rows are not unique and y is no yardstick any more)
        scale = np.array([0.1, 0.3, 1.0, 3.0])[np.arange(nb) % 4]
        Q = base.Q[:nb] * scale[:, None]
        s = _handle(base.P, base.q, base.A, base.l, base.u, adaptive_rho_interval=25)
        x, y, rec = s._solver.hip_batch_solve_lockstep_direct(q=Q, l=base.L[:nb], u=base.U[:nb])
        RHO_BATCH.append((x, y, rec, s._solver.lockstep_direct_last_record(), Q))
    return RHO_BATCH[0]


def test_rho_per_problem(base):
    """adaptive_rho_interval = 25 and q scales that make the elements update rho at different iterations (read from the records): every element is
    certified, and S is inverted once per problem at the start and once more per rho update of that problem -- not per chunk event."""
    x, y, rec, last, Q = _rho_batch(base)
    nb = len(Q)
    upd = rec[:, REC_RHOUPD].astype(int)
    print('rho updates per element:', upd, 'final rho:', np.unique(rec[:, REC_RHO]).size, 'distinct values; factorisations', last['factorisations'])
    assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all()
    assert len(set(upd.tolist())) > 1 and np.unique(rec[:, REC_RHO]).size > 1      # different numbers of updates, different rho at the end
    assert last['chunks'] == 2
    assert last['chunks'] < last['factorisations'] < last['chunks'] * (1 + upd.max()) * 64      # (every lane at the start and at every update: what a per-chunk refactorisation would cost)
    assert last['factorisations'] == nb + upd.sum()                                   # the start, then exactly the problems whose rho_bar changed
    for b in range(nb):
        _certify(base.P, Q[b], base.A, base.L[b], base.U[b], x[b], y[b], rec[b, REC_OBJ])


def test_rho_per_problem_against_the_single_handle(base):
    """The same batch held to the single handle at ATOL = 2e-6, as test_every_element_against_the_single_handle holds the base batch; with these scales every element is inside as measured on an MI355X."""
    x, y, rec, last, Q = _rho_batch(base)
    nb = len(Q)
    dev = []
    for b, r in enumerate(_single(_handle(base.P, base.q, base.A, base.l, base.u, adaptive_rho_interval=25), Q, base.L[:nb], base.U[:nb])):
        assert r.info.status_val == S.OSQP_SOLVED
        dev.append((_close(x[b], r.x), _close(y[b], r.y)))
    dev = np.array(dev)
    print('deviation from the single handle: worst |dx| %.2e |dy| %.2e (relative); over ATOL: %s' % (dev[:, 0].max(), dev[:, 1].max(), np.nonzero((dev > ATOL).any(axis=1))[0]))
    assert (dev <= ATOL).all(), (np.nonzero((dev > ATOL).any(axis=1))[0], dev.max(axis=0))


def test_warm_start(base):
    sl = slice(60, 66)                                                                 # the batch's own elements: their solutions are base.x / base.y
    x, y, rec = base.s._solver.hip_batch_solve_lockstep_direct(q=base.Q[sl], l=base.L[sl], u=base.U[sl], x0=base.x[sl], y0=base.y[sl])
    assert (rec[:, REC_STATUS] == S.OSQP_SOLVED).all()
    assert (rec[:, REC_ITER] < base.rec[sl, REC_ITER]).all(), (rec[:, REC_ITER], base.rec[sl, REC_ITER])
    for b in range(6):
        assert _close(x[b], base.x[sl][b]) <= ATOL and _close(y[b], base.y[sl][b]) <= ATOL


def test_declines(base, monkeypatch):
    """A banded handle without Woodbury rows, a lasso handle (more than 128 dense rows), a Woodbury handle whose short rows have two entries -- and,
    as the header says, a handle that works on a permuted copy."""
    na, k = base.NA, base.K
    Pb, qb, Ab, lb, ub = problems.banded_qp(400, window=40)
    Pl, ql, Al, ll, ul = problems.lasso_qp(nf=150, ns=200)
    pair = sp.diags([np.ones(na), -np.ones(na - 1)], [0, 1], shape=(na, na))          # x_i - x_{i+1}: two entries per short row
    A2 = sp.vstack([sp.csr_matrix(base.A)[:k + 1], sp.hstack([pair, sp.csc_matrix((na, k))])], format='csc')
    l2, u2 = np.concatenate([base.l[:k + 1], -np.ones(na)]), np.concatenate([base.u[:k + 1], np.ones(na)])
    cases = [('banded', (Pb, qb, Ab, lb, ub), 0), ('lasso', (Pl, ql, Al, ll, ul), None), ('two-entry rows', (base.P, base.q, A2, l2, u2), k + 1)]
    for name, data, rows in cases:
        s = _handle(*data, eps_abs=1e-6, eps_rel=1e-6)
        if rows is not None:
            assert s._solver.hip_stats()['woodbury_rows'] == rows, name
        for call in (lambda: s._solver.hip_batch_solve_lockstep_direct(q=np.tile(data[1], (3, 1))), lambda: s._solver.hip_batch_solve_lockstep_direct_device(0, None, None, None, None, None, None)):
            with pytest.raises(ValueError) as e:
                call()
            assert e.value.code == NOT_IMPL, name
        assert s._solver.lockstep_direct_last_record()['chunks'] == 0
    monkeypatch.setenv('OSQP_HIP_REORDER', '2')
    s = _handle(base.P, base.q, base.A, base.l, base.u)
    assert s._solver.hip_stats()['reordered'] == 1 and s._solver.hip_stats()['woodbury_rows'] == 5
    with pytest.raises(ValueError) as e:
        s._solver.hip_batch_solve_lockstep_direct(q=base.Q[:3])
    assert e.value.code == NOT_IMPL


@pytest.mark.parametrize('device', ['cpu', 'cuda'])
def test_torch_layer(base, device):
    import torch
    from osqp_amd.nn.torch import OSQP as Layer
    nb = 3
    Pc, Ac = sp.csc_matrix(base.P), sp.csc_matrix(base.A)
    Pc.sort_indices(); Ac.sort_indices()
    pco, aco = Pc.tocoo(), Ac.tocoo()
    mk = lambda **kw: Layer((pco.row, pco.col), Pc.shape, (aco.row, aco.col), Ac.shape, eps_rel=EPS, eps_abs=EPS, max_iter=200000, **kw)
    vals = [Pc.data, base.Q[:nb], Ac.data, base.L[:nb], base.U[:nb]]
    direct, loop = mk(large_batch='lockstep_direct'), mk(large_batch='loop')
    ts = [torch.tensor(np.array(v), dtype=torch.float64, device=device) for v in vals]
    with torch.no_grad():
        x, xl = direct(*ts), loop(*ts)
    assert x.device == ts[1].device and x.shape == (nb, base.n)
    X, Xl = x.cpu().numpy(), xl.cpu().numpy()
    assert np.abs(X - Xl).max() / (1 + np.abs(Xl).max()) <= ATOL
    assert direct.setup_count == 1 and loop.setup_count == 1
    assert direct._solver._solver.lockstep_direct_last_record()['chunks'] == 1
    assert loop._solver._solver.lockstep_direct_last_record()['chunks'] == 0           # the loop layer still loops
    with torch.no_grad():
        direct(*ts)
    assert direct.setup_count == 1
    with pytest.raises(ValueError):
        mk(large_batch='other')


@pytest.mark.parametrize('device', ['cpu', 'cuda'])
def test_torch_layer_on_a_declining_handle(base, device):
    """large_batch='lockstep_direct' on a handle the route declines (banded, no Woodbury rows) answers as large_batch='lockstep' answers on a handle
    IT declines (the portfolio's Woodbury handle): ValueError with OSQP_FUNC_NOT_IMPLEMENTED, no silent loop."""
    import torch
    from osqp_amd.nn.torch import OSQP as Layer
    raised = []
    for data, route in ((problems.banded_qp(400, window=40), 'lockstep_direct'), ((base.P, base.q, base.A, base.l, base.u), 'lockstep')):
        P, q, A, l, u = data
        Pc, Ac = sp.csc_matrix(P), sp.csc_matrix(A)
        Pc.sort_indices(); Ac.sort_indices()
        pco, aco = Pc.tocoo(), Ac.tocoo()
        layer = Layer((pco.row, pco.col), Pc.shape, (aco.row, aco.col), Ac.shape, eps_rel=1e-6, eps_abs=1e-6, large_batch=route)
        ts = [torch.tensor(np.array(v), dtype=torch.float64, device=device) for v in (Pc.data, np.tile(q, (3, 1)), Ac.data, np.tile(l, (3, 1)), np.tile(u, (3, 1)))]
        with torch.no_grad(), pytest.raises(ValueError) as e:
            layer(*ts)
        raised.append(str(e.value))
    assert raised[0] == raised[1] == str(int(osqp_amd.SolverError.OSQP_FUNC_NOT_IMPLEMENTED))
