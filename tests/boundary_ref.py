"""Reference, bounds and judge of the kernel-level tests of the CHUNK BOUNDARY of a single-QP solve (osqp-python_amd/csrc/backend_hip.hip: k_res_m, k_res_n,
the two-level fold put_partial -> k_res_final, k_inf_primal, k_inf_dual_p, k_inf_dual_a, k_set_rho, k_init_guess, k_precond, and the device-driven group
ctl_group with k_decide running csrc/policy.h) -- numpy / scipy only, no GPU.  Written once, used by two tiers: tests/test_gpu_boundary_kernels.py runs the
batteries below on handles of the product through the diagnostic entry osqp_hip_test_boundary (POKE seven scaled vectors, RUN the boundary, PEEK the
residual block and what a rho change leaves), tests/test_boundary_ref.py runs the same batteries through the same entry on the host simulator and on a
numpy stand-in with planted mistakes, which they have to reject.

THE QUANTITIES (Ref).  On the scaled problem of pcg_ref.Scaled (P~, A~, q~) with the handle's D, E, c, Dinv = 1 / D, Einv = 1 / E and the scaled, clamped
bounds l~ = E max(l, -1e30), u~ = E min(u, 1e30), from the poked x, dx, z, y, dy, in np.longdouble:
    m-side, row i of A~:   ax = (A~ x)_i, pr = ax - z_i:   R_PRI / R_AX / R_Z (_S: |.|, _U: |Einv_i .|), R_DY_S = |dy_i|, R_DY_U = |E_i dy_i|  (maxima),
                           R_PINF_LHS = sum u~_i max(dy_i, 0) + l~_i min(dy_i, 0),   R_SUPP = sum of u~_i y_i (y_i > 0, u~_i finite) or l~_i y_i (y_i < 0, l~_i finite)
    n-side, row j:         px = (P~ x)_j, aty = (A~' y)_j, dr = px + q~_j + aty:   R_DUA / R_PX / R_ATY (_S, _U with Dinv_j), R_DX_S = |dx_j|, R_DX_U = |D_j dx_j|,
                           R_QN_S = |q~_j|, R_QN_U = |Dinv_j q~_j|  (maxima),   R_XPX = sum x_j px_j, R_QX = sum q~_j x_j, R_QDX = sum q~_j dx_j
    second stage:          R_ATDY = |(A~' dy)_j| (_U: Dinv_j), R_PDX = |(P~ dx)_j| (_U: Dinv_j)  (maxima),   R_ADX_VIOL = the number of rows whose (A~ dx)_i
                           (unscaled: Einv_i times it) lies beyond +thr on a finite upper or beyond -thr on a finite lower side
A maximum is NaN as soon as one of its rows is (step_rules.h nanmax); a NaN in y does not reach R_SUPP (both comparisons of support_finite are false).

THE BOUNDS, derived (u = 2^-53, gamma_k = k u / (1 - k u)):
  * a row's sum of k products, summed in any order in fp64, is off by at most gamma_k sum |a| |x|.  The engine's scaled values are not the reference's: each is
    the product of up to 2 factors per equilibration pass (<= 10 passes and the cost pass) where Scaled multiplies the accumulated D, E, c once -- at most
    DATA = 64 roundings between the two, so a row carries gamma_(k + DATA) sum |a| |x|;
  * the epilogue of a row (the subtraction of sigma x or z, the sum px + q + aty, the product with Einv / Dinv) is at most two roundings on each magnitude
    it combines; an honest fp64 evaluation has to stay below 1/8 of a bound (the twin rule below), so the epilogue adds EPI = 8 * 2 u times those magnitudes;
  * |max_i f_i - max_i g_i| <= max_i |f_i - g_i|: a maximum over rows carries the largest row bound;
  * a sum over N rows carries gamma_(N + DATA) sum |term| plus what its terms carry (R_XPX: |x_j| times the row bound of px_j).
R_Z_S, R_DY_S, R_DX_S copy an input: bound 0, compared exactly.  R_ADX_VIOL is a count, compared exactly; adx_inputs chooses thr so that no row lies within
64 x its row bound of +-thr.  The fp64 twin (SciPy's CSR products, numpy's pairwise sums: another order of summation) has to stay below 1/8 of every bound
(check_twin), the project's rule in tests/test_pcg_ref.py.

AFTER A RHO CHANGE (rho_change).  rho_i = 1e-6 on a loose row, eqf rho_bar on an equality row, rho_bar elsewhere (step_rules.h row_rho; classes from the scaled
bounds, eqf from the handle's rho vector); rho_inv = 1 / rho, t0 = rho zt, ztg = zt, xg = xsp = xt bitwise; v = rho z - y within 2 u (|rho z| + |y|) (one
product, one sum, contracted or not); Minv_j = 1 / (P~_jj + sigma + sum_i rho_i A~_ij^2): positive terms, relative gamma_(k + DATA + 4).

THE BATTERIES.  check_mode0 (dense draw, one-hot inputs, planted maxima, NaN, the violation count) and the scenarios of check_mode1 are functions of an
`entry` callable: the GPU tier passes the product's, the CPU tier the host simulator's and Standin's.
"""
import numpy as np
import scipy.sparse as sp

import pcg_ref
import wb_ref

L = np.longdouble
U = 2.0 ** -53
DATA = 64
EPI = 16.0 * U
INFTY = 1e30
VALIDATION, NOT_IMPLEMENTED = 1, 10
NAMES = ('R_PRI_U', 'R_AX_U', 'R_Z_U', 'R_PRI_S', 'R_AX_S', 'R_Z_S', 'R_DY_U', 'R_DY_S', 'R_PINF_LHS', 'R_SUPP',
         'R_DUA_U', 'R_PX_U', 'R_ATY_U', 'R_DUA_S', 'R_PX_S', 'R_ATY_S', 'R_DX_U', 'R_DX_S', 'R_XPX', 'R_QX', 'R_QDX', 'R_QN_S', 'R_QN_U',
         'R_ATDY_U', 'R_ATDY_S', 'R_PDX_U', 'R_PDX_S', 'R_ADX_VIOL')
SUMS = ('R_PINF_LHS', 'R_SUPP', 'R_XPX', 'R_QX', 'R_QDX', 'R_ADX_VIOL')
M_SIDE = NAMES[:10]
STAGE1 = NAMES[:23]
PINF_Q, DINF_Q = ('R_ATDY_U', 'R_ATDY_S'), ('R_PDX_U', 'R_PDX_S', 'R_ADX_VIOL')
NEED_PINF, NEED_DINF = 1, 2
CTL_RUNNING, CTL_DONE, CTL_NEED_HOST = 0, 1, 2
SOLVED, PRIMAL_INFEASIBLE, DUAL_INFEASIBLE, NON_CVX = 1, 3, 5, 9          # osqp_status_type (include/osqp_hip.h)
PLANTS = ('max_drops_last_partial', 'sum_drops_last_partial', 'u_without_scaling', 'px_keeps_sigma_x', 'pdx_without_sigma_dx', 'support_l_u_swapped',
          'nan_swallowed_by_max', 'v_from_old_rho', 'ztg_not_reset')
WG_ROWS = 256                                     # the stand-in's workgroups: 256 consecutive rows each
VEC = ('x', 'dx', 'xt', 'z', 'y', 'dy', 'zt')


def gamma(k):
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------------------------------------------ the data of a handle
class Data:
    """The scaled problem of a set-up handle and what the boundary kernels read besides: D, E, their inverses, the clamped scaled bounds."""

    def __init__(self, s, D, E, c, l, u):
        self.s, self.n, self.m = s, s.n, s.m
        self.D, self.E = np.asarray(D, dtype=np.float64), np.asarray(E, dtype=np.float64)
        self.Dinv, self.Einv = 1.0 / self.D, 1.0 / self.E
        self.c, self.cinv = float(c), 1.0 / float(c)
        self.l = self.E * np.maximum(np.asarray(l, dtype=np.float64), -INFTY)
        self.u = self.E * np.minimum(np.asarray(u, dtype=np.float64), INFTY)
        self.ufin, self.lfin = self.u < INFTY * 1e-4, self.l > -INFTY * 1e-4
        self.absP, self.absA, self.absAT = abs(s.P).tocsr(), abs(s.A).tocsr(), abs(s.AT).tocsr()
        self.kP, self.kA, self.kAT = np.diff(s.P.indptr), np.diff(s.A.indptr), np.diff(s.AT.indptr)
        self.free = ~self.ufin & ~self.lfin

    def rows(self):
        """the three positions of the m-side one-hot / planted inputs: first row, last row, the longest row of A (a row of its own workgroup where it has one)"""
        if self.m == 0:
            return ()
        return tuple(dict.fromkeys((0, self.m - 1, int(np.argmax(self.kA)) if self.kA.max() > self.kA.min() else max(self.m - 2, 0))))

    def cols(self):
        if self.n == 0:
            return ()
        kB = self.kP + self.kAT
        return tuple(dict.fromkeys((0, self.n - 1, int(np.argmax(kB)) if kB.max() > kB.min() else max(self.n - 2, 0))))


def data_of(solver, P, q, A, l, u, sigma, alpha):
    D, E, c = solver.hip_scaling()
    return Data(pcg_ref.scaled_of(solver, P, q, A, l, u, sigma, alpha), D, E, c, l, u)


def draw(d, seed):
    """the seeded normal vectors of the dense draw; dy is 0 on the rows that are free on both sides (their bounds are +-1e30 E: one such term would bury every
    other term of R_PINF_LHS under its rounding error)"""
    rng = np.random.default_rng(seed)
    v = {k: rng.standard_normal(d.n if k in ('x', 'dx', 'xt') else d.m) for k in VEC}
    v['dy'][d.free] = 0.0
    one_l, one_u = d.ufin & ~d.lfin, d.lfin & ~d.ufin           # (one-sided rows: dy on the finite side, for the same reason)
    v['dy'][one_l] = np.abs(v['dy'][one_l]); v['dy'][one_u] = -np.abs(v['dy'][one_u])
    return v


def zeros(d):
    return {k: np.zeros(d.n if k in ('x', 'dx', 'xt') else d.m) for k in VEC}


# ------------------------------------------------------------------------------------------------------------------------------ the quantities
def _mx(v):
    """a maximum of absolute values as the kernels keep it: NaN as soon as one row is"""
    if v.size == 0:
        return v.dtype.type(0)
    return v.dtype.type(np.nan) if np.isnan(v).any() else np.abs(v).max()


def _bmax(b):
    return float(np.max(b)) if b.size else 0.0


def support_term(l, u, dy):
    return u * np.fmax(dy, 0) + l * np.fmin(dy, 0)


def support_finite(d, l, u, y):
    with np.errstate(invalid='ignore'):
        return np.where((y > 0) & d.ufin, u * y, np.where((y < 0) & d.lfin, l * y, 0 * l))


def adx_violates(d, a, thr):
    with np.errstate(invalid='ignore'):
        return (d.ufin & (a > thr)) | (d.lfin & (a < -thr))


class Ref:
    """Every quantity of the residual block from the poked vectors in the number type T, and (T = long double) the bound of each."""

    def __init__(self, d, vec, T=L, need=NEED_PINF | NEED_DINF, thr=0.0, unscaled=0):
        s, o = d.s, d.s.ops(T)
        c = lambda a: np.asarray(a, dtype=T)
        x, dx, z, y, dy = (c(vec[k]) for k in ('x', 'dx', 'z', 'y', 'dy'))
        D, E, Dinv, Einv, q, lo, hi, sig = c(d.D), c(d.E), c(d.Dinv), c(d.Einv), c(s.q), c(d.l), c(d.u), T(s.sigma)
        v = {}
        with np.errstate(invalid='ignore', over='ignore'):
            ax = o.A(x) if d.m else np.zeros(0, dtype=T)
            pr = ax - z
            v['R_PRI_U'], v['R_AX_U'], v['R_Z_U'] = _mx(Einv * pr), _mx(Einv * ax), _mx(Einv * z)
            v['R_PRI_S'], v['R_AX_S'], v['R_Z_S'] = _mx(pr), _mx(ax), _mx(z)
            v['R_DY_U'], v['R_DY_S'] = _mx(E * dy), _mx(dy)
            t_lhs, t_sup = support_term(lo, hi, dy), support_finite(d, lo, hi, y)
            v['R_PINF_LHS'], v['R_SUPP'] = t_lhs.sum(dtype=T), t_sup.sum(dtype=T)
            px, aty = o.P(x) + (x - x), (o.AT(y) if d.m else np.zeros(d.n, dtype=T))      # (x - x: row j of B always holds sigma on its diagonal, so a NaN in x_j reaches px_j)
            dr = px + q + aty
            v['R_DUA_U'], v['R_PX_U'], v['R_ATY_U'] = _mx(Dinv * dr), _mx(Dinv * px), _mx(Dinv * aty)
            v['R_DUA_S'], v['R_PX_S'], v['R_ATY_S'] = _mx(dr), _mx(px), _mx(aty)
            v['R_DX_U'], v['R_DX_S'] = _mx(D * dx), _mx(dx)
            v['R_XPX'], v['R_QX'], v['R_QDX'] = (x * px).sum(dtype=T), (q * x).sum(dtype=T), (q * dx).sum(dtype=T)
            v['R_QN_S'], v['R_QN_U'] = _mx(q), _mx(Dinv * q)
            atdy = o.AT(dy) if d.m else np.zeros(d.n, dtype=T)
            pdx = o.P(dx) + (dx - dx)
            adx = o.A(dx) if d.m else np.zeros(0, dtype=T)
            au = Einv * adx if unscaled else adx
            v['R_ATDY_U'], v['R_ATDY_S'] = _mx(Dinv * atdy), _mx(atdy)
            v['R_PDX_U'], v['R_PDX_S'] = _mx(Dinv * pdx), _mx(pdx)
            v['R_ADX_VIOL'] = T(np.count_nonzero(adx_violates(d, au, thr)))
        if not (need & NEED_PINF):
            v['R_ATDY_U'] = v['R_ATDY_S'] = None          # (not written by this call)
        if not (need & NEED_DINF):
            v['R_PDX_U'] = v['R_PDX_S'] = v['R_ADX_VIOL'] = None
        self.v, self.d, self.need, self.thr, self.unscaled = v, d, need, thr, unscaled
        self.adx, self.rows = au, dict(ax=ax, px=px, aty=aty)
        if T is not L:
            return
        # ---- the bounds (fp64 arithmetic on magnitudes; NaN / inf rows are judged as NaN, not by a bound)
        f = lambda a: np.nan_to_num(np.abs(np.asarray(a, dtype=np.float64)), nan=0.0, posinf=0.0)
        ax_, z_, y_, dy_, x_, dx_, q_ = f(ax), f(z), f(y), f(dy), f(x), f(dx), f(q)
        gA, gP, gAT = gamma(d.kA + DATA), gamma(d.kP + DATA + 2), gamma(d.kAT + DATA)
        e_ax = gA * (d.absA @ x_) if d.m else np.zeros(0)
        e_pr = e_ax + EPI * (ax_ + z_)
        e_px = gP * (d.absP @ x_ + 2 * s.sigma * x_) + EPI * f(px)
        e_aty = gAT * (d.absAT @ y_) if d.m else np.zeros(d.n)
        e_dr = e_px + e_aty + EPI * (f(px) + q_ + f(aty))
        e_atdy = gAT * (d.absAT @ dy_) if d.m else np.zeros(d.n)
        e_pdx = gP * (d.absP @ dx_ + 2 * s.sigma * dx_) + EPI * f(pdx)
        self.e_adx = (gA * (d.absA @ dx_) + EPI * f(adx)) * (d.Einv if unscaled else 1.0) if d.m else np.zeros(0)
        b = {}
        b['R_PRI_U'], b['R_PRI_S'] = _bmax(d.Einv * e_pr + EPI * f(Einv * pr)), _bmax(e_pr)
        b['R_AX_U'], b['R_AX_S'] = _bmax(d.Einv * e_ax + EPI * f(Einv * ax)), _bmax(e_ax)
        b['R_Z_U'], b['R_Z_S'] = _bmax(EPI * f(Einv * z)), 0.0
        b['R_DY_U'], b['R_DY_S'] = _bmax(EPI * f(E * dy)), 0.0
        b['R_PINF_LHS'] = gamma(d.m + DATA) * float(f(t_lhs).sum())
        b['R_SUPP'] = gamma(d.m + DATA) * float(f(t_sup).sum())
        b['R_DUA_U'], b['R_DUA_S'] = _bmax(d.Dinv * e_dr + EPI * f(Dinv * dr)), _bmax(e_dr)
        b['R_PX_U'], b['R_PX_S'] = _bmax(d.Dinv * e_px + EPI * f(Dinv * px)), _bmax(e_px)
        b['R_ATY_U'], b['R_ATY_S'] = _bmax(d.Dinv * e_aty + EPI * f(Dinv * aty)), _bmax(e_aty)
        b['R_DX_U'], b['R_DX_S'] = _bmax(EPI * f(D * dx)), 0.0
        b['R_XPX'] = float((x_ * e_px).sum()) + gamma(d.n + DATA) * float((x_ * (d.absP @ x_)).sum())
        b['R_QX'], b['R_QDX'] = gamma(d.n + DATA) * float((q_ * x_).sum()), gamma(d.n + DATA) * float((q_ * dx_).sum())
        b['R_QN_S'], b['R_QN_U'] = _bmax(EPI * q_), _bmax(2 * EPI * f(Dinv * q))
        b['R_ATDY_U'], b['R_ATDY_S'] = _bmax(d.Dinv * e_atdy + EPI * f(Dinv * atdy)), _bmax(e_atdy)
        b['R_PDX_U'], b['R_PDX_S'] = _bmax(d.Dinv * e_pdx + EPI * f(Dinv * pdx)), _bmax(e_pdx)
        b['R_ADX_VIOL'] = 0.0
        self.b = b

    def check_twin(self, twin):
        """the fp64 twin stays below 1/8 of every bound; where the reference is NaN the twin is"""
        for k in NAMES:
            r, t = self.v[k], twin.v[k]
            if r is None:
                continue
            if np.isnan(r):
                assert np.isnan(t), k
            else:
                assert abs(L(t) - r) <= self.b[k] / 8, '%s: the fp64 twin is off by %.3e, an eighth of the bound is %.3e' % (k, float(abs(L(t) - r)), self.b[k] / 8)


def judge(out, st, ref, worst, where, skip=()):
    """One answer of the entry's mode 0 (or the residual block of a group) against the reference and its bounds."""
    assert st == 0, 'the entry answered %d (%s)' % (st, where)
    res = out['res']
    assert tuple(res) == NAMES, 'the order of the residual block is not the reference\'s (%s)' % where
    for k in NAMES:
        r = ref.v[k]
        if r is None or k in skip:
            continue
        got = float(res[k])
        if np.isnan(r):
            assert np.isnan(got), '%s: %r where the reference is NaN -- error inf against the tolerance 0 (%s)' % (k, got, where)
            continue
        assert not np.isnan(got), '%s: NaN where the reference is %r -- error inf against the tolerance 0 (%s)' % (k, float(r), where)
        err = float(abs(L(got) - r))
        if ref.b[k] == 0.0:
            assert err == 0.0, '%s: %r, error %.3e against the tolerance 0 (%s)' % (k, got, err, where)
        else:
            worst.note(k, err, ref.b[k], where)


def same_res(a, b, what, where):
    assert np.array_equal(wb_ref.bits(a['res_vec']), wb_ref.bits(b['res_vec'])), 'res: %s are not bit-identical (%s): %s' % (
        what, where, [k for k in NAMES if wb_ref.bits(a['res'][k]) != wb_ref.bits(b['res'][k])])


# ------------------------------------------------------------------------------------------------------------------------------ the inputs of the count
def adx_inputs(d, seed, unscaled):
    """(dx, thr) of the R_ADX_VIOL case: a seeded normal dx and a threshold in the widest gap between two neighbouring values of |A~ dx| (unscaled: |Einv A~ dx|)
    around their median, on the rows with a finite side; asserted here: in the reference no such row lies within 64 x its row bound of +-thr, and rows lie on
    both sides of it."""
    rng = np.random.default_rng(seed)
    vec = zeros(d)
    vec['dx'] = rng.standard_normal(d.n)
    r = Ref(d, vec, L, NEED_DINF, 0.0, unscaled)
    live = d.ufin | d.lfin
    a = np.sort(np.asarray(np.abs(r.adx), dtype=np.float64)[live])
    lo, hi = len(a) // 4, max(3 * len(a) // 4, len(a) // 4 + 2)
    k = lo + int(np.argmax(np.diff(a[lo:hi])))
    thr = 0.5 * (a[k] + a[k + 1])
    r = Ref(d, vec, L, NEED_DINF, thr, unscaled)
    dist = np.abs(np.abs(np.asarray(r.adx, dtype=np.float64)) - thr)[live]
    assert (dist > 64 * r.e_adx[live]).all(), 'a row of A dx within 64 x its bound of the threshold'
    assert 0 < float(r.v['R_ADX_VIOL']) < np.count_nonzero(live)
    return vec, thr


# ------------------------------------------------------------------------------------------------------------------------------ mode 0
def call(entry, vec, **kw):
    return entry(*[vec[k] for k in VEC], **kw)


def check_mode0(entry, spmv, d, worst, where, seed=11, other=None):
    """The mode 0 battery on one handle.  entry: hip_test_boundary's signature; spmv(vec [n + m]) -> (P~ + sigma I) vec[:n] + A~' vec[n:] with the HANDLE's own
    scaled values (osqp_hip_test_spmv, which = 1: a one-hot vector reads a row or a column exactly).  other: the entry of a second handle that has to agree
    bitwise (graph replay / eager).  Returns the number of calls judged."""
    n, m, sig = d.n, d.m, d.s.sigma
    both = NEED_PINF | NEED_DINF
    calls = 0
    # ---- dense draw: within bound, a repeat bit-identical, the other handle bit-identical
    vec = draw(d, seed)
    ref = Ref(d, vec, L, both, 0.75, 0)
    ref.check_twin(Ref(d, vec, np.float64, both, 0.75, 0))
    st, out = call(entry, vec, need=both, thr=0.75)
    judge(out, st, ref, worst, where + ', dense draw')
    st2, out2 = call(entry, vec, need=both, thr=0.75)
    assert st2 == 0
    same_res(out, out2, 'two runs of one handle', where)
    if other is not None:
        st3, out3 = call(other, vec, need=both, thr=0.75)
        assert st3 == 0
        same_res(out, out3, 'graph replay and eager launches', where)
    calls += 2
    if m == 0:
        for k in M_SIDE + PINF_Q + ('R_ATY_U', 'R_ATY_S', 'R_ADX_VIOL'):
            assert out['res'][k] == 0.0, '%s is %r on a problem without constraints (%s)' % (k, out['res'][k], where)
    # ---- one-hot dy = e_i: exact
    for i in d.rows():
        vec = zeros(d)
        vec['dy'][i] = 1.0
        st, out = call(entry, vec, need=NEED_PINF)
        assert st == 0
        row = spmv(np.concatenate([np.zeros(n), vec['dy']]))
        want = dict(R_DY_S=1.0, R_DY_U=d.E[i], R_PINF_LHS=float(support_term(d.l[i], d.u[i], 1.0)), R_ATDY_S=np.abs(row).max(), R_ATDY_U=np.abs(d.Dinv * row).max())
        _exact(out, want, ('R_PDX_U', 'R_PDX_S', 'R_ADX_VIOL'), d, where + ', dy = e_%d' % i)
        calls += 1
    # ---- one-hot dx = e_j: exact
    for j in d.cols():
        vec = zeros(d)
        vec['dx'][j] = 1.0
        st, out = call(entry, vec, need=NEED_DINF, thr=0.0)
        assert st == 0
        col = spmv(np.concatenate([vec['dx'], np.zeros(m)]))
        col[j] = col[j] - sig * 1.0
        want = dict(R_DX_S=1.0, R_DX_U=d.D[j], R_QDX=d.s.q[j], R_PDX_S=np.abs(col).max(), R_PDX_U=np.abs(d.Dinv * col).max())
        _exact(out, want, ('R_ATDY_U', 'R_ATDY_S', 'R_ADX_VIOL'), d, where + ', dx = e_%d' % j)
        calls += 1
    # ---- planted maximum: one entry of z, then of x, scaled by 2^40
    for key, pos in (('z', d.rows()), ('x', d.cols())):
        for p in pos:
            vec = draw(d, seed + 1)
            vec[key][p] = np.ldexp(vec[key][p], 40)
            ref = Ref(d, vec, L, 0)
            st, out = call(entry, vec)
            judge(out, st, ref, worst, where + ', %s[%d] x 2^40' % (key, p))
            big = ('R_Z_S', 'R_PRI_S') if key == 'z' else ('R_PX_S', 'R_AX_S')      # (the maxima do land in that entry's rows: of P~ or of A~)
            assert max(float(ref.v[k]) for k in big) > 2.0 ** 20, big
            calls += 1
    # ---- NaN: one in x, one in y, first and last position
    for key, size in (('x', n), ('y', m)):
        for p in dict.fromkeys((0, size - 1)) if size else ():
            vec = draw(d, seed + 2)
            vec[key][p] = np.nan
            ref = Ref(d, vec, L, 0)
            assert any(np.isnan(ref.v[k]) for k in STAGE1) and not all(np.isnan(ref.v[k]) for k in STAGE1)
            st, out = call(entry, vec)
            judge(out, st, ref, worst, where + ', NaN in %s[%d]' % (key, p))
            calls += 1
    # ---- the violation count, exactly
    if m:
        for unscaled in (0, 1):
            vec, thr = adx_inputs(d, seed + 3, unscaled)
            ref = Ref(d, vec, L, NEED_DINF, thr, unscaled)
            st, out = call(entry, vec, need=NEED_DINF, thr=thr, unscaled=unscaled)
            judge(out, st, ref, worst, where + ', violation count, unscaled = %d' % unscaled)
            calls += 1
    return calls


def _exact(out, want, untouched, d, where):
    """a one-hot input: the listed quantities exactly, every other quantity of the first stage that has no q in it exactly 0"""
    res = out['res']
    for k, w in want.items():
        assert res[k] == w, '%s: %r, exactly %r is expected -- error %.3e against the tolerance 0 (%s)' % (k, res[k], w, abs(res[k] - w), where)
    zero = ('R_PRI_U', 'R_AX_U', 'R_Z_U', 'R_PRI_S', 'R_AX_S', 'R_Z_S', 'R_SUPP', 'R_PX_U', 'R_ATY_U', 'R_PX_S', 'R_ATY_S', 'R_XPX', 'R_QX', 'R_DY_U', 'R_DY_S',
            'R_PINF_LHS', 'R_DX_U', 'R_DX_S', 'R_QDX')
    for k in zero:
        if k not in want:
            assert res[k] == 0.0, '%s: %r, exactly 0 is expected -- error against the tolerance 0 (%s)' % (k, res[k], where)
    assert res['R_DUA_S'] == res['R_QN_S'] and res['R_DUA_U'] == res['R_QN_U'], 'the dual residual of a zero point is q: error against the tolerance 0 (%s)' % where


# ------------------------------------------------------------------------------------------------------------------------------ after a rho change
def row_classes(d):
    """step_rules.h row_class on the scaled bounds: -1 loose, 1 equality, 0 inequality"""
    return np.where((d.l < -INFTY * 1e-4) & (d.u > INFTY * 1e-4), -1, np.where(d.u - d.l < 1e-4, 1, 0))


def rho_vector(d, rho_bar, rho_old, rho_bar_old):
    cls = row_classes(d)
    eq = rho_old[cls == 1]
    eqf = float(round(eq[0] / rho_bar_old)) if eq.size else 1.0
    return np.where(cls == -1, 1e-6, np.where(cls == 1, eqf * rho_bar, rho_bar))


def check_rho_change(out, d, vec, rho_bar, rho_old, rho_bar_old, diagonal, worst, where):
    """what k_set_rho, k_init_guess and k_precond leave after the group changed rho_bar"""
    s = d.s
    rho = rho_vector(d, rho_bar, rho_old, rho_bar_old)
    eq = lambda k, w: _bitwise(out[k], w, k, where)
    eq('rho', rho); eq('rho_inv', 1.0 / rho); eq('t0', rho * vec['zt']); eq('ztg', vec['zt']); eq('xg', vec['xt']); eq('xsp', vec['xt'])
    if d.m:
        z, y, r = (np.asarray(a, dtype=L) for a in (vec['z'], vec['y'], rho))
        err = np.abs(np.asarray(out['v'], dtype=L) - (r * z - y))
        bound = 2 * U * (np.abs(rho * vec['z']) + np.abs(vec['y'])) + 1e-300
        worst.note('v', float((err / bound).max()), 1.0, where)
    if diagonal:
        kd = s.ops(L).kdiag(s, rho)
        err = np.abs(np.asarray(out['Minv'], dtype=L) - L(1) / kd) * kd
        worst.note('Minv', float(err.max()), gamma(int(d.kAT.max() if d.m else 0) + DATA + 4), where)
    return rho


def _bitwise(a, w, k, where):
    assert np.array_equal(wb_ref.bits(a), wb_ref.bits(w)), '%s: not bit for bit what is expected -- error %.3e against the tolerance 0 (%s)' % (
        k, float(np.abs(np.asarray(a) - np.asarray(w)).max()) if len(a) else 0.0, where)


# ------------------------------------------------------------------------------------------------------------------------------ the rules, for the inputs' margins
class Rules:
    """The first stage of a check as policy.h / term_rules.h state it, on a reference block, with the ratio of the two sides of every comparison that
    decides the scenario: the CPU tier asserts each at least a factor 2 from 1."""

    def __init__(self, d, ref, settings, rho_bar):
        v = {k: (float(x) if x is not None else 0.0) for k, x in ref.v.items()}
        unsc = bool(settings['scaling']) and not settings.get('scaled_termination', False)
        ea, er, epi, edi = settings['eps_abs'], settings['eps_rel'], settings.get('eps_prim_inf', 1e-4), settings.get('eps_dual_inf', 1e-4)
        sfx = '_U' if unsc else '_S'
        ci = d.cinv if settings['scaling'] else 1.0
        self.prim_res = 0.0 if d.m == 0 else v['R_PRI' + sfx]
        self.dual_res = d.cinv * v['R_DUA_U'] if unsc else v['R_DUA_S']
        self.obj = (0.5 * v['R_XPX'] + v['R_QX']) * ci
        self.dual_obj = (-0.5 * v['R_XPX'] - v['R_SUPP']) * ci
        self.gap = self.obj - self.dual_obj
        self.non_cvx = not (self.prim_res <= INFTY and self.dual_res <= INFTY)
        self.ratios = {}
        with np.errstate(all='ignore'):
            pn = max(v['R_AX' + sfx], v['R_Z' + sfx])
            dn = (d.cinv if unsc else 1.0) * max(v['R_ATY' + sfx], v['R_PX' + sfx], v['R_QN' + sfx])
            self.pri_ok = d.m == 0 or self.prim_res < ea + er * pn
            self.dua_ok = self.dual_res < ea + er * dn
            if d.m:
                self.ratios['pri'] = self.prim_res / (ea + er * pn)
            self.ratios['dua'] = self.dual_res / (ea + er * dn)
            nd_p, nd_d = v['R_DY' + sfx], v['R_DX' + sfx]
            sc = d.c if unsc else 1.0
            self.need = 0
            if d.m and not self.pri_ok:
                self.ratios['pinf_nd'] = nd_p / epi
                if nd_p > epi:
                    self.ratios['pinf_lhs'] = v['R_PINF_LHS'] / (-epi * nd_p) if v['R_PINF_LHS'] < 0 else 0.0
                    self.need |= NEED_PINF if v['R_PINF_LHS'] < -epi * nd_p else 0
            if not self.dua_ok:
                self.ratios['dinf_nd'] = nd_d / edi
                if nd_d > edi:
                    self.ratios['dinf_qdx'] = v['R_QDX'] / (-sc * edi * nd_d) if v['R_QDX'] < 0 else 0.0
                    self.need |= NEED_DINF if v['R_QDX'] < -sc * edi * nd_d else 0
            self.nd_p, self.nd_d, self.thr_d, self.unsc, self.sc, self.epi, self.edi = nd_p, nd_d, edi * nd_d, int(unsc), sc, epi, edi
            pr = v['R_PRI_S'] / (max(v['R_AX_S'], v['R_Z_S']) + 1e-10)
            du = v['R_DUA_S'] / (max(v['R_ATY_S'], v['R_PX_S'], v['R_QN_S']) + 1e-10)
            self.rho_estimate = min(max(rho_bar * np.sqrt(pr / (du + 1e-10)), 1e-6), 1e6)
        rel = lambda k: (ref.b[k] / abs(v[k]) if v[k] else 0.0)
        self.rho_estimate_bound = self.rho_estimate * (0.5 * sum(rel(k) for k in ('R_PRI_S', 'R_AX_S', 'R_Z_S', 'R_DUA_S', 'R_ATY_S', 'R_PX_S', 'R_QN_S')) + 8 * U)
        b = ref.b
        self.bounds = dict(obj_val=(0.5 * b['R_XPX'] + b['R_QX']) * ci + EPI * (0.5 * abs(v['R_XPX']) + abs(v['R_QX'])) * ci,
                           prim_res=b['R_PRI' + sfx], dual_res=(d.cinv * b['R_DUA_U'] + EPI * self.dual_res) if unsc else b['R_DUA_S'],
                           dual_obj_val=(0.5 * b['R_XPX'] + b['R_SUPP']) * ci + EPI * (0.5 * abs(v['R_XPX']) + abs(v['R_SUPP'])) * ci)
        self.bounds['duality_gap'] = self.bounds['obj_val'] + self.bounds['dual_obj_val'] + EPI * (abs(self.obj) + abs(self.dual_obj))
        self.info = dict(obj_val=self.obj, prim_res=self.prim_res, dual_res=self.dual_res, dual_obj_val=self.dual_obj, duality_gap=self.gap)

    def decided(self, keys):
        """every listed comparison at least a factor 2 from equality"""
        for k in keys:
            r = self.ratios[k]
            assert r >= 2.0 or r <= 0.5, 'the comparison %s has its two sides within a factor 2 (ratio %.3g)' % (k, r)


# ------------------------------------------------------------------------------------------------------------------------------ the numpy stand-in
class Standin:
    """Mode 0 of the entry on plain fp64 numpy (the twin's arithmetic) and the kernels after a rho change, optionally with ONE planted mistake."""

    def __init__(self, d, plant=None, rho=None, rho_bar=0.1):
        self.d, self.plant, self.rho, self.rho_bar = d, plant, rho, rho_bar

    def spmv(self, vec):
        s = self.d.s
        return s.P @ vec[:s.n] + s.sigma * vec[:s.n] + (s.AT @ vec[s.n:] if s.m else 0.0)

    def __call__(self, x, dx, xt, z, y, dy, zt, mode=0, need=0, thr=0.0, unscaled=0, **kw):
        d, plant = self.d, self.plant
        vec = dict(zip(VEC, (np.asarray(a, dtype=np.float64) for a in (x, dx, xt, z, y, dy, zt))))
        dd = d
        if plant == 'u_without_scaling':
            dd = _Shallow(d, Dinv=np.ones(d.n), Einv=np.ones(d.m), D=np.ones(d.n), E=np.ones(d.m))
        if plant == 'support_l_u_swapped':
            dd = _Shallow(d, l=d.u, u=d.l)
        r = Ref(dd, vec, np.float64, need, thr, unscaled)
        v = dict(r.v)
        sig = d.s.sigma
        # (P~ + sigma I) x - sigma x as the kernels form it: the diagonal of B holds the rounded sum
        bx, bdx = d.s.P @ vec['x'] + sig * vec['x'], d.s.P @ vec['dx'] + sig * vec['dx']
        r2 = _with_px(dd, vec, r, bx if plant == 'px_keeps_sigma_x' else bx - sig * vec['x'])
        v.update({k: r2[k] for k in ('R_PX_U', 'R_PX_S', 'R_DUA_U', 'R_DUA_S', 'R_XPX')})
        if need & NEED_DINF:
            pdx = bdx if plant == 'pdx_without_sigma_dx' else bdx - sig * vec['dx']
            v['R_PDX_U'], v['R_PDX_S'] = _mx(dd.Dinv * pdx), _mx(pdx)
        if plant in ('max_drops_last_partial', 'sum_drops_last_partial', 'nan_swallowed_by_max'):
            v = self._partials(dd, vec, need, thr, unscaled, v)
        res = np.array([np.nan if v[k] is None else float(v[k]) for k in NAMES])
        out = dict(res_vec=res, res=dict(zip(NAMES, res)))
        return 0, out

    def _partials(self, d, vec, need, thr, unscaled, v):
        """the same quantities from per-workgroup partials (WG_ROWS rows each), with the planted fold"""
        plant = self.plant
        out = dict(v)

        def fold(rows_n, names):
            if rows_n == 0:
                return
            last = (rows_n - 1) // WG_ROWS * WG_ROWS
            for k in names:
                if v[k] is None:
                    continue
                keep = np.ones(rows_n, dtype=bool)
                per = self._row_values(d, vec, k, thr, unscaled)
                if k in SUMS:
                    if plant == 'sum_drops_last_partial':
                        keep[last:] = False
                    out[k] = per[keep].sum()
                else:
                    if plant == 'max_drops_last_partial':
                        keep[last:] = False
                    a = np.abs(per[keep])
                    out[k] = (np.nanmax(a) if (a.size and not np.isnan(a).all()) else 0.0) if plant == 'nan_swallowed_by_max' else _mx(a)
        fold(d.m, M_SIDE + ('R_ADX_VIOL',))
        fold(d.n, NAMES[10:27])
        return out

    def _row_values(self, d, vec, k, thr, unscaled):
        s = d.s
        x, dx, z, y, dy = (vec[a] for a in ('x', 'dx', 'z', 'y', 'dy'))
        with np.errstate(invalid='ignore', over='ignore'):
            if k in M_SIDE or k == 'R_ADX_VIOL':
                ax = s.A @ x
                adx = s.A @ dx
                return dict(R_PRI_U=d.Einv * (ax - z), R_AX_U=d.Einv * ax, R_Z_U=d.Einv * z, R_PRI_S=ax - z, R_AX_S=ax, R_Z_S=z, R_DY_U=d.E * dy, R_DY_S=dy,
                            R_PINF_LHS=support_term(d.l, d.u, dy), R_SUPP=support_finite(d, d.l, d.u, y),
                            R_ADX_VIOL=adx_violates(d, d.Einv * adx if unscaled else adx, thr).astype(np.float64))[k]
            px, aty, q = s.P @ x, s.AT @ y, s.q
            dr = px + q + aty
            return dict(R_DUA_U=d.Dinv * dr, R_PX_U=d.Dinv * px, R_ATY_U=d.Dinv * aty, R_DUA_S=dr, R_PX_S=px, R_ATY_S=aty, R_DX_U=d.D * dx, R_DX_S=dx,
                        R_XPX=x * px, R_QX=q * x, R_QDX=q * dx, R_QN_S=q, R_QN_U=d.Dinv * q, R_ATDY_U=d.Dinv * (s.AT @ dy), R_ATDY_S=s.AT @ dy,
                        R_PDX_U=d.Dinv * (s.P @ dx), R_PDX_S=s.P @ dx)[k]

    def rho_change(self, vec, rho_bar_new):
        """what the group leaves after a rho change (check_rho_change's `out`)"""
        d, s, plant = self.d, self.d.s, self.plant
        rho = rho_vector(d, rho_bar_new, self.rho, self.rho_bar)
        v_rho = self.rho if plant == 'v_from_old_rho' else rho
        ztg = np.zeros(d.m) if plant == 'ztg_not_reset' else vec['zt'].copy()
        Minv = 1.0 / s.ops(np.float64).kdiag(s, rho)
        return dict(rho=rho, rho_inv=1.0 / rho, v=v_rho * vec['z'] - vec['y'], t0=rho * vec['zt'], ztg=ztg, xg=vec['xt'].copy(), xsp=vec['xt'].copy(), Minv=Minv)


class _Shallow:
    """a Data with some fields replaced"""

    def __init__(self, d, **kw):
        self.__dict__.update(d.__dict__)
        self.__dict__.update(kw)
        if 'l' in kw:
            self.ufin, self.lfin = self.u < INFTY * 1e-4, self.l > -INFTY * 1e-4


def _with_px(d, vec, r, px):
    with np.errstate(invalid='ignore'):
        dr = px + d.s.q + r.rows['aty']
        return dict(R_PX_U=_mx(d.Dinv * px), R_PX_S=_mx(px), R_DUA_U=_mx(d.Dinv * dr), R_DUA_S=_mx(dr), R_XPX=(vec['x'] * px).sum())


# ------------------------------------------------------------------------------------------------------------------------------ mode 1: the device-driven group
def variant_problem(P, q, A, l, u):
    """The problem of the certificate scenarios, from a shape's: the last row of A becomes a copy of the row before it and the two contradict each other
    (a'x in [1, 2] and in [-2, -1]); row 0 gets the bounds [-3, -0.5]; one column j0 that none of these rows touches becomes a direction of unbounded
    descent: row and column j0 of P are zeroed (the pattern stays), q_j0 = 1, and every row of A that touches j0 is free on both sides.
    Returns (P, q, A, l, u, j0)."""
    A = sp.csr_matrix(A).copy(); A.sort_indices()
    m, n = A.shape
    A = sp.vstack([A[:m - 1], A[m - 2]], format='csr')
    l, u, q = np.array(l, dtype=np.float64), np.array(u, dtype=np.float64), np.array(q, dtype=np.float64)
    l[m - 2], u[m - 2], l[m - 1], u[m - 1], l[0], u[0] = 1.0, 2.0, -2.0, -1.0, -3.0, -0.5
    taken = set(A[0].indices) | set(A[m - 2].indices)
    Ac = sp.csc_matrix(A)
    j0 = next(j for j in range(n // 2, n) if j not in taken and Ac.indptr[j + 1] > Ac.indptr[j])
    Pc = sp.csc_matrix(P).copy()
    Pc.data[Pc.indptr[j0]:Pc.indptr[j0 + 1]] = 0.0
    Pc = sp.csr_matrix(Pc); Pc.data[Pc.indptr[j0]:Pc.indptr[j0 + 1]] = 0.0
    q[j0] = 1.0
    touch = Ac.indices[Ac.indptr[j0]:Ac.indptr[j0 + 1]]
    l[touch], u[touch] = -np.inf, np.inf
    return sp.csc_matrix(Pc), q, sp.csc_matrix(A), l, u, j0


def scenario(d, which, sol=None, j0=None, seed=31):
    """(vec, entry arguments) of a mode 1 scenario.  sol: (x, y) UNSCALED of the solved problem (scenario c); j0: variant_problem's (scenario f)."""
    s = d.s
    vec = draw(d, seed)
    kw = dict(mode=1, iter=50, at_check=1, chunk_done=1, status_in=CTL_RUNNING)
    if which == 'a':
        kw.update(chunk_done=0)
    elif which == 'b':
        kw.update(at_check=0, iter=30)
    elif which == 'c':
        x, y = sol
        vec = zeros(d)
        vec['x'] = d.Dinv * x
        vec['y'] = d.c * d.Einv * y if d.m else np.zeros(0)
        vec['z'] = np.minimum(np.maximum(s.A @ vec['x'], d.l), d.u) if d.m else np.zeros(0)
        vec['xt'], vec['zt'] = vec['x'].copy(), vec['z'].copy()
        kw.update(iter=75)
    elif which == 'd':
        vec['dx'][:] = 0.0; vec['dy'][:] = 0.0
        if d.m:
            vec['z'] = s.A @ vec['x'] + 1e-4 * vec['z']
    elif which in ('e', 'e2'):
        vec['x'][:] = 0.0; vec['y'][:] = 0.0; vec['dx'][:] = 0.0; vec['dy'][:] = 0.0
        vec['dy'][d.m - 1], vec['dy'][d.m - 2] = d.Einv[d.m - 1], -d.Einv[d.m - 2]
        if which == 'e2':
            vec['dy'][0] = d.Einv[0]
        kw.update(iter=25)
    elif which == 'f':
        vec['x'][:] = 0.0; vec['y'][:] = 0.0; vec['dx'][:] = 0.0; vec['dy'][:] = 0.0
        vec['dx'][j0] = -d.Dinv[j0]
        kw.update(iter=25)
    elif which == 'g':
        kw.update(status_in=CTL_DONE)
    elif which == 'h':
        vec['x'][0] = np.nan
        vec['dx'][:] = 0.0; vec['dy'][:] = 0.0
    return vec, kw


def scenario_expectation(d, which, vec, settings, rho_bar):
    """What the reference says of a scenario's inputs, with the margins asserted: every comparison that decides it has its two sides a factor 2 apart.
    Returns (ref, rules)."""
    ref = Ref(d, vec, L, NEED_PINF | NEED_DINF, 0.0, 0)
    ru = Rules(d, ref, settings, rho_bar)
    if which == 'c':
        ru.decided([k for k in ('pri', 'dua') if k in ru.ratios])
        assert ru.pri_ok and ru.dua_ok and not ru.non_cvx
        gap_ratio = abs(ru.gap) / (settings['eps_abs'] + settings['eps_rel'] * max(abs(ru.obj), abs(ru.dual_obj)))
        assert gap_ratio <= 0.5, gap_ratio
    elif which == 'd':
        ru.decided(list(ru.ratios))
        assert not ru.dua_ok and ru.need == 0                  # (z follows A x: the primal test may pass, the dual one fails by far, no certificate is asked for)
        r = ru.rho_estimate / rho_bar
        assert (r > 10.0 or r < 0.1) and (d.m == 0 or 2e-6 < ru.rho_estimate < 5e5), 'the rho estimate %.3e is no decided update of %.3e' % (ru.rho_estimate, rho_bar)
    elif which in ('e', 'e2', 'f'):
        ru.decided(list(ru.ratios))
        assert ru.need == (NEED_DINF if which == 'f' else NEED_PINF), ru.need
        unsc = ru.unsc
        ref2 = Ref(d, vec, L, ru.need, ru.thr_d, unsc)
        if which == 'f':
            lhs, rhs = float(ref2.v['R_PDX_U' if unsc else 'R_PDX_S']), ru.sc * ru.edi * ru.nd_d
            assert lhs <= 0.5 * rhs and float(ref2.v['R_ADX_VIOL']) == 0.0
            dist = np.abs(np.abs(np.asarray(ref2.adx, dtype=np.float64)) - ru.thr_d)[d.ufin | d.lfin]
            assert (dist > 64 * ref2.e_adx[d.ufin | d.lfin]).all(), 'a row of A dx within 64 x its bound of the threshold'
        else:
            lhs, rhs = float(ref2.v['R_ATDY_U' if unsc else 'R_ATDY_S']), ru.epi * ru.nd_p
            assert (lhs <= 0.5 * rhs) if which == 'e' else (lhs >= 2.0 * rhs), (lhs, rhs)
        ref.v.update({k: ref2.v[k] for k in PINF_Q + DINF_Q}); ref.b.update({k: ref2.b[k] for k in PINF_Q + DINF_Q})
    elif which == 'h':
        assert ru.non_cvx
    return ref, ru


def check_ctl_equal_nan(out, where):
    """dev == host field by field: ints exactly, doubles bitwise (two NaNs are equal whatever their payloads)"""
    dev, host = out['dev'], out['host']
    assert dev.keys() == host.keys()
    for k in dev:
        a, b = dev[k], host[k]
        if isinstance(a, float):
            same = (np.isnan(a) and np.isnan(b)) or wb_ref.bits(a) == wb_ref.bits(b)
        else:
            same = a == b
        assert same, 'Ctl.%s: the device left %r, the host\'s rules give %r -- error against the tolerance 0 (%s)' % (k, a, b, where)


PEEKED = ('rho', 'rho_inv', 'v', 't0', 'ztg', 'xg', 'xsp', 'Minv')


def unchanged(out, before, where):
    for k in PEEKED:
        _bitwise(out[k], before[k], k, where + ': changed by a group that had to leave it')


def res_zero(out, names, where):
    for k in names:
        assert out['res'][k] == 0.0, '%s: %r left by a kernel that had to idle -- error against the tolerance 0 (%s)' % (k, out['res'][k], where)


def check_mode1(entry, d, settings, rho_bar, diagonal, worst, where, sol=None, tight_factor=None):
    """Scenarios a, b, c, d, g, h on a handle of the shape's own problem.  entry: hip_test_boundary's signature; settings: what the handle was set up with;
    rho_bar: the handle's.  Every call's dev == host.  Returns the scenario d answer (for the caller's keep = 1 leg)."""
    launches = 11 + (1 if diagonal else 0)
    def run(vec, **kw):
        """mode 0 on the same vectors first: what it peeks of rho, v, t0, ztg, xg, xsp, Minv is the state a group that changes no rho has to leave"""
        st0, before = call(entry, vec)
        st, out = call(entry, vec, **kw)
        assert st0 == 0 and st == 0
        return before, out
    rho_old = call(entry, draw(d, 31))[1]['rho']
    # ---- (a) the chunk is unfinished
    vec, kw = scenario(d, 'a')
    before, out = run(vec, **kw)
    st = 0
    assert st == 0 and out['launches'] == launches
    check_ctl_equal_nan(out, where + ' (a)')
    res_zero(out, NAMES, where + ' (a)'); unchanged(out, before, where + ' (a)')
    dev = out['dev']
    assert dev['status'] == CTL_RUNNING and dev['rho_flag'] == 0 and dev['boundaries'] == 0 and dev['iter'] == 0, dev
    # ---- (b) finished, not at a check
    vec, kw = scenario(d, 'b')
    before, out = run(vec, **kw)
    st = 0
    assert st == 0
    check_ctl_equal_nan(out, where + ' (b)')
    res_zero(out, NAMES, where + ' (b)'); unchanged(out, before, where + ' (b)')
    dev = out['dev']
    assert dev['status'] == CTL_RUNNING and dev['boundaries'] == 1 and dev['iter'] == 30 and 30 < dev['ch_next'] <= 50 and dev['rho_flag'] == 0, dev
    assert out['tol_rel'] == dev['tol_rel'], (out['tol_rel'], dev['tol_rel'])
    want_abs = dev['tol_abs'] if not dev['ch_tight'] or tight_factor is None else max(tight_factor * dev['tol_abs'], 1e-13)
    assert out['tol_abs'] == want_abs, 'the PCG tolerance of the next chunk on the device: %r, expected %r (%s)' % (out['tol_abs'], want_abs, where)
    # ---- (g) the solve is over: the whole group idles
    vec, kw = scenario(d, 'g')
    before, out = run(vec, **kw)
    st = 0
    assert st == 0
    check_ctl_equal_nan(out, where + ' (g)')
    res_zero(out, NAMES, where + ' (g)'); unchanged(out, before, where + ' (g)')
    assert out['dev']['status'] == CTL_DONE and out['dev']['boundaries'] == 0
    # ---- (h) NaN in x at a check
    vec, kw = scenario(d, 'h')
    scenario_expectation(d, 'h', vec, settings, rho_bar)
    before, out = run(vec, **kw)
    check_ctl_equal_nan(out, where + ' (h)')
    assert out['dev']['status'] == CTL_DONE and out['dev']['osqp_status'] == NON_CVX, out['dev']
    res_zero(out, PINF_Q + DINF_Q, where + ' (h)'); unchanged(out, before, where + ' (h)')
    # ---- (c) converged iterates, loose eps
    if sol is not None:
        vec, kw = scenario(d, 'c', sol=sol)
        ref, ru = scenario_expectation(d, 'c', vec, settings, rho_bar)
        base_c, out = run(vec, **kw)
        check_ctl_equal_nan(out, where + ' (c)')
        dev = out['dev']
        assert dev['status'] == CTL_DONE and dev['osqp_status'] == SOLVED and dev['iter'] == 75 and dev['rho_flag'] == 0, dev
        ref.v.update({k: None for k in PINF_Q + DINF_Q})
        judge(out, 0, ref, worst, where + ' (c)')
        res_zero(out, PINF_Q + DINF_Q, where + ' (c)'); unchanged(out, base_c, where + ' (c)')
        for k, want in ru.info.items():
            worst.note('info.' + k, abs(dev[k] - want), ru.bounds[k] + 1e-300, where + ' (c)')
    # ---- (d) far from converged at an adaptation point: rho changes
    vec, kw = scenario(d, 'd')
    ref, ru = scenario_expectation(d, 'd', vec, settings, rho_bar)
    outs = []
    for groups in (1, 2):
        st, out = call(entry, vec, groups=groups, **kw)
        assert st == 0 and out['launches'] == groups * launches
        check_ctl_equal_nan(out, where + ' (d, groups %d)' % groups)
        dev = out['dev']
        assert dev['status'] == CTL_RUNNING and dev['rho_flag'] == (1 if groups == 1 else 0) and dev['rho_updates'] == 1 and dev['boundaries'] == 1 and dev['iter'] == 50, dev
        assert dev['rho_bar'] == dev['rho_estimate']
        worst.note('rho_estimate', abs(dev['rho_estimate'] - ru.rho_estimate), ru.rho_estimate_bound, where + ' (d)')
        ref.v.update({k: None for k in PINF_Q + DINF_Q})
        judge(out, 0, ref, worst, where + ' (d)')
        res_zero(out, PINF_Q + DINF_Q, where + ' (d)')
        check_rho_change(out, d, vec, dev['rho_bar'], rho_old, rho_bar, diagonal, worst, where + ' (d, groups %d)' % groups)
        outs.append(out)
    for k in PEEKED + ('res_vec',):                                         # "must not repeat the rho update": the second group changes nothing
        _bitwise(outs[1][k], outs[0][k], k, where + ' (d): the second group changed it')
    for k, a in outs[0]['dev'].items():
        if k != 'rho_flag':
            assert a == outs[1]['dev'][k], 'Ctl.%s after one group %r, after two %r -- error against the tolerance 0 (%s)' % (k, a, outs[1]['dev'][k], where)
    return vec, kw, outs[0]


def check_certificates(entry, d, settings, rho_bar, j0, worst, where):
    """Scenarios e, e', f on a handle of variant_problem."""
    for which in ('e', 'e2', 'f'):
        vec, kw = scenario(d, which, j0=j0)
        ref, ru = scenario_expectation(d, which, vec, settings, rho_bar)
        st, before = call(entry, vec)
        assert st == 0
        st, out = call(entry, vec, **kw)
        w = '%s (%s)' % (where, which)
        assert st == 0
        check_ctl_equal_nan(out, w)
        dev = out['dev']
        idle = DINF_Q if which != 'f' else PINF_Q
        ref.v.update({k: None for k in idle})
        judge(out, 0, ref, worst, w)
        res_zero(out, idle, w)
        assert dev['need'] == (NEED_DINF if which == 'f' else NEED_PINF) and dev['stage2'] == 0 and dev['iter'] == 25 and dev['rho_flag'] == 0, dev
        if which == 'e2':
            assert dev['status'] == CTL_RUNNING and dev['boundaries'] == 1 and 25 < dev['ch_next'] <= 50, dev
        else:
            assert dev['status'] == CTL_DONE and dev['osqp_status'] == (DUAL_INFEASIBLE if which == 'f' else PRIMAL_INFEASIBLE), dev
        unchanged(out, before, w)
