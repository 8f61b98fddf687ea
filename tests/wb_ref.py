"""Cases, references, tolerances and checks of the kernel-level tests of the Woodbury correction (osqp-python_amd/csrc/woodbury_hip.hip, wbdirect_hip.hip;
DESIGN.md section 4.7) -- numpy / scipy only, no GPU.  Written once, used by two tiers: tests/test_gpu_woodbury_kernels.py runs it on a handle of the
product through the diagnostic entry osqp_hip_test_woodbury, tests/test_wb_ref.py on the numpy stand-in below (Standin), where it also has to notice
planted mistakes.

APPLY tier (check_apply).  The entry runs wb_factor and wb_apply unchanged on a right-hand side of the test and returns u = M^-1 r, x~, 1 / D0, the dense
system S (row space) or T (column space), its inverse, the rho vector and the partial results the PCG would fold.  The reference is built in
np.longdouble from the CALLER's P, A, sigma, the rho vector the entry returned and the handle's scaling:
    P~ = c D P D,  A~ = E A D;   D0_j = P~_jj + sigma + sum over the short rows of rho_i A~_ij^2;   S = diag(1 / rho_L) + A~_L D0^-1 A~_L';
    T = D0_C + A~_d' diag(w) A~_d on the dense columns C,  w_a = rho_a / (1 + rho_a sigma_a),  sigma_a = sum over the singletons of row a of A~_aj^2 / D0_j;
    M = diag(D0) + A~_L' diag(rho_L) A~_L;   u_ref = M^-1 r.
u_ref is a solve with M ITSELF: an fp64 solve (Cholesky of the dense M up to order DENSE_M_MAX, the fp64 evaluation of the formulas above it), refined
with residuals r - M u of M's own definition in np.longdouble until the correction is below 2^-60 of the solution.  Where K0 is diagonal the file also
asserts M = K (entrywise up to order DENSE_M_MAX, structurally -- P~ diagonal, one entry per short row -- above).

TOLERANCE.  Measured against the reference, never against the kernels: e64 is the relative error (max norm) of a plain fp64 numpy evaluation of the same
formulas (1 / D0, S by a matrix product, np.linalg.inv, the three products; the column-space formulas for that form) against the long-double value, and
    err <= 64 max(e64, nsum 2^-53) scale ,   nsum = the longest sum of the operation,  scale = the max norm of the reference quantity.
The 64 covers another order of summation and Gauss-Jordan in place of LAPACK.  This is not a stability bound: it works because an indexing mistake on
these inputs is >= 1e-4, eight orders above.  CONDITION, asserted for every case: e64 <= 1e-12.  S / T and 1 / D0 are held to it in every component;
S^-1 through || S_ref S^-1 - I ||_max against the same product with the fp64 inverse (orders above FULL_RESIDUAL_MAX: on RESIDUAL_COLS columns, among
them the first, the last and the neighbours of every multiple of 64 -- the long-double product of the whole matrix would take minutes).

ITERATION tier (check_iterations).  The direct modes that never call wb_apply (wbdirect_hip.hip, the fused column-space iteration) are compared after
k = 1, 2, 3 ADMM iterations (max_iter = k, no rho adaptation, no polish) with a long-double run of the textbook iteration with an exact solve with K,
from a cold start and from a warm start; e64 from an fp64 run of the same iteration whose solve is the fp64 evaluation of the apply tier's formulas.  Conditions asserted on the reference: at every iteration rows
clamp low, clamp high and stay free; no value that is projected lies within 1e-6 of a bound (fp64 cannot flip a branch); cond_2(K) <= 1e7.
"""
import contextlib
import functools
import os

import numpy as np
import scipy.linalg
import scipy.sparse as sp

L = np.longdouble
U = 2.0 ** -53
TAIL = 16
FACTOR = 64.0
E64_MAX = 1e-12
LONG = 128                      # a row with more entries is a long row (backend.h kLongRow)
SMALL_MAX = 128                 # ... up to this many of them: the small form (kWbMaxRows)
DENSE_M_MAX = 700
FULL_RESIDUAL_MAX = 320
RESIDUAL_COLS = 48
NOT_IMPLEMENTED, VALIDATION = 10, 1         # OSQP_FUNC_NOT_IMPLEMENTED, OSQP_DATA_VALIDATION_ERROR (include/osqp_hip.h)

# ------------------------------------------------------------------------------------------------------------------------------ cases
SMALL_R = [1, 2, 7, 63, 64, 65, 127, 128]
SMALL_N = [129, 136, 137, 160, 161, 192, 193, 257]
# 20 of the 64 pairs: every r and every n at least twice, the corners, r on both sides of the 64-lane edges with n on both sides of the slice / unroll edges
SMALL_PAIRS = [(1, 129), (1, 193), (2, 136), (2, 257), (7, 137), (7, 160), (7, 192), (63, 129), (63, 161), (64, 136), (64, 192), (65, 137), (65, 193),
               (127, 160), (127, 257), (127, 161), (128, 129), (128, 193), (128, 257), (2, 161)]
ROW_CASES = [(129, 140), (130, 141), (191, 150), (257, 161), (1030, 140)]                      # (r, n); three columns untouched: ct = n - 3 takes both parities
COL_CASES = [(130, 176, 1), (131, 180, 2), (200, 270, 1), (200, 267, 2), (1540, 2060, 1)]      # (cd, r, singletons per row); the last: 129-entry rows


def small_cases():
    out = []
    for k, (r, n) in enumerate(SMALL_PAIRS):
        for k0diag in (True, False):
            out.append(dict(form='small', r=r, n=n, k0diag=k0diag, seed=100 + k, scaling=10 if k % 5 == 3 else 0))
    return out


def row_cases():
    # (more long rows than columns: rho A_L' A_L has full rank and M^-1 r = D0^-1 (r - A_L' h) cancels all of r but 1 / (1 + rho sigma_max^2 / D0) of it -- the
    #  digits the fp64 evaluation loses there are e64's.  Entries of 4 / sqrt(r), and 0.03 of that in the equality rows, whose rho is 1000 times the others' on
    #  a problem this small, keep rho sigma_max^2 / D0 of order one and e64 within the condition.)
    return [dict(form='row', r=r, n=n, k0diag=True, seed=300 + k, scaling=0, long_scale=4.0 / np.sqrt(r), eq_scale=0.03) for k, (r, n) in enumerate(ROW_CASES)]


def col_cases():
    return [dict(form='col', cd=cd, r=r, singles=s, k0diag=True, seed=400 + k, scaling=0, rowlen=129 if cd > 1000 else None) for k, (cd, r, s) in enumerate(COL_CASES)]


def case_id(c):
    if c['form'] == 'col':
        return 'col-cd%d-r%d-s%d' % (c['cd'], c['r'], c['singles'])
    return '%s-r%d-n%d-%s%s' % (c['form'], c['r'], c['n'], 'diag' if c['k0diag'] else 'offdiag', '-scaled' if c['scaling'] else '')


ENV = {'small': {}, 'row': {'OSQP_HIP_WOODBURY_DUAL': '0'}, 'col': {'OSQP_HIP_WOODBURY_DUAL': '1'}}


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _values(rng, k):
    """entries away from zero: magnitudes in [0.25, 1.75], random signs"""
    return (0.25 + 1.5 * rng.random(k)) * rng.choice([-1.0, 1.0], k)


@functools.lru_cache(maxsize=None)
def _problem(key):
    c = dict(key)
    rng = np.random.default_rng(c['seed'])
    rows = []                                   # (columns, values, kind): kind 'eq' | 'box'
    if c['form'] == 'col':
        cd, r, s = c['cd'], c['r'], c['singles']
        n = cd + r * s + 1                      # dense columns, singleton columns, one column no long row touches
        perm = rng.permutation(n)               # (the three kinds of column interleaved)
        dense, single, free = perm[:cd], perm[cd:cd + r * s].reshape(r, s), perm[cd + r * s:]
        want = (c['rowlen'] - s) if c['rowlen'] else None
        pats = [rng.choice(cd, want if want else int(rng.integers(LONG + 1 - s, cd + 1)), replace=False) for _ in range(r)]
        cnt = np.zeros(cd, dtype=int)
        for p in pats:
            cnt[p] += 1
        if want is None:
            for j in np.flatnonzero(cnt < 2):        # a dense column has two or more long-row entries
                for a in rng.permutation(r):
                    if j not in pats[a]:
                        pats[a] = np.append(pats[a], j); cnt[j] += 1
                        if cnt[j] >= 2:
                            break
        assert cnt.min() >= 2, 'a dense column with fewer than two long-row entries'
        for a in range(r):
            cols = np.concatenate([dense[pats[a]], single[a]])
            vals = np.concatenate([_values(rng, len(pats[a])), [-1.0, 0.5][:s]])
            rows.append((cols, vals, 'eq' if a % 3 == 0 else 'box'))
        for j in np.concatenate([dense, free, single[::7, 0]]):
            rows.append((np.array([j]), _values(rng, 1), 'box'))
        pdiag = 0.5 + rng.random(n)
        P = sp.diags(pdiag, format='csc')
    else:
        n, r = c['n'], c['r']
        free = rng.choice(n, min(3, n - (LONG + 1)), replace=False)
        avail = np.setdiff1d(np.arange(n), free)
        for a in range(r):
            cols = rng.choice(avail, int(rng.integers(LONG + 1, len(avail) + 1)), replace=False)
            rows.append((cols, c.get('long_scale', 1.0) * (c.get('eq_scale', 1.0) if a % 3 == 0 else 1.0) * _values(rng, len(cols)), 'eq' if a % 3 == 0 else 'box'))
        if c['k0diag']:
            for j in range(n):
                rows.append((np.array([j]), (c.get('eq_scale', 1.0) if j % 11 == 4 else 1.0) * _values(rng, 1), 'eq' if j % 11 == 4 else 'box'))
            rows.append((np.array([5]), _values(rng, 1), 'box'))                    # a column with two one-entry rows
            P = sp.diags(0.5 + rng.random(n), format='csc')
        else:
            for i in range(n // 2):
                cols = rng.choice(n, int(rng.integers(2, 6)), replace=False)
                rows.append((cols, _values(rng, len(cols)), 'eq' if i % 11 == 4 else 'box'))
            off = 0.3 * _values(rng, n - 1) * (rng.random(n - 1) < 0.6)
            P = sp.diags([off, 2.0 + rng.random(n), off], [-1, 0, 1], format='csc')
    order = rng.permutation(len(rows))          # (long rows anywhere among the short ones)
    rows = [rows[i] for i in order]
    m = len(rows)
    ri = np.concatenate([np.full(len(cv[0]), i) for i, cv in enumerate(rows)])
    A = sp.csc_matrix((np.concatenate([cv[1] for cv in rows]), (ri, np.concatenate([cv[0] for cv in rows]))), shape=(m, n))
    A.sort_indices()
    x0 = 0.3 * rng.standard_normal(n)
    mid = A @ x0
    eq = np.array([cv[2] == 'eq' for cv in rows])
    # bounds around A x0: some of them tight enough to be active at once, some wide
    half = np.where(rng.random(m) < 0.5, 0.05, 0.8) * (0.5 + rng.random(m))
    shift = 0.4 * rng.standard_normal(m)
    l = np.where(eq, mid + shift, mid + shift - half); u = np.where(eq, mid + shift, mid + shift + half)
    q = rng.standard_normal(n)
    P = sp.csc_matrix(P); P.sort_indices()
    return dict(P=P, q=q, A=A, l=l, u=u, n=n, m=m)


def problem(c):
    return _problem(tuple(sorted((k, v) for k, v in c.items())))


def settings(c, **kw):
    st = dict(verbose=False, scaling=c['scaling'], adaptive_rho=False, polishing=False, rho=0.1, sigma=1e-6, alpha=1.6, max_iter=50, eps_abs=1e-9, eps_rel=1e-9)
    st.update(kw)
    return st


def right_hand_sides(c):
    n = problem(c)['n']
    rng = np.random.default_rng(c['seed'] + 7)
    e0, e1 = np.zeros(n), np.zeros(n)
    e0[0] = 1.0; e1[n - 1] = -2.5
    return [rng.standard_normal(n), 10.0 ** rng.uniform(-3, 3, n) * rng.standard_normal(n), e0, e1]


# ------------------------------------------------------------------------------------------------------------------------------ handles
class Product:
    """A set-up handle of the product (the GPU tier's subject)."""

    def __init__(self, c, environment=None, **kw):
        import osqp_amd
        self.c, p = c, problem(c)
        self.A = p['A'].copy()
        self.st = settings(c, **kw)
        with env(**dict(ENV[c['form']], **(environment or {}))):
            self.model = osqp_amd.OSQP(algebra='hip')
            self.model.setup(p['P'], p['q'], self.A, p['l'], p['u'], **self.st)
        self.solver = self.model._solver
        self.sigma = self.st['sigma']

    def test(self, r, x0=None, **kw):
        return self.solver.hip_test_woodbury(r, x0, **kw)

    def scaling(self):
        return self.solver.hip_scaling()

    def set_rho(self, rho):
        self.model.update_settings(rho=rho)

    def set_Ax(self, Ax):
        self.model.update(Ax=Ax)
        self.A = sp.csc_matrix((Ax, self.A.indices, self.A.indptr), shape=self.A.shape)


class Standin:
    """The same interface on plain fp64 numpy: the three forms of M^-1 as the kernels evaluate them (row space: S, S^-1; column space: the singletons
    eliminated row by row, T on the dense columns), the engine's rho rule (equality rows 1000 x up to n = 256, 10 x above), the engine's own equilibration (computed by the host simulator) where a case asks for scaling.
    plant: one of PLANTS -- a single mistake of the kind a kernel could have."""
    PLANTS = ('S_drops_last_column', 'rho_for_its_inverse', 'singleton_dropped_from_sigma', 'untouched_column_zero', 'xs_overwritten', 'S_row_swapped_in_idx')

    def __init__(self, c, plant=None, **kw):
        self.c, p = c, problem(c)
        self.p, self.A, self.plant = p, p['A'].copy(), plant
        self.st = settings(c, **kw)
        self.sigma, self.rho_bar = self.st['sigma'], self.st['rho']
        rng = np.random.default_rng(c['seed'] + 1)
        n, m = p['n'], p['m']
        self.D, self.E, self.cc = np.ones(n), np.ones(m), 1.0
        if c['scaling']:                        # the engine's own equilibration of this problem, from the host simulator (the conditions depend on it)
            from hostsim_util import hostsim
            with hostsim():
                self.D, self.E, self.cc = Product(c, **kw).scaling()
        self.xs_state = rng.standard_normal(n)

    def scaling(self):
        return self.D, self.E, self.cc

    def set_rho(self, rho):
        self.rho_bar = rho

    def set_Ax(self, Ax):
        self.A = sp.csc_matrix((Ax, self.A.indices, self.A.indptr), shape=self.A.shape)

    def rho_vec(self):
        return self.rho_bar * np.where(self.p['l'] == self.p['u'], 1000.0 if self.p['n'] <= 256 else 10.0, 1.0)      # (the engine's rule: Engine::mixed_eq_factor)

    def test(self, r, x0=None, refactor=1, parity=0, direct=0, lens=None):
        n, m = self.p['n'], self.p['m']
        if lens or not (parity in (0, 1) and direct in (0, 1)) or len(r) != n or (direct and (x0 is None or len(x0) != n)) or (not direct and x0 is not None and len(x0)):
            return VALIDATION, None
        s = structure(self.A, self.c['form'])
        rho = self.rho_vec()
        f = Formulas(self.p['P'], self.A, self.sigma, rho, self.scaling(), s, np.float64, plant=self.plant)
        u = f.apply(np.asarray(r, dtype=np.float64))
        out = {k: np.full(v + TAIL, np.nan) for k, v in (('u', n), ('xs', n), ('dinv0', n), ('S', s['order'] ** 2), ('Sinv', s['order'] ** 2), ('rho', m))}
        out['idx'] = np.full(s['order'] + TAIL, -1, dtype=np.int32)
        out['u'][:n] = u
        out['xs'][:n] = (u if self.plant == 'xs_overwritten' else np.asarray(x0) + u) if direct else self.xs_state
        out['dinv0'][:n] = f.Dinv0
        out['S'][:s['order'] ** 2] = f.S.ravel(); out['Sinv'][:s['order'] ** 2] = f.Sinv.ravel()
        out['rho'][:m] = rho
        idx = np.array(s['idx'])
        if self.plant == 'S_row_swapped_in_idx' and len(idx) > 1:
            idx[[0, 1]] = idx[[1, 0]]
        out['idx'][:s['order']] = idx
        rr = np.asarray(r, dtype=np.float64)
        out.update(form={'small': 0, 'row': 1, 'col': 2}[self.c['form']], order=s['order'], rows=len(s['long']), exact=int(self.c['k0diag']), info=(1 if self.c['form'] == 'small' else 0, 0),
                   done=int(direct), iters=int(direct), gamma=float(rr @ u), rnorm=float(np.abs(rr).max()))
        return 0, out


# ------------------------------------------------------------------------------------------------------------------------------ reference
def structure(A, form):
    """Long rows (more than LONG entries), and for the column-space form the kinds of the columns: 1 dense (two or more long-row entries), 2 singleton, 0 none."""
    R = sp.csr_matrix(A)
    cnt = np.diff(R.indptr)
    long_ = np.flatnonzero(cnt > LONG)
    per_col = np.asarray((sp.csr_matrix(R[long_]) != 0).sum(axis=0)).ravel()
    s = dict(long=long_, short=np.flatnonzero(cnt <= LONG), kind=np.where(per_col >= 2, 1, np.where(per_col == 1, 2, 0)))
    if form == 'col':
        s['dcol'] = np.flatnonzero(s['kind'] == 1)
        s['idx'], s['order'] = s['dcol'], len(s['dcol'])
    else:
        s['idx'], s['order'] = long_, len(long_)
    return s


class Formulas:
    """D0, S or T, its inverse and M^-1 r by the formulas of the header in the number type T (np.float64: the e64 evaluation and the stand-in;
    np.longdouble: the reference of D0, S, T).  s['idx'] fixes the order of S's rows / T's columns."""

    def __init__(self, P, A, sigma, rho, scal, s, T, plant=None, system=True):      # system = False: D0 and the long rows only, no S / T
        D, E, c = scal
        self.T, self.s, self.plant = T, s, plant
        n = A.shape[1]
        Ab = sp.csr_matrix(sp.diags(E) @ A @ sp.diags(D))          # (fp64 products of the scaling: one rounding each, as the engine's own scaled copy has)
        Ab.sort_indices()
        Pb = sp.csc_matrix(c * (sp.diags(D) @ P @ sp.diags(D)))
        self.Ab, self.Pb, self.n = Ab, Pb, n
        rho = np.asarray(rho, dtype=T)
        self.rho = rho
        d0 = np.asarray(Pb.diagonal(), dtype=T) + T(sigma)
        sh = sp.csr_matrix(Ab[s['short']])
        contrib = np.repeat(rho[s['short']], np.diff(sh.indptr)) * np.asarray(sh.data, dtype=T) ** 2
        np.add.at(d0, sh.indices, contrib)
        self.D0, self.Dinv0 = d0, T(1) / d0
        self.rows = list(s['idx']) if 'dcol' not in s else list(s['long'])
        AL = sp.csr_matrix(Ab[self.rows])
        self.AL = AL
        self.rhoL = rho[self.rows]
        r = len(self.rows)
        if not system:
            return
        if 'dcol' in s:
            self._column_space(AL, r)
            return
        Ad = np.asarray(AL.toarray(), dtype=T)
        self.Ad = Ad
        cols = slice(0, n - 1) if plant == 'S_drops_last_column' else slice(0, n)
        S = (Ad[:, cols] * self.Dinv0[cols]) @ Ad[:, cols].T
        S[np.arange(r), np.arange(r)] += self.rhoL if plant == 'rho_for_its_inverse' else T(1) / self.rhoL
        self.S = S
        self.Sinv = np.linalg.inv(S) if T is np.float64 else None

    def _column_space(self, AL, r):
        T, s, n = self.T, self.s, self.n
        kind, dcol = s['kind'], s['dcol']
        cmap = np.full(n, -1); cmap[dcol] = np.arange(len(dcol))
        self.cmap = cmap
        val = np.asarray(AL.data, dtype=T)
        rowof = np.repeat(np.arange(r), np.diff(AL.indptr))
        sing = kind[AL.indices] == 2
        self.sing_row, self.sing_col, self.sing_val = rowof[sing], AL.indices[sing], val[sing]
        terms = self.sing_val ** 2 * self.Dinv0[self.sing_col]
        if self.plant == 'singleton_dropped_from_sigma':
            terms = terms.copy(); terms[len(terms) // 2] = 0
        sg = np.zeros(r, dtype=T)
        np.add.at(sg, self.sing_row, terms)
        self.w = self.rhoL / (T(1) + self.rhoL * sg)
        dn = kind[AL.indices] == 1
        self.d_row, self.d_col, self.d_val = rowof[dn], cmap[AL.indices[dn]], val[dn]
        cd = len(dcol)
        Tm = np.zeros((cd, cd), dtype=T)
        if T is np.float64:
            Adn = sp.csr_matrix((self.d_val, (self.d_row, self.d_col)), shape=(r, cd))
            Tm = np.asarray((Adn.T @ sp.diags(self.w) @ Adn).toarray())
        else:
            ptr = np.concatenate([[0], np.cumsum(np.bincount(self.d_row, minlength=r))])
            for a in range(r):                                     # (no column twice in a row: the fancy-indexed += adds every cell once)
                cols, v = self.d_col[ptr[a]:ptr[a + 1]], self.d_val[ptr[a]:ptr[a + 1]]
                Tm[np.ix_(cols, cols)] += self.w[a] * np.outer(v, v)
        Tm[np.arange(cd), np.arange(cd)] += self.D0[dcol]
        self.S = Tm
        self.Sinv = np.linalg.inv(Tm) if T is np.float64 else None

    def apply(self, r):
        """M^-1 r in fp64 by the form's formulas (with Sinv: the kernels' or np.linalg.inv's)"""
        T = self.T
        r = np.asarray(r, dtype=T)
        if 'dcol' not in self.s:
            g = self.Ad @ (self.Dinv0 * r)
            h = self.Sinv @ g
            u = self.Dinv0 * (r - self.Ad.T @ h)
            touched = self.s['kind'] != 0
        else:
            rr = len(self.rows)
            beta = np.zeros(rr, dtype=T)
            np.add.at(beta, self.sing_row, self.sing_val * self.Dinv0[self.sing_col] * r[self.sing_col])
            gc = r[self.s['dcol']].copy()
            np.subtract.at(gc, self.d_col, self.d_val * (self.w * beta)[self.d_row])
            xc = self.Sinv @ gc
            t = beta.copy()
            np.add.at(t, self.d_row, self.d_val * xc[self.d_col])
            rt = self.w * t
            u = self.Dinv0 * r
            u[self.s['dcol']] = xc
            u[self.sing_col] = (r[self.sing_col] - self.sing_val * rt[self.sing_row]) * self.Dinv0[self.sing_col]
            touched = self.s['kind'] != 0
        if self.plant == 'untouched_column_zero':
            u = np.where(touched, u, 0.0)
        return u


def _ld_rows(M):
    """CSR in long double: (indptr, indices, values) of a matrix whose rows are all non-empty, for row sums by np.add.reduceat"""
    M = sp.csr_matrix(M); M.sort_indices()
    assert (np.diff(M.indptr) > 0).all()
    return M.indptr[:-1], M.indices, np.asarray(M.data, dtype=L)


class Reference:
    """The long-double side for one state of a handle (matrices, rho vector, scaling)."""

    def __init__(self, P, A, sigma, rho, scal, form, system=True):      # system = False (iteration tier): M as an operator and its solves only
        self.s = s = structure(A, form)
        self.f64 = Formulas(P, A, sigma, rho, scal, s, np.float64)
        self.ld = f = Formulas(P, A, sigma, rho, scal, s, L, system=system)
        self.n, self.order, self.form = A.shape[1], s['order'], form
        self.nsum = max(self.n, s['order'], len(s['long']))
        # M = diag(D0) + A_L' diag(rho_L) A_L as an operator in long double, from its definition
        self.rp, self.ci, self.v = _ld_rows(f.AL)
        T_ = sp.csr_matrix(sp.csr_matrix(f.AL).T); T_.sort_indices()
        self.tcols = np.flatnonzero(np.diff(T_.indptr) > 0)
        self.trp, self.tri, self.tv = T_.indptr[:-1][np.diff(T_.indptr) > 0], T_.indices, np.asarray(T_.data, dtype=L)
        self.k0diag = self._k0_is_diagonal()
        if self.n <= DENSE_M_MAX:
            Ad = np.asarray(f.AL.toarray(), dtype=L)
            self.M = np.diag(f.D0) + (Ad.T * f.rhoL) @ Ad
            self.chol = scipy.linalg.cho_factor(np.asarray(self.M, dtype=np.float64))
            if self.k0diag:
                Ab = np.asarray(f.Ab.toarray(), dtype=L)
                K = np.asarray(f.Pb.toarray(), dtype=L) + L(sigma) * np.eye(self.n, dtype=L) + (Ab.T * np.asarray(rho, dtype=L)) @ Ab
                assert np.abs(K - self.M).max() <= 64 * self.nsum * U * np.abs(K).max(), 'K0 is diagonal and M is not K'
        self.e64, self._cond = {}, None
        if not system:
            return
        self.e64['dinv0'] = _rel(self.f64.Dinv0, f.Dinv0)
        self.e64['S'] = _rel(self.f64.S, f.S)
        self.rescols = np.arange(self.order) if self.order <= FULL_RESIDUAL_MAX else self._residual_columns()
        self.e64['Sinv'] = self.residual(self.f64.Sinv)

    def _k0_is_diagonal(self):
        f = self.ld
        Pb = sp.coo_matrix(f.Pb)
        return bool((Pb.row == Pb.col).all() or (Pb.data[Pb.row != Pb.col] == 0).all()) and bool((np.diff(sp.csr_matrix(f.Ab).indptr)[self.s['short']] <= 1).all())

    def _residual_columns(self):
        o = self.order
        last = (o - 1) // 64 * 64
        rng = np.random.default_rng(o)
        return np.unique(np.concatenate([[0, 1, 63, 64, 65, last - 1, last, last + 1, o - 2, o - 1], rng.choice(o, RESIDUAL_COLS - 10, replace=False)]).astype(int))

    def residual(self, Sinv):
        """|| S_ref Sinv - I ||_max on the residual columns, the product in long double"""
        cols = self.rescols
        R = self.ld.S @ np.asarray(Sinv, dtype=L)[:, cols]
        R[cols, np.arange(len(cols))] -= 1
        return float(np.abs(R).max())

    def M_mul(self, x):
        y = self.ld.rhoL * np.add.reduceat(self.v * x[self.ci], self.rp)
        out = self.ld.D0 * x
        out[self.tcols] += np.add.reduceat(self.tv * y[self.tri], self.trp)
        return out

    def solve64(self, r):
        """M^-1 r in plain fp64 by the form's formulas, as in the apply tier (1 / D0, S or T by a matrix product, np.linalg.inv, the three products): the
        e64 of the iteration tier measures what fp64 loses on the route the kernels take.  (A Cholesky factorisation of K itself is backward stable
        in K and loses less where S is ill-conditioned -- r = 127 rows on n = 129 columns -- which no Woodbury evaluation in fp64 can match.)"""
        return self.f64.apply(np.asarray(r, dtype=np.float64))

    def cond(self):
        """cond_2(M): from the dense matrix, or from the largest eigenvalues of M and M^-1 as operators"""
        if self._cond is None:
            self._cond = self._cond2()
        return self._cond

    def _cond2(self):
        if self.n <= DENSE_M_MAX:
            return float(np.linalg.cond(np.asarray(self.M, dtype=np.float64)))
        import scipy.sparse.linalg as spl
        op = spl.LinearOperator((self.n, self.n), matvec=lambda v: np.asarray(self.M_mul(np.asarray(v, dtype=L).ravel()), dtype=np.float64), dtype=np.float64)
        inv = spl.LinearOperator((self.n, self.n), matvec=lambda v: self.f64.apply(np.asarray(v).ravel()), dtype=np.float64)
        hi = spl.eigsh(op, k=1, which='LA', tol=1e-3, return_eigenvectors=False)[0]
        lo = spl.eigsh(inv, k=1, which='LA', tol=1e-3, return_eigenvectors=False)[0]
        return float(hi * lo)

    def solve(self, r, strict=True):
        """(u_ref, u64): M^-1 r by refinement on M itself, and the plain fp64 evaluation of the form's formulas.  strict: the correction falls below 2^-60
        of the solution (the apply tier's rule); not strict (right-hand sides of the iteration tier, whose solutions are a small remainder of D0^-1 r: the
        long-double residual itself stops the corrections earlier): the correction has stopped shrinking (cond(M) 2^-64 of the solution is all a
        long-double residual allows) below 2^-50 of the solution -- still three orders under the smallest tolerance, 64 n 2^-53."""
        step = np.inf
        u64 = self.f64.apply(r)
        inner = (lambda v: scipy.linalg.cho_solve(self.chol, v)) if self.n <= DENSE_M_MAX else self.f64.apply
        rl = np.asarray(r, dtype=L)
        x = np.asarray(inner(np.asarray(r, dtype=np.float64)), dtype=L)
        for it in range(12):
            res = rl - self.M_mul(x)
            dx = np.asarray(inner(np.asarray(res, dtype=np.float64)), dtype=L)
            x = x + dx
            step, last = float(np.abs(dx).max()), (step if it else np.inf)
            if step <= 2.0 ** -60 * np.abs(x).max() or (not strict and step >= 0.25 * last and step <= 2.0 ** -50 * np.abs(x).max()):
                break
        else:
            raise AssertionError('the refinement of the reference solve did not converge')
        assert np.abs(rl - self.M_mul(x)).max() <= 2.0 ** -56 * (np.abs(rl).max() + np.abs(self.ld.D0).max() * np.abs(x).max()) * self.nsum, 'reference residual'
        return x, u64


def _rel(a, ref):
    return float(np.abs(np.asarray(a, dtype=L) - ref).max() / np.abs(ref).max())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def tolerance(e64, nsum, scale):
    return FACTOR * max(e64, nsum * U) * float(scale)


# ------------------------------------------------------------------------------------------------------------------------------ checks
class Worst(dict):
    """worst ratio to the tolerance per quantity; .e64: the largest e64 per quantity (the condition's margin)"""

    def __init__(self):
        super().__init__()
        self.e64 = {}

    def note(self, what, err, tol, where):
        ratio = float(err) / tol
        self[what] = max(self.get(what, 0.0), ratio)
        assert ratio <= 1.0, '%s: error %.3e against the tolerance %.3e (%s)' % (what, float(err), tol, where)


def _canvas(out, name, count, where):
    a = out[name]
    assert a.size == count + TAIL, (name, a.size, count)
    if name == 'idx':
        assert (a[count:] == -1).all(), 'idx: a cell behind the listed count was written (%s)' % where
        return a[:count]
    assert np.isnan(a[count:]).all(), '%s: a cell behind the listed count was written (%s)' % (name, where)
    assert np.isfinite(a[:count]).all(), '%s: a cell of the listed count was not written, or is not finite (%s)' % (name, where)
    return a[:count]


def check_state(h, c, worst, label, parities=(0, 1), directs=(0, 1), nrhs=4):
    """All calls of one state of the handle (its current matrices and rho): the first with refactor = 1, then every right-hand side with refactor = 0,
    parity and direct alternating so that all four combinations occur.  Returns (reference, u of the first right-hand side, rho vector)."""
    p = problem(c)
    n, m = p['n'], p['m']
    rhs = right_hand_sides(c)[:nrhs]
    rng = np.random.default_rng(c['seed'] + 3)
    ref, first = None, None
    combos = [pd for pd in ((0, 0), (1, 1), (1, 0), (0, 1)) if pd[0] in parities and pd[1] in directs]      # (two right-hand sides see both values of both)
    for k, r in enumerate(rhs):
        par, direct = combos[k % len(combos)]
        x0 = rng.standard_normal(n) if direct else None
        where = '%s, %s, rhs %d, parity %d, direct %d' % (case_id(c), label, k, par, direct)
        st, out = h.test(r, x0, refactor=int(k == 0), parity=par, direct=direct)
        assert st == 0, (st, where)
        rho = _canvas(out, 'rho', m, where)
        if ref is None:
            ref = Reference(p['P'], h.A, h.sigma, rho, h.scaling(), c['form'])
            for k_, v in ref.e64.items():
                worst.e64[k_] = max(worst.e64.get(k_, 0.0), v)
                assert v <= E64_MAX, 'condition e64 <= %.0e missed by %s: %.3e (%s)' % (E64_MAX, k_, v, where)
            assert ref.k0diag == c['k0diag']
        assert out['form'] == {'small': 0, 'row': 1, 'col': 2}[c['form']] and out['order'] == ref.order and out['rows'] == len(ref.s['long']), (out['form'], out['order'], out['rows'], where)
        idx = _canvas(out, 'idx', ref.order, where)
        assert np.array_equal(np.sort(idx), ref.s['idx']), 'idx is not the list of long rows / dense columns (%s)' % where
        # the reference lists rows / columns ascending: bring S, Sinv into that order
        o = np.argsort(idx)
        S = _canvas(out, 'S', ref.order ** 2, where).reshape(ref.order, ref.order)[np.ix_(o, o)]
        Sinv = _canvas(out, 'Sinv', ref.order ** 2, where).reshape(ref.order, ref.order)[np.ix_(o, o)]
        dinv0 = _canvas(out, 'dinv0', n, where)
        u = _canvas(out, 'u', n, where)
        f = ref.ld
        worst.note('Dinv0', np.abs(dinv0 - f.Dinv0).max(), tolerance(ref.e64['dinv0'], ref.nsum, np.abs(f.Dinv0).max()), where)
        worst.note('T' if c['form'] == 'col' else 'S', np.abs(S - f.S).max(), tolerance(ref.e64['S'], ref.nsum, np.abs(f.S).max()), where)
        worst.note('Sinv', ref.residual(Sinv), tolerance(ref.e64['Sinv'], ref.nsum, 1.0), where)
        u_ref, u64 = ref.solve(r)
        e64 = _rel(u64, u_ref)
        worst.e64['u'] = max(worst.e64.get('u', 0.0), e64)
        assert e64 <= E64_MAX, 'condition e64 <= %.0e missed by u: %.3e (%s)' % (E64_MAX, e64, where)
        worst.note('u', np.abs(u - u_ref).max(), tolerance(e64, ref.nsum, np.abs(u_ref).max()), where)
        rl = np.asarray(r, dtype=L)
        g_ref = rl @ u_ref
        e64g = float(abs(L(np.asarray(r) @ u64) - g_ref) / abs(g_ref))
        worst.note('gamma', abs(L(out['gamma']) - g_ref), tolerance(e64g, ref.nsum, abs(g_ref)), where)
        assert out['rnorm'] == np.abs(r).max(), (out['rnorm'], np.abs(r).max(), where)
        if direct:
            xs = _canvas(out, 'xs', n, where)
            xs_ref = np.asarray(x0, dtype=L) + u_ref
            worst.note('xs', np.abs(xs - xs_ref).max(), tolerance(_rel(x0 + u64, xs_ref), ref.nsum, np.abs(xs_ref).max()), where)
            assert out['done'] == 1 and out['iters'] == 1, (out['done'], out['iters'], where)
        else:
            _canvas(out, 'xs', n, where)
            assert out['done'] == 0, (out['done'], where)
        if c['k0diag']:
            assert out['exact'] == 1, 'K0 is diagonal: the direct mode must be on (%s)' % where
        else:
            assert out['exact'] == 0, 'K0 is not diagonal: M is not K, the direct mode must be off (%s)' % where
        if c['form'] == 'small':
            assert out['info'][0] == 1, (out['info'], where)
        if first is None:
            first = (u.copy(), S.copy(), dinv0.copy(), rho.copy())
    return ref, first


def check_apply(h, c, worst=None, nrhs=4, updates=True):
    """One case on one handle: the handle as set up, then after update_settings(rho) and after update(Ax) -- each against the reference of the new data
    and different from the state before."""
    worst = Worst() if worst is None else worst
    _, before = check_state(h, c, worst, 'as set up', nrhs=nrhs)
    if not updates:
        return worst
    h.set_rho(0.37)
    _, after = check_state(h, c, worst, 'after rho = 0.37', nrhs=2)
    assert not np.array_equal(before[3], after[3]) and np.abs(after[0] - before[0]).max() > 1e-4 * np.abs(before[0]).max(), 'the rho update changed nothing'
    before = after
    rng = np.random.default_rng(c['seed'] + 5)
    Ax = h.A.data * (1 + 0.05 * rng.standard_normal(h.A.nnz))
    h.set_Ax(Ax)
    _, after = check_state(h, c, worst, 'after new A values', nrhs=2)
    assert np.array_equal(before[3], after[3]), 'new matrix values changed the rho vector'
    assert np.abs(after[0] - before[0]).max() > 1e-4 * np.abs(before[0]).max() and np.abs(after[1] - before[1]).max() > 1e-4 * np.abs(before[1]).max(), 'the matrix update changed nothing'
    return worst


def check_repeatable(h, c):
    """Two calls with the same arguments return the same bits."""
    r = right_hand_sides(c)[0]
    x0 = np.cos(np.arange(len(r)))
    a, b = h.test(r, x0, refactor=1, parity=1, direct=1), h.test(r, x0, refactor=1, parity=1, direct=1)
    assert a[0] == 0 and b[0] == 0
    for k in ('u', 'xs', 'dinv0', 'S', 'Sinv', 'rho'):
        assert np.array_equal(bits(a[1][k]), bits(b[1][k])), '%s differs between two calls' % k
    assert all(a[1][k] == b[1][k] for k in ('gamma', 'rnorm', 'done', 'iters', 'exact', 'info'))


def check_rejections(h, c):
    """Every length and flag the entry lists, one at a time off by one or out of range: OSQP_DATA_VALIDATION_ERROR, nothing written."""
    n = problem(c)['n']
    r = np.ones(n)
    for kw in (dict(parity=2), dict(parity=-1), dict(direct=2), dict(direct=1), dict(x0=np.ones(n)), dict(direct=1, x0=np.ones(n - 1)), dict(r=np.ones(n + 1)), dict(r=np.ones(n - 1))):
        kw = dict(kw)
        st, out = h.test(kw.pop('r', r), kw.pop('x0', None), **kw)
        assert st == VALIDATION, (st, kw)
        if out is not None:
            assert all(np.isnan(out[k]).all() for k in ('u', 'xs', 'dinv0', 'S', 'Sinv', 'rho')) and (out['idx'] == -1).all()
    for name in ('u_len', 'xs_len', 'dinv0_len', 's_len', 'sinv_len', 'rho_len', 'idx_len'):
        for delta in (-1, 1, -TAIL):
            st, out = h.test(r, None, lens={name: _listed(h, c, name) + delta})
            assert st == VALIDATION, (st, name, delta)


def _listed(h, c, name):
    p = problem(c)
    o = structure(h.A, c['form'])['order']
    return {'u_len': p['n'], 'xs_len': p['n'], 'dinv0_len': p['n'], 's_len': o * o, 'sinv_len': o * o, 'rho_len': p['m'], 'idx_len': o}[name] + TAIL


# ------------------------------------------------------------------------------------------------------------------------------ iteration tier
ITER_R = [1, 2, 63, 65, 127, 128]
ITER_N = [129, 191, 192, 193]
ITER_PAIRS = [(1, 129), (2, 191), (63, 192), (65, 193), (127, 129), (128, 193), (2, 192), (128, 191)]
# name -> (environment at setup, what hip_stats() must say after a solve)
SMALL_FORMS = {
    'unfused': ({'OSQP_HIP_WOODBURY_FUSED': '0'}, dict(woodbury_direct=1)),
    'two-launch': ({'OSQP_HIP_WOODBURY_FUSED': '2'}, dict(woodbury_direct=2, woodbury_one_launch=0)),
    'one-launch': ({'OSQP_HIP_WOODBURY_FUSED': '1'}, dict(woodbury_direct=2, woodbury_one_launch=1)),
    'slots': ({'OSQP_HIP_WOODBURY_FUSED': '2', 'OSQP_HIP_DEVICE_DRIVEN': '2'}, dict(woodbury_direct=2, woodbury_one_launch=0)),
}


def iter_cases():
    # (eq_scale: the entries of equality rows, whose rho is 1000 times the others' up to n = 256, are 0.03 of the others' -- rho a^2 of one order in all
    #  rows keeps cond(K) near 1e3 and the fp64 run of the iteration, e64, within its condition)
    out = [dict(form='small', r=r, n=n, k0diag=True, seed=600 + k, scaling=0, eq_scale=0.03, long_scale=min(1.0, 4.0 / np.sqrt(r))) for k, (r, n) in enumerate(ITER_PAIRS)]      # (long_scale: as in row_cases -- with r near n the fp64 Woodbury route loses its digits in S)
    out.append(dict(form='small', r=7, n=257, k0diag=True, seed=660, scaling=10, long_scale=0.1))      # scaling on (equilibration would undo eq_scale: n above 256, where equality rows weigh 10 x; rows of one norm: E stays within a factor of six, which y = E y~ / c carries into e64)
    out.append(dict(form='small', r=3, n=5185, k0diag=True, seed=650, scaling=0, long_scale=0.1))      # (entries of 0.1: rho sigma_max^2 / D0 of order ten, as in row_cases)          # 82 workgroups of 64 columns: the partials fold in two batches
    return out


def large_iter_cases():
    """(name, case, environment, expected hip_stats): the device-factorised forms' direct modes"""
    row = dict(form='row', r=130, n=141, k0diag=True, seed=700, scaling=0, long_scale=4.0 / np.sqrt(130), eq_scale=0.03)
    col = dict(form='col', cd=130, r=176, singles=1, k0diag=True, seed=701, scaling=0, rowlen=None)
    col2 = dict(form='col', cd=131, r=180, singles=2, k0diag=True, seed=702, scaling=0, rowlen=None)
    blk = dict(form='col', cd=512, r=700, singles=1, k0diag=True, seed=703, scaling=0, rowlen=None)
    return [('row-space', row, {'OSQP_HIP_WOODBURY_DUAL': '0'}, dict(woodbury_direct=1, woodbury_dual_cols=0)),
            ('column-space-unfused', col, {'OSQP_HIP_WOODBURY_FUSED': '0'}, dict(woodbury_direct=1, woodbury_dual_cols=130, woodbury_fused_iteration=0)),
            ('column-space-fused-csr', col2, {'OSQP_HIP_WOODBURY_FUSED': '2'}, dict(woodbury_direct=1, woodbury_dual_cols=131, woodbury_fused_iteration=1)),
            ('column-space-thin', col, {'OSQP_HIP_WOODBURY_FUSED': '1'}, dict(woodbury_direct=1, woodbury_dual_cols=130, woodbury_fused_iteration=1)),
            ('dense-block', blk, {'OSQP_HIP_WOODBURY_FUSED': '1'}, dict(woodbury_direct=1, woodbury_dual_cols=512, woodbury_fused_iteration=(2, 3)))]


class Rows:
    """A sparse matrix in the number type T: products with it and with its transpose by row sums (np.add.reduceat over the non-empty rows)."""

    def __init__(self, M, T):
        self.T, self.shape = T, M.shape
        self.parts = []
        for X in (sp.csr_matrix(M), sp.csr_matrix(sp.csr_matrix(M).T)):
            X.sort_indices()
            ne = np.diff(X.indptr) > 0
            self.parts.append((np.flatnonzero(ne), X.indptr[:-1][ne], X.indices, np.asarray(X.data, dtype=T), X.shape[0]))

    def _mul(self, k, x):
        rows, ptr, ci, v, cnt = self.parts[k]
        out = np.zeros(cnt, dtype=self.T)
        out[rows] = np.add.reduceat(v * x[ci], ptr)
        return out

    def mul(self, x):
        return self._mul(0, x)

    def tmul(self, y):
        return self._mul(1, y)


def admm_reference(c, A, rho, sigma, alpha, scal, k, x0, y0, T, plant=None):
    """k iterations of the textbook ADMM iteration (_osqp.py:644-703; exact solve with K) on the scaled problem in the number type T; returns (x, y) unscaled
    and the facts the conditions are about.  rho: the rho vector of the scaled problem.  The solve with K is the solve with M of the apply tier (K0 is
    diagonal in every case of this tier: Reference asserts M = K): refined on K's definition in long double, plain fp64 for T = np.float64.
    plant = 'wrong_bound': the first row that clamps low is set to its upper bound."""
    p = problem(c)
    ref = _k_reference(tuple(sorted(c.items())), A.data.tobytes(), np.asarray(rho, dtype=np.float64).tobytes(), sigma, tuple(np.asarray(v, dtype=np.float64).tobytes() for v in scal[:2]), float(scal[2]))
    assert ref.k0diag
    D, E, cc = np.asarray(scal[0], dtype=T), np.asarray(scal[1], dtype=T), T(scal[2])
    Ab = Rows(ref.ld.Ab, T)
    qb, lb, ub = cc * D * np.asarray(p['q'], dtype=T), E * np.asarray(p['l'], dtype=T), E * np.asarray(p['u'], dtype=T)
    rho = np.asarray(rho, dtype=T)
    solve = (lambda b: ref.solve(b, strict=False)[0]) if T is L else ref.solve64
    x = np.asarray(x0, dtype=T) / D
    y = cc * np.asarray(y0, dtype=T) / E
    z = Ab.mul(x)
    facts = []
    alpha = T(alpha)
    rng_ = ub > lb
    for it in range(k):
        xt = solve(T(sigma) * x - qb + Ab.tmul(rho * z - y))
        zt = Ab.mul(xt)
        x = alpha * xt + (1 - alpha) * x
        zr = alpha * zt + (1 - alpha) * z
        pre = zr + y / rho
        znew = np.minimum(np.maximum(pre, lb), ub)
        lo, hi = pre < lb, pre > ub
        if plant == 'wrong_bound' and (lo & rng_).any():
            i = np.flatnonzero(lo & rng_)[0]
            znew[i] = ub[i]
        facts.append(dict(low=int((lo & rng_).sum()), high=int((hi & rng_).sum()), free=int((~lo & ~hi & rng_).sum()),
                          margin=float(np.minimum(np.abs(pre - lb), np.abs(pre - ub))[rng_].min())))
        y = y + rho * (zr - znew)
        z = znew
    return D * x, E * y / cc, dict(cond=ref.cond(), iterations=facts)


@functools.lru_cache(maxsize=4)
def _k_reference(key_c, Ax, rho, sigma, DE, cc):
    c = dict(key_c)
    p = problem(c)
    A = sp.csc_matrix((np.frombuffer(Ax), p['A'].indices, p['A'].indptr), shape=p['A'].shape)
    return Reference(p['P'], A, sigma, np.frombuffer(rho), (np.frombuffer(DE[0]), np.frombuffer(DE[1]), cc), c['form'], system=False)


def iteration_starts(c):
    p = problem(c)
    rng = np.random.default_rng(c['seed'] + 11)
    return [('cold', np.zeros(p['n']), np.zeros(p['m'])), ('warm', 0.5 * rng.standard_normal(p['n']), 0.3 * rng.standard_normal(p['m']))]


def check_iterations(run, c, A, rho, scal, sigma, alpha, worst, label, ks=(1, 2, 3)):
    """run(k, x0, y0) -> (x, y) after exactly k iterations from (x0, y0).  A: the handle's current matrix (the caller's numbering and scale)."""
    p = problem(c)
    for name, x0, y0 in iteration_starts(c):
        for k in ks:
            where = '%s, %s, %s start, %d iterations' % (case_id(c), label, name, k)
            xr, yr, facts = admm_reference(c, A, rho, sigma, alpha, scal, k, x0, y0, L)
            x64, y64, _ = admm_reference(c, A, rho, sigma, alpha, scal, k, x0, y0, np.float64)
            assert facts['cond'] <= 1e7, (facts['cond'], where)
            for f in facts['iterations']:
                assert f['low'] > 0 and f['high'] > 0 and f['free'] > 0, (f, where)
                assert f['margin'] >= 1e-6, (f, where)
            ex, ey = _rel(x64, xr), _rel(y64, yr)
            worst.e64['x'] = max(worst.e64.get('x', 0.0), ex); worst.e64['y'] = max(worst.e64.get('y', 0.0), ey)
            assert ex <= E64_MAX and ey <= E64_MAX, (ex, ey, where)
            x, y = run(k, x0, y0)
            nsum = max(p['n'], p['m'])
            worst.note('x', np.abs(x - xr).max(), tolerance(ex, nsum, np.abs(xr).max()), where)
            worst.note('y', np.abs(y - yr).max(), tolerance(ey, nsum, np.abs(yr).max()), where)
    return worst


class ProductIterations:
    """run(k, x0, y0) on a handle of the product: max_iter = k, warm_start(x0, y0) (zeros: the cold start), solve.  The form is chosen by the environment at
    setup and confirmed by hip_stats() after every solve; the rho vector comes through the diagnostic entry."""

    def __init__(self, c, environment, expect, alpha=1.6):
        self.h = Product(c, environment, alpha=alpha, max_iter=1, warm_starting=True)
        self.c, self.expect, self.alpha = c, expect, alpha

    def rho(self):
        st, out = self.h.test(np.zeros(problem(self.c)['n']), None, refactor=0)
        assert st == 0, st
        return out['rho'][:problem(self.c)['m']].copy()

    def __call__(self, k, x0, y0):
        m = self.h.model
        m.update_settings(max_iter=k)
        m.warm_start(x=x0, y=y0)
        r = m.solve()
        assert r.info.iter == k, (r.info.iter, k)
        s = self.h.solver.hip_stats()
        for key, want in self.expect.items():
            assert (int(s[key]) in want) if isinstance(want, tuple) else (int(s[key]) == want), (key, s[key], want)
        return np.array(r.x), np.array(r.y)


def check_iteration_form(run, c, worst, name):
    """The k = 1, 2, 3 runs of one form from both starts, then again after update_settings(rho = 0.37): the refactorisation and what hangs on S^-1."""
    h = run.h
    check_iterations(run, c, h.A, run.rho(), h.scaling(), h.sigma, run.alpha, worst, name)
    before = run.rho()
    h.set_rho(0.37)
    assert not np.array_equal(before, run.rho())
    check_iterations(run, c, h.A, run.rho(), h.scaling(), h.sigma, run.alpha, worst, name + ', rho = 0.37')
    return worst
