"""References, cases, bounds and checks for the kernel-level tests of the banded LDL' factor and substitutions (osqp-python_amd/csrc/band_ldl.h) -- numpy
only, no GPU.  Both tiers use this one module: tests/test_gpu_band_kernels.py runs the checks on the kernels through the diagnostic entry
osqp_hip_test_band (one workgroup: band_clear, scatter, band_factor, band_solve per right-hand side), tests/test_band_ref.py runs them on the host
simulator's textbook loops and shows that results which are subtly wrong miss them.

Layout (band_ldl.h): entry (r, c), c <= r <= c + bw, at image[FRONT + c W + (r - c)], W = bw + 8; 8 zeros in front, every column ends in 8 zeros, the
columns are n rounded up to a multiple of 8, 64 doubles of slack behind.  After the factorisation the slots hold the unit-lower L^ (strictly lower
part, diagonal slots zero) and dinv = 1 / D.

Cases (lower triangle only: symmetric by construction; the entries of the input band with c + k >= n hold NaN -- they must never be read)
  dd       a full band of uniform [-1, 1] entries under a diagonal that dominates its row by 1 .. 2
  kkt      sigma I + P_diag + A' diag(rho) A, sigma = 1e-6, every row of A with up to three entries inside a window of bw + 1 columns (every other row with
           an entry at both ends of its window, so that the outermost diagonal of the band is populated), rho = 1e-1 on
           about 70 % of the rows and 1e2 on the others, P_diag zero on half of the columns and fewer rows than columns: what the product factors,
           condition number 1e8 .. 1e9
  narrow   a tridiagonal matrix declared with bw = 56: the outer diagonals are stored zeros
  guard    (GUARD checks) offdiagonal entries uniform in [-1, 1] / (4 (bw + 1)), diagonal in [0.75, 1]: by Gershgorin every eigenvalue, hence every
           pivot of an elimination without pivoting, lies in (0.25, 1]

Bounds, u = 2^-53, gamma_k = k u / (1 - k u), references in np.longdouble -- derived, none of them measured on the code under test
  factor   |K - L^ D^ L^'| <= gamma_{bw+16} |L^| D^ |L^'| componentwise on the band, D^ = 1 / dinv: at most bw products per entry plus the fixed
           roundings of 1 / sqrt, the two rescalings by di and di^2 and the reconstruction (16 worst case)
  solve    |b - L^ D^ L^' x^| <= gamma_{2bw+4} (|L^| D^ |L^'|) |x^| componentwise, b and x^ in band order, on the call's OWN factor: two unit-triangular
           solves of at most bw terms each, one scaling, two of slack.  With the factor bound this ties x^ to K without a condition number.
  GUARD    the factor bound against K + delta e_c* e_c*', delta from an np.longdouble run of the same pivot rule.  The long-double pivot differs from
           the kernel's by the FORWARD error of row c* of the factor; on the guard class (condition number < 6) that is a few u of the row's
           magnitude, inside the 16 u the bound leaves.  The reference asserts that every pivot it meets is 0.25 away from 0 and, where the rule
           fires, from pivot_floor: kernel and reference cannot decide differently.
"""
import functools

import numpy as np

L = np.longdouble
U = L(2.0) ** -53
NB, FRONT, SLACK, MAX_BW = 8, 8, 64, 56
SENTINEL = -3.5e77                     # (finite, no value of the test data comes near)
SIGMA = 1e-6
STATUS_INVALID = 1                     # OSQP_DATA_VALIDATION_ERROR

SIZES = [1, 2, 8, 9, 57, 63, 64, 65, 72, 73, 120, 121, 127, 128, 129, 136, 137, 185, 191, 192, 193, 200, 240]
BWS = [0, 1, 7, 8, 9, 31, 55, 56]
INSTANTIATIONS = [(64, 0), (256, 0), (256, 1)]          # (threads, guard): the three forms the product runs
GUARD_KINDS = ['magnitude', 'floor', 'nan']


def gamma(k):
    return L(k) * U / (1 - L(k) * U)


def band_stride(bw):
    return bw + NB


def band_cols(n):
    return (n + NB - 1) // NB * NB


def band_slot(bw, c, r):
    return c * band_stride(bw) + (r - c)


def band_doubles(n, bw):
    return FRONT + band_cols(n) * band_stride(bw) + SLACK


def bws_for(n):
    return [b for b in BWS if b <= n - 1]


def classes_for(n, bw):
    return ['dd', 'kkt'] + (['narrow'] if bw == MAX_BW else [])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------------------------ cases
def to_band(K, bw):
    """(n, bw + 1) input band of the dense lower triangle: band[c, k] = K[c + k, c]; NaN where c + k >= n."""
    n = K.shape[0]
    band = np.full((n, bw + 1), np.nan)
    for k in range(bw + 1):
        band[:n - k, k] = np.diagonal(K, -k)
    return band


def diagonals(band):
    """Kd[k, c] = K[c + k][c] in np.longdouble, zero where c + k >= n."""
    return np.where(np.isnan(band), 0.0, band).T.astype(L)


def dense_matrix(cls, n, bw, seed=0):
    rng = np.random.default_rng([{'dd': 1, 'kkt': 2, 'narrow': 3, 'guard': 4}[cls], n, bw, seed])
    i, j = np.indices((n, n))
    inband = (i > j) & (i - j <= bw)
    if cls == 'dd':
        K = np.where(inband, rng.uniform(-1, 1, (n, n)), 0.0)
        K = K + K.T
        return K + np.diag(np.abs(K).sum(axis=1) + rng.uniform(1, 2, n))
    if cls == 'guard':
        K = np.where(inband, rng.uniform(-1, 1, (n, n)) / (4 * (bw + 1)), 0.0)
        K = K + K.T
        return K + np.diag(rng.uniform(0.75, 1.0, n))
    if cls == 'narrow':
        off = rng.uniform(-1, 1, n - 1)
        K = np.diag(off, -1) + np.diag(off, 1)
        return K + np.diag(np.abs(K).sum(axis=1) + rng.uniform(0.5, 1.5, n))
    m = max(1, n // 2)
    A = np.zeros((m, n))
    for r in range(m):
        s = int(rng.integers(0, n - bw)) if r else n - bw - 1           # (row 0: the window that ends in the last column)
        win = np.arange(s, s + bw + 1)
        cols = rng.choice(win, size=min(3, win.size), replace=False)
        if r % 2 == 0 and win.size >= 2:                               # (every other row spans its whole window: the outermost diagonal is populated)
            cols = np.unique(np.r_[win[0], win[-1], cols[0]])
        A[r, cols] = rng.standard_normal(cols.size)
    rho = np.where(rng.uniform(size=m) < 0.7, 1e-1, 1e2)
    pdiag = np.where(rng.uniform(size=n) < 0.5, 0.0, rng.uniform(0.1, 1.0, n))
    K = A.T @ (rho[:, None] * A) + np.diag(pdiag + SIGMA)
    return np.tril(K) + np.tril(K, -1).T


@functools.lru_cache(maxsize=None)
def case(cls, n, bw):
    """One (class, n, bw): the input band, its long-double diagonals, both permutations and the right-hand sides.  Computed once, never changed."""
    K = dense_matrix(cls, n, bw)
    band = to_band(K, bw)
    rng = np.random.default_rng([99, n, bw])
    units = sorted({j for j in (0, 63, 64, 127, 128, 191, 192, n - 1) if 0 <= j < n})
    rhs = np.vstack([rng.standard_normal(n), np.ones(n)] + [np.eye(n)[j] for j in units])
    c = dict(cls=cls, n=n, bw=bw, band=band, Kd=diagonals(band), perms=(np.arange(n, dtype=np.int32), rng.permutation(n).astype(np.int32)), rhs=rhs)
    for v in (band, c['Kd'], rhs) + c['perms']:
        v.setflags(write=False)
    return c


# ------------------------------------------------------------------------------------------------------------------------------ the call
class Out:
    def __init__(self, x, image, dinv, bad, n, bw, nrhs):
        self.x, self.image, self.dinv, self.bad, self.n, self.bw, self.nrhs = x, image, dinv, bad, n, bw, nrhs

    def copy(self):
        return Out(self.x.copy(), self.image.copy(), self.dinv.copy(), self.bad, self.n, self.bw, self.nrhs)

    def solutions(self):
        return self.x[:self.nrhs * self.n].reshape(self.nrhs, self.n)


def call(solver, n, bw, band, perm, rhs, threads=256, guard=0, pivot_floor=0.0):
    rhs = np.asarray(rhs, dtype=np.float64).reshape(-1, n)
    st, x, image, dinv, bad = solver.hip_test_band(n, bw, band, perm, rhs, np.full(rhs.shape[0] * n + 16, SENTINEL), threads=threads, guard=guard, pivot_floor=pivot_floor)
    assert st == 0, st
    return Out(x, image, dinv, bad, n, bw, rhs.shape[0])


# ------------------------------------------------------------------------------------------------------------------------------ checks
def slot_mask(n, bw):
    mask = np.zeros(band_doubles(n, bw), dtype=bool)
    for c in range(n):
        kmax = min(bw, n - 1 - c)
        mask[FRONT + band_slot(bw, c, c) + 1:FRONT + band_slot(bw, c, c) + 1 + kmax] = True
    return mask


def check_padding(out):
    """(a): everything of the image outside the strictly lower slots is zero, the sentinels behind x are untouched, every x cell is written."""
    n, bw = out.n, out.bw
    assert out.image.size == band_doubles(n, bw)
    pad = out.image[~slot_mask(n, bw)]
    assert (pad == 0.0).all(), '%d cells of the image outside the factor are not zero (first at %d)' % (int((pad != 0.0).sum()), int(np.flatnonzero(~slot_mask(n, bw))[np.flatnonzero(pad != 0.0)[0]]))
    want = bits(np.full(1, SENTINEL))[0]
    assert (bits(out.x[out.nrhs * n:]) == want).all(), 'a sentinel behind x changed'
    assert out.x.size == out.nrhs * n + 16
    assert (bits(out.x[:out.nrhs * n]) != want).all(), 'an x cell was not written'


def factor_of(out):
    """(Ld, d): Ld[k, c] = L^[c + k][c] with the unit diagonal in Ld[0], zero where c + k >= n; d = 1 / dinv -- both np.longdouble."""
    n, bw = out.n, out.bw
    Ld = np.zeros((bw + 1, n), dtype=L)
    Ld[0] = 1
    cols = out.image[FRONT:FRONT + n * band_stride(bw)].reshape(n, band_stride(bw))
    for k in range(1, bw + 1):
        Ld[k, :n - k] = cols[:n - k, k]
    return Ld, 1 / out.dinv.astype(L)


def ldl_band(Ld, d):
    """R[k, c] = (L D L')[c + k][c] = sum_t L[c + k][c - t] d[c - t] L[c][c - t] on the band."""
    bw, n = Ld.shape[0] - 1, Ld.shape[1]
    R = np.zeros((bw + 1, n), dtype=L)
    for k in range(bw + 1):
        for t in range(bw - k + 1):
            w = n - k - t
            if w > 0:
                R[k, t:n - k] += Ld[k + t, :w] * d[:w] * Ld[t, :w]
    return R


def ldl_apply(Ld, d, X):
    """L D L' X for X [nrhs, n] in band order."""
    bw, n = Ld.shape[0] - 1, Ld.shape[1]
    Y = np.zeros(X.shape, dtype=L)
    for k in range(bw + 1):
        Y[:, :n - k] += Ld[k, :n - k] * X[:, k:]
    Y *= d
    Z = np.zeros(X.shape, dtype=L)
    for k in range(bw + 1):
        Z[:, k:] += Ld[k, :n - k] * Y[:, :n - k]
    return Z


def worst_ratio(err, bound, valid, what):
    ratio = np.where(valid, err / np.where(bound > 0, bound, 1), 0)
    assert not (valid & (bound <= 0) & (err > 0)).any(), what + ' bound missed: an error where the bound is zero'
    w = float(ratio.max()) if ratio.size else 0.0
    assert w <= 1.0, '%s bound missed at %s: error %.3e = %.3g x the bound' % (what, np.unravel_index(int(ratio.argmax()), ratio.shape), float(err.flat[int(ratio.argmax())]), w)
    return w


def check_factor(out, Kd, bad=0):
    """(b): returns the worst ratio to the bound."""
    n, bw = out.n, out.bw
    assert out.bad == bad, out.bad
    assert np.isfinite(out.dinv).all() and (out.dinv > 0).all(), 'dinv not finite and positive'
    assert np.isfinite(out.image).all()
    Ld, d = factor_of(out)
    valid = np.arange(bw + 1)[:, None] + np.arange(n)[None, :] < n
    return worst_ratio(np.abs(Kd - ldl_band(Ld, d)), gamma(bw + 16) * ldl_band(np.abs(Ld), d), valid, 'factor')


def check_solve(out, perm, rhs):
    """(c): on the call's own factor; returns the worst ratio to the bound."""
    n, bw = out.n, out.bw
    rhs = np.asarray(rhs, dtype=np.float64).reshape(-1, n)
    X = out.solutions()
    assert np.isfinite(X).all(), 'x not finite'
    Ld, d = factor_of(out)
    Xb, Bb = X[:, perm].astype(L), rhs[:, perm].astype(L)
    return worst_ratio(np.abs(Bb - ldl_apply(Ld, d, Xb)), gamma(2 * bw + 4) * ldl_apply(np.abs(Ld), d, np.abs(Xb)), np.ones(Xb.shape, dtype=bool), 'solve')


def same_bits(a, b, what):
    assert np.array_equal(bits(a), bits(b)), '%s: %d doubles differ (first at %d)' % (what, int((bits(a) != bits(b)).sum()), int(np.flatnonzero(bits(a) != bits(b))[0]))


def check_case(solver, cls, n, bw, instantiations=INSTANTIATIONS):
    """(a), (b), (c) and (e) of one (class, n, bw) on every instantiation, both permutations and every right-hand side.  Returns
    {(threads, guard): (worst factor ratio, worst solve ratio)}."""
    c = case(cls, n, bw)
    rhs, worst, runs = c['rhs'], {}, {}
    chunks = [rhs[i:i + 8] for i in range(0, rhs.shape[0], 8)]
    for threads, guard in instantiations:
        wf = ws = 0.0
        first = None
        for pi, perm in enumerate(c['perms']):
            for ci, chunk in enumerate(chunks):
                out = call(solver, n, bw, c['band'], perm, chunk, threads, guard, pivot_floor=SIGMA)
                check_padding(out)
                if first is None:
                    first = out
                    wf = check_factor(out, c['Kd'])
                else:                                                  # (the factor depends on nothing but the matrix)
                    assert out.bad == 0
                    same_bits(out.image, first.image, 'image of a later call')
                    same_bits(out.dinv, first.dinv, 'dinv of a later call')
                ws = max(ws, check_solve(out, perm, chunk))
                runs[threads, guard, pi, ci] = out
        worst[threads, guard] = (wf, ws)
        # (e) the same call twice; one right-hand side alone against the same one as the last of eight
        perm = c['perms'][1]
        again = call(solver, n, bw, c['band'], perm, chunks[-1], threads, guard, pivot_floor=SIGMA)
        last = runs[threads, guard, 1, len(chunks) - 1]
        for f in ('x', 'image', 'dinv'):
            same_bits(getattr(again, f), getattr(last, f), '%s of the same call twice' % f)
        eight = np.vstack([rhs[(1 + i) % rhs.shape[0]] for i in range(7)] + [rhs[0]])
        alone, among = call(solver, n, bw, c['band'], perm, rhs[:1], threads, guard, pivot_floor=SIGMA), call(solver, n, bw, c['band'], perm, eight, threads, guard, pivot_floor=SIGMA)
        same_bits(alone.solutions()[0], among.solutions()[7], 'a right-hand side alone against the last of eight')
    if (64, 0) in instantiations and (256, 0) in instantiations:       # (e) the workgroup size changes no bit
        for pi in range(2):
            for ci in range(len(chunks)):
                for f in ('x', 'image', 'dinv'):
                    same_bits(getattr(runs[64, 0, pi, ci], f), getattr(runs[256, 0, pi, ci], f), '%s, 64 against 256 threads' % f)
    return worst


# ------------------------------------------------------------------------------------------------------------------------------ GUARD
def guard_rule(pv, floor):
    """band_factor's GUARD rule: (pivot used, replaced?)."""
    if not (pv > 0) or pv > 1e300:
        a = abs(pv)
        return (a if (a > floor and a <= 1e300) else L(1)), True
    return pv, False


def guard_reference(band, bw, floor):
    """K = L D L' by rows in np.longdouble with the GUARD rule.  Returns (pivots as met, the diagonal of K + delta e e' the run factored, bad)."""
    n = band.shape[0]
    K = np.asarray(band, dtype=L)                                       # [c, k] = K[c + k][c]; NaN only where it is never read -- or on the diagonal (the nan kind)
    Lm, D, met, diag, bad = np.zeros((n, n), dtype=L), np.zeros(n, dtype=L), np.zeros(n, dtype=L), np.zeros(n, dtype=L), 0
    for c in range(n):
        lo = max(0, c - bw)
        acc = (Lm[c, lo:c] ** 2 * D[lo:c]).sum()
        pv = K[c, 0] - acc
        met[c] = pv
        assert np.isnan(pv) or abs(pv) >= 0.25, 'the reference meets a pivot within 0.25 of zero: %r' % float(pv)
        D[c], hit = guard_rule(pv, floor)
        if hit:
            bad = 1
            assert np.isnan(pv) or abs(abs(pv) - floor) >= 0.25, 'the reference meets a pivot within 0.25 of pivot_floor: %r' % float(pv)
        diag[c] = D[c] + acc
        for r in range(c + 1, min(n - 1, c + bw) + 1):
            lr = max(0, r - bw)
            Lm[r, c] = (K[c, r - c] - (Lm[r, lr:c] * Lm[c, lr:c] * D[lr:c]).sum()) / D[c]
    return met, diag, bad


@functools.lru_cache(maxsize=None)
def guard_case(n, bw, cstar, kind):
    """The guard class with K[c*][c*] lowered so that the pivot met there is <= -0.5 (pivot_floor 0.5: replaced by its magnitude), -0.5 under
    pivot_floor 1 (replaced by 1) or NaN (replaced by 1).  Returns (band, pivot_floor, Kd of the matrix the rule makes of it)."""
    band = to_band(dense_matrix('guard', n, bw), bw)
    met, _, bad = guard_reference(band, bw, 0.0)
    assert bad == 0 and (met > 0.25).all() and (met <= 1.0).all()
    p = float(met[cstar])
    floor = 0.5 if kind == 'magnitude' else 1.0
    band[cstar, 0] = np.nan if kind == 'nan' else band[cstar, 0] - (2 * p + 1 if kind == 'magnitude' else p + 0.5)
    met, diag, bad = guard_reference(band, bw, floor)
    assert bad == 1
    if kind == 'magnitude':
        assert met[cstar] <= -0.5
    elif kind == 'floor':
        assert -floor < met[cstar] < 0
    Kd = diagonals(band)
    Kd[0, cstar] = diag[cstar]
    band.setflags(write=False)
    return band, floor, Kd


def guard_points(n):
    return sorted({0, n // 2, n - 1})


def guard_bws(n):
    b = bws_for(n)
    return sorted({b[-1]} | ({7} if 7 in b else set()))


def check_guard(solver, n, bw, cstar, kind):
    """(d): bad == 1 and the factor bound against the matrix the rule makes.  Returns the worst ratio."""
    band, floor, Kd = guard_case(n, bw, cstar, kind)
    rhs = case('dd', n, bw)['rhs'][:2]
    perm = case('dd', n, bw)['perms'][1]
    out = call(solver, n, bw, band, perm, rhs, 256, 1, pivot_floor=floor)
    check_padding(out)
    w = check_factor(out, Kd, bad=1)
    check_solve(out, perm, rhs)
    return w


# ------------------------------------------------------------------------------------------------------------------------------ rejections
def check_rejections(solver):
    """Arguments the entry must refuse before anything is launched; a valid call works afterwards."""
    n, bw = 65, 8
    c = case('dd', n, bw)
    ok = dict(n=n, bw=bw, band=c['band'], perm=c['perms'][1], rhs=c['rhs'][:2])

    def status(**kw):
        a = dict(ok, **kw)
        return solver.hip_test_band(a['n'], a['bw'], a['band'], a['perm'], a['rhs'], None, threads=a.get('threads', 256), guard=a.get('guard', 0))[0]

    assert status() == 0
    repeat = c['perms'][1].copy()
    repeat[3] = repeat[4]
    outside = c['perms'][1].copy()
    outside[0] = n
    big = 300                                                                       # band_doubles(300, 56) + 2 * 304 doubles = 157 KB > the 144 KB cap
    for bad in (dict(bw=57, band=np.zeros((n, 58))), dict(bw=n, band=np.zeros((n, n + 1))), dict(perm=repeat), dict(perm=outside), dict(threads=128),
                dict(threads=64, guard=1), dict(guard=2), dict(n=big, bw=56, band=np.zeros((big, 57)), perm=np.arange(big), rhs=np.zeros((1, big))),
                dict(n=0, bw=0, band=np.zeros(0), perm=np.zeros(0), rhs=None), dict(bw=-1), dict(band=c['band'][:-1]), dict(perm=c['perms'][1][:-1]),
                dict(rhs=np.zeros((9, n))), dict(rhs=np.zeros(n + 1))):
        assert status(**bad) == STATUS_INVALID, sorted(bad)
    out = call(solver, n, bw, c['band'], c['perms'][1], c['rhs'][:2])
    check_padding(out)
    check_factor(out, c['Kd'])
    check_solve(out, c['perms'][1], c['rhs'][:2])


# ------------------------------------------------------------------------------------------------------------------------------ emulation
def emulate(n, bw, band, perm, rhs, drop_update=None, short_kmax=False, unfinished=False, mix_perm=False):
    """band_factor's right-looking ORDER of operations and textbook substitutions in plain doubles, in the kernel's layout -- with, on request, one of
    the mistakes the checks have to notice: drop_update = (c, a) skips the trailing update of step c on the slot (row c + bw, column c + a), the band's
    edge; short_kmax: kmax one too small in the last bw columns; unfinished: the forward pass leaves the last term of its last element out (of the
    last element that has one, and the last term that is not zero); mix_perm: out[k] instead of out[perm[k]]."""
    W, F = band_stride(bw), FRONT
    rhs = np.asarray(rhs, dtype=np.float64).reshape(-1, n)
    img, dinv = np.zeros(band_doubles(n, bw)), np.zeros(n)
    for c in range(n):
        k = min(bw, n - 1 - c) + 1
        img[F + c * W:F + c * W + k] = band[c, :k]
    for c in range(n):
        with np.errstate(invalid='ignore'):                            # (a planted mistake may leave a negative pivot: NaN from here on)
            di = 1.0 / np.sqrt(img[F + c * W])
        kmax = min(bw, n - 1 - c)
        if short_kmax and c >= n - bw:
            kmax = max(0, min(bw, n - 2 - c))
        col = img[F + c * W + 1:F + c * W + 1 + kmax] * di
        img[F + c * W + 1:F + c * W + 1 + kmax] = col
        dinv[c] = di
        for a in range(1, kmax + 1):
            upd = col[a - 1:] * col[a - 1]
            if drop_update == (c, a) and kmax == bw:
                upd = upd.copy()
                upd[-1] = 0.0
            img[F + (c + a) * W:F + (c + a) * W + kmax - a + 1] -= upd
    for c in range(n):
        img[F + c * W + 1:F + c * W + 1 + bw] *= dinv[c]
        dinv[c] *= dinv[c]
        img[F + c * W] = 0.0
    x = np.full(rhs.shape[0] * n + 16, SENTINEL)
    rows = [e for e in range(n) if img[F + np.arange(max(0, e - bw), e) * W + (e - np.arange(max(0, e - bw), e))].any()]
    last_row = rows[-1] if unfinished and rows else -1                  # (the last row of L^ that has an entry: in the kkt class not always n - 1)
    for s in range(rhs.shape[0]):
        v = rhs[s][perm].copy()
        for e in range(n):
            js = np.arange(max(0, e - bw), e)
            if e == last_row:
                js = js[:np.flatnonzero(img[F + js * W + (e - js)])[-1]]
            v[e] -= (img[F + js * W + (e - js)] * v[js]).sum()
        v *= dinv
        for i in range(n - 1, -1, -1):
            js = np.arange(i + 1, min(n - 1, i + bw) + 1)
            v[i] -= (img[F + i * W + (js - i)] * v[js]).sum()
        if mix_perm:
            x[s * n:(s + 1) * n] = v
        else:
            x[s * n + perm] = v
    return Out(x, img, dinv, 0, n, bw, rhs.shape[0])


# ------------------------------------------------------------------------------------------------------------------------------ the one-iteration probe
# One ADMM iteration of the batch kernels from a cold start with alpha = 1 and bounds far away returns x = -K^-1 q, K = P + sigma I + rho A'A: the
# band assembled and factored by k_batch_admm itself and solved by band_solve (variant `direct`, 64 threads) or by the register-resident n <= 128 form
# (variant `direct256`).  (n, seed, entries per row): chosen on the host simulator, which reports the band width of the symbolic analysis
# (hip_stats()['batch_direct_bw']); tests/test_band_ref.py asserts the conditions, the GPU tier asserts them again from the same stat.
PROBE_RHO = 0.1
PROBE_SETTINGS = dict(scaling=0, alpha=1.0, rho=PROBE_RHO, sigma=SIGMA, adaptive_rho=False, max_iter=1, polishing=True, verbose=False, warm_starting=False)
PROBE_CASES = [(100, 0, 3), (100, 4, 3), (124, 5, 2), (64, 2, 3), (136, 7, 2)]          # band widths 55, 56, 37, 41, 36
PROBE_MAX_NNZ = 1536


@functools.lru_cache(maxsize=None)
def probe_problem(n, seed, per_row):
    import scipy.sparse as sp
    rng = np.random.default_rng([7, n, seed])
    A = (sp.random(n, n, density=(per_row - 1) / n, random_state=rng, data_rvs=rng.standard_normal) + sp.identity(n)).tocsc()
    P = sp.diags(rng.uniform(0.5, 1.5, n)).tocsc()
    Q = rng.standard_normal((2, n))
    return P, A, Q


def probe_conditions(stats):
    """stats: [(n, bw, nnz(A), nnz(B))] of PROBE_CASES."""
    assert any(64 < n <= 128 and bw >= 48 for n, bw, _, _ in stats), stats
    assert any(121 <= n <= 128 and bw >= 32 for n, bw, _, _ in stats), stats
    assert any(n <= 64 for n, bw, _, _ in stats), stats
    assert any(n == 136 for n, bw, _, _ in stats), stats
    assert all(0 <= bw <= MAX_BW and a <= PROBE_MAX_NNZ and b <= PROBE_MAX_NNZ for n, bw, a, b in stats), stats


def probe_bound_ratio(P, A, q, x, bw):
    """(i): ||q + K x||_2 / (gamma_{3 (bw + 2) + a} n ||K||_2 ||x||_2) in np.longdouble, a = 2 + the most entries in a column of A."""
    n = A.shape[1]
    Ad = np.asarray(A.todense(), dtype=L)
    K = np.asarray(P.todense(), dtype=L) + L(SIGMA) * np.eye(n, dtype=L) + L(PROBE_RHO) * (Ad.T @ Ad)
    a = 2 + int(np.diff(A.tocsc().indptr).max())
    res = np.sqrt(((np.asarray(q, dtype=L) + K @ np.asarray(x, dtype=L)) ** 2).sum())
    norm_k = L(np.linalg.norm(np.asarray(K, dtype=np.float64), 2)) * (1 + L(2.0) ** -40)          # (the fp64 2-norm of K, rounded up: 1e-12 against a bound of 100 u)
    return float(res / (gamma(3 * (bw + 2) + a) * n * norm_k * np.sqrt((np.asarray(x, dtype=L) ** 2).sum())))
