"""References and case machinery for the kernel-level tests of the dense fp64 routines (osqp-python_amd/csrc/dense_hip.hip) -- numpy only, no GPU.

What is here
  gemm_ref          beta C0 + alpha A B in np.longdouble (numpy's own loops, no BLAS) and the magnitude product the componentwise bound scales with
  pack / unpack     a logical matrix inside a flat canvas at element strides and an offset; the cells outside it hold NaN (operands: an out-of-range load
                    that is USED poisons the result) or a sentinel (C: an out-of-range store changes its bits) -- neither needs a fault to be seen
  spd / indefinite  Q diag(lambda) Q' with lambda log-spaced on [1, kappa]; the same with one eigenvalue -1, permuted so that the first negative pivot of an
                    elimination without pivoting falls into a chosen 64-column block
  inverse_ref       np.linalg.inv + three Newton steps X += X (I - A X) in np.longdouble, its residual asserted
  gj_emulate        the kernel's ALGORITHM in numpy doubles: 64-column block steps, P = A_kk^-1 by Gauss-Jordan without pivoting, R = P A_k:, a rank-64
                    update, A_ik = -A_ik P.  It gives the error such an elimination has on a matrix (the yardstick of the ill-conditioned cases) and
                    lets the CPU tier confirm that the accuracy bound of the well-conditioned cases is one the algorithm itself keeps.
  check_*           one case each, with its assertions, on any object that has hip_test_dense (osqp_amd.ext_hip.OSQPSolver): the GPU tier
                    (tests/test_gpu_dense_kernels.py) runs them on the kernels, the CPU tier (tests/test_dense_ref.py) on the host simulator's plain loops,
                    which proves canvases, masks, references and bounds before they meet a kernel.

Bounds (none of them measured on the code under test)
  GEMM, componentwise   |C - C_ref| <= (K + 4) 2^-52 (|alpha| |A| |B| + |beta| |C0|): the inner-product bound gamma_K for ANY order of summation, fused or not,
                        plus the roundings of the two scalings and the final sum.
  inverse               max|X - X_ref| / max|X_ref| <= n 2^-52 kappa; gj_emulate stays well below it on every (n, kappa) of the tests (asserted by the CPU tier).
  inverse, kappa = 1e8  forming P = A_kk^-1 explicitly loses digits (dense_hip.hip's header): the kernel's error <= 32 x gj_emulate's error on the same matrix
                        (another order of summation and fused multiply-adds in the updates; not a constant).
  smallest pivot        the pivots of an elimination without pivoting are fixed by the matrix (ratios of leading principal minors), blocked or not:
                        pivots_ref computes them in np.longdouble.  A block of fewer than 64 columns is padded with the identity, which contributes pivots 1.
"""
import functools

import numpy as np

EPS = 2.0 ** -52
SENTINEL = -3.5e77                     # (finite, no value a product of the test data comes near)
NB = 64                                # block step of dense_spd_inverse, tile of dense_gemm
STATUS_BAD_STRIDES = 7                 # OSQP_ALGEBRA_LOAD_ERROR: the routine's own error, reported at the C ABI

GEMM_SHAPES = [(1, 1, 1), (63, 65, 15), (64, 64, 16), (65, 63, 17), (130, 70, 33), (70, 130, 50), (64, 1, 64), (5, 64, 64), (33, 33, 0)]
GEMM_LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]          # (A contiguous along K, B contiguous along K)
GEMM_SCALARS = [(1.0, 0.0), (-1.0, 1.0), (0.75, -0.5)]
SYM_N = [1, 31, 32, 33, 64, 65, 97, 130]
SYM_K = [1, 17, 40]
INV_N = [1, 2, 63, 64, 65, 127, 128, 129, 193, 200, 256]
INV_KAPPA = [1e2, 1e4]
ILL_N = [65, 200]
ILL_KAPPA = 1e8
ILL_FACTOR = 32.0
LOOKAHEAD_N = [65, 193, 200]
INDEFINITE = [(200, 0), (200, 2), (129, 2)]                                          # (order, block of the first negative pivot); (129, 2): the one-column tail


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------------------------ canvases
def pack(mat, s_r, s_c, offset, fill, tail=4):
    """mat inside a flat canvas: element (i, j) at offset + i s_r + j s_c; every other cell = fill.  Returns (canvas, mask of the matrix' cells)."""
    mat = np.asarray(mat, dtype=np.float64)
    r, c = mat.shape
    last = offset + (max(r, 1) - 1) * s_r + (max(c, 1) - 1) * s_c
    canvas = np.full(last + 1 + tail, fill, dtype=np.float64)
    mask = np.zeros(canvas.size, dtype=bool)
    idx = (offset + s_r * np.arange(r)[:, None] + s_c * np.arange(c)[None, :]).ravel()
    assert len(np.unique(idx)) == idx.size, 'strides alias'
    canvas[idx] = mat.ravel()
    mask[idx] = True
    return canvas, mask


def unpack(canvas, shape, s_r, s_c, offset):
    r, c = shape
    return canvas[offset + s_r * np.arange(r)[:, None] + s_c * np.arange(c)[None, :]]


def assert_canvas_untouched(after, mask, fill):
    want = bits(np.full(1, fill))[0]
    got = bits(after)[~mask]
    assert (got == want).all(), '%d canvas cells outside the matrix changed' % int((got != want).sum())


# ------------------------------------------------------------------------------------------------------------------------------ GEMM
def gemm_ref(A, B, C0, alpha, beta):
    """(beta C0 + alpha A B, |alpha| |A| |B| + |beta| |C0|) in np.longdouble.  beta == 0: C0 is not an operand (it may hold NaN)."""
    L = np.longdouble
    A, B = np.asarray(A, dtype=L), np.asarray(B, dtype=L)
    M, N = A.shape[0], B.shape[1]
    prod = A @ B if A.shape[1] else np.zeros((M, N), dtype=L)
    mag = np.abs(A) @ np.abs(B) if A.shape[1] else np.zeros((M, N), dtype=L)
    ref, mag = L(alpha) * prod, abs(L(alpha)) * mag
    if beta != 0.0:
        C0 = np.asarray(C0, dtype=L)
        ref, mag = ref + L(beta) * C0, mag + abs(L(beta)) * np.abs(C0)
    return ref, mag


def assert_componentwise(C, ref, mag, K):
    assert np.isfinite(C).all(), 'not finite: an operand cell outside the matrix (NaN) or C under beta = 0 was read'
    err = np.abs(np.asarray(C, dtype=np.longdouble) - ref)
    bound = (K + 4) * EPS * mag
    bad = err > bound
    assert not bad.any(), 'componentwise bound missed at %s: error %.3e against %.3e' % (np.argwhere(bad)[0], float(err[bad].max()), float(bound[bad].min()))


@functools.lru_cache(maxsize=None)
def gemm_operands(M, N, K):
    rng = np.random.default_rng(1000003 * M + 1009 * N + K)
    return rng.standard_normal((M, K)), rng.standard_normal((K, N)), rng.standard_normal((M, N))


def gemm_case(shape, layout, scalars, colmajor):
    """The canvases of one GEMM case: operands with a leading dimension 3 above the need and an offset, C with cs_i = N + 5 (or column-major, cs_j = M + 2)."""
    (M, N, K), (ak, bk), (alpha, beta) = shape, layout, scalars
    A, B, C0 = gemm_operands(M, N, K)
    if beta == 0.0:
        C0 = np.full((M, N), np.nan)
    a_str = (K + 3, 1) if ak else (1, M + 3)                  # (as_i, as_k)
    b_str = (1, K + 3) if bk else (N + 3, 1)                  # (bs_k, bs_j)
    c_str = (1, M + 2) if colmajor else (N + 5, 1)            # (cs_i, cs_j)
    offs = (5, 7, 9)
    ca, _ = pack(A, a_str[0], a_str[1], offs[0], np.nan)
    cb, _ = pack(B, b_str[0], b_str[1], offs[1], np.nan)
    cc, mask = pack(C0, c_str[0], c_str[1], offs[2], SENTINEL, tail=max(c_str) + 4)      # (a whole row / column of sentinels behind the matrix: a store one past the edge lands in it)
    return dict(A=A, B=B, C0=C0, ca=ca, cb=cb, cc=cc, mask=mask, a_str=a_str, b_str=b_str, c_str=c_str, offs=offs)


def check_gemm(solver, shape, layout, scalars, colmajor=False):
    (M, N, K), (alpha, beta) = shape, scalars
    c = gemm_case(shape, layout, scalars, colmajor)
    st, out, _ = solver.hip_test_dense(0, c['cc'], c['ca'], c['cb'], M=M, N=N, K=K, alpha=alpha, beta=beta,
                                       a_strides=c['a_str'], b_strides=c['b_str'], c_strides=c['c_str'], offsets=c['offs'])
    assert st == 0, st
    assert_canvas_untouched(out, c['mask'], SENTINEL)
    ref, mag = gemm_ref(c['A'], c['B'], c['C0'], alpha, beta)
    assert_componentwise(unpack(out, (M, N), c['c_str'][0], c['c_str'][1], c['offs'][2]), ref, mag, K)


def check_gemm_rejects_bad_strides(solver):
    """An operand without a unit stride: the routine's error comes back as the entry's status and C is as it was."""
    A, B, C0 = gemm_operands(5, 6, 7)
    cc, _ = pack(C0, 6, 1, 0, SENTINEL)
    for a_str, b_str in (((14, 2), (6, 1)), ((7, 1), (12, 2)), ((14, 2), (12, 2))):
        ca, _ = pack(A, a_str[0], a_str[1], 0, np.nan)
        cb, _ = pack(B, b_str[0], b_str[1], 0, np.nan)
        st, out, _ = solver.hip_test_dense(0, cc, ca, cb, M=5, N=6, K=7, alpha=1.0, beta=0.0, a_strides=a_str, b_strides=b_str, c_strides=(6, 1))
        assert st == STATUS_BAD_STRIDES, st
        assert (bits(out) == bits(cc)).all()


def check_entry_rejects_operands_outside_their_buffers(solver):
    """The entry itself refuses (OSQP_DATA_VALIDATION_ERROR = 1) what would address a cell outside a buffer: nothing is launched."""
    A, B, C0 = gemm_operands(5, 6, 7)
    ca, cb, cc = A.ravel(), B.ravel(), C0.ravel()
    ok = dict(M=5, N=6, K=7, a_strides=(7, 1), b_strides=(6, 1), c_strides=(6, 1))
    assert solver.hip_test_dense(0, cc, ca, cb, **ok)[0] == 0
    for bad in (dict(M=6), dict(N=7), dict(K=8), dict(a_strides=(8, 1)), dict(b_strides=(7, 1)), dict(c_strides=(7, 1)), dict(offsets=(1, 0, 0)), dict(offsets=(0, 0, 1)),
                dict(c_strides=(-6, 1))):
        assert solver.hip_test_dense(0, cc, ca, cb, **dict(ok, **bad))[0] == 1, bad
    assert solver.hip_test_dense(2, np.zeros(16), N=4, c_strides=(3, 1))[0] == 1          # ld < n
    assert solver.hip_test_dense(2, np.zeros(15), N=4, c_strides=(4, 1))[0] == 1


# ------------------------------------------------------------------------------------------------------------------------------ symmetric form
def check_gemm_sym(solver, N, K, form, pad):
    """form 'T': W is K x N row-major, C = W' W (strides (1, N; N, 1)); form 'S': W is N x K row-major, C = W W' (strides (K, 1; 1, K)) -- the two the product
    uses (woodbury_hip.hip).  ld = N + pad."""
    alpha = 0.75
    rng = np.random.default_rng(7919 * N + 31 * K + (form == 'S'))
    if form == 'T':
        W = rng.standard_normal((K, N))
        A, B, a_str, b_str = W.T, W, (1, N), (N, 1)
    else:
        W = rng.standard_normal((N, K))
        A, B, a_str, b_str = W, W.T, (K, 1), (1, K)
    cw, _ = pack(W, W.shape[1], 1, 3, np.nan)
    ld = N + pad
    cc, mask = pack(np.full((N, N), SENTINEL), ld, 1, 2, SENTINEL, tail=ld + 4)                        # (beta = 0: what C holds does not matter; the block's cells are masked)
    st, out, _ = solver.hip_test_dense(1, cc, cw, cw, N=N, K=K, alpha=alpha, a_strides=a_str, b_strides=b_str, c_strides=(ld, 1), offsets=(3, 3, 2))
    assert st == 0, st
    assert_canvas_untouched(out, mask, SENTINEL)
    C = unpack(out, (N, N), ld, 1, 2)
    ref, mag = gemm_ref(A, B, None, alpha, 0.0)
    assert_componentwise(C, ref, mag, K)
    assert (bits(C) == bits(C.T)).all(), 'the mirror is not bitwise symmetric'


# ------------------------------------------------------------------------------------------------------------------------------ SPD inverse
def _orthogonal(n, seed):
    Q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, n)))
    return Q


@functools.lru_cache(maxsize=None)
def spd(n, kappa, seed=0):
    lam = np.logspace(0.0, np.log10(kappa), n) if n > 1 else np.array([kappa])
    Q = _orthogonal(n, 100 * n + seed)
    A = (Q * lam) @ Q.T
    A = 0.5 * (A + A.T)
    A.setflags(write=False)
    return A


def inverse_ref(A, tol):
    """A^-1 to working precision of np.longdouble; tol: the relative tolerance the caller compares against (the reference's own residual is 1e-3 of it)."""
    L = np.longdouble
    n = A.shape[0]
    Al, X, I = np.asarray(A, dtype=L), np.asarray(np.linalg.inv(A), dtype=L), np.eye(n, dtype=L)
    for _ in range(3):
        X = X + X @ (I - Al @ X)
    res = float(np.abs(I - Al @ X).max())
    assert res < 1e-3 * tol, 'reference inverse: residual %.3e against %.3e' % (res, 1e-3 * tol)
    return X


def pivots_ref(A):
    """The pivots of an elimination without pivoting (np.longdouble)."""
    S = np.array(A, dtype=np.longdouble)
    n = S.shape[0]
    piv = np.empty(n, dtype=np.longdouble)
    for k in range(n):
        piv[k] = S[k, k]
        if k + 1 < n:
            S[k + 1:, k + 1:] -= np.outer(S[k + 1:, k], S[k, k + 1:]) / S[k, k]
    return piv


def gj_emulate(A):
    """dense_spd_inverse's algorithm in numpy doubles (whole matrix kept current, the lower triangle mirrored at the end).  Returns (X, smallest pivot)."""
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    minpiv = np.inf
    for k0 in range(0, n, NB):
        k1 = min(k0 + NB, n)
        P = A[k0:k1, k0:k1].copy()
        for k in range(k1 - k0):                               # P = A_kk^-1, Gauss-Jordan without pivoting, in place
            p = P[k, k]
            minpiv = min(minpiv, p) if p == p else p
            col = P[:, k].copy()
            row = P[k, :] / p
            row[k] = 1.0 / p
            P -= np.outer(col, row)
            P[:, k] = -col / p
            P[k, :] = row
        out = np.r_[0:k0, k1:n]
        R = P @ A[k0:k1][:, out]
        Ck = A[out][:, k0:k1]
        A[np.ix_(out, out)] -= Ck @ R
        A[np.ix_(out, np.arange(k0, k1))] = -Ck @ P
        A[np.ix_(np.arange(k0, k1), out)] = R
        A[k0:k1, k0:k1] = P
    iu = np.triu_indices(n, 1)
    A[iu[1], iu[0]] = A[iu]
    return A, float(minpiv)


def rel_err(X, Xref):
    return float(np.abs(np.asarray(X, dtype=np.longdouble) - Xref).max() / np.abs(Xref).max())


def inverse_bound(n, kappa):
    return n * EPS * kappa


@functools.lru_cache(maxsize=None)
def inverse_case(n, kappa):
    """(A, X_ref, the smallest pivot an exact elimination meets incl. the identity padding of a partial block, gj_emulate's relative error)."""
    A = spd(n, kappa)
    Xref = inverse_ref(A, inverse_bound(n, kappa))
    piv = float(pivots_ref(A).min())
    if n % NB:
        piv = min(piv, 1.0)
    emu = rel_err(gj_emulate(A)[0], Xref)
    return A, Xref, piv, emu


def run_inverse(solver, A, pad):
    n = A.shape[0]
    ld = n + pad
    cc, mask = pack(A, ld, 1, 0, SENTINEL, tail=ld + 4)
    st, out, minpiv = solver.hip_test_dense(2, cc, N=n, c_strides=(ld, 1))
    assert st == 0, st
    assert_canvas_untouched(out, mask, SENTINEL)
    return unpack(out, (n, n), ld, 1, 0), minpiv


def assert_pivot(minpiv, A, piv_ref, kappa):
    """minpiv > 0 and at most the largest diagonal entry (a pivot never exceeds the diagonal entry it started from), at most 1 where a partial block is padded
    with the identity -- and, sharper than both, equal to the smallest pivot of an exact elimination up to the rounding the elimination can have."""
    n = A.shape[0]
    assert minpiv > 0, minpiv
    assert minpiv <= (min(1.0, A.diagonal().max()) if n % NB else A.diagonal().max()), (minpiv, A.diagonal().max())
    assert abs(minpiv - piv_ref) <= inverse_bound(n, kappa) * abs(piv_ref), (minpiv, piv_ref)


def check_inverse(solver, n, kappa, pad):
    A, Xref, piv, _ = inverse_case(n, kappa)
    X, minpiv = run_inverse(solver, A, pad)
    assert np.isfinite(X).all()
    err = rel_err(X, Xref)
    print('inverse n=%d kappa=%.0e ld=n+%d: error %.3e (bound %.3e), minpiv %.6g (exact %.6g)' % (n, kappa, pad, err, inverse_bound(n, kappa), minpiv, piv))
    assert err <= inverse_bound(n, kappa), (err, inverse_bound(n, kappa))
    assert (bits(X) == bits(X.T)).all(), 'the inverse is not bitwise symmetric'
    assert_pivot(minpiv, A, piv, kappa)
    return err


def check_inverse_ill_conditioned(solver, n):
    """kappa = 1e8: against the error of the same elimination in numpy on the same matrix.  Returns (kernel's error, emulation's error)."""
    A, Xref, _, emu = inverse_case(n, ILL_KAPPA)
    X, minpiv = run_inverse(solver, A, 0)
    assert np.isfinite(X).all()
    err = rel_err(X, Xref)
    print('inverse n=%d kappa=%.0e: error %.3e, numpy emulation of the algorithm %.3e (LAPACK: %.3e)' % (n, ILL_KAPPA, err, emu, rel_err(np.linalg.inv(A), Xref)))
    assert err <= ILL_FACTOR * emu, (err, emu)
    assert minpiv > 0
    return err, emu


# ------------------------------------------------------------------------------------------------------------------------------ not positive definite
def first_negative_pivot(A):
    piv = pivots_ref(A)
    neg = np.nonzero(~(piv > 0))[0]
    return int(neg[0]) if neg.size else -1


@functools.lru_cache(maxsize=None)
def indefinite(n, block, kappa=1e2):
    """The generator's matrix with its smallest eigenvalue set to -1, permuted symmetrically so that the first pivot that is not positive has its index in
    [64 block, 64 (block + 1)) -- for n = 129, block 2, that is the one-column tail.  A leading minor turns negative once the leading coordinates carry
    most of the eigenvector v of -1; with the Haar-distributed Q of the generator that happens only near the end, whatever the permutation.  So v is
    prescribed (column 0 of the seeded normal matrix before its QR): components falling like 0.3^i, 91 % of its mass in one coordinate -- and the
    permutation puts the heavy coordinates at the chosen place, the light ones in front.  The place of the first negative pivot is asserted."""
    lam = np.logspace(0.0, np.log10(kappa), n)
    lam[0] = -1.0
    G = np.random.default_rng(100 * n + 77).standard_normal((n, n))
    G[:, 0] = 0.3 ** np.minimum(np.arange(n), 40)
    Q, _ = np.linalg.qr(G)
    A = (Q * lam) @ Q.T
    A = 0.5 * (A + A.T)
    lo, hi = NB * block, min(NB * (block + 1), n)
    start = lo + 8 if hi - lo > 16 else lo                    # heavy coordinates 0, 1, 2, .. go to start, start + 1, ..; the lightest fill the front
    heavy = min(n - start, 40)
    perm = np.r_[np.arange(n - 1, n - 1 - start, -1), np.arange(heavy), np.arange(heavy, n - start)]
    assert sorted(perm) == list(range(n))
    B = np.ascontiguousarray(A[np.ix_(perm, perm)])
    first = first_negative_pivot(B)
    assert lo <= first < hi, 'first negative pivot at %d, wanted in [%d, %d)' % (first, lo, hi)
    B.setflags(write=False)
    return B


def check_indefinite(solver, n, block):
    """Numbers only: nothing faults, the contents are not asserted -- the smallest pivot must say 'not positive definite' (what wb_factor_large throws on)."""
    _, minpiv = run_inverse(solver, indefinite(n, block), 0)
    assert not (minpiv > 0), minpiv
    return minpiv
