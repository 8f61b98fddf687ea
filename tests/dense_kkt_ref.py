"""References and the judge of the kernel-level tests of the dense KKT mode (osqp-python_amd/csrc/densekkt_hip.hip) -- numpy only, no GPU.

What is here
  dense             a scipy matrix as a dense array of a given dtype, every STORED entry added at its place: a repeated (i, j) sums, as in the engine
  form              K = c D P D + sigma I + (E A D)' diag(rho) (E A D)  from the RAW P and A, the D, E, c of osqp_hip_get_scaling, sigma and a rho vector,
                    in np.longdouble (the reference) or np.float64 (the yardstick); the caller's numbering
  apply             x~ = x_g + K^-1 r:  np.longdouble by LAPACK + iterative refinement to the working precision of long double (its residual asserted),
                    np.float64 by an explicit inverse and one product -- the device's own algorithm class
  judge             a device value passes if  max |value - ref| <= 64 x max(e64, nsum 2^-53) x max |ref| :  e64 is the relative error of the fp64 numpy
                    evaluation of the same quantity against the long-double one (the rule of the project's other kernel tiers, tests/wb_ref.py tolerance()),
                    floored by the roundings nsum summands can have so that a numpy evaluation that happens to be exact does not ask for exactness.
                    Nothing in it is measured on the code under test.
  planted mistakes  FORM_MISTAKES / APPLY_MISTAKES: wrong evaluations the judge must catch (tests/test_dense_kkt_ref.py proves it does, on the CPU tier)
"""
import numpy as np
import scipy.sparse as sp

L = np.longdouble
U = 2.0 ** -53
FACTOR = 64.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def dense(M, dtype):
    M = sp.coo_matrix(M)
    out = np.zeros(M.shape, dtype=dtype)
    np.add.at(out, (M.row, M.col), M.data.astype(dtype))
    return out


def stored_coo(M):
    """(row, col, value) of every STORED entry of a CSC matrix, duplicates kept (scipy's own conversions may sum them)."""
    M = sp.csc_matrix(M)
    col = np.repeat(np.arange(M.shape[1]), np.diff(M.indptr))
    return M.indices.copy(), col, M.data.copy()


def dense_stored(M, dtype, overwrite=False):
    """dense(), from the stored entries themselves; overwrite: a repeated (i, j) keeps its LAST value (a planted mistake)."""
    r, c, v = stored_coo(M)
    out = np.zeros(M.shape, dtype=dtype)
    if overwrite:
        out[r, c] = v.astype(dtype)
    else:
        np.add.at(out, (r, c), v.astype(dtype))
    return out


def form(P, A, D, E, c, sigma, rho, dtype=L, mistake=None):
    """K in the caller's numbering.  P: the full symmetric matrix (as problems.py returns it); mistake: one of FORM_MISTAKES."""
    n = P.shape[0]
    Pd = dense_stored(P, dtype)
    if mistake == 'p_one_triangle':
        Pd = np.triu(Pd)
    Ad = dense_stored(A, dtype, overwrite=(mistake == 'duplicate_overwritten'))
    D, E, rho = np.asarray(D, dtype=dtype), np.asarray(E, dtype=dtype), np.array(rho, dtype=dtype)
    if mistake == 'rho_row_missing':
        rho[np.argmax(np.abs(Ad).sum(axis=1))] = 1.0
    Ps = dtype(c) * (D[:, None] * Pd * D[None, :])
    As = E[:, None] * Ad * D[None, :]
    K = Ps + As.T @ (rho[:, None] * As)
    if mistake != 'sigma_missing':
        K = K + dtype(sigma) * np.eye(n, dtype=dtype)
    return K


def form_device_order(P, A, D, E, c, sigma, rho):
    """The numpy stand-in of the device's formation, fp64, in the device's own order: W = sqrt(rho) .* (E A D), W' W, then P + sigma I added."""
    As = np.asarray(E)[:, None] * dense_stored(A, np.float64) * np.asarray(D)[None, :]
    W = np.sqrt(np.asarray(rho, dtype=np.float64))[:, None] * As
    K = W.T @ W
    K += (c * (np.asarray(D)[:, None] * dense_stored(P, np.float64) * np.asarray(D)[None, :]) + sigma * np.eye(P.shape[0]))
    return K


def apply(K, r, xg, dtype=L, mistake=None):
    """x~ = x_g + K^-1 r.  np.longdouble: the reference (K given in long double); np.float64: explicit inverse, one product.  mistake: one of APPLY_MISTAKES."""
    n = K.shape[0]
    if dtype is np.float64:
        K64 = np.asarray(K, dtype=np.float64)
        u = np.linalg.inv(K64) @ np.asarray(r, dtype=np.float64)
    else:
        Kl, rl = np.asarray(K, dtype=L), np.asarray(r, dtype=L)
        K64 = np.asarray(K, dtype=np.float64)
        u = np.asarray(np.linalg.solve(K64, np.asarray(r, dtype=np.float64)), dtype=L)
        step = np.inf
        for _ in range(12):                                    # (ends at the working precision of long double, or where the steps stop shrinking below 2^-50)
            res = rl - Kl @ u
            du = np.asarray(np.linalg.solve(K64, np.asarray(res, dtype=np.float64)), dtype=L)
            u = u + du
            step, last = float(np.abs(du).max()), step
            if step <= 2.0 ** -60 * float(np.abs(u).max()) or (step >= 0.25 * last and step <= 2.0 ** -50 * float(np.abs(u).max())):
                break
        else:
            raise AssertionError('the refinement of the reference solve did not converge')
        assert float(np.abs(rl - Kl @ u).max()) <= 2.0 ** -58 * n * float(np.abs(Kl).max() * np.abs(u).max() + np.abs(rl).max()), 'reference residual'
    xs = np.asarray(xg, dtype=u.dtype) + u
    if mistake == 'xg_not_added':
        xs = u.copy()
    if mistake == 'last_row_dropped':
        xs = xs.copy(); xs[n - 1] = np.asarray(xg, dtype=u.dtype)[n - 1]
    return xs, u


FORM_MISTAKES = ('sigma_missing', 'rho_row_missing', 'p_one_triangle', 'duplicate_overwritten')
APPLY_MISTAKES = ('xg_not_added', 'last_row_dropped')


def rel(a, ref):
    ref = np.asarray(ref, dtype=L)
    return float(np.abs(np.asarray(a, dtype=L) - ref).max() / np.abs(ref).max())


def tolerance(e64, nsum):
    return FACTOR * max(e64, nsum * U)


def judge(value, ref, f64, nsum):
    """(passes, relative error of value, the tolerance).  ref: long double; f64: the fp64 numpy evaluation of the same quantity."""
    assert np.isfinite(np.asarray(value, dtype=np.float64)).all(), 'not finite'
    tol = tolerance(rel(f64, ref), nsum)
    err = rel(value, ref)
    return err <= tol, err, tol


def with_duplicate(A, seed=0):
    """A with one stored entry split in two (same (i, j), values 0.25 v and 0.75 v): the same matrix, one more stored entry."""
    A = sp.csc_matrix(A); A.sort_indices()
    rng = np.random.default_rng(seed)
    k = int(rng.integers(0, A.nnz))
    j = int(np.searchsorted(A.indptr, k, side='right') - 1)
    data = np.insert(A.data, k, 0.25 * A.data[k]); data[k + 1] = 0.75 * A.data[k]
    indices = np.insert(A.indices, k, A.indices[k])
    indptr = A.indptr.copy(); indptr[j + 1:] += 1
    B = sp.csc_matrix((data, indices, indptr), shape=A.shape)
    assert B.nnz == A.nnz + 1 and B.has_canonical_format is False
    return B


def rho_vector(l, u, rho_bar, eq_factor=1e3):
    """A rho vector by constraint class (the reference's rule): eq_factor rho_bar on equality rows, rho_bar elsewhere (1e-6 on rows without bounds)."""
    l, u = np.asarray(l), np.asarray(u)
    rho = np.full(l.size, float(rho_bar))
    rho[(u - l) < 1e-4] = eq_factor * rho_bar
    rho[(l < -1e20) & (u > 1e20)] = 1e-6
    return rho
