"""Sparse restatement of tests/adjoint_ref.py -- the yardstick of the adjoint tests at the sizes of the PCG path (a helper, not a test).

Same active-set rule, same system  [P, A_a'; A_a, 0] [r_x; r_a] = -[dx; dy_a],  same outputs; K_a is built with scipy.sparse.bmat and factorised
with scipy.sparse.linalg.splu.  dP and dA are returned at the stored entries (upper triangle of P, CSC order; A in CSC order).  sigma_min(K_a) is
estimated by inverse iteration on the LU factors (K_a is symmetric: the iteration converges to the eigenvalue of smallest magnitude).
tests/test_adjoint_sparse_reference_cpu.py pins this helper to the dense one."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def full_symmetric(P):
    P = sp.csc_matrix(P)
    if abs(sp.tril(P, -1)).sum() == 0.0:
        P = P + sp.triu(P, 1).T
    return sp.csc_matrix(P)


def active_set(A, l, u, x, y):
    z = sp.csr_matrix(A) @ x
    low = z - l < -y
    upp = ~low & (u - z < y)
    eq = l == u
    low = np.where(eq, y < 0, low)
    upp = np.where(eq, ~(y < 0), upp)
    return low, upp


def kkt(P, A, low, upp):
    P, A = full_symmetric(P), sp.csr_matrix(A)
    act = np.nonzero(low | upp)[0]
    Aa = A[act]
    K = sp.bmat([[P, Aa.T], [Aa, None]], format='csc') if len(act) else P
    return sp.csc_matrix(K), act


def stored_entries(P, A):
    """(rows, cols) of the upper triangle of P in CSC order and of A in CSC order: where dP and dA are evaluated."""
    Pt, Ac = sp.triu(sp.csc_matrix(P), format='csc'), sp.csc_matrix(A)
    Pt.sort_indices(); Ac.sort_indices()
    pc, ac = Pt.tocoo(), Ac.tocoo()
    return (pc.row, pc.col), (ac.row, ac.col)


def gradients(P, A, x, y, r_x, r_y):
    """dP, dA at the stored entries from (x, y, r_x, r_y) by the formulas of adjoint_ref."""
    (pr, pc), (ar, ac) = stored_entries(P, A)
    return 0.5 * (r_x[pr] * x[pc] + r_x[pc] * x[pr]), y[ar] * r_x[ac] + r_y[ar] * x[ac]


def sigma_min(lu, size, iters=30, seed=0):
    v = np.random.default_rng(seed).standard_normal(size)
    v /= np.linalg.norm(v)
    s = np.inf
    for _ in range(iters):
        w = lu.solve(v)
        nw = np.linalg.norm(w)
        s = 1.0 / nw
        v = w / nw
    return float(s)


def adjoint(P, A, l, u, x, y, dx, dy=None, want_sigma=True):
    """dict(dP, dq, dA, dl, du, r_x, r_y, low, upp, K, act, g, residual, sigma_min); dP / dA at the stored entries."""
    A = sp.csr_matrix(A)
    n, m = A.shape[1], A.shape[0]
    l, u, x, y, dx = (np.asarray(a, dtype=float) for a in (l, u, x, y, dx))
    dy = np.zeros(m) if dy is None else np.asarray(dy, dtype=float)
    low, upp = active_set(A, l, u, x, y)
    K, act = kkt(P, A, low, upp)
    g = -np.concatenate([dx, dy[act]])
    lu = spla.splu(K)
    r = lu.solve(g)
    r = r + lu.solve(g - K @ r)                      # one step of refinement: the residual at rounding level
    r_x, r_y = r[:n], np.zeros(m)
    r_y[act] = r[n:]
    dP, dA = gradients(P, A, x, y, r_x, r_y)
    res = float(np.abs(g - K @ r).max() / max(np.abs(g).max(), 1e-300))
    return dict(dP=dP, dq=r_x.copy(), dA=dA, dl=np.where(low, -r_y, 0.0), du=np.where(upp, -r_y, 0.0), r_x=r_x, r_y=r_y, low=low, upp=upp, K=K, act=act,
                g=g, residual=res, sigma_min=sigma_min(lu, K.shape[0]) if want_sigma else None)


def certificate(P, A, l, u, x, y, dx, dy, dq, dl, du):
    """max |g - K_a r| / max |g| of a returned (dq, dl, du) against K_a and g rebuilt from the caller's data: r_x = dq, r_y = -(dl + du)."""
    m = sp.csc_matrix(A).shape[0]
    dy = np.zeros(m) if dy is None else np.asarray(dy, dtype=float)
    low, upp = active_set(A, l, u, x, y)
    K, act = kkt(P, A, low, upp)
    g = -np.concatenate([dx, dy[act]])
    r = np.concatenate([dq, -(dl + du)[act]])
    return float(np.abs(g - K @ r).max() / max(np.abs(g).max(), 1e-300)), g, r, int(len(act))
