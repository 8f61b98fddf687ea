"""Dense numpy statement of the adjoint derivatives of a QP solution -- the yardstick of the adjoint tests (a helper, not a test).

QP:  min 1/2 x'Px + q'x  s.t.  l <= Ax <= u,  solved to (x, y), z = Ax.

Active set (polish's rule): row i is lower-active if z_i - l_i < -y_i, otherwise upper-active if u_i - z_i < y_i; a row with l_i == u_i is
always active -- lower if y_i < 0, upper otherwise.  With A_a the active rows and incoming gradients dx = dL/dx, dy = dL/dy (None: 0):

    [ P    A_a' ] [ r_x ]     [ dx   ]
    [ A_a  0    ] [ r_a ] = - [ dy_a ],      r_y = r_a on the active rows, 0 elsewhere

    dq = r_x;  dl_i = -r_y,i on lower-active rows;  du_i = -r_y,i on upper-active rows;
    dP_ij = (r_x,i x_j + r_x,j x_i) / 2  (symmetric: the same value in either triangle);   dA_ij = y_i r_x,j + r_y,i x_j.

dP and dA are returned dense; a caller compares them at the stored entries of P and A.
"""
import numpy as np
import scipy.sparse as sp

EPS = np.finfo(float).eps


def _dense(M):
    return M.toarray() if sp.issparse(M) else np.asarray(M, dtype=float)


def full_symmetric(P):
    """The full symmetric matrix of a P given as its upper triangle or in full."""
    P = _dense(P)
    if np.abs(np.tril(P, -1)).max(initial=0.0) == 0.0:
        P = P + np.triu(P, 1).T
    return P


def active_set(A, l, u, x, y):
    A = _dense(A)
    z = A @ x
    low = z - l < -y
    upp = ~low & (u - z < y)
    eq = l == u
    low = np.where(eq, y < 0, low)
    upp = np.where(eq, ~(y < 0), upp)
    return low, upp


def kkt(P, A, low, upp):
    P, A = full_symmetric(P), _dense(A)
    act = np.nonzero(low | upp)[0]
    Aa = A[act]
    n, k = P.shape[0], len(act)
    K = np.zeros((n + k, n + k))
    K[:n, :n] = P; K[:n, n:] = Aa.T; K[n:, :n] = Aa
    return K, act


def adjoint(P, A, l, u, x, y, dx, dy=None):
    """dict(dP, dq, dA, dl, du, r_x, r_y, low, upp, K, act) of the section above; K is the unregularised KKT matrix of the active set."""
    P, A = full_symmetric(P), _dense(A)
    n, m = P.shape[0], A.shape[0]
    l, u, x, y, dx = (np.asarray(a, dtype=float) for a in (l, u, x, y, dx))
    dy = np.zeros(m) if dy is None else np.asarray(dy, dtype=float)
    low, upp = active_set(A, l, u, x, y)
    K, act = kkt(P, A, low, upp)
    g = -np.concatenate([dx, dy[act]])
    if len(act) > n or np.linalg.matrix_rank(K) < K.shape[0]:
        r = np.linalg.lstsq(K, g, rcond=None)[0]
    else:
        r = np.linalg.solve(K, g)
    r_x, r_y = r[:n], np.zeros(m)
    r_y[act] = r[n:]
    dP = 0.5 * (np.outer(r_x, x) + np.outer(x, r_x))
    dA = np.outer(y, r_x) + np.outer(r_y, x)
    return dict(dP=dP, dq=r_x.copy(), dA=dA, dl=np.where(low, -r_y, 0.0), du=np.where(upp, -r_y, 0.0), r_x=r_x, r_y=r_y, low=low, upp=upp, K=K, act=act)


def conditions(P, A, l, u, x, y):
    """(smallest slack of an inactive side, smallest |y| of an active inequality row, sigma_min(K_a), cond_2(K_a)): what makes the active set --
    and with it the derivative -- well defined.  inf where there is no such row."""
    A = _dense(A)
    low, upp = active_set(A, l, u, x, y)
    z = A @ x
    inact = ~(low | upp)
    slack = np.minimum(z - l, u - z)[inact].min(initial=np.inf)
    ineq = (low | upp) & (l != u)
    ymin = np.abs(y[ineq]).min(initial=np.inf)
    K, _ = kkt(P, A, low, upp)
    sv = np.linalg.svd(K, compute_uv=False)
    return float(slack), float(ymin), float(sv.min()), float(sv.max() / sv.min())


def solve_bound(K, delta=1e-6, refine=3):
    """What a solve of K r = g by `refine` + 1 steps of iterative refinement on the delta-regularised matrix may miss, relative to max |r|:
    ten times the larger of the rounding floor 1e3 eps cond_2(K) and the contraction (delta / sigma_min(K))^(refine + 1)."""
    sv = np.linalg.svd(K, compute_uv=False)
    return 10.0 * max(1e3 * EPS * sv.max() / sv.min(), (delta / sv.min()) ** (refine + 1))
