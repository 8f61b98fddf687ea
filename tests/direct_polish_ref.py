"""A plain fp64 numpy restatement of polish on the direct lockstep route (osqp-python_amd/csrc/lockstep_hip.hip lockstep_direct_chunk, "polish"), in
UNSCALED units, for one problem.  It is given the ADMM point (x, y) and runs the recurrence the route runs:

  classify   z = A x; a row is active on the lower side if z - l < -y or l == u (an equality row always is), on the upper side if u - z < y; b = the bound.
  rho        1 / delta on the active rows, RHO_MIN = 1e-6 on the others -- the inactive DENSE rows too.
  matrices   the rows of A with more than LONG_ROW entries are the dense rows A_L, the others have one entry (A_S), P is diagonal:
             D0 = diag(P) + sigma + A_S' rho_S A_S (diagonal),  S = diag(1 / rho_L) + A_L D0^-1 A_L'  (inverted once).
  a step     rhs = sigma x - q + A'(rho z - y);  one Woodbury refinement of x~ against it:  r = rhs - K x~,  p = D0^-1 r,
             x~ += p - D0^-1 A_L' S^-1 A_L p;  then x = x~ (alpha = 1), z~ = A x~, z = b on the active rows and z~ + y / rho on the free ones,
             y += rho (z~ - z) -- which is 0 on the free rows.
  the end    z = A x, (z, y) projected on the normal cone of [l, u]: y = (z + y) - clip(z + y, l, u).

`mistake` plants one of two errors a route like this can make (tests/test_direct_polish_ref.py shows that the check against the oracle sees both):
  'dense_rho'  an inactive dense row keeps 1 / delta in place of RHO_MIN;
  'free_y'     the free rows are not freed in the z / y step: z = b and y += rho (z~ - b) on every row."""
import numpy as np
import scipy.sparse as sp

RHO_MIN = 1e-6
LONG_ROW = 128


def direct_polish(P, q, A, l, u, x, y, steps, delta=1e-6, sigma=1e-6, mistake=None):
    A = sp.csr_matrix(A)
    Pd = sp.csc_matrix(P).diagonal()
    assert abs(sp.csc_matrix(P) - sp.diags(Pd)).max() == 0.0, 'the route wants a diagonal P'
    long_ = np.diff(A.indptr) > LONG_ROW
    AL, AS = A[long_].toarray(), A[~long_]
    assert (np.diff(AS.indptr) == 1).all(), 'the route wants one entry in every other row'
    z = A @ x
    low = (z - l < -y) | (l == u)
    act = low | (~low & (u - z < y))
    b = np.where(low, l, u)
    rho = np.where(act, 1.0 / delta, RHO_MIN)
    if mistake == 'dense_rho':
        rho[long_] = 1.0 / delta
    D0 = Pd + sigma + AS.T.multiply(AS.T) @ rho[~long_]
    Sinv = np.linalg.inv(np.diag(1.0 / rho[long_]) + (AL / D0) @ AL.T)
    x, xt = x.copy(), x.copy()
    z, y = np.where(act, b, z), np.where(act, y, 0.0)
    for _ in range(steps):
        rhs = sigma * x - q + A.T @ (rho * z - y)
        r = rhs - ((Pd + sigma) * xt + A.T @ (rho * (A @ xt)))
        p = r / D0
        xt = xt + (p - (AL.T @ (Sinv @ (AL @ p))) / D0)
        x, zt = xt.copy(), A @ xt
        if mistake == 'free_y':
            z = b
        else:
            z = np.where(act, b, zt + y / rho)
        y = y + rho * (zt - z)
    t = A @ x + y
    return x, t - np.clip(t, l, u)
