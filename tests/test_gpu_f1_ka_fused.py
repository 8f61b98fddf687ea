"""GPU tier: f1_ka_body (pcg_hip.hip) computes what it computed before its two transposed passes were fused: a workgroup's last row block runs
A_g' v and A_g' t0 as ONE staged pass (second product array and second tvec in the block's dead stream image); a block that another one follows keeps
the two passes.

The fused pass changes no summation order, so every case compares with == : info.iter, info.rho_updates, float.hex(info.obj_val), the SHA-256 of x and
y (and of the certificates of the infeasible cases), the status and the solve's PCG iteration total -- for graph replay and for eager launches --
against PARENT.  PARENT was recorded on an MI355X from the PARENT commit's build of the engine (the library of that commit
named in OSQP_HIP_LIBRARY, `record(name, graph)` of this file called for every case and both modes, which gave the same record twice in every case);
`_digest` is the whole of the comparison, so a record is re-taken the same way.

Cases -- the smallest shapes at which the fused pass can go wrong (last_ka .. warm_update), and three kept as regression records of the launches around
it, F_1's fold and a KA launch of its own (start_meets, low_cap, k_one):
  last_ka        banded_qp(30000), check_termination = 1: one row block per workgroup, every KA is a chunk's last
  mid_chunk      the same QP, check_termination = 25, adaptive_rho_interval = 50, max_iter = 110 (no multiple of 25, stops unsolved): KAs inside a
                 chunk, chunk starts behind a rho update (the SCATTER_ONLY body), a last chunk cut short
  two_blocks     banded_qp(110000, window = 40): 2019 row blocks on 1024 workgroups (D = 2; at the generator's default window the half-full blocks of
                 this size need more than four replicas and the form is refused) -- most workgroups run the two-pass sequence for their first
                 block and the fused one for their second, the others hold one block
  mix            banded_qp(30000, long_range = 0.02): far columns, whose second sums come from the second product array (MIX instantiations)
  primal_inf     banded_qp(30000) with one row repeated under bounds that cross ([1, 1] against [-1, -1]): the boundary reads dy
  dual_inf       the same QP with a column of zero curvature, free rows and q_j = -1: the boundary reads dx
  warm_update    solve; update(q, l, u); solve with warm_starting and polishing: two records
  start_meets    solve; warm start at the solution; solve: ADMM iterations whose PCG start meets the tolerance (F_1 with k = 0 iterations)
  low_cap        cg_max_iter = 1 (the cap escalates while the inner solver stalls): PCGs that end at their cap -- F_1's fold sets the tolerance, the
                 launch applies no operator, and KA runs as a launch of its own
  k_one          banded_qp(30000, nnz_per_row = 1, window = 40) with the diagonal of P alone: K = P + sigma I + A' rho A is diagonal, the Jacobi
                 preconditioner is its inverse, and every PCG takes ONE iteration (F_0, F_1, detect + KA) or none (19 945 PCG iterations in the
                 20 000 ADMM iterations it is given: 55 starts meet the tolerance)
"""
import functools
import hashlib
import os
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_amd
import problems

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')

_SETTINGS = dict(eps_abs=1e-6, eps_rel=1e-6, max_iter=20000, adaptive_rho_interval=50, check_termination=25, verbose=False)


# ------------------------------------------------------------------------------------------------ the problems
def _banded(n, diag_p=False, **kw):
    Pfull, q, A, l, u = problems.banded_qp(n, **kw)
    if diag_p:
        Pfull = sp.diags(Pfull.diagonal(), format='csc')
    return sp.triu(Pfull, format='csc'), q, sp.csc_matrix(A), l, u


def _primal_infeasible(n):
    """Row i repeated as row i + 1, with  A_i x = 1  against  A_i x = -1."""
    P, q, A, l, u = _banded(n)
    Ar = sp.csr_matrix(A)
    i = Ar.shape[0] // 2
    A = sp.vstack([Ar[:i + 1], Ar[i], Ar[i + 2:]]).tocsc()
    l, u = l.copy(), u.copy()
    l[i] = u[i] = 1.0
    l[i + 1] = u[i + 1] = -1.0
    return P, q, A, l, u


def _dual_infeasible(n):
    """Column j: no curvature (its entries of P set to zero, the pattern kept), every row of A that holds it free, q_j = -1: unbounded along e_j."""
    Pfull, q, A, l, u = problems.banded_qp(n)
    j = n // 2
    Pc = sp.csc_matrix(Pfull).copy()
    Pc.sort_indices()
    Pc.data[Pc.indptr[j]:Pc.indptr[j + 1]] = 0.0
    Pr = sp.csr_matrix(Pc)
    Pr.data[Pr.indptr[j]:Pr.indptr[j + 1]] = 0.0
    Ac = sp.csc_matrix(A)
    rows = Ac.indices[Ac.indptr[j]:Ac.indptr[j + 1]]
    l, u, q = l.copy(), u.copy(), q.copy()
    l[rows], u[rows], q[j] = -np.inf, np.inf, -1.0
    return sp.triu(sp.csc_matrix(Pr), format='csc'), q, Ac, l, u


# name -> (problem, settings, scenario, far columns, status of the last solve)
CASES = {
    'last_ka': (lambda: _banded(30000), dict(check_termination=1), 'solve', False, 'OSQP_SOLVED'),
    'mid_chunk': (lambda: _banded(30000), dict(max_iter=110), 'solve', False, 'OSQP_MAX_ITER_REACHED'),
    'two_blocks': (lambda: _banded(110000, window=40), {}, 'solve', False, 'OSQP_SOLVED'),
    'mix': (lambda: _banded(30000, long_range=0.02), {}, 'solve', True, 'OSQP_SOLVED'),
    'primal_inf': (lambda: _primal_infeasible(30000), {}, 'solve', False, 'OSQP_PRIMAL_INFEASIBLE'),
    'dual_inf': (lambda: _dual_infeasible(30000), {}, 'solve', False, 'OSQP_DUAL_INFEASIBLE'),
    'warm_update': (lambda: _banded(30000), {}, 'warm_update', False, 'OSQP_SOLVED'),
    'start_meets': (lambda: _banded(30000), {}, 'start_meets', False, 'OSQP_SOLVED'),
    'low_cap': (lambda: _banded(30000), dict(cg_max_iter=1, max_iter=200), 'solve', False, 'OSQP_MAX_ITER_REACHED'),
    'k_one': (lambda: _banded(30000, diag_p=True, nnz_per_row=1, window=40), {}, 'solve', False, 'OSQP_MAX_ITER_REACHED'),
}


@functools.lru_cache(maxsize=1)
def _problem(name):                                       # (built once for the two modes of a case)
    return CASES[name][0]()


# ------------------------------------------------------------------------------------------------ a case's record
def _sha(v):
    return None if v is None else hashlib.sha256(np.ascontiguousarray(v, dtype=np.float64).tobytes()).hexdigest()[:16]


def _digest(m, r):
    st = m._solver.hip_stats()
    return (int(r.info.status_val), int(r.info.iter), int(r.info.rho_updates), float(r.info.obj_val).hex(), _sha(r.x), _sha(r.y),
            _sha(r.prim_inf_cert), _sha(r.dual_inf_cert), int(st['pcg_iters_total']))


def record(name, graph):
    """The case on a fresh handle (one-launch form, graph replay or eager launches): (records of its solves, engine statistics of the handle)"""
    _, settings, scenario, _, _ = CASES[name]
    P, q, A, l, u = _problem(name)
    names = ('OSQP_HIP_F1', 'OSQP_HIP_GRAPH')
    old = {k: os.environ.get(k) for k in names}
    os.environ['OSQP_HIP_F1'], os.environ['OSQP_HIP_GRAPH'] = '1', '1' if graph else '0'
    try:
        st = dict(_SETTINGS)
        st.update(settings)
        m = osqp_amd.OSQP()
        m.setup(P, q, A, l, u, **st)
        first = m.solve()
        out = [_digest(m, first)]
        if scenario == 'warm_update':
            rng = np.random.default_rng(5)
            m.update(q=q + 0.05 * rng.standard_normal(len(q)), l=l - 0.1, u=u + 0.1)
            m.update_settings(warm_starting=True, polishing=True)
            out.append(_digest(m, m.solve()))
        elif scenario == 'start_meets':
            m.update_settings(warm_starting=True)
            m.warm_start(x=first.x, y=first.y)
            out.append(_digest(m, m.solve()))
        return tuple(out), m._solver.hip_stats()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# (status_val, iter, rho_updates, obj_val, sha256 x, sha256 y, sha256 prim_inf_cert, sha256 dual_inf_cert, pcg_iters_total) per solve
PARENT = {
    'dual_inf': ((5, 25, 0, '-0x1.93e5939a08ceap+99', 'b24052c9a086db1d', '9956b1d1755f08bc', '9956b1d1755f08bc', '25d0665b67af5069', 120),),
    'k_one': ((7, 20000, 6, '-0x1.5c8d5623a9fa0p+13', '149c80768a7332fb', '6ff537a69dba6dd2', '9956b1d1755f08bc', 'b24052c9a086db1d', 19945),),
    'last_ka': ((1, 320, 3, '-0x1.c24c8f9eaf6bbp+11', '78ead9b44c6dc50a', '7fda6a87b296d09a', '9956b1d1755f08bc', 'b24052c9a086db1d', 2089),),
    'low_cap': ((7, 200, 1, '-0x1.c24c904caf33dp+11', 'dbae5eb7f4c6cf9c', '650d22e9d375aa72', '9956b1d1755f08bc', 'b24052c9a086db1d', 950),),
    'mid_chunk': ((7, 110, 1, '-0x1.c25709d5c217fp+11', 'bfe729b947c20910', '55b848349fa3088d', '9956b1d1755f08bc', 'b24052c9a086db1d', 627),),
    'mix': ((1, 400, 3, '-0x1.bf1e2e88f86b8p+11', '511db72e3ae023db', '2102ac501fd4e9f3', '9956b1d1755f08bc', 'b24052c9a086db1d', 2017),),
    'primal_inf': ((3, 125, 2, '0x1.93e5939a08ceap+99', 'b24052c9a086db1d', '9956b1d1755f08bc', 'b97840f9f7726e67', 'b24052c9a086db1d', 960),),
    'start_meets': ((1, 375, 3, '-0x1.c24c8f87b32cdp+11', '4ab67fec8248e17d', '120e47fa4526568c', '9956b1d1755f08bc', 'b24052c9a086db1d', 1840), (1, 25, 0, '-0x1.c24c8f79c4b80p+11', 'cdb3a55e652b982f', '6c5fb7c469537b6a', '9956b1d1755f08bc', 'b24052c9a086db1d', 68)),
    'two_blocks': ((1, 825, 4, '-0x1.9a01f01cd0b7bp+13', '991f36eace8affb4', '786c6da6e97a9867', '6f064ebd6b0ea954', 'e6b6c706012bd255', 5037),),
    'warm_update': ((1, 375, 3, '-0x1.c24c8f87b32cdp+11', '4ab67fec8248e17d', '120e47fa4526568c', '9956b1d1755f08bc', 'b24052c9a086db1d', 1840), (1, 475, 3, '-0x1.3db474f32264cp+12', 'c897c89e294343d0', '7926b9f609316621', '9956b1d1755f08bc', 'b24052c9a086db1d', 1040)),
}


@pytest.mark.parametrize('graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('name', list(CASES))
def test_equals_parent_build(name, graph):
    _, settings, _, far, status = CASES[name]
    got, stats = record(name, graph)
    for k, rec in enumerate(got):
        print('%s %s solve %d: %r' % (name, 'graph' if graph else 'eager', k, rec))
    # the case runs what its name says
    assert int(stats['pcg_fused']) == 2 and 1 <= int(stats['f1_replicas']) <= 4, stats
    assert (stats['f1_far_columns'] > 0) == far, stats
    assert got[-1][0] == getattr(osqp_amd.SolverStatus, status)
    if name == 'k_one':
        assert int(stats['pcg_iters_max']) == 1 and 0 < got[0][8] < got[0][1], (stats, got)      # every PCG: one iteration, some: none
    if name == 'mid_chunk':
        assert got[0][1] == 110 and got[0][2] >= 1, got     # stopped off a chunk boundary, behind at least one rho update
    assert got == PARENT[name]
