"""GPU tier: the F launches of the one-launch form (pcg_hip.hip f1_iteration) compute what they computed before f1_fold_finish fetched its three
further inputs -- the PCG tolerance, gamma_{k-2}, alpha_{k-2} -- with scalar loads instead of vector loads behind the partials.  The values are the
same words of the same arrays: what can go wrong is a scalar cache that still holds an earlier launch's word (the tolerance is rewritten by F_1 of every
ADMM iteration, the history by every F_k), in graph replay or in eager launches.  The cases are also the record of the form that was measured and
dropped (DESIGN.md section 4.2 "The fold's scalars as scalar loads": the first block's requests ahead of the fold), whose failure modes they were
chosen for; that form passed them too.

No value and no summation order changes, so every case compares with == : status, info.iter, info.rho_updates, float.hex(info.obj_val), the SHA-256 of
x, y and the two certificates, and the solve's PCG iteration total -- for graph replay and for eager launches -- against PARENT.  PARENT was recorded
on an MI355X from the PARENT commit's build of the engine (that commit's library named in OSQP_HIP_LIBRARY, `record(name, graph)` of this file called
for every case and both modes, twice: both takes gave the same records); `_digest` is the whole of the comparison, so a record is re-taken the same way.

Cases:
  one_block        banded_qp(30000), check_termination = 1: one row block per workgroup (and workgroups without one); every F_k reads the tolerance that
                   F_1 of the same ADMM iteration wrote and the history its predecessors wrote
  mid_chunk        the same QP, max_iter = 110: the SCATTER_ONLY chunk start, then F_0, which has no fold
  two_blocks       banded_qp(110000, window = 40): 2019 row blocks on 1024 workgroups
  second_element   test_gpu_f1_wave_trim's w448 (gather windows of 340 - 479 columns): the lanes' second window element is real in every wave
  mix              banded_qp(30000, long_range = 0.02): far columns (MIX instantiations)
  low_cap          cg_max_iter = 1: PCGs that end at their cap -- F_1's fold sets the tolerance, the launch applies no operator, KA is a launch of its own
  k0               solve; warm start at the solution; solve (test_gpu_f1_ka_fused's start_meets): F_1's fold finds the START inside the tolerance and KA
                   runs in that launch
  k1               test_gpu_f1_ka_fused's k_one QP (every PCG takes one iteration or none), max_iter = 2000, then the same warm-started re-solve:
                   F_2's fold -- the first that reads the history -- says "converged" in every ADMM iteration
  one_block_plain  one_block with OSQP_HIP_F1_WT=0 set before setup (PARENT taken with the same setting): the WT = false instantiations
  d1, d2, d3       test_gpu_f1's problems for D = 1, 2, 3 replica vectors (the cases above run D = 2, 3 and 4): every instantiation
  warm_update      solve; update(q, l, u); solve with warm start and polish
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
_WIDE = dict(n=36000, m=51400, window=340, diag_p=True)     # test_gpu_f1_wave_trim CASES['w448']


def _banded(n, diag_p=False, **kw):
    Pfull, q, A, l, u = problems.banded_qp(n, **kw)
    if diag_p:
        Pfull = sp.diags(Pfull.diagonal(), format='csc')
    return sp.triu(Pfull, format='csc'), q, sp.csc_matrix(A), l, u


# name -> (problem, settings, scenario, far columns, write-through stores, replica count or None, status of the last solve)
CASES = {
    'one_block': (lambda: _banded(30000), dict(check_termination=1), 'solve', False, True, None, 'OSQP_SOLVED'),
    'mid_chunk': (lambda: _banded(30000), dict(max_iter=110), 'solve', False, True, None, 'OSQP_MAX_ITER_REACHED'),
    'two_blocks': (lambda: _banded(110000, window=40), {}, 'solve', False, True, None, 'OSQP_SOLVED'),
    'second_element': (lambda: _banded(**_WIDE), {}, 'solve', False, True, None, 'OSQP_SOLVED'),
    'mix': (lambda: _banded(30000, long_range=0.02), {}, 'solve', True, True, None, 'OSQP_SOLVED'),
    'low_cap': (lambda: _banded(30000), dict(cg_max_iter=1, max_iter=200), 'solve', False, True, None, 'OSQP_MAX_ITER_REACHED'),
    'k0': (lambda: _banded(30000), {}, 'start_meets', False, True, None, 'OSQP_SOLVED'),
    'k1': (lambda: _banded(30000, diag_p=True, nnz_per_row=1, window=40), dict(max_iter=2000), 'start_meets', False, True, None, 'OSQP_MAX_ITER_REACHED'),
    'one_block_plain': (lambda: _banded(30000), dict(check_termination=1), 'solve', False, False, None, 'OSQP_SOLVED'),
    'd1': (lambda: _banded(60000, m=60000, window=1, nnz_per_row=1), {}, 'solve', False, True, 1, 'OSQP_SOLVED'),
    'd2': (lambda: _banded(40000, m=80000, window=20, nnz_per_row=3), {}, 'solve', False, True, 2, 'OSQP_SOLVED'),
    'd3': (lambda: _banded(40000, m=80000, window=60, nnz_per_row=5), {}, 'solve', False, True, 3, 'OSQP_SOLVED'),
    'warm_update': (lambda: _banded(30000), {}, 'warm_update', False, True, None, 'OSQP_SOLVED'),
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
    _, settings, scenario, _, wt, _, _ = CASES[name]
    P, q, A, l, u = _problem(name)
    names = ('OSQP_HIP_F1', 'OSQP_HIP_GRAPH', 'OSQP_HIP_F1_WT')
    old = {k: os.environ.get(k) for k in names}
    os.environ['OSQP_HIP_F1'], os.environ['OSQP_HIP_GRAPH'] = '1', '1' if graph else '0'
    if not wt:
        os.environ['OSQP_HIP_F1_WT'] = '0'
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
    'one_block': ((1, 320, 3, '-0x1.c24c8f9eaf6bbp+11', '78ead9b44c6dc50a', '7fda6a87b296d09a', '9956b1d1755f08bc', 'b24052c9a086db1d', 2089),),
    'mid_chunk': ((7, 110, 1, '-0x1.c25709d5c217fp+11', 'bfe729b947c20910', '55b848349fa3088d', '9956b1d1755f08bc', 'b24052c9a086db1d', 627),),
    'two_blocks': ((1, 825, 4, '-0x1.9a01f01cd0b7bp+13', '991f36eace8affb4', '786c6da6e97a9867', '6f064ebd6b0ea954', 'e6b6c706012bd255', 5037),),
    'second_element': ((1, 300, 2, '-0x1.b16e77f0a650bp+12', 'f1a277c2e76e7fa4', '6e14ff8b1b485b5c', '6eccc856a2aeefec', '9dee687e0a46113c', 1477),),
    'mix': ((1, 400, 3, '-0x1.bf1e2e88f86b8p+11', '511db72e3ae023db', '2102ac501fd4e9f3', '9956b1d1755f08bc', 'b24052c9a086db1d', 2017),),
    'low_cap': ((7, 200, 1, '-0x1.c24c904caf33dp+11', 'dbae5eb7f4c6cf9c', '650d22e9d375aa72', '9956b1d1755f08bc', 'b24052c9a086db1d', 950),),
    'k0': ((1, 375, 3, '-0x1.c24c8f87b32cdp+11', '4ab67fec8248e17d', '120e47fa4526568c', '9956b1d1755f08bc', 'b24052c9a086db1d', 1840), (1, 25, 0, '-0x1.c24c8f79c4b80p+11', 'cdb3a55e652b982f', '6c5fb7c469537b6a', '9956b1d1755f08bc', 'b24052c9a086db1d', 68),),
    'k1': ((7, 2000, 6, '-0x1.5c8d5b2775530p+13', 'fa5a93af1ff3db94', 'fa9ec3d95b2c576b', '9956b1d1755f08bc', 'b24052c9a086db1d', 1945), (7, 2000, 0, '-0x1.5c8d5b10b0dd2p+13', 'b9345e45f14833e5', '4bdc442a3c9f23ce', '9956b1d1755f08bc', 'b24052c9a086db1d', 2000),),
    'one_block_plain': ((1, 320, 3, '-0x1.c24c8f9eaf6bbp+11', '78ead9b44c6dc50a', '7fda6a87b296d09a', '9956b1d1755f08bc', 'b24052c9a086db1d', 2089),),
    'd1': ((1, 175, 1, '-0x1.8fa422e1b98efp+14', '831d33ca5bba7573', '403242173003bf1c', '9956b1d1755f08bc', '9956b1d1755f08bc', 146),),
    'd2': ((1, 1550, 1, '-0x1.993cd901731d8p+12', '58889cdb6b3306a4', 'd6146ece843b36fb', '933e613d0f055580', '8b52f57a0c70b91c', 8578),),
    'd3': ((1, 575, 3, '-0x1.24cb1e478cd48p+12', '1a9e7f1dc5e001a5', 'ec47a4103b12a2f4', '933e613d0f055580', '8b52f57a0c70b91c', 3005),),
    'warm_update': ((1, 375, 3, '-0x1.c24c8f87b32cdp+11', '4ab67fec8248e17d', '120e47fa4526568c', '9956b1d1755f08bc', 'b24052c9a086db1d', 1840), (1, 475, 3, '-0x1.3db474f32264cp+12', 'c897c89e294343d0', '7926b9f609316621', '9956b1d1755f08bc', 'b24052c9a086db1d', 1040),),
}


@pytest.mark.parametrize('graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('name', list(CASES))
def test_equals_parent_build(name, graph):
    _, settings, _, far, _, D, status = CASES[name]
    got, stats = record(name, graph)
    for k, rec in enumerate(got):
        print('%s %s solve %d: %r' % (name, 'graph' if graph else 'eager', k, rec))
    # the case runs what its name says
    assert int(stats['pcg_fused']) == 2 and 1 <= int(stats['f1_replicas']) <= 4, stats
    assert D is None or int(stats['f1_replicas']) == D, stats
    assert (stats['f1_far_columns'] > 0) == far, stats
    assert got[-1][0] == getattr(osqp_amd.SolverStatus, status)
    if name == 'mid_chunk':
        assert got[0][1] == 110 and got[0][2] >= 1, got     # stopped off a chunk boundary, behind at least one rho update
    if name == 'low_cap':
        assert stats['pcg_unconverged'] > 0 or stats['cg_cap_escalations'] > 0, stats      # the cap did bind
    if name == 'k1':
        assert int(stats['pcg_iters_max']) == 1, stats        # every PCG: one iteration or none
    assert got == PARENT[name]
