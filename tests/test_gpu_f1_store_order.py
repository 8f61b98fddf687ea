"""GPU tier: f1_body (pcg_hip.hip) computes what it computed before the results of a block's own columns were taken out of flight at the stream wait:
x~, p, s, r (F_k) and r_0, x~_prev, x~ (F_0) of the own columns in the lanes' FIRST window element are held in registers and stored behind the
products phase, next to the request of the next block's stream, instead of in front of f1_stream_wait().  The own columns in the second window
element and those outside the window keep their stores, and so does f1_ka_body (its dx, x, x_g were tried the same way and put back); the KA cases
below are the record of the launches around the F body.

No value and no summation order changes, so every case compares with == : status, info.iter, info.rho_updates, float.hex(info.obj_val), the SHA-256 of
x and y and the solve's PCG iteration total -- for graph replay and for eager launches -- against PARENT.  PARENT was recorded on an MI355X from the
PARENT commit's build of the engine (that commit's library named in OSQP_HIP_LIBRARY, `record(name, graph)` of this file called for every case and both
modes, twice: both takes gave the same records); `_digest` is the whole of the comparison, so a record is re-taken the same way.

Cases -- the smallest shapes at which a deferred store can go wrong:
  one_block        banded_qp(30000), check_termination = 1: one row block per workgroup; F_0, F, detect + KA, every KA is a chunk's last
  mid_chunk        the same QP, check_termination = 25, adaptive_rho_interval = 50, max_iter = 110: KAs inside a chunk, and the SCATTER_ONLY chunk start,
                   which holds no own results and must still wait for its stream
  two_blocks       banded_qp(110000, window = 40): 2019 row blocks on 1024 workgroups -- a workgroup's first block is followed by another: the held
                   stores of block 1 leave before block 2's, next to the request of block 2's stream
  second_element   banded_qp(36000, m = 51400, window = 340) with the diagonal of P alone (test_gpu_f1_wave_trim's w448): gather windows of 340 - 479
                   columns, 140 own columns per block.  `_own_beyond` (the plan's windows recomputed on the CPU, as test_gpu_f1_wave_trim does) counts
                   the row blocks that hold an own column at window position >= 256, i.e. in a lane's SECOND window element: 256 of the 257 blocks
                   (the test prints and asserts the count) -- blocks whose own columns are partly held and partly stored at once; on one_block's
                   and two_blocks' QPs, as on the benchmark's, that count is 0 and all own columns are held
  mix              banded_qp(30000, long_range = 0.02): far columns (MIX instantiations)
  low_cap          cg_max_iter = 1: PCGs that end at their cap -- the vec_only launch, whose own columns all take the loop that kept its stores
  one_block_plain, two_blocks_plain
                   the two cases again with OSQP_HIP_F1_WT=0 set before setup (PARENT taken with the same setting): the WT = false instantiations
  warm_update      solve; update(q, l, u); solve with warm start and polish: the x, dx, x_g that KA leaves are read by the boundary and by polish
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
import test_gpu_f1_wave_trim as wave_trim

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')

_SETTINGS = dict(eps_abs=1e-6, eps_rel=1e-6, max_iter=20000, adaptive_rho_interval=50, check_termination=25, verbose=False)
_WIDE = dict(n=36000, m=51400, window=340, diag_p=True)     # test_gpu_f1_wave_trim CASES['w448']


def _banded(n, diag_p=False, **kw):
    Pfull, q, A, l, u = problems.banded_qp(n, **kw)
    if diag_p:
        Pfull = sp.diags(Pfull.diagonal(), format='csc')
    return sp.triu(Pfull, format='csc'), q, sp.csc_matrix(A), l, u


# name -> (problem, settings, scenario, far columns, write-through stores, status of the last solve)
CASES = {
    'one_block': (lambda: _banded(30000), dict(check_termination=1), 'solve', False, True, 'OSQP_SOLVED'),
    'mid_chunk': (lambda: _banded(30000), dict(max_iter=110), 'solve', False, True, 'OSQP_MAX_ITER_REACHED'),
    'two_blocks': (lambda: _banded(110000, window=40), {}, 'solve', False, True, 'OSQP_SOLVED'),
    'second_element': (lambda: _banded(**_WIDE), {}, 'solve', False, True, 'OSQP_SOLVED'),
    'mix': (lambda: _banded(30000, long_range=0.02), {}, 'solve', True, True, 'OSQP_SOLVED'),
    'low_cap': (lambda: _banded(30000), dict(cg_max_iter=1, max_iter=200), 'solve', False, True, 'OSQP_MAX_ITER_REACHED'),
    'one_block_plain': (lambda: _banded(30000), dict(check_termination=1), 'solve', False, False, 'OSQP_SOLVED'),
    'two_blocks_plain': (lambda: _banded(110000, window=40), {}, 'solve', False, False, 'OSQP_SOLVED'),
    'warm_update': (lambda: _banded(30000), {}, 'warm_update', False, True, 'OSQP_SOLVED'),
}


@functools.lru_cache(maxsize=1)
def _problem(name):                                       # (built once for the two modes of a case)
    return CASES[name][0]()


# ------------------------------------------------------------------------------------------------ own columns in the second window element
def _own_beyond(P, A, pos=256):
    """Engine::plan_f1 (strict windows, no far columns; test_gpu_f1_wave_trim._plan_on with the windows' origins kept): the number of row blocks that
    hold an own column at gather-window position >= pos, and the number of row blocks."""
    m, n = A.shape
    Ar = sp.csr_matrix(A); Ar.sort_indices()
    Pr = sp.csr_matrix(P); Pr.sort_indices()
    rp, rj = Ar.indptr, Ar.indices
    rb = wave_trim._blocks(rp, wave_trim._KCHUNK)
    if wave_trim._plan_on(rb, Ar, Pr, n, m) is None:       # Engine::setup: full blocks where the default ones need too many replicas
        rb = wave_trim._blocks(rp, wave_trim._F1CHUNK) if int(rp[-1]) > wave_trim._KGRID * wave_trim._F1CHUNK else wave_trim._blocks_target(rp, wave_trim._F1CHUNK - 24)
    pl = wave_trim._plan_on(rb, Ar, Pr, n, m)
    assert pl is not None
    nb = pl['nb']
    cs = np.concatenate([[0], np.cumsum(pl['own'])])
    prp, pcol = Pr.indptr, Pr.indices
    count = 0
    for b in range(nb):
        cols = rj[rp[rb[b]]:rp[rb[b + 1]]]
        lo, hi = cols.min(), cols.max()
        if cs[b + 1] > cs[b]:
            lo, hi = min(lo, cs[b]), max(hi, cs[b + 1] - 1)
        a0, wl = lo, hi - lo + 1
        assert wl == pl['scatter'][b]
        g0, g1 = a0, a0 + wl
        if prp[cs[b + 1]] > prp[cs[b]]:
            pc = pcol[prp[cs[b]]:prp[cs[b + 1]]]
            g0, g1 = min(g0, pc.min()), max(g1, pc.max() + 1)
        if g1 - g0 > wave_trim._F1WIN or 4 * (g1 - g0) > 5 * wl:
            g0, g1 = a0, a0 + wl
        assert g1 - g0 == pl['gather'][b]
        own_in = [j for j in (cs[b], cs[b + 1] - 1) if cs[b + 1] > cs[b] and g0 <= j < g1]
        count += any(j - g0 >= pos for j in own_in)
    return count, nb


# ------------------------------------------------------------------------------------------------ a case's record
def _sha(v):
    return None if v is None else hashlib.sha256(np.ascontiguousarray(v, dtype=np.float64).tobytes()).hexdigest()[:16]


def _digest(m, r):
    st = m._solver.hip_stats()
    return (int(r.info.status_val), int(r.info.iter), int(r.info.rho_updates), float(r.info.obj_val).hex(), _sha(r.x), _sha(r.y), int(st['pcg_iters_total']))


def record(name, graph):
    """The case on a fresh handle (one-launch form, graph replay or eager launches): (records of its solves, engine statistics of the handle)"""
    _, settings, scenario, _, wt, _ = CASES[name]
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
        out = [_digest(m, m.solve())]
        if scenario == 'warm_update':
            rng = np.random.default_rng(5)
            m.update(q=q + 0.05 * rng.standard_normal(len(q)), l=l - 0.1, u=u + 0.1)
            m.update_settings(warm_starting=True, polishing=True)
            out.append(_digest(m, m.solve()))
        return tuple(out), m._solver.hip_stats()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# (status_val, iter, rho_updates, obj_val, sha256 x, sha256 y, pcg_iters_total) per solve
PARENT = {
    'one_block': ((1, 320, 3, '-0x1.c24c8f9eaf6bbp+11', '78ead9b44c6dc50a', '7fda6a87b296d09a', 2089),),
    'mid_chunk': ((7, 110, 1, '-0x1.c25709d5c217fp+11', 'bfe729b947c20910', '55b848349fa3088d', 627),),
    'two_blocks': ((1, 825, 4, '-0x1.9a01f01cd0b7bp+13', '991f36eace8affb4', '786c6da6e97a9867', 5037),),
    'second_element': ((1, 300, 2, '-0x1.b16e77f0a650bp+12', 'f1a277c2e76e7fa4', '6e14ff8b1b485b5c', 1477),),
    'mix': ((1, 400, 3, '-0x1.bf1e2e88f86b8p+11', '511db72e3ae023db', '2102ac501fd4e9f3', 2017),),
    'low_cap': ((7, 200, 1, '-0x1.c24c904caf33dp+11', 'dbae5eb7f4c6cf9c', '650d22e9d375aa72', 950),),
    'one_block_plain': ((1, 320, 3, '-0x1.c24c8f9eaf6bbp+11', '78ead9b44c6dc50a', '7fda6a87b296d09a', 2089),),
    'two_blocks_plain': ((1, 825, 4, '-0x1.9a01f01cd0b7bp+13', '991f36eace8affb4', '786c6da6e97a9867', 5037),),
    'warm_update': ((1, 375, 3, '-0x1.c24c8f87b32cdp+11', '4ab67fec8248e17d', '120e47fa4526568c', 1840), (1, 475, 3, '-0x1.3db474f32264cp+12', 'c897c89e294343d0', '7926b9f609316621', 1040)),
}


@pytest.mark.parametrize('graph', [True, False], ids=['graph', 'eager'])
@pytest.mark.parametrize('name', list(CASES))
def test_equals_parent_build(name, graph):
    _, settings, _, far, _, status = CASES[name]
    got, stats = record(name, graph)
    for k, rec in enumerate(got):
        print('%s %s solve %d: %r' % (name, 'graph' if graph else 'eager', k, rec))
    # the case runs what its name says
    assert int(stats['pcg_fused']) == 2 and 1 <= int(stats['f1_replicas']) <= 4, stats
    assert (stats['f1_far_columns'] > 0) == far, stats
    assert got[-1][0] == getattr(osqp_amd.SolverStatus, status)
    if name == 'mid_chunk':
        assert got[0][1] == 110 and got[0][2] >= 1, got     # stopped off a chunk boundary, behind at least one rho update
    if name == 'second_element' and graph:
        P, _, A, _, _ = _problem(name)
        beyond, nb = _own_beyond(sp.csc_matrix(P + sp.triu(P, 1).T), A)
        print('second_element: %d of %d row blocks hold an own column at window position >= 256' % (beyond, nb))
        assert beyond > 0
    assert got == PARENT[name]
