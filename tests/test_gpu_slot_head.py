"""GPU tier: the F1 slot kernel's head as kernel arguments (pcg_hip.hip k_slot1: the stream, the block records, nblk, the parity, the
partials, the phase records and the device copy of Dev).  Captured strings bake those arguments in; every solve through them must equal
the same solve with graphs off, bit for bit -- on fresh handles and after rho, settings and matrix-value updates on the same handle."""
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


def _handle(P, q, A, l, u, graph, **kw):
    old = {k: os.environ.get(k) for k in ('OSQP_HIP_F1', 'OSQP_HIP_GRAPH')}
    os.environ['OSQP_HIP_F1'] = '1'
    os.environ['OSQP_HIP_GRAPH'] = '1' if graph else '0'
    try:
        st = dict(_SETTINGS)
        st.update(kw)
        m = osqp_amd.OSQP(); m.setup(P, q, A, l, u, **st)
        return m
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _same(ra, rb):
    assert ra.info.iter == rb.info.iter
    assert np.array_equal(ra.x, rb.x) and np.array_equal(ra.y, rb.y)
    assert ra.info.obj_val == rb.info.obj_val


def _problem(kind):
    if kind == 'banded':
        P, q, A, l, u = problems.banded_qp(30000, window=40)
    elif kind == 'mixed':
        P, q, A, l, u = problems.banded_qp(60000, window=120, long_range=0.02)
    else:
        P, q, A, l, u = problems.banded_qp(100000, window=200)          # configs[1]
    return sp.triu(P, format='csc'), q, sp.csc_matrix(A), l, u


@pytest.mark.parametrize('kind', ['banded', 'mixed', 'wide'])
def test_slot_head_graph_matches_eager(kind):
    P, q, A, l, u = _problem(kind)
    mg, me = _handle(P, q, A, l, u, True), _handle(P, q, A, l, u, False)
    sg = mg._solver.hip_stats()
    assert int(sg['pcg_fused']) == 2 and 1 <= int(sg['f1_replicas']) <= 4, sg
    if kind == 'mixed':
        assert sg['f1_far_columns'] > 0, sg                # per-block mixing (MIX) on
    rg, re_ = mg.solve(), me.solve()
    assert rg.info.status_val == osqp_amd.SolverStatus.OSQP_SOLVED
    _same(rg, re_)
    _same(mg.solve(), me.solve())                         # a second solve replays the strings captured by the first


def test_slot_head_updates_graph_matches_eager():
    # the same sequence of updates on a handle with captured strings and on one without: a stale argument in a string would show here
    P, q, A, l, u = _problem('banded')
    hs = [_handle(P, q, A, l, u, g, adaptive_rho=False) for g in (True, False)]
    assert int(hs[0]._solver.hip_stats()['pcg_fused']) == 2
    rng = np.random.default_rng(7)
    Ax = A.data * (1.0 + 0.05 * rng.standard_normal(A.nnz))
    Px = P.data * (1.0 + 0.05 * rng.random(P.nnz))
    steps = [lambda m: None,
             lambda m: m.update_settings(rho=0.5),
             lambda m: m.update_settings(alpha=1.4, check_termination=10),
             lambda m: m.update(Ax=Ax),
             lambda m: m.update(Px=Px)]
    for step in steps:
        res = []
        for m in hs:
            step(m)
            res.append(m.solve())
        assert res[0].info.status_val == osqp_amd.SolverStatus.OSQP_SOLVED
        _same(res[0], res[1])
    # and the last state against a fresh handle of the same data and settings (a different start: close, not identical)
    Ab, Pb = A.copy(), P.copy()
    Ab.data, Pb.data = Ax, Px
    mf = _handle(Pb, q, Ab, l, u, True, adaptive_rho=False, rho=0.5, alpha=1.4, check_termination=10)
    rf = mf.solve()
    assert rf.info.status_val == osqp_amd.SolverStatus.OSQP_SOLVED
    assert np.abs(rf.x - res[0].x).max() / (1 + np.abs(rf.x).max()) < 1e-4


# KA-heavy: a termination check after every ADMM iteration, so that every KA launch's outputs are read back at once.  The iteration
# count and objective are those of the build before the head moved into kernel arguments (same GPU, same inputs).
KA_HEAVY_ITER = 533
KA_HEAVY_OBJ = -3595.406663755929


def test_slot_head_ka_heavy_matches_parent():
    P, q, A, l, u = _problem('banded')
    mg, me = _handle(P, q, A, l, u, True, check_termination=1), _handle(P, q, A, l, u, False, check_termination=1)
    rg, re_ = mg.solve(), me.solve()
    assert rg.info.status_val == osqp_amd.SolverStatus.OSQP_SOLVED
    _same(rg, re_)
    assert rg.info.iter == KA_HEAVY_ITER
    assert rg.info.obj_val == KA_HEAVY_OBJ
