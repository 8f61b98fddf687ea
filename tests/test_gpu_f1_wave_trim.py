"""GPU tier: the F1 bodies request, stage and sum per WAVE (pcg_hip.hip f1_body / f1_ka_body: a wave whose lanes would all be clamped for an element
of a stage issues nothing for it), and a replica's columns between its windows are zeroed once at setup instead of in every launch.

A wrong wave predicate shows where a window's width crosses a multiple of 64 lanes, not at the workload's size: the cases below are the smallest
F1-eligible problems whose gather / scatter widths fall on both sides of 128, 192, 256 and 320 columns, below 64 and beyond 448, with own-column
counts on both sides of 64 and 128, and two band-plus-long-range problems whose waves 2 - 3 are active through their far slots only.  `_plan`
recomputes the plan's widths on the CPU (Engine::plan_f1 without far columns) and the test checks it against what the engine reports.

Every case: the one-launch form is taken; it agrees with the two-kernel form; graph replay equals eager launches bit for bit; iteration count and
objective equal those of the build before this change (recorded on the same GPU type from the parent commit's build, compared with ==)."""
import os
import re
import tempfile
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_amd
import problems

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')

_SETTINGS = dict(eps_abs=1e-6, eps_rel=1e-6, max_iter=20000, adaptive_rho_interval=50, check_termination=25, verbose=False)
_KGRID, _KCHUNK, _F1CHUNK, _F1WIN, _F1MAXD = 1024, 2048, 1024, 512, 4          # backend.h


# ------------------------------------------------------------------------------------------------ the plan's widths, on the CPU
def _blocks_target(rp, target):                           # engine_internal.hpp build_row_blocks_target (no long rows here)
    m, rb, r = len(rp) - 1, [0], 0
    while r < m:
        start, acc = r, 0
        while r < m and r - start < 1024:
            l2 = rp[r + 1] - rp[r]
            if acc + l2 > target and r > start:
                break
            acc += l2; r += 1
        rb.append(r)
    return rb


def _blocks(rp, cap):                                     # build_row_blocks
    nnz = int(rp[-1]); k = max(1, (nnz + _KGRID * cap - 1) // (_KGRID * cap))
    while True:
        target = max(128, (nnz + _KGRID * k - 1) // (_KGRID * k))
        for _ in range(40):
            if target > cap:
                break
            rb = _blocks_target(rp, target)
            if len(rb) - 1 <= _KGRID * k:
                return rb
            target = min(cap + 1, target + max(1, target // 50))
        k += 1


def _plan_on(rb, A, P, n, m):                             # Engine::plan_f1, strict windows
    rp, rj, nb = A.indptr, A.indices, len(rb) - 1
    if nb < _KGRID // 4:
        return None
    lo0, hi0 = np.empty(nb, int), np.empty(nb, int)
    for b in range(nb):
        k0, k1 = rp[rb[b]], rp[rb[b + 1]]
        if rb[b + 1] - rb[b] > 512 or k1 - k0 > _F1CHUNK:
            return None
        lo0[b], hi0[b] = rj[k0:k1].min(), rj[k0:k1].max()
        if hi0[b] - lo0[b] + 1 > _F1WIN:
            return None
    cs = np.zeros(nb + 1, int)
    for g in range(1, nb):
        lo, up = max(cs[g - 1], min(lo0[g], n)), hi0[g - 1] + 1
        cs[g] = min(max(rb[g] * n // m, lo), up) if lo <= up else lo
        cs[g] = min(max(cs[g], cs[g - 1]), n)
    cs[nb] = n
    a0, wl = np.empty(nb, int), np.empty(nb, int)
    for b in range(nb):
        lo, hi = lo0[b], hi0[b]
        if cs[b + 1] > cs[b]:
            lo, hi = min(lo, cs[b]), max(hi, cs[b + 1] - 1)
        if hi - lo + 1 > _F1WIN:
            return None
        a0[b], wl[b] = lo, hi - lo + 1
    D = next((t for t in range(1, _F1MAXD + 1) if all(a0[g] + wl[g] <= a0[g + t] for g in range(nb - t))), 0)
    if not D:
        return None
    prp, pcol = P.indptr, P.indices
    if any(cs[b + 1] - cs[b] > 512 or prp[cs[b + 1]] - prp[cs[b]] > 256 for b in range(nb)):      # kF1MaxOwn, kF1PChunk
        return None
    gl = np.empty(nb, int)
    for b in range(nb):
        g0, g1 = a0[b], a0[b] + wl[b]
        if prp[cs[b + 1]] > prp[cs[b]]:
            pc = pcol[prp[cs[b]]:prp[cs[b + 1]]]
            g0, g1 = min(g0, pc.min()), max(g1, pc.max() + 1)
        if g1 - g0 > _F1WIN or 4 * (g1 - g0) > 5 * wl[b]:
            g0, g1 = a0[b], a0[b] + wl[b]
        gl[b] = g1 - g0
    return dict(nb=nb, D=D, gather=gl, scatter=wl, own=np.diff(cs))


def _plan(P, A):
    m, n = A.shape
    Ar = sp.csr_matrix(A); Ar.sort_indices()
    Pr = sp.csr_matrix(P); Pr.sort_indices()
    pl = _plan_on(_blocks(Ar.indptr, _KCHUNK), Ar, Pr, n, m)
    if pl is None:                                        # Engine::setup: full blocks where the default ones need too many replicas
        nnz = int(Ar.indptr[-1])
        rb = _blocks(Ar.indptr, _F1CHUNK) if nnz > _KGRID * _F1CHUNK else _blocks_target(Ar.indptr, _F1CHUNK - 24)
        pl = _plan_on(rb, Ar, Pr, n, m)
    return pl


# ------------------------------------------------------------------------------------------------ the cases
# name -> (banded_qp arguments, settings, {stage: widths that must fall on both sides of each listed boundary}, parent iter, parent obj_val)
# Widths (min / median / max over the row blocks, from _plan; printed by the test):
#   w64    gather  30 /  41 /  48   scatter  28 /  38 /  39   own  20
#   w128   gather  88 / 126 / 160   scatter  88 / 126 / 129   own  50
#   w192   gather 174 / 189 / 237   scatter 146 / 189 / 194   own 100
#   w256   gather 178 / 251 / 259   scatter 178 / 251 / 259   own 100
#   w320   gather 225 / 315 / 324   scatter 225 / 315 / 324   own 100   (the headline problem's regime: 196 / 290 / 363)
#   w448   gather 340 / 464 / 479   scatter 340 / 464 / 479   own 140
# (A block's own rows of P + sigma I hold at most 256 entries -- one per lane -- and banded_qp's P has two entries per column: more than 128 own
#  columns need a P of fewer entries.  w448 keeps the diagonal of the generator's P alone.)
CASES = {
    'w64': (dict(n=20000, window=20), {}, dict(below=64), 675, -2327.662528837834),
    'w128': (dict(n=20000, nnz_per_row=10, window=80), {}, dict(gather=[128], scatter=[128], own_below=64), 525, -1716.2818595676226),
    'w192': (dict(n=30000, window=95), {}, dict(gather=[192], scatter=[192], own_between=(64, 128)), 525, -3644.7343989110736),
    'w256': (dict(n=30000, window=160), {}, dict(gather=[256], scatter=[256]), 500, -3556.5554037324778),
    'w320': (dict(n=30000, window=225), {}, dict(gather=[320], scatter=[320]), 425, -3590.2516908208804),
    'w320_ka_heavy': (dict(n=30000, window=225), dict(check_termination=1), dict(gather=[320], scatter=[320]), 411, -3590.2516935911494),
    'w448': (dict(n=36000, m=51400, window=340, diag_p=True), {}, dict(above=448, own_above=128), 300, -6934.904282235783),
    'far_2pct': (dict(n=20000, window=40, long_range=0.02), {}, None, 350, -2419.349504658517),
    'far_02pct': (dict(n=20000, window=40, long_range=0.002), {}, None, 975, -2425.4431140085867),
}


def _problem(n, diag_p=False, **kw):
    """banded_qp as (full P, upper triangle of P, A, ...)"""
    Pfull, q, A, l, u = problems.banded_qp(n, **kw)
    if diag_p:
        Pfull = sp.diags(Pfull.diagonal(), format='csc')
    return Pfull, sp.triu(Pfull, format='csc'), q, sp.csc_matrix(A), l, u


def _handle(P, q, A, l, u, f1, graph, log=False, **kw):
    """A handle set up under the given form; log: the engine's own report of its plan (stderr, OSQP_HIP_SETUP_TIMING) is returned too."""
    names = ('OSQP_HIP_F1', 'OSQP_HIP_GRAPH', 'OSQP_HIP_SETUP_TIMING')
    old = {k: os.environ.get(k) for k in names}
    os.environ['OSQP_HIP_F1'] = '1' if f1 else '0'
    os.environ['OSQP_HIP_GRAPH'] = '1' if graph else '0'
    text = ''
    try:
        st = dict(_SETTINGS)
        st.update(kw)
        m = osqp_amd.OSQP()
        if not log:
            m.setup(P, q, A, l, u, **st)
        else:
            os.environ['OSQP_HIP_SETUP_TIMING'] = '1'
            with tempfile.TemporaryFile() as tf:
                keep = os.dup(2)
                os.dup2(tf.fileno(), 2)
                try:
                    m.setup(P, q, A, l, u, **st)
                finally:
                    os.dup2(keep, 2); os.close(keep)
                tf.seek(0)
                text = tf.read().decode(errors='replace')
        return (m, text) if log else m
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _rel(a, b):
    return np.abs(a - b).max() / (1 + np.abs(b).max())


def _fmt(v):
    return '%d / %d / %d' % (v.min(), np.median(v), v.max())


def _check_coverage(name, pl, want, report):
    """The case does fall where its name says (the CPU plan), and the CPU plan is the engine's (block count, replicas, widest scatter window, means)."""
    print('%s: %d row blocks, D = %d, gather %s, scatter %s, own %s (min / median / max)' % (name, pl['nb'], pl['D'], _fmt(pl['gather']), _fmt(pl['scatter']), _fmt(pl['own'])))
    mt = re.search(r'F1 plan: (\d+) row blocks, D = (\d+), scatter window ([\d.]+) columns on average \(max (\d+)\), gather window ([\d.]+), own columns ([\d.]+)', report)
    assert mt, report
    print('%s: engine: %s' % (name, mt.group(0)))
    assert (int(mt.group(1)), int(mt.group(2)), int(mt.group(4))) == (pl['nb'], pl['D'], pl['scatter'].max())
    assert abs(float(mt.group(3)) - pl['scatter'].mean()) < 0.06 and abs(float(mt.group(5)) - pl['gather'].mean()) < 0.06 and abs(float(mt.group(6)) - pl['own'].mean()) < 0.06
    both = np.concatenate([pl['gather'], pl['scatter']])
    if 'below' in want:
        assert both.max() <= want['below']
    if 'above' in want:
        assert np.median(pl['gather']) > want['above'] and np.median(pl['scatter']) > want['above']
    for stage in ('gather', 'scatter'):
        for edge in want.get(stage, []):
            assert pl[stage].min() < edge < pl[stage].max(), (stage, edge)
    if 'own_below' in want:
        assert pl['own'].max() < want['own_below']
    if 'own_between' in want:
        assert want['own_between'][0] < np.median(pl['own']) < want['own_between'][1]
    if 'own_above' in want:
        assert np.median(pl['own']) > want['own_above']


@pytest.mark.parametrize('name', list(CASES))
def test_wave_trim_case(name):
    args, settings, want, parent_iter, parent_obj = CASES[name]
    Pfull, P, q, A, l, u = _problem(**args)
    (mg, report), me, m0 = _handle(P, q, A, l, u, True, True, log=True, **settings), _handle(P, q, A, l, u, True, False, **settings), _handle(P, q, A, l, u, False, True, **settings)
    sg, s0 = mg._solver.hip_stats(), m0._solver.hip_stats()
    assert int(sg['pcg_fused']) == 2 and 1 <= int(sg['f1_replicas']) <= 4, sg
    assert int(s0['pcg_fused']) == 1 and int(s0['f1_replicas']) == 0
    if want is None:
        print('%s: engine: %s' % (name, ' '.join(ln for ln in report.splitlines() if 'F1 plan' in ln)))
        assert sg['f1_far_columns'] > 0, sg                # per-block mixing: far slots in the lanes of waves 2 - 3
    else:
        assert sg['f1_far_columns'] == 0, sg
        _check_coverage(name, _plan(Pfull, A), want, report)
    rg, re_, r0 = mg.solve(), me.solve(), m0.solve()
    print('%s: F1 iter %d obj_val %r; two-kernel iter %d; |dx| %.2e |dy| %.2e' % (name, rg.info.iter, rg.info.obj_val, r0.info.iter, _rel(rg.x, r0.x), _rel(rg.y, r0.y)))
    assert rg.info.status_val == r0.info.status_val == osqp_amd.SolverStatus.OSQP_SOLVED
    # the two-kernel form
    assert rg.info.iter == r0.info.iter
    assert _rel(rg.x, r0.x) < 1e-4 and _rel(rg.y, r0.y) < 1e-4          # (tests/test_gpu_f1.py: two iterates that both stopped at residuals <= 1e-6)
    # graph replay against eager launches
    assert rg.info.iter == re_.info.iter and rg.info.obj_val == re_.info.obj_val
    assert np.array_equal(rg.x, re_.x) and np.array_equal(rg.y, re_.y)
    # the parent commit's build
    assert rg.info.iter == parent_iter
    assert rg.info.obj_val == parent_obj


def test_replica_gaps_stay_zero_through_updates_and_a_warm_start():
    """The replicas' gaps are zeroed at setup alone: a second solve on the same handle -- after new values of A, a new rho and a warm start, through
    the strings captured by the first -- equals the same sequence on a fresh handle with eager launches, bit for bit."""
    P, q, A, l, u = problems.banded_qp(30000, window=225)
    P, A = sp.triu(P, format='csc'), sp.csc_matrix(A)
    rng = np.random.default_rng(11)
    Ax = A.data * (1.0 + 0.05 * rng.standard_normal(A.nnz))
    x0, y0 = 0.1 * rng.standard_normal(A.shape[1]), 0.1 * rng.standard_normal(A.shape[0])
    out = []
    for graph in (True, False):
        m = _handle(P, q, A, l, u, True, graph, adaptive_rho=False)
        assert int(m._solver.hip_stats()['pcg_fused']) == 2
        first = m.solve()
        m.update(Ax=Ax)
        m.update_settings(rho=0.4)
        m.warm_start(x=x0, y=y0)
        out.append((first, m.solve()))
    for a, b in zip(out[0], out[1]):
        assert a.info.status_val == osqp_amd.SolverStatus.OSQP_SOLVED
        assert a.info.iter == b.info.iter and a.info.obj_val == b.info.obj_val
        assert np.array_equal(a.x, b.x) and np.array_equal(a.y, b.y)
    assert out[0][0].info.obj_val != out[0][1].info.obj_val          # (the update did change the problem)
