"""GPU tier: the dense fp64 kernels of the device-factorised Woodbury correction (dense_hip.hip: strided GEMM on v_mfma_f64_16x16x4, block Gauss-Jordan
inverse of an SPD matrix) through the paths that use them -- the row-space and the column-space form of the correction (OSQPHipPolicy::woodbury_dual)
against the oracle; sizes that are no multiple of the 64 x 64 tile or of the 64-column block step, and one shape on the block boundaries (column-space
order 128 = two full block steps, row-space order 193 = three and a one-column tail).  These kernels are the only route: the retired switch
OSQPHipPolicy::woodbury_vendor (OSQP_HIP_WOODBURY_VENDOR=1) is accepted and changes nothing.  The inverse's lookahead stream and events belong to the
handle: two handles driven in turn from one thread, one of them destroyed on the way, each reproduce their solitary runs.
The kernels on their own: tests/test_gpu_dense_kernels.py."""
import contextlib
import os
import warnings

import numpy as np
import pytest

import osqp_amd
import problems
from oracle import Oracle, SOLVED

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _rel(a, b):
    return np.abs(a - b).max() / (1 + np.abs(b).max())


@pytest.mark.parametrize('nf,ns', [(150, 333), (301, 650), (128, 193)])
@pytest.mark.parametrize('dual', ['1', '0'])
def test_own_dense_kernels_equal_the_oracle_and_ignore_the_retired_vendor_switch(nf, ns, dual):
    P, q, A, l, u = problems.lasso_qp(nf, ns)
    xo, yo, io = Oracle().setup(P, q, A, l, u, eps_abs=1e-9, eps_rel=1e-9, max_iter=200000).solve()
    assert io.status_val == SOLVED
    res = {}
    for vendor in ('0', '1'):
        with _env(OSQP_HIP_WOODBURY_DUAL=dual, OSQP_HIP_WOODBURY_VENDOR=vendor):
            m = osqp_amd.OSQP()
            m.setup(P, q, A, l, u, eps_abs=1e-8, eps_rel=1e-8, verbose=False, max_iter=50000)
            r = m.solve(raise_error=True)
            res[vendor] = (r, m._solver.hip_stats(), m._solver.hip_preconditioner())
    for vendor in ('0', '1'):                                          # (the same route: the same stats and the same name)
        _, s, name = res[vendor]
        assert s['woodbury_rows'] == ns and s['woodbury_direct'] == 1, (vendor, s, name)
        assert (s['woodbury_dual_cols'] == nf) == (dual == '1')
        assert 'matrix cores' in name and 'vendor' not in name
    r0, r1 = res['0'][0], res['1'][0]
    assert _rel(r0.x, xo) < 5e-6 and _rel(r0.y, yo) < 2e-5
    print('retired switch: iter %d / %d, x %.3e, y %.3e, bitwise %s' % (r0.info.iter, r1.info.iter, _rel(r0.x, r1.x), _rel(r0.y, r1.y),
                                                                         np.array_equal(r0.x, r1.x) and np.array_equal(r0.y, r1.y)))
    assert r1.info.iter == r0.info.iter and _rel(r0.x, r1.x) < 1e-7 and _rel(r0.y, r1.y) < 1e-6


def test_two_handles_on_one_thread_each_own_their_lookahead_stream():
    """dense_spd_inverse's lookahead stream and its four events live in the handle (hip_common.h Impl::gj).  Two handles on one thread -- column space,
    order 128: two full block steps; row space, order 193: three and a one-column tail, so every factorisation runs a pivot on the auxiliary stream --
    are solved in turn, then one is destroyed and the other solved again: every solve reproduces the same solve of a handle that ran alone.  The
    cache of inverses is off, so that every cold solve factorises again (asserted)."""
    P, q, A, l, u = problems.lasso_qp(128, 193)

    def handle(dual):
        with _env(OSQP_HIP_WOODBURY_DUAL=dual, OSQP_HIP_WOODBURY_CACHE='0'):
            m = osqp_amd.OSQP()
            m.setup(P, q, A, l, u, eps_abs=1e-8, eps_rel=1e-8, verbose=False, max_iter=50000, warm_starting=False)
        return m

    def solve(m):                                                      # a cold solve: rho back to its initial value
        m.update_settings(rho=0.1)
        r = m.solve(raise_error=True)
        s = m._solver.hip_stats()
        assert s['woodbury_direct'] == 1 and s['woodbury_factorisations'] >= 1, s
        return r.info.iter, r.info.rho_updates, r.x.copy(), r.y.copy()

    alone = {}
    for dual, reps in (('1', 2), ('0', 3)):
        m = handle(dual)
        alone[dual] = [solve(m) for _ in range(reps)]
        del m
    a, b = handle('1'), handle('0')
    got = {'1': [], '0': []}
    for _ in range(2):
        got['1'].append(solve(a))
        got['0'].append(solve(b))
    del a                                                              # (osqp_cleanup: releases a's stream and events, not b's)
    got['0'].append(solve(b))
    for dual in ('1', '0'):
        for k, (g, w) in enumerate(zip(got[dual], alone[dual])):
            print('dual %s solve %d: iter %d / %d, rho updates %d / %d, x %.3e, y %.3e' % (dual, k, g[0], w[0], g[1], w[1], _rel(g[2], w[2]), _rel(g[3], w[3])))
            assert g[:2] == w[:2] and _rel(g[2], w[2]) < 1e-7 and _rel(g[3], w[3]) < 1e-6, (dual, k)
