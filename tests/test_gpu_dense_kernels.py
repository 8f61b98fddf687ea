"""GPU tier, kernel level: the dense fp64 routines of osqp-python_amd/csrc/dense_hip.hip -- the strided v_mfma_f64_16x16x4 GEMM in its four operand layouts,
the upper-tiles-plus-mirror symmetric form, the block Gauss-Jordan inverse with its pivot running ahead on a second stream -- on test data through the
diagnostic entry osqp_hip_test_dense, against np.longdouble references (tests/dense_ref.py: cases, canvases, bounds and where each bound comes from).
tests/test_gpu_dense.py reaches the same kernels only through whole ADMM solves, which forgive a lot; tests/test_dense_ref.py proves this file's machinery
on plain loops.

Smallest pivot: the cases are SPD with eigenvalues in [1, kappa], so every pivot of the elimination is >= 1; `minpiv <= min(1, max diag A)` can therefore
hold only where a partial block brings the identity padding's pivot 1 in (n no multiple of 64).  For n = 64, 128, 256 the test asks minpiv <= max diag A,
and for every n that minpiv equals the smallest pivot of an exact elimination (np.longdouble) within n 2^-52 kappa -- sharper than either bound."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import dense_ref as D

pytestmark = pytest.mark.gpu


def _handle():
    import osqp_amd
    m = osqp_amd.OSQP(algebra='hip')
    m.setup(sp.identity(4, format='csc'), np.ones(4), sp.identity(4, format='csc'), -np.ones(4), np.ones(4), verbose=False)
    return m


@pytest.fixture(scope='module')
def solver():
    m = _handle()
    yield m._solver


_layout_id = lambda l: 'A%s-B%s' % ('k' if l[0] else 'i', 'k' if l[1] else 'j')       # noqa: E731


@pytest.mark.parametrize('scalars', D.GEMM_SCALARS, ids=lambda s: 'alpha%g-beta%g' % s)
@pytest.mark.parametrize('layout', D.GEMM_LAYOUTS, ids=_layout_id)
@pytest.mark.parametrize('shape', D.GEMM_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_gemm_componentwise_in_nan_and_sentinel_canvases(solver, shape, layout, scalars):
    D.check_gemm(solver, shape, layout, scalars)


@pytest.mark.parametrize('layout', D.GEMM_LAYOUTS, ids=_layout_id)
@pytest.mark.parametrize('shape', D.GEMM_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_gemm_column_major_result(solver, shape, layout):
    D.check_gemm(solver, shape, layout, D.GEMM_SCALARS[2], colmajor=True)


def test_gemm_rejects_operands_without_a_unit_stride(solver):
    D.check_gemm_rejects_bad_strides(solver)
    D.check_entry_rejects_operands_outside_their_buffers(solver)


@pytest.mark.parametrize('pad', [0, 3], ids=['ld=N', 'ld=N+3'])
@pytest.mark.parametrize('form', ['T', 'S'], ids=["T=W'W", "S=WW'"])
@pytest.mark.parametrize('K', D.SYM_K)
@pytest.mark.parametrize('N', D.SYM_N)
def test_gemm_sym_bound_bitwise_symmetry_and_canvas(solver, N, K, form, pad):
    D.check_gemm_sym(solver, N, K, form, pad)


@pytest.mark.parametrize('pad', [0, 5], ids=['ld=n', 'ld=n+5'])
@pytest.mark.parametrize('kappa', D.INV_KAPPA)
@pytest.mark.parametrize('n', D.INV_N)
def test_spd_inverse_accuracy_symmetry_padding_and_pivot(solver, n, kappa, pad):
    D.check_inverse(solver, n, kappa, pad)


@pytest.mark.parametrize('n', D.ILL_N)
def test_spd_inverse_ill_conditioned_against_the_algorithms_own_error(solver, n):
    """kappa = 1e8.  Measured on an MI355X (kernel / numpy emulation of the same block elimination): n = 65: 1.02e-04 / 1.20e-04; n = 200: 2.6e-08 / 2.8e-08
    (DESIGN.md section 6)."""
    D.check_inverse_ill_conditioned(solver, n)


@pytest.mark.parametrize('n,block', D.INDEFINITE, ids=['block0', 'block2-second-stream', 'one-column-tail'])
def test_spd_inverse_reports_a_matrix_that_is_not_positive_definite(solver, n, block):
    D.check_indefinite(solver, n, block)


def _lookahead_child():
    """Runs in the child process of the test below (OSQP_HIP_GJ_LOOKAHEAD=0 is read once per process): the pivot block inverted in line, on one stream."""
    s = _handle()._solver
    out = {'errors': {str(n): D.check_inverse(s, n, 1e4, 0) for n in D.LOOKAHEAD_N}, 'indefinite_minpiv': D.check_indefinite(s, 200, 2)}
    print('RESULT ' + json.dumps(out))


def test_spd_inverse_without_lookahead_in_one_child_process():
    env = dict(os.environ, OSQP_HIP_GJ_LOOKAHEAD='0', PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    r = subprocess.run([sys.executable, '-c', 'import test_gpu_dense_kernels as t; t._lookahead_child()'], env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')][-1][7:])
    for n in D.LOOKAHEAD_N:
        assert res['errors'][str(n)] <= D.inverse_bound(n, 1e4), (n, res)
    assert not (res['indefinite_minpiv'] > 0), res
