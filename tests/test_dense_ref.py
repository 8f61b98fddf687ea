"""CPU tier of the dense kernel tests: the machinery of tests/test_gpu_dense_kernels.py (canvas packing, masks, references, bounds) on the host simulator's
plain-loop implementation of the same three routines (tests/hostsim/backend_host.cpp) -- every GEMM and symmetric case, every inverse order, the same
assertions -- and, without any library, the two facts the GPU tier's inverse bound rests on: the numpy emulation of the kernel's block algorithm keeps
n 2^-52 kappa on every (n, kappa) of the GPU test, and the np.longdouble reference meets its residual condition."""
import numpy as np
import pytest
import scipy.sparse as sp

import dense_ref as D
from hostsim_util import hostsim


@pytest.fixture(scope='module')
def solver():
    with hostsim():
        import osqp_amd
        m = osqp_amd.OSQP(algebra='hip')
        m.setup(sp.identity(4, format='csc'), np.ones(4), sp.identity(4, format='csc'), -np.ones(4), np.ones(4), verbose=False)
        yield m._solver


@pytest.mark.parametrize('colmajor', [False, True])
@pytest.mark.parametrize('layout', D.GEMM_LAYOUTS, ids=lambda l: 'A%s-B%s' % ('k' if l[0] else 'i', 'k' if l[1] else 'j'))
@pytest.mark.parametrize('shape', D.GEMM_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_gemm_machinery_on_plain_loops(solver, shape, layout, colmajor):
    for scalars in (D.GEMM_SCALARS[2:] if colmajor else D.GEMM_SCALARS):
        D.check_gemm(solver, shape, layout, scalars, colmajor)


def test_gemm_rejections_on_plain_loops(solver):
    D.check_gemm_rejects_bad_strides(solver)
    D.check_entry_rejects_operands_outside_their_buffers(solver)


@pytest.mark.parametrize('form', ['T', 'S'])
@pytest.mark.parametrize('N', D.SYM_N)
def test_sym_machinery_on_plain_loops(solver, N, form):
    for K in D.SYM_K:
        for pad in (0, 3):
            D.check_gemm_sym(solver, N, K, form, pad)


@pytest.mark.parametrize('kappa', D.INV_KAPPA)
@pytest.mark.parametrize('n', D.INV_N)
def test_inverse_machinery_on_plain_loops(solver, n, kappa):
    for pad in (0, 5):
        D.check_inverse(solver, n, kappa, pad)


@pytest.mark.parametrize('n', D.ILL_N)
def test_ill_conditioned_inverse_on_plain_loops(solver, n):
    D.check_inverse_ill_conditioned(solver, n)


@pytest.mark.parametrize('n,block', D.INDEFINITE)
def test_indefinite_is_reported_by_plain_loops(solver, n, block):
    D.check_indefinite(solver, n, block)


@pytest.mark.parametrize('kappa', D.INV_KAPPA)
@pytest.mark.parametrize('n', D.INV_N)
def test_block_emulation_keeps_the_inverse_bound(n, kappa):
    """The bound the GPU tier asserts is one the algorithm keeps in plain doubles (inverse_case asserts the reference's residual on the way): a failure
    here is the reference's or the bound's, never the kernel's."""
    A, Xref, piv, emu = D.inverse_case(n, kappa)
    assert emu <= D.inverse_bound(n, kappa) / 16, (emu, D.inverse_bound(n, kappa))
    X, minpiv = D.gj_emulate(A)
    assert (D.bits(X) == D.bits(X.T)).all()
    if n % D.NB == 0:                                          # (the emulation does not pad a partial block)
        D.assert_pivot(minpiv, A, piv, kappa)


def test_reference_residual_condition_and_pivots():
    """inverse_ref refuses a reference that is not 1000 x better than the tolerance it serves; pivots_ref and the indefinite generator agree on where the
    first negative pivot is."""
    A = D.spd(65, 1e4)
    X = D.inverse_ref(A, D.inverse_bound(65, 1e4))
    assert np.abs(np.eye(65) - np.asarray(A, dtype=np.longdouble) @ X).max() < 1e-3 * D.inverse_bound(65, 1e4)
    with pytest.raises(AssertionError):
        D.inverse_ref(A, 1e-19)
    for n, block in D.INDEFINITE:
        first = D.first_negative_pivot(D.indefinite(n, block))
        assert D.NB * block <= first < min(n, D.NB * (block + 1))
        assert not (D.gj_emulate(D.indefinite(n, block))[1] > 0)
    ref, mag = D.gemm_ref(np.ones((2, 3)), np.ones((3, 2)), np.full((2, 2), np.nan), 1.0, 0.0)
    assert (ref == 3).all() and (mag == 3).all()
