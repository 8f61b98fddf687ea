"""CPU tier: the references and the judge of tests/dense_kkt_ref.py, before they meet a kernel (tests/test_gpu_dense_kkt_kernels.py): a numpy stand-in of
the device's formation and apply passes the judge, and every planted mistake -- the ways such kernels go wrong -- is caught by it."""
import numpy as np
import pytest

import dense_kkt_ref as ref
import problems

SIGMA = 1e-6


def case(name):
    if name == 'random130':
        P, q, A, l, u = problems.random_qp(n=130, m=260, density=0.15)
    else:
        n = int(name)
        P, q, A, l, u = problems.banded_qp(n, window=min(20, n), seed=n)
    A = ref.with_duplicate(A, seed=5)
    n, m = P.shape[0], A.shape[0]
    rng = np.random.default_rng(11 + n)
    D, E, c = np.exp(0.3 * rng.standard_normal(n)), np.exp(0.3 * rng.standard_normal(m)), 0.7
    rho = ref.rho_vector(l, u, 0.1)
    return P, A, D, E, c, rho, rng.standard_normal(n), rng.standard_normal(n)


CASES = ['63', '65', 'random130']


@pytest.mark.parametrize('name', CASES)
def test_stand_in_passes_and_planted_formation_mistakes_are_caught(name):
    P, A, D, E, c, rho, r, xg = case(name)
    m = A.shape[0]
    KL = ref.form(P, A, D, E, c, SIGMA, rho)
    K64 = ref.form(P, A, D, E, c, SIGMA, rho, dtype=np.float64)
    assert (ref.bits(K64) != ref.bits(ref.form_device_order(P, A, D, E, c, SIGMA, rho))).any()      # (another order of operations: not the yardstick itself)
    ok, err, tol = ref.judge(ref.form_device_order(P, A, D, E, c, SIGMA, rho), KL, K64, m + 2)
    assert ok, (err, tol)
    for mistake in ref.FORM_MISTAKES:
        bad = ref.form(P, A, D, E, c, SIGMA, rho, dtype=np.float64, mistake=mistake)
        ok, err, tol = ref.judge(bad, KL, K64, m + 2)
        assert not ok, (mistake, err, tol)


@pytest.mark.parametrize('name', CASES)
def test_stand_in_passes_and_planted_apply_mistakes_are_caught(name):
    P, A, D, E, c, rho, r, xg = case(name)
    n = P.shape[0]
    KL = ref.form(P, A, D, E, c, SIGMA, rho)
    xL, uL = ref.apply(KL, r, xg)
    x64, u64 = ref.apply(KL, r, xg, dtype=np.float64)
    # the stand-in: the inverse of the fp64 K in the device's order of formation, applied row by row
    Kinv = np.linalg.inv(ref.form_device_order(P, A, D, E, c, SIGMA, rho))
    stand = xg + np.array([Kinv[i] @ r for i in range(n)])
    ok, err, tol = ref.judge(stand, xL, x64, n)
    assert ok, (err, tol)
    for mistake in ref.APPLY_MISTAKES:
        bad, _ = ref.apply(KL, r, xg, dtype=np.float64, mistake=mistake)
        ok, err, tol = ref.judge(bad, xL, x64, n)
        assert not ok, (mistake, err, tol)


def test_a_repeated_entry_is_stored_and_summed():
    P, q, A, l, u = problems.banded_qp(40, window=10, seed=1)
    B = ref.with_duplicate(A, seed=3)
    assert B.nnz == A.nnz + 1
    assert np.abs(ref.dense_stored(B, np.float64) - A.toarray()).max() <= 1e-15 * np.abs(A.toarray()).max()
    assert np.abs(ref.dense_stored(B, np.float64, overwrite=True) - A.toarray()).max() > 1e-3 * np.abs(A.data).min()
