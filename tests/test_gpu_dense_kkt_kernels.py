"""GPU tier: the kernels of the dense KKT mode (osqp-python_amd/csrc/densekkt_hip.hip) through osqp_hip_test_dense_kkt -- the formation of K and the hot
path x~ = x_g + K^-1 r_0 against the long-double restatement of tests/dense_kkt_ref.py, judged by its rule (64 x the error of an fp64 numpy evaluation of
the same quantity).  Sizes on both sides of the inverse's 64-column block, even n (16-byte loads, two rows per workgroup) and odd n (8-byte loads, a last
row without a partner), one unstructured problem, a handle whose A stores an entry twice, a handle after update_data_mat."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_amd
import problems
import dense_kkt_ref as ref

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
ST = dict(eps_abs=1e-6, eps_rel=1e-6, max_iter=20000, adaptive_rho_interval=50, check_termination=25, verbose=False)
SIGMA = 1e-6                                     # the default setting
VALIDATION, NOT_IMPLEMENTED = 1, 10

CASES = {
    'banded63': lambda: problems.banded_qp(63, window=16, seed=63),
    'banded64': lambda: problems.banded_qp(64, window=16, seed=64),
    'banded65': lambda: problems.banded_qp(65, window=16, seed=65),
    'banded130': lambda: problems.banded_qp(130, window=30, seed=130),
    'banded257': lambda: problems.banded_qp(257, window=40, seed=257),
    'random130': lambda: problems.random_qp(n=130, m=260, density=0.15),
}


def enabled(P, q, A, l, u):
    m = osqp_amd.OSQP(algebra='hip'); m.setup(P, q, A, l, u, **ST)
    assert m._solver.hip_dense_kkt(True) == 0
    return m


def engine_order(m):
    pc, pr = m._solver.hip_get_reordering()
    return np.asarray(pc, dtype=np.int64), np.asarray(pr, dtype=np.int64)[:m._solver.m]


def check_form(m, P, A):
    """FORM against the reference; returns (K as the device formed it, the long-double K), both in the engine's numbering."""
    s = m._solver
    n, mm = s.n, s.m
    st, out = s.hip_test_dense_kkt('form')
    assert st == 0 and out['order'] == n
    assert np.isnan(out['K'][n * n:]).all() and np.isnan(out['rho'][mm:]).all()          # exactly the listed counts are written
    K, rho_e = out['K'][:n * n].reshape(n, n), out['rho'][:mm]
    pc, pr = engine_order(m)
    rho = np.empty(mm); rho[pr] = rho_e
    assert np.isfinite(rho).all() and (rho > 0).all()
    D, E, c = s.hip_scaling()
    KL = ref.form(P, A, D, E, c, SIGMA, rho)[np.ix_(pc, pc)]
    K64 = ref.form(P, A, D, E, c, SIGMA, rho, dtype=np.float64)[np.ix_(pc, pc)]
    ok, err, tol = ref.judge(K, KL, K64, mm + 2)
    print('form n=%d m=%d: error %.3e, tolerance %.3e' % (n, mm, err, tol))
    assert ok, (err, tol)
    assert (ref.bits(K) == ref.bits(K.T)).all(), 'K is not bitwise symmetric'
    return K, KL


def check_apply(m, KL, seed=0):
    s = m._solver
    n = s.n
    rng = np.random.default_rng(1000 + n + seed)
    r, xg = rng.standard_normal(n), rng.standard_normal(n)
    st, out = s.hip_test_dense_kkt('apply', r=r, xg=xg)
    assert st == 0 and out['state'] == 1
    assert np.isnan(out['xs'][n:]).all() and np.isnan(out['u'][n:]).all()
    assert out['done'] == 1 and out['iters'] == 0                                          # a converged solve of no PCG iteration
    xs, u = out['xs'][:n], out['u'][:n]
    xL, uL = ref.apply(KL, r, xg)
    x64, u64 = ref.apply(KL, r, xg, dtype=np.float64)
    for what, dev, lo, f64 in (('x~', xs, xL, x64), ('u', u, uL, u64)):
        ok, err, tol = ref.judge(dev, lo, f64, n)
        print('apply n=%d %s: error %.3e, tolerance %.3e' % (n, what, err, tol))
        assert ok, (what, err, tol)
    assert (ref.bits(xs) == ref.bits(xg + u)).all()                                        # x~ = x_g + u, one rounding
    return xs


@pytest.mark.parametrize('name', list(CASES))
def test_form_and_apply_against_the_long_double_reference(name):
    P, q, A, l, u = CASES[name]()
    m = enabled(P, q, A, l, u)
    rec = m._solver.hip_dense_kkt_record()
    assert rec['state'] == 1 and rec['order'] == P.shape[0] and rec['factorisations'] == 1 and rec['min_pivot'] > 0 and rec['probe'] <= 1e-6
    K, KL = check_form(m, P, A)
    check_apply(m, KL)
    assert m._solver.hip_dense_kkt_record()['factorisations'] == 1                         # (the diagnostic re-factorisation is not one of the handle's)


def test_a_repeated_entry_of_A_adds_up():
    P, q, A, l, u = problems.banded_qp(65, window=16, seed=7)
    Adup = ref.with_duplicate(A, seed=2)
    m = osqp_amd.OSQP(algebra='hip'); m.setup(P, q, Adup, l, u, **ST)                      # (the front end hands stored entries through as they are)
    assert m._solver.hip_dense_kkt(True) == 0
    K, KL = check_form(m, P, Adup)
    K1, _ = check_form(enabled(P, q, A, l, u), P, A)
    assert np.abs(K - K1).max() <= 1e-13 * np.abs(K1).max()                                # the same matrix, stored differently
    check_apply(m, KL)


def test_update_data_mat_refactorises_from_the_new_values():
    P, q, A, l, u = problems.banded_qp(130, window=30, seed=11)
    m = enabled(P, q, A, l, u)
    Pu = sp.triu(P, format='csc')
    m.update(Px=1.1 * Pu.data, Ax=1.1 * A.data)
    rec = m._solver.hip_dense_kkt_record()
    assert rec['state'] == 1 and rec['factorisations'] == 2
    K, KL = check_form(m, 1.1 * P, 1.1 * A)
    check_apply(m, KL)


@pytest.mark.parametrize('name', ['banded64', 'banded65'])
def test_two_factorisations_of_the_same_data_are_bit_identical(name):
    P, q, A, l, u = CASES[name]()
    m = enabled(P, q, A, l, u)
    n = P.shape[0]
    rng = np.random.default_rng(5)
    r, xg = rng.standard_normal(n), rng.standard_normal(n)
    got = []
    for _ in range(2):
        st, f = m._solver.hip_test_dense_kkt('form')
        st2, a = m._solver.hip_test_dense_kkt('apply', r=r, xg=xg)                         # (the inverse, seen through its product with a fixed vector)
        st3, p = m._solver.hip_test_dense_kkt('probe')
        assert st == st2 == st3 == 0
        got.append((ref.bits(f['K'][:n * n]), ref.bits(a['xs'][:n]), ref.bits(a['u'][:n]), f['minpiv'], p['probe']))
    for x, y in zip(*got):
        assert np.array_equal(x, y)
    assert got[0][4] == m._solver.hip_dense_kkt_record()['probe'] <= 1e-6                  # PROBE repeats the factorisation's own probe


def test_entry_validates_before_any_launch_and_leaves_the_handle_as_it_was():
    P, q, A, l, u = CASES['banded65']()
    a, b = enabled(P, q, A, l, u), enabled(P, q, A, l, u)
    s, n = a._solver, P.shape[0]
    r = np.ones(n)
    assert s.hip_test_dense_kkt(3)[0] == VALIDATION and s.hip_test_dense_kkt(-1)[0] == VALIDATION
    for bad in (dict(k_len=n * n), dict(rho_len=0), dict(r_len=n), dict(xs_len=n + 16)):
        assert s.hip_test_dense_kkt('form', lens=bad)[0] == VALIDATION, bad
    for bad in (dict(r_len=n - 1), dict(xg_len=n + 1), dict(xs_len=n), dict(u_len=n + 17), dict(k_len=16)):
        assert s.hip_test_dense_kkt('apply', r=r, xg=r, lens=bad)[0] == VALIDATION, bad
    assert s.hip_test_dense_kkt('apply', r=r)[0] == VALIDATION                              # x_g missing
    assert s.hip_test_dense_kkt('probe', r=r)[0] == VALIDATION
    off = osqp_amd.OSQP(algebra='hip'); off.setup(P, q, A, l, u, **ST)
    assert off._solver.hip_test_dense_kkt('probe')[0] == NOT_IMPLEMENTED                   # the mode is off
    # every op on a, none on b: the solves that follow are the same solve
    for op, kw in (('form', {}), ('apply', dict(r=r, xg=2 * r)), ('probe', {})):
        assert s.hip_test_dense_kkt(op, **kw)[0] == 0
    ra, rb = a.solve(), b.solve()
    assert ra.info.status_val == rb.info.status_val == 1 and ra.info.iter == rb.info.iter
    assert np.array_equal(ra.x, rb.x) and np.array_equal(ra.y, rb.y)
