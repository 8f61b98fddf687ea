"""CPU tier: osqp-python_amd/csrc/step_rules.h -- the row class and rho, the finite-side predicates, the load scaling, the z / y and x steps, the
residual rows and the polish / adjoint rules that the batch kernels, the single-QP kernels and the host driver share -- behind
tests/hostsim/step_probe.cpp.  The probe is built with -ffp-contract=off, and what is expected is restated HERE from the reference's
description with the same order of operations (_osqp.py:505-522 set_rho_vec, :660-703 update_x / project / update_z / update_y, :728-846 the
residuals and infeasibility terms, :1328 / :1357-1358 / :1505-1506 the scaling of q, l, u, x, y, :1719-1720 the active set, :1773-1793 the
normal cone and the accept test): every comparison is ==, never a tolerance."""
import ctypes as C
from fractions import Fraction
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'hostsim', 'step_probe.cpp')
OUT = os.path.join(ROOT, 'tests', '_build', 'libstep_probe.so')
DEPS = [SRC] + [os.path.join(ROOT, 'osqp-python_amd', 'csrc', h) for h in ('step_rules.h', 'term_rules.h')] + [os.path.join(ROOT, 'include', 'osqp_hip.h')]

# _osqp.py:25-45
RHO_MIN, RHO_EQ_OVER_RHO_INEQ, RHO_TOL, OSQP_INFTY, MIN_SCALING = 1e-06, 1e03, 1e-04, 1e30, 1e-04
FIELDS = ('pri_u ax_u z_u pri_s ax_s z_s dy_u dy_s pinf_lhs dua_u px_u aty_u dua_s px_s aty_s dxn_u dxn_s qn_u qn_s xpx qx qdx').split()
D_ = C.c_double
DP = C.POINTER(D_)


@pytest.fixture(scope='module')
def lib():
    if not (os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(f) for f in DEPS)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'include'), '-o', OUT, SRC])
    L = C.CDLL(OUT)
    sig = dict(sr_nanmax=(D_, [D_] * 2), sr_row_class=(C.c_int, [D_, D_, C.c_int]), sr_row_rho=(D_, [C.c_int, D_, D_]), sr_eq_weight=(D_, [C.c_int, D_]),
               sr_upper_is_finite=(C.c_int, [D_]), sr_lower_is_finite=(C.c_int, [D_]), sr_adx_violates=(C.c_int, [D_] * 4), sr_support_term=(D_, [D_] * 3),
               sr_support_finite=(D_, [D_] * 3), sr_clamp_lower=(D_, [D_]), sr_clamp_upper=(D_, [D_]), sr_in_q=(D_, [D_] * 3), sr_in_l=(D_, [D_] * 2),
               sr_in_u=(D_, [D_] * 2), sr_in_x=(D_, [D_] * 2), sr_in_y=(D_, [D_] * 3), sr_step_row=(None, [D_] * 7 + [DP]), sr_step_col=(None, [D_] * 3 + [DP]),
               sr_residuals=(None, [C.c_int, C.c_int, DP, DP, D_] + [DP] * 11), sr_polish_active=(C.c_int, [D_] * 4), sr_adjoint_active=(C.c_int, [D_] * 4),
               sr_normal_cone=(None, [D_] * 3 + [DP]), sr_polish_accept=(C.c_int, [D_] * 4), sr_consts=(None, [DP]))
    for name, (res, args) in sig.items():
        getattr(L, name).restype = res; getattr(L, name).argtypes = args
    return L


def arr(v):
    v = [float(e) for e in np.ravel(v)]
    return (D_ * len(v))(*v)


def same(a, b):
    """== that also holds for a NaN on both sides"""
    return a == b or (a != a and b != b)


# ---- the reference's rules, restated
def ref_class(l, u, rho_is_vec=1):                              # _osqp.py:505-518
    if not rho_is_vec:
        return 0
    if l < -OSQP_INFTY * MIN_SCALING and u > OSQP_INFTY * MIN_SCALING:
        return -1
    return 1 if u - l < RHO_TOL else 0


def ref_rho(cls, rho_bar, rho_eq):                              # :520-522
    return RHO_MIN if cls == -1 else (rho_eq if cls == 1 else rho_bar)


def fma(a, b, c):
    """a b + c rounded once (exact rational arithmetic, then the correctly rounded conversion)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def ref_step_row(alpha, a, rho, z, y, l, u):                    # :678-703 (z_prev + y / rho, projected; dy = rho (relaxed - z))
    zr = fma(alpha, a, (1.0 - alpha) * z)                       # (the rule fixes which product of the sum is exact: step_rules.h)
    zn = min(max(zr + y / rho, l), u)
    dy = rho * (zr - zn)
    return zn, y + dy, dy


def ref_nanmax(r, a):
    return a if (a > r or a != a) else r


def test_constants(lib):
    c = (D_ * 4)()
    lib.sr_consts(c)
    assert list(c) == [MIN_SCALING, RHO_TOL, RHO_MIN, RHO_EQ_OVER_RHO_INEQ]


def test_row_class_at_and_around_the_thresholds(lib):
    big = OSQP_INFTY * MIN_SCALING
    up, dn = math.nextafter(big, math.inf), math.nextafter(big, 0.0)
    cases = [(-up, up), (-big, up), (-up, big), (-big, big), (-dn, up), (-up, dn),           # loose needs BOTH sides strictly beyond
             (-OSQP_INFTY, OSQP_INFTY), (-1e35, 1e35), (-OSQP_INFTY, 1.0), (1.0, OSQP_INFTY), (-1e35, 0.0),
             (2.0, 2.0), (0.0, 0.0), (-OSQP_INFTY, -OSQP_INFTY), (OSQP_INFTY, OSQP_INFTY)]
    for l0 in (0.0, 1.0, -3.5, 1e3):                                                         # u - l at and on both sides of RHO_TOL
        for w in (RHO_TOL, math.nextafter(RHO_TOL, 0.0), math.nextafter(RHO_TOL, 1.0), 0.5 * RHO_TOL, 2 * RHO_TOL):
            cases.append((l0, l0 + w))
    seen = set()
    for l, u in cases:
        for vec in (1, 0):
            got = lib.sr_row_class(l, u, vec)
            assert got == ref_class(l, u, vec), (l, u, vec)
            seen.add(got)
    assert seen == {-1, 0, 1}
    assert lib.sr_row_class(-up, up, 1) == -1 and lib.sr_row_class(-big, big, 1) == 0 and lib.sr_row_class(-up, up, 0) == 0
    assert lib.sr_row_class(2.0, 2.0, 1) == 1 and lib.sr_row_class(2.0, 2.0, 0) == 0
    # beyond OSQP_INFTY the load rules clamp first: the class is that of the clamped, scaled bounds
    for E in (1.0, 0.37, 12.5):
        for l, u in ((-1e35, 1e35), (-1e35, 3.0), (1e31, 1e33), (-1e33, -1e31)):
            ls, us = lib.sr_in_l(E, l), lib.sr_in_u(E, u)
            assert (ls, us) == (E * max(l, -OSQP_INFTY), E * min(u, OSQP_INFTY))
            assert lib.sr_row_class(ls, us, 1) == ref_class(E * max(l, -OSQP_INFTY), E * min(u, OSQP_INFTY))
    assert lib.sr_row_class(lib.sr_in_l(1.0, 1e31), lib.sr_in_u(1.0, 1e33), 1) == 1          # both clamp to +OSQP_INFTY: an equality


def test_row_rho_and_eq_weight(lib):
    for rho_bar in (0.1, 1e-6, 37.5, 1e6):
        for eqf in (1e3, 10.0, 1.0):
            rho_eq = eqf * rho_bar
            for cls in (-1, 0, 1):
                assert lib.sr_row_rho(cls, rho_bar, rho_eq) == ref_rho(cls, rho_bar, rho_eq)
            assert lib.sr_row_rho(-1, rho_bar, rho_eq) == RHO_MIN and lib.sr_row_rho(1, rho_bar, rho_eq) == rho_eq and lib.sr_row_rho(0, rho_bar, rho_eq) == rho_bar
    assert lib.sr_row_rho(1, 0.1, 1e3 * 0.1) == RHO_EQ_OVER_RHO_INEQ * 0.1
    for mixed in (10.0, 1e3, 2.5):
        assert lib.sr_eq_weight(1, mixed) == RHO_EQ_OVER_RHO_INEQ and lib.sr_eq_weight(0, mixed) == mixed


def test_step_row(lib):
    out = (D_ * 3)()
    seen = set()
    rng = np.random.default_rng(7)
    rows = [(0.3, 0.2, 0.5, -1.0, 1.0), (5.0, 0.2, 0.5, -1.0, 1.0), (-5.0, 0.2, 0.5, -1.0, 1.0), (0.3, 0.2, -40.0, -1.0, 1.0), (0.3, 0.2, 40.0, -1.0, 1.0),
            (0.7, 0.7, 0.1, 0.7, 0.7)]
    rows += [tuple(rng.standard_normal(3)) + (-abs(rng.standard_normal()), abs(rng.standard_normal())) for _ in range(40)]
    for alpha in (1.0, 1.6):
        for rho in (0.1, 100.0, RHO_MIN):                      # RHO_MIN: a loose row (y / rho is then huge unless y = 0)
            for a, z, y, l, u in rows:
                if rho == RHO_MIN:
                    l, u, y = -OSQP_INFTY, OSQP_INFTY, y * 1e-9
                lib.sr_step_row(alpha, a, rho, z, y, l, u, out)
                zn, yn, dy = ref_step_row(alpha, a, rho, z, y, l, u)
                assert (out[0], out[1], out[2]) == (zn, yn, dy), (alpha, rho, a, z, y, l, u)
                seen.add('below' if zn == l else ('above' if zn == u else 'inactive'))
                if rho == RHO_MIN:
                    assert l < zn < u
    assert seen == {'below', 'above', 'inactive'}
    # the dividing form is the contract: found by search, inputs at which  zr + y * (1 / rho)  rounds differently -- the rule gives the divided one
    found = 0
    for a, z, y in rng.standard_normal((200, 3)):
        for rho in (0.3, 0.7, 3.0):
            zr = fma(1.6, a, (1.0 - 1.6) * z)
            if zr + y / rho != zr + y * (1.0 / rho):
                lib.sr_step_row(1.6, a, rho, z, y, -OSQP_INFTY, OSQP_INFTY, out)
                assert out[0] == zr + y / rho and out[0] != zr + y * (1.0 / rho)
                found += 1
    assert found > 0


def test_step_col(lib):
    out = (D_ * 2)()
    rng = np.random.default_rng(8)
    for alpha in (1.0, 1.6):
        for xs, x in rng.standard_normal((30, 2)):
            lib.sr_step_col(alpha, xs, x, out)
            xn = fma(1.0 - alpha, x, alpha * xs)               # _osqp.py:660-668 (the rule fixes which product of the sum is exact)
            assert (out[0], out[1]) == (xn, xn - x)


def test_load_rules_and_their_product_order(lib):
    rng = np.random.default_rng(9)
    found_y = found_q = False
    for _ in range(400):
        c, d, e, v = np.exp(rng.standard_normal(4))
        v = v * (1 if rng.random() < 0.5 else -1)
        assert lib.sr_in_q(c, d, v) == c * d * v                                     # :1328  c D q: (c D) q
        assert lib.sr_in_x(v, d) == v * d                                            # :1505
        assert lib.sr_in_y(v, e, c) == v * e * c                                     # :1506 then the cost scaling: (y Einv) c
        assert lib.sr_in_l(e, v) == e * v and lib.sr_in_u(e, v) == e * v             # :1357-1358 (inside the clamp)
        # values at which another order rounds differently: the test would not see a reordering otherwise
        if v * e * c != v * (e * c) and v * e * c != (c * e) * v:
            found_y = True
            assert lib.sr_in_y(v, e, c) != v * (e * c)
        if c * d * v != c * (d * v):
            found_q = True
            assert lib.sr_in_q(c, d, v) != c * (d * v)
    assert found_y and found_q
    for v in (-1e35, -OSQP_INFTY, -3.0, 0.0, 4.0, OSQP_INFTY, 1e35):
        assert lib.sr_clamp_lower(v) == max(v, -OSQP_INFTY) and lib.sr_clamp_upper(v) == min(v, OSQP_INFTY)
        assert lib.sr_in_l(0.5, v) == 0.5 * max(v, -OSQP_INFTY) and lib.sr_in_u(0.5, v) == 0.5 * min(v, OSQP_INFTY)
    assert lib.sr_clamp_lower(-1e35) == -OSQP_INFTY and lib.sr_clamp_upper(1e35) == OSQP_INFTY


def test_finite_sides(lib):
    big = OSQP_INFTY * MIN_SCALING
    up, dn = math.nextafter(big, math.inf), math.nextafter(big, 0.0)
    for v, fin in ((dn, 1), (big, 0), (up, 0), (OSQP_INFTY, 0), (0.0, 1), (-OSQP_INFTY, 1)):
        assert lib.sr_upper_is_finite(v) == fin == int(v < OSQP_INFTY * MIN_SCALING)
        assert lib.sr_lower_is_finite(-v) == fin == int(-v > -OSQP_INFTY * MIN_SCALING)
    thr = 0.25
    for l, u in ((-1.0, 1.0), (-OSQP_INFTY, 1.0), (-1.0, OSQP_INFTY), (-OSQP_INFTY, OSQP_INFTY)):
        for a in (-1.0, -thr, 0.0, thr, 1.0):
            ref = (u < OSQP_INFTY * MIN_SCALING and a > thr) or (l > -OSQP_INFTY * MIN_SCALING and a < -thr)      # :861-872
            assert lib.sr_adx_violates(a, l, u, thr) == int(ref), (a, l, u)
    assert lib.sr_adx_violates(1.0, -1.0, 1.0, thr) == 1 and lib.sr_adx_violates(1.0, -1.0, OSQP_INFTY, thr) == 0
    assert lib.sr_adx_violates(-1.0, -1.0, 1.0, thr) == 1 and lib.sr_adx_violates(-1.0, -OSQP_INFTY, 1.0, thr) == 0
    for l, u in ((-2.0, 3.0), (-OSQP_INFTY, 3.0), (-2.0, OSQP_INFTY)):
        for dy in (-0.7, 0.0, 0.4):
            assert lib.sr_support_term(l, u, dy) == u * max(dy, 0.0) + l * min(dy, 0.0)                           # :811-813
            ref = u * dy if (dy > 0 and u < OSQP_INFTY * MIN_SCALING) else (l * dy if (dy < 0 and l > -OSQP_INFTY * MIN_SCALING) else 0.0)
            assert lib.sr_support_finite(l, u, dy) == ref


def ref_residuals(A, P, sigma, x, z, y, dx, dy, q, l, u, D, E):
    """_osqp.py:728-751 (primal), :766-794 (dual), :796-813, :836-846 and the objective's terms :705-712; every norm folded over the rows in index order
    with the NaN-propagating maximum, every product a left-to-right sum as a kernel forms it"""
    m, n = A.shape
    R = dict.fromkeys(FIELDS, 0.0)

    def mx(k, v):
        R[k] = ref_nanmax(R[k], abs(v))
    for i in range(m):
        ax = 0.0
        for j in range(n):
            ax += A[i, j] * x[j]
        ei, pr = 1.0 / E[i], ax - z[i]
        mx('pri_u', ei * pr); mx('ax_u', ei * ax); mx('z_u', ei * z[i]); mx('pri_s', pr); mx('ax_s', ax); mx('z_s', z[i])
        mx('dy_u', E[i] * dy[i]); mx('dy_s', dy[i])
        # (a NaN step: C's fmax / fmin drop it where np.maximum / np.minimum pass it on -- the kernels have always used the former here; the NaN reaches
        #  the termination rules through dy_u / dy_s of the same row, asserted below)
        dp, dm = (0.0, 0.0) if dy[i] != dy[i] else (max(dy[i], 0.0), min(dy[i], 0.0))
        R['pinf_lhs'] += u[i] * dp + l[i] * dm
    for j in range(n):
        sp = sa = 0.0
        for k in range(n):
            sp += (P[j, k] + (sigma if k == j else 0.0)) * x[k]
        for i in range(m):
            sa += A[i, j] * y[i]
        px = sp - sigma * x[j]
        dr, di = px + q[j] + sa, 1.0 / D[j]
        mx('dua_u', di * dr); mx('px_u', di * px); mx('aty_u', di * sa); mx('dua_s', dr); mx('px_s', px); mx('aty_s', sa)
        mx('dxn_u', D[j] * dx[j]); mx('dxn_s', dx[j]); mx('qn_s', q[j]); mx('qn_u', di * q[j])
        R['xpx'] += x[j] * px; R['qx'] += q[j] * x[j]; R['qdx'] += q[j] * dx[j]
    return R


def _dense_example(nan_at=None):
    rng = np.random.default_rng(11)
    A = rng.standard_normal((3, 2)); Ph = rng.standard_normal((2, 2)); P = Ph @ Ph.T
    v = dict(x=rng.standard_normal(2), z=rng.standard_normal(3), y=rng.standard_normal(3), dx=rng.standard_normal(2), dy=rng.standard_normal(3),
             q=rng.standard_normal(2), l=-np.abs(rng.standard_normal(3)), u=np.abs(rng.standard_normal(3)), D=np.exp(rng.standard_normal(2)),
             E=np.exp(rng.standard_normal(3)))
    if nan_at:
        v[nan_at[0]][nan_at[1]] = np.nan
    return A, P, 1e-6, v


@pytest.mark.parametrize('nan_at', [None, ('z', 1), ('x', 0), ('dy', 2), ('q', 1)])
def test_residual_rows(lib, nan_at):
    A, P, sigma, v = _dense_example(nan_at)
    out = (D_ * 22)()
    lib.sr_residuals(3, 2, arr(A), arr(P), sigma, *[arr(v[k]) for k in ('x', 'z', 'y', 'dx', 'dy', 'q', 'l', 'u', 'D', 'E')], out)
    ref = ref_residuals(A, P, sigma, **v)
    for k, f in enumerate(FIELDS):
        assert same(out[k], ref[f]), (f, out[k], ref[f])
    # the norms against numpy on the same products (a NaN entry must come through: np.max propagates it, as nanmax does and fmax would not)
    ax = np.array([sum(A[i, j] * v['x'][j] for j in range(2)) for i in range(3)])
    got = dict(zip(FIELDS, out))
    assert same(got['pri_s'], np.max(np.abs(ax - v['z']))) and same(got['z_s'], np.max(np.abs(v['z']))) and same(got['dy_s'], np.max(np.abs(v['dy'])))
    assert same(got['dxn_s'], np.max(np.abs(v['dx']))) and same(got['qn_s'], np.max(np.abs(v['q']))) and same(got['z_u'], np.max(np.abs(v['z'] / v['E'])))
    if nan_at == ('z', 1):
        assert math.isnan(got['pri_s']) and math.isnan(got['z_u']) and not math.isnan(got['ax_s']) and not math.isnan(got['dua_s'])
    if nan_at == ('x', 0):
        assert all(math.isnan(got[f]) for f in ('pri_s', 'ax_u', 'dua_u', 'px_s', 'xpx', 'qx'))
    if nan_at == ('dy', 2):
        assert math.isnan(got['dy_s']) and math.isnan(got['dy_u'])
    if nan_at is None:
        assert not any(math.isnan(e) for e in out)


def test_nanmax(lib):
    nan = float('nan')
    for r, a in ((0.0, 1.0), (1.0, 0.5), (1.0, nan), (nan, 1.0), (nan, nan), (-math.inf, -3.0), (2.0, 2.0)):
        assert same(lib.sr_nanmax(r, a), ref_nanmax(r, a))
    assert math.isnan(lib.sr_nanmax(1.0, nan)) and math.isnan(lib.sr_nanmax(nan, 1.0))      # a NaN enters and stays (fmax would drop it both times)


def test_polish_active_and_the_equality_override(lib):
    def ref(z, l, u, y):                                        # _osqp.py:1719-1720; a row in both index sets enters once, at its lower bound
        low = z - l < -y
        upp = (u - z < y) and not low
        return (1 if low else 0) | (2 if upp else 0)
    cases = [(0.0, -1.0, 1.0, 0.0), (-1.0, -1.0, 1.0, -0.5), (1.0, -1.0, 1.0, 0.5), (-0.99, -1.0, 1.0, -0.5), (0.99, -1.0, 1.0, 0.5),
             (0.0, -1.0, 1.0, 2.0), (0.0, -1.0, 1.0, -2.0), (2.0, 2.0, 2.0, 0.0), (2.0, 2.0, 2.0, 0.3), (2.0, 2.0, 2.0, -0.3)]
    for z, l, u, y in cases:
        assert lib.sr_polish_active(z, l, u, y) == ref(z, l, u, y), (z, l, u, y)
    # active on both sides: both of the reference's tests hold (they can only with u - l < 0): the row enters once, at its lower bound
    z, l, u, y = 0.0, 1.0, 0.5, 0.8
    assert (z - l < -y) and (u - z < y)
    assert lib.sr_polish_active(z, l, u, y) == 1
    assert {lib.sr_polish_active(*c) for c in cases} == {0, 1, 2}
    # the adjoint's override: an equality row (l == u) is always active, lower for y < 0, else upper; other rows follow polish's rule
    for z, l, u, y in cases:
        want = (1 if y < 0.0 else 2) if l == u else ref(z, l, u, y)
        assert lib.sr_adjoint_active(z, l, u, y) == want
    assert lib.sr_polish_active(2.0, 2.0, 2.0, 0.0) == 0 and lib.sr_adjoint_active(2.0, 2.0, 2.0, 0.0) == 2
    assert lib.sr_adjoint_active(2.0, 2.0, 2.0, -0.3) == 1


def test_normal_cone(lib):
    out = (D_ * 2)()
    for t, l, u in ((0.3, -1.0, 1.0), (1.7, -1.0, 1.0), (-2.5, -1.0, 1.0), (0.1 + 0.2, 0.3, 0.3), (5.0, -OSQP_INFTY, OSQP_INFTY)):
        lib.sr_normal_cone(t, l, u, out)
        zc = min(max(t, l), u)                                  # :670-674
        assert (out[0], out[1]) == (zc, t - zc)


def test_polish_accept(lib):
    def ref(pri, dua, pri0, dua0):                              # :1786-1793
        return (pri < pri0 and dua < dua0) or (pri < pri0 and dua0 < 1e-10) or (dua < dua0 and pri0 < 1e-10)
    cases = [(1e-6, 1e-6, 1e-3, 1e-3, True),                    # both improved
             (1e-6, 1e-3, 1e-3, 1e-3, False), (1e-3, 1e-6, 1e-3, 1e-3, False),
             (1e-6, 1e-11, 1e-3, 1e-12, True),                  # primal improved, dual was negligible
             (1e-6, 1e-9, 1e-3, 1e-10, False),                  # (1e-10 itself is not below 1e-10)
             (1e-11, 1e-6, 1e-12, 1e-3, True),                  # dual improved, primal was negligible
             (1e-9, 1e-6, 1e-10, 1e-3, False), (1e-3, 1e-3, 1e-3, 1e-3, False)]
    for pri, dua, pri0, dua0, want in cases:
        assert bool(lib.sr_polish_accept(pri, dua, pri0, dua0)) == ref(pri, dua, pri0, dua0) == want, (pri, dua, pri0, dua0)
