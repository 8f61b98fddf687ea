"""CPU tier: the duality-gap rules of the batch family (settings.check_dualgap; osqp-python_amd/csrc/term_rules.h term_dual_obj, term_gap_ok,
batch_check_gap, batch_record_gap) behind tests/hostsim/gap_probe.cpp, against a Python restatement of the single handle's rule (policy.h ctl_info /
ctl_stage1: dual_obj = (-1/2 x'Px - supp) cinv, gap = obj - dual_obj, "solved" additionally needs |gap| < eps_abs + eps_rel max(|obj|, |dual_obj|), x 10 on
the approximate pass at max_iter) -- and the numpy stand-in of k_ls_supp with its judge (tests/gap_ref.py), which must pass the stand-in and catch four
planted mistakes."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import gap_ref as G
from test_batch_rules import FIELDS, GO_ON, MAX_ITER, NON_CVX, PINF, DINF, SOLVED, SOLVED_INACC, arr, block, ref_check, settings
from test_policy_rules import ROOT

SRC = os.path.join(ROOT, 'tests', 'hostsim', 'gap_probe.cpp')
OUT = os.path.join(ROOT, 'tests', '_build', 'libgap_probe.so')
DEPS = [SRC] + [os.path.join(ROOT, 'osqp-python_amd', 'csrc', h) for h in ('term_rules.h', 'step_rules.h')]
DP = C.POINTER(C.c_double)
SET = ('eps_abs', 'eps_rel', 'eps_pinf', 'eps_dinf', 'c', 'cinv', 'm', 'unscaled', 'scaling')


@pytest.fixture(scope='module')
def lib():
    if not (os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(f) for f in DEPS)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'include'), '-o', OUT, SRC])
    L = C.CDLL(OUT)
    L.gp_check.argtypes = [DP, DP, C.c_int, C.c_int, C.c_int, DP, C.c_int, C.c_double, DP]; L.gp_check.restype = C.c_int
    L.gp_check_plain.argtypes = [DP, DP, C.c_int, C.c_int, C.c_int, DP, DP]; L.gp_check_plain.restype = C.c_int
    L.gp_gap_ok.argtypes = [DP] + [C.c_double] * 3 + [C.c_int]; L.gp_gap_ok.restype = C.c_int
    L.gp_record.argtypes = [DP, C.c_int, C.c_double]
    L.gp_supp.argtypes = [C.c_int, DP, DP, DP]; L.gp_supp.restype = C.c_double
    return L


def ref_gap_check(S, R, supp, it, max_iter, at_check, **kw):
    """The check with the gap, pass by pass.  One pass is ref_check (tests/test_batch_rules.py) below max_iter -- its exact pass alone --, on the settings as
    they are or with every eps x 10 (the approximate pass: the same tests at ten times the tolerances, _osqp.py:1012-1016); where it says SOLVED and the gap
    test of that pass fails, the pass decides nothing: both residual tests passed, so no infeasibility test was even asked.  -> (status, dual_obj, gap)"""
    ci = S['cinv'] if S['scaling'] else 1.0
    obj = (0.5 * R['xpx'] + R['qx']) * ci
    dual_obj = (-0.5 * R['xpx'] - supp) * ci
    gap = obj - dual_obj

    def one(approx):
        f = 10.0 if approx else 1.0
        st = ref_check(dict(S, **{k: f * S[k] for k in ('eps_abs', 'eps_rel', 'eps_pinf', 'eps_dinf')}), R, 0, 1, 1, **kw)[0]
        if st == SOLVED and not G.gap_ok_values(obj, dual_obj, gap, S['eps_abs'], S['eps_rel'], approx):
            st = GO_ON
        return st + 1 if (approx and st in (SOLVED, PINF, DINF)) else st

    for approx in (0, 1):
        if not at_check or (approx and it < max_iter):
            break
        st = one(approx)
        if st != GO_ON:
            return st, dual_obj, gap
    return (MAX_ITER if it >= max_iter else GO_ON), dual_obj, gap


def run(lib, S, R, supp, gap_on=1, it=25, max_iter=4000, at_check=1, atdy=(0, 0), pdx=(0, 0), adx_ok=True):
    out = arr([0] * 7)
    st = lib.gp_check(arr([S[k] for k in SET]), arr([R[k] for k in FIELDS]), it, max_iter, at_check, arr(list(atdy) + list(pdx) + [1.0 if adx_ok else 0.0]), gap_on, supp, out)
    return st, list(out)


def agree(lib, S, R, supp, **kw):
    st, out = run(lib, S, R, supp, **kw)
    want = ref_gap_check(S, R, supp, kw.get('it', 25), kw.get('max_iter', 4000), kw.get('at_check', 1), **{k: v for k, v in kw.items() if k in ('atdy', 'pdx', 'adx_ok')})
    assert st == want[0], (st, want, out)
    assert out[5] == want[1] and (out[6] == want[2] or (math.isnan(out[6]) and math.isnan(want[2]))), (out, want)      # dual_obj and gap bit for bit
    return st, out


CONVERGED = dict(pri_s=1e-4, dua_s=1e-4, pri_u=1e-4, dua_u=1e-4)


def _supp_for_gap(R, S, gap):
    """the support sum that gives this gap: gap = (xpx + qx + supp) cinv"""
    return gap / (S['cinv'] if S['scaling'] else 1.0) - R['xpx'] - R['qx']


def test_gap_just_below_and_just_above_the_tolerance_on_the_exact_pass(lib):
    S, R = settings(), block(**CONVERGED)                    # obj = (1 - 3) = -2; eps 1e-3: the tolerance is 1e-3 + 1e-3 max(2, |dual_obj|)
    for gap, want in ((2.9e-3, SOLVED), (3.1e-3, GO_ON), (-2.9e-3, SOLVED), (-3.1e-3, GO_ON)):
        st, out = agree(lib, S, R, _supp_for_gap(R, S, gap))
        assert st == want and out[0] == -2.0 and abs(out[6] - gap) < 1e-14, (gap, st, out)
    # the cost scale enters obj, dual_obj and the gap alike (the problem's own cinv on the per-problem-matrix forms)
    S2 = settings(c=0.5, cinv=2.0)
    assert agree(lib, S2, R, _supp_for_gap(R, S2, 4.9e-3))[0] == SOLVED and agree(lib, S2, R, _supp_for_gap(R, S2, 5.1e-3))[0] == GO_ON      # 1e-3 + 1e-3 * 4
    assert agree(lib, settings(scaling=0, cinv=2.0), R, _supp_for_gap(R, settings(scaling=0), 2.9e-3))[0] == SOLVED                           # no scaling: no cinv


def test_the_same_on_the_approximate_pass_at_max_iter(lib):
    S, R = settings(), block(**CONVERGED)
    at = dict(it=4000, max_iter=4000)
    for gap, want in ((2.9e-3, SOLVED), (3.1e-3, SOLVED_INACC), (2.9e-2, SOLVED_INACC), (3.1e-2, MAX_ITER), (-3.1e-2, MAX_ITER)):
        assert agree(lib, S, R, _supp_for_gap(R, S, gap), **at)[0] == want, gap
    # residuals between eps and 10 eps: the exact pass fails on them, the approximate one asks for the gap at 10 x
    R2 = block(pri_s=5e-3, dua_s=5e-3)
    assert agree(lib, S, R2, _supp_for_gap(R2, S, 2.9e-2), **at)[0] == SOLVED_INACC and agree(lib, S, R2, _supp_for_gap(R2, S, 3.1e-2), **at)[0] == MAX_ITER
    assert agree(lib, S, R2, _supp_for_gap(R2, S, 1e-9), it=3975, max_iter=4000)[0] == GO_ON
    # between checks nothing is tested, the gap included
    assert agree(lib, S, R, _supp_for_gap(R, S, 1e-9), at_check=0)[0] == GO_ON and agree(lib, S, R, _supp_for_gap(R, S, 1e-9), at_check=0, **at)[0] == MAX_ITER


def test_objectives_of_opposite_signs(lib):
    """obj = +0.5, dual_obj = -0.5 (far apart: fails), and a pair straddling zero inside the tolerance: the normalisation is the larger absolute value"""
    S = settings()
    R = block(xpx=3.0, qx=-1.0, **CONVERGED)                 # obj = 0.5;  dual_obj = -1.5 - supp
    st, out = agree(lib, S, R, -1.0)
    assert out[0] == 0.5 and out[5] == -0.5 and out[6] == 1.0 and st == GO_ON
    R = block(xpx=2e-4, qx=2e-4, **CONVERGED)                # obj = 3e-4;  supp = 4e-4: dual_obj = -5e-4, gap = 8e-4 < 1e-3 + 1e-3 * 5e-4
    st, out = agree(lib, S, R, 4e-4)
    assert out[0] > 0 > out[5] and st == SOLVED
    st, out = agree(lib, S, R, 1.2e-3)                       # dual_obj = -1.3e-3, gap = 1.6e-3
    assert out[0] > 0 > out[5] and st == GO_ON


def test_an_infeasibility_certificate_is_found_with_the_setting_as_without(lib):
    S = settings()
    assert agree(lib, S, block(pinf_lhs=-1.0, dy_s=2.0), 0.3, atdy=(9.0, 1e-4))[0] == PINF
    assert agree(lib, S, block(qdx=-1.0, dxn_s=2.0), 0.3, pdx=(9.0, 1e-4))[0] == DINF
    assert agree(lib, S, block(pri_s=math.nan), 0.3)[0] == NON_CVX


def _generator_blocks():
    """every (settings, block, keywords) that tests/test_batch_rules.py runs through batch_check"""
    nan = math.nan
    yield settings(), block(pri_s=1e-4, dua_s=1e-4, pri_u=1e-4, dua_u=1.5e-3), {}
    yield settings(), block(pri_s=1e-4, dua_s=2.1e-3), {}
    Ru = block(pri_u=1e-4, dua_u=0.8e-3, px_u=0, aty_u=0, qn_u=0, pri_s=0.5, dua_s=0.5)
    yield settings(unscaled=1, c=1.0, cinv=1.0), Ru, {}
    yield settings(unscaled=1, c=0.5, cinv=2.0), Ru, {}
    yield settings(scaling=0, cinv=2.0), block(pri_s=1e-4, dua_s=1e-4), {}
    yield settings(m=0), block(pri_s=5.0, pri_u=5.0, dua_s=1e-4, pinf_lhs=-1.0), {}
    for atdy in ((9.0, 1e-4), (0.0, 3e-4)):
        yield settings(), block(pinf_lhs=-1.0, dy_s=2.0), dict(atdy=atdy)
    yield settings(), block(pinf_lhs=-1e-4, dy_s=2.0), {}
    yield settings(unscaled=1), block(pinf_lhs=-1.0, dy_u=2.0, dy_s=0.0), dict(atdy=(1e-4, 9.0))
    for kw in (dict(pdx=(9.0, 1e-4)), dict(pdx=(9.0, 1e-4), adx_ok=False), dict(pdx=(0.0, 3e-4))):
        yield settings(), block(qdx=-1.0, dxn_s=2.0), kw
    yield settings(), block(qdx=-1e-4, dxn_s=2.0), {}
    Rd = block(qdx=-1.5e-4, dxn_u=2.0, dxn_s=0.0)
    for c, pdx in ((0.5, 0.9e-4), (1.0, 0.9e-4), (0.5, 1.1e-4)):
        yield settings(unscaled=1, c=c, cinv=1 / c), Rd, dict(pdx=(pdx, 9.0))
    for kw in (dict(pri_s=nan), dict(dua_s=nan), dict(pri_s=2e30), dict(dua_s=2e30), dict(pri_s=nan, dua_s=1e-4, ax_s=math.inf)):
        yield settings(), block(**kw), {}
    for R, kw in ((block(pri_s=5e-3, dua_s=5e-3), dict(it=4000, max_iter=4000)), (block(pri_s=5e-3, dua_s=5e-3), dict(it=3975, max_iter=4000)),
                  (block(pri_s=5e-2, dua_s=5e-3), dict(it=4000, max_iter=4000)), (block(pinf_lhs=-1.0, dy_s=2.0), dict(it=4000, max_iter=4000, atdy=(0.0, 1.5e-3))),
                  (block(pinf_lhs=-1.0, dy_s=2.0), dict(it=3975, max_iter=4000, atdy=(0.0, 1.5e-3))), (block(qdx=-1.0, dxn_s=2.0), dict(it=4000, max_iter=4000, pdx=(0.0, 1.5e-3))),
                  (block(pri_s=1e-4, dua_s=1e-4), dict(at_check=0)), (block(pri_s=1e-4, dua_s=1e-4), dict(at_check=0, it=4000, max_iter=4000))):
        yield settings(), R, kw


def test_flag_off_is_batch_check_on_every_block_of_the_generator(lib):
    """batch_check_gap with gap_on = 0 -- whatever supp holds, a NaN included -- against batch_check as it was and against test_batch_rules.py's restatement:
    the status, obj, prim_res, dual_res, the second stages asked for and the A dx threshold, bit for bit"""
    seen = set()
    for S, R, kw in _generator_blocks():
        s2 = arr(list(kw.get('atdy', (0, 0))) + list(kw.get('pdx', (0, 0))) + [1.0 if kw.get('adx_ok', True) else 0.0])
        plain = arr([0] * 5)
        st0 = lib.gp_check_plain(arr([S[k] for k in SET]), arr([R[k] for k in FIELDS]), kw.get('it', 25), kw.get('max_iter', 4000), kw.get('at_check', 1), s2, plain)
        want = ref_check(S, R, kw.get('it', 25), kw.get('max_iter', 4000), kw.get('at_check', 1), kw.get('atdy', (0, 0)), kw.get('pdx', (0, 0)), kw.get('adx_ok', True))
        assert st0 == want[0] and int(plain[3]) == want[4]
        for supp in (0.0, 7.5, -1e30, math.nan):
            st, out = run(lib, S, R, supp, gap_on=0, **kw)
            assert st == st0 and np.array_equal(np.array(out[:5]), np.array(list(plain)), equal_nan=True), (S, R, kw, supp)
            assert out[5] == 0.0 and out[6] == 0.0
        seen.add(st0)
    assert {SOLVED, SOLVED_INACC, GO_ON, MAX_ITER, PINF, DINF, NON_CVX} <= seen


def test_a_nan_in_the_support_sum_never_reports_solved(lib):
    S, R = settings(), block(**CONVERGED)
    for supp in (math.nan, math.inf, -math.inf):
        st, out = run(lib, S, R, supp)
        assert st == GO_ON and not abs(out[6]) < math.inf, (supp, st, out)
        assert run(lib, S, R, supp, it=4000, max_iter=4000)[0] == MAX_ITER
        assert run(lib, S, R, supp, gap_on=0)[0] == SOLVED
    assert not lib.gp_gap_ok(arr([S[k] for k in SET]), -2.0, math.nan, math.nan, 0) and not lib.gp_gap_ok(arr([S[k] for k in SET]), -2.0, math.nan, math.nan, 1)
    assert lib.gp_gap_ok(arr([S[k] for k in SET]), -2.0, -2.001, 1e-3, 0) and not lib.gp_gap_ok(arr([S[k] for k in SET]), -2.0, -2.004, 4e-3, 0)


def test_column_eleven_follows_the_record(lib):
    rc = arr([7.0] * 13)
    lib.gp_record(rc, SOLVED, 1.25e-6)
    assert list(rc) == [1.0, 75.0, -2.5, 1e-7, 2e-7, 0.3, 2.0, 410.0, 0.0, 0.0, 0.25, 1.25e-6, 7.0]
    for st in (SOLVED_INACC, MAX_ITER, 8):
        lib.gp_record(rc, st, -3.0); assert rc[11] == -3.0
    for st in (PINF, PINF + 1, DINF, DINF + 1, NON_CVX):     # x or y is a certificate, or nothing is finite: the record describes no point
        lib.gp_record(rc, st, 1.0); assert math.isnan(rc[11]) and rc[0] == st


# ---------------------------------------------------------------------------------------------------------------- the stand-in of k_ls_supp and its judge
def _rows(m, seed, zeros=True):
    """(m, 64) bounds and duals: two-sided, equality, both sides infinite, only upper, only lower; y of both signs and exactly zero; magnitudes by lane"""
    rng = np.random.default_rng(seed)
    sc = 2.0 ** ((np.arange(G.W) % 9) - 4.0)
    lo = rng.standard_normal((m, G.W)) * sc
    kind = rng.integers(0, 5, size=(m, G.W))
    l = np.where((kind == 2) | (kind == 3), -1e30, lo)
    u = np.where(kind == 1, lo, np.where((kind == 2) | (kind == 4), 1e30, lo + (0.1 + rng.random((m, G.W))) * sc))
    y = rng.standard_normal((m, G.W)) * sc
    if zeros:
        y[rng.random((m, G.W)) < 0.15] = 0.0
    return l, u, y


@pytest.mark.parametrize('m,Gr', [(1, 1), (37, 5), (130, 9), (605, 38), (4100, 256)])
def test_the_stand_in_passes_its_judge_and_is_the_probe_sum(lib, m, Gr):
    l, u, y = _rows(m, m)
    part = G.standin_supp(l, u, y, Gr)
    ratio = G.judge_supp(part, l, u, y, Gr)
    print('stand-in: ratio to the bound', m, Gr, ratio, 'roundings', G.supp_roundings(m, Gr))
    t = G.support_terms(l, u, y, np.float64)
    assert m < 37 or ((t > 0).any() and (t < 0).any() and (t == 0).any())
    if Gr == 1 and m == 1:                                   # one term: the partial is the term of step_rules.h support_finite itself
        for b in range(G.W):
            assert part[0, b] == lib.gp_supp(1, arr(l[:, b]), arr(u[:, b]), arr(y[:, b]))
    # no lane reads another: a lane's partials do not change when every other lane's data does
    l2, u2, y2 = _rows(m, m + 1000)
    l2[:, 7], u2[:, 7], y2[:, 7] = l[:, 7], u[:, 7], y[:, 7]
    assert np.array_equal(G.standin_supp(l2, u2, y2, Gr)[:, 7], part[:, 7])


def test_support_terms_are_the_header_s(lib):
    l, u, y = _rows(50, 3)
    t = G.support_terms(l, u, y, np.float64)
    for i in range(50):
        for b in (0, 5, 63):
            assert t[i, b] == lib.gp_supp(1, arr([l[i, b]]), arr([u[i, b]]), arr([y[i, b]]))
    for lv, uv, yv, want in ((-1e30, 2.0, 3.0, 6.0), (-1e30, 2.0, -3.0, 0.0), (-1.0, 1e30, 3.0, 0.0), (-1.0, 1e30, -3.0, 3.0), (-1e30, 1e30, 3.0, 0.0), (-1.0, 2.0, 0.0, 0.0),
                             (-1.0, 2.0, -0.0, 0.0), (-G.FINITE, G.FINITE, 1.0, 0.0), (-G.FINITE, G.FINITE, -1.0, 0.0), (-0.99e26, 0.99e26, 1.0, 0.99e26)):
        assert lib.gp_supp(1, arr([lv]), arr([uv]), arr([yv])) == want == float(G.support_terms([lv], [uv], [yv], np.float64)[0])


MISTAKES = {
    'an infinite side counted': lambda l, u, y: np.where(y > 0, u * y, np.where(y < 0, l * y, 0.0)),
    'the sign test on y dropped': lambda l, u, y: np.where(u < G.FINITE, u * y, np.where(l > -G.FINITE, l * y, 0.0)),
    'l and u swapped': lambda l, u, y: G.support_terms(u, l, y, np.float64),
}


@pytest.mark.parametrize('what', list(MISTAKES) + ['a partial of the neighbouring lane added'])
def test_the_judge_catches_the_planted_mistake(what):
    m, Gr = 130, 9
    l, u, y = _rows(m, 11)
    if what in MISTAKES:
        with np.errstate(over='ignore', invalid='ignore'):
            part = G.standin_supp(l, u, y, Gr, term=MISTAKES[what])
    else:
        part = G.standin_supp(l, u, y, Gr)
        part[3] = part[3] + np.roll(part[3], 1)
    with pytest.raises(AssertionError):
        G.judge_supp(part, l, u, y, Gr)
