"""GPU tier, kernel level: the lockstep block-vector kernels of osqp-python_amd/csrc/lockstep_hip.hip, ONE LAUNCH AT A TIME, against np.longdouble references
(tests/lockstep_ref.py: layout from the carve, one reference per op, the bound and where it comes from; tests/test_lockstep_ref.py proves that machinery on
a numpy stand-in of every op and shows that it notices ten planted mistakes).  The diagnostic entry osqp_hip_test_lockstep pokes a random work block (and matrix
block) into the route's resident blocks, launches the named kernel with the arguments and the grid a solve uses, and hands the blocks back; the judge
then checks the op's outputs against  err <= 64 max(e64, k 2^-53) scale  per lane and vector, the frozen lanes bit for bit, and EVERY other double and int
of both blocks and of the caller's arrays bit-unchanged.

Handles of the PCG route (each with the handle's matrices and with per-problem matrices):
  T  n = 3, m = 0        G = 1, empty strips, no row of A
  S  n = 70, m = 37      G = 5, ragged strips, two n tiles, A's rows of 0 .. 9 and 67 entries, P parts of 1 .. 6 entries, every row class
  C  n = 4100, m = 130   G clamped at 256, rpw = 5 / 1 (row passes only)
  R  S on a reordered handle (pc / pr in the tile paths, pvmap / avmap in the assembly)
Every op runs with 64 live lanes and with count = 6, one frozen lane, PCG off in two lanes and rho unchanged in two (C included); on S every family also
with count = 1 and with count = 63 and such lanes; the load ops with warm = 0 and 1.

Worst ratio to the bound per family and handle as measured on the MI355X (a record, not a tolerance: the assertion is ratio <= 1; the per-op figures
go to util.record_deviation's file and DESIGN.md section 6), handle's matrices / per-problem matrices:
  transposes  T 0.014 / 0.015   S 0.015 / 0.015   R 0.015 / 0.015          (load_n, load_m, store_n, store_m; init, begin and the assembly are exact)
  rows        T 0.016 / 0.016   S 0.014 / 0.014   C 0.011 / 0.011   R 0.014 / 0.014      (on S, C, R the worst is upd; their sums -- minv, initz, rhs, t, kp, resm, resn -- 0.001 .. 0.010)
  pcg         T 0.015 / 0.016   S 0.014 / 0.014   R 0.014 / 0.014
  matrices    T 0.015   S 0.015   R 0.015                                   (norms, scale, cost, cost_apply, finish)
Handles of the direct route (lockstep_ref.DIRECT_HANDLES: factor-model QPs with a dense F, every long row above 128 entries; shared and per-problem matrices):
  D1 D7 D9 D33   r = 1, 7, 9, 33 at n about 200: GC = 4 < 8; r below 8, odd, two groups of eight columns of S, a second a0 pass, a wave whose second row is past r
  D9w            r = 9 at n = 581: GC = 10 = 8 + 2, n mod 64 = 5 (the last column block shorter than the unroll)
  D128           r = 128: the inversion's dynamic LDS above 64 KB, 16 rows of h per workgroup and 8 workgroups
  D2x            r = 2 at n = 8201: cb = 128, GC = 65 (prod, setl, x only)
Measured there: direct factor (d0, s, inv and the residual of S^-1; cond_2(S) <= 6.1) 0.013 / 0.013 at r = 1 and <= 0.009 from r = 7 on; direct solve (prod x3,
prod2, setl 0 / 1, h, x) 0.016 / 0.016 (h at r = 1; otherwise <= 0.011), vals and wt exact; the PCG-route kernels that route reuses, on D7 through the view
and over n + r rows: transposes 0.015 / 0.015, rows 0.016 / 0.016, matrices 0.015.
No check failed on the GPU: no kernel was changed."""
import os
import warnings

import numpy as np
import pytest

import osqp_amd
from osqp_amd import ext_hip
from util import record_deviation

import lockstep_ref as R

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
VALIDATION = ext_hip.osqp_error_type.OSQP_DATA_VALIDATION_ERROR
NOT_IMPL = ext_hip.osqp_error_type.OSQP_FUNC_NOT_IMPLEMENTED
ST = dict(eps_abs=1e-8, eps_rel=1e-8, max_iter=50000, adaptive_rho_interval=50, check_termination=25, scaling=10, cg_max_iter=20)
EQ_FACTOR = 7.0
FAMILIES = {
    'transposes': ('load_n', 'load_m', 'init', 'store_n', 'store_m'),
    'rows': ('minv', 'initz', 'rhs', 't', 'kp', 'upd', 'resm', 'resn'),
    'pcg': ('setrho', 'cgupd', 'cgp', 'cginit', 'cgalpha', 'cgbeta'),
    'matrices': ('begin', 'asm_a', 'asm_p', 'norms', 'scale', 'cost', 'cost_apply', 'finish'),
}
M_ONLY = ('load_m', 'store_m', 'initz', 't', 'resm', 'setrho')
DIRECT_FAMILIES = {
    'transposes': ('load_n', 'load_m', 'init', 'store_n', 'store_m'),
    'rows': ('initz', 'rhs', 'upd', 'resm', 'resn', 'setrho'),
    'matrices': ('begin', 'asm_a', 'asm_p', 'norms', 'scale', 'cost', 'cost_apply', 'finish'),
    'direct factor': ('d0', 's', 'inv'),
    'direct solve': ('prod_x', 'prod_xs', 'prod_p', 'prod2', 'setl0', 'setl1', 'h', 'x', 'vals', 'wt'),
}


def _problem(name):
    if name in R.DIRECT_HANDLES:
        return R.problem_D(*R.DIRECT_HANDLES[name])
    P, q, A, l, u = {'T': R.problem_T, 'S': R.problem_S, 'C': R.problem_C, 'R': R.problem_S}[name]()
    return P, q, A, np.where(np.isinf(l), -1e30, l), np.where(np.isinf(u), 1e30, u)


class Live:
    """a handle of the test on the GPU and what the references need of it"""
    def __init__(self, name):
        self.name = name
        P, q, A, l, u = _problem(name)
        old = os.environ.get('OSQP_HIP_REORDER')
        os.environ['OSQP_HIP_REORDER'] = '2' if name == 'R' else '0'
        try:
            self.s = osqp_amd.OSQP(algebra='hip')
            self.s.setup(P, q, A, l, u, verbose=False, **ST)
        finally:
            if old is None:
                del os.environ['OSQP_HIP_REORDER']
            else:
                os.environ['OSQP_HIP_REORDER'] = old
        sv = self.sv = self.s._solver
        assert sv.hip_stats()['reordered'] == (1 if name == 'R' else 0)
        sv.hip_set_rho_eq_factor(EQ_FACTOR)
        _, sz = sv.hip_test_lockstep_sizes()
        self.route = int(name in R.DIRECT_HANDLES)
        if self.route:
            assert sz['r'] == R.DIRECT_HANDLES[name][1] + 1 and sz['dws_need'] > 0, sz      # the direct route takes the handle, with every long row found
        st, out = sv.hip_test_lockstep(['rhs'], np.zeros(sz['dws_need' if self.route else 'ws_need']), route=self.route, handle=True, maps=True, view=bool(self.route))
        assert st == 0, st
        pc, pr = sv.hip_get_reordering()
        self.H = R.Handle.from_entry(out, sv.get_settings(), pc, pr, EQ_FACTOR, q)
        need = ('dws_need', 'dmat_need') if self.route else ('ws_need', 'mat_need')
        assert self.H.lay.ws_doubles == sz[need[0]] and self.H.lay.mat_doubles == sz[need[1]] and self.H.G == sz['G']
        assert not self.route or (self.H.lay.GC, self.H.lay.cb, self.H.lay.nv) == (sz['GC'], sz['cb'], sz['nv'])

    def run(self, ops, b0, case):
        st, out = self.sv.hip_test_lockstep(ops, b0.ws, mat_ws=b0.mat, route=self.route, **case.kw())
        assert st == 0, (ops, st)
        return R.Blk(b0.lay, out['ws'], out['mat_ws']), out


_live = {}


def live(name):
    if name not in _live:
        _live[name] = Live(name)
    return _live[name]


def _ops(H, family, mat):
    return [op for op in FAMILIES[family] if (H.m > 0 or op not in M_ONLY) and not (op == 'asm_a' and H.m == 0)]


CONFIGS = [dict(count=64), dict(count=6, frozen=(2,), cgoff=(1, 4), rhooff=(0, 3))]
CONFIGS_S = CONFIGS + [dict(count=1), dict(count=63, frozen=(5,), cgoff=(7,), rhooff=(9,))]      # S: every count the issue names
# handle x family x mat, the combinations that exist: the matrices of a chunk need mat (the entry rejects them without: tested below), C is there for the
# clamped grid of the row passes
CASES = [(name, family, mat) for name in ('T', 'S', 'C', 'R') for family in FAMILIES for mat in (0, 1)
         if (mat or family != 'matrices') and (name != 'C' or family == 'rows')]


@pytest.mark.parametrize('name,family,mat', CASES, ids=['%s-%s-mat%d' % c for c in CASES])
def test_every_launch_against_its_own_formula(name, family, mat):
    L = live(name)
    H = L.H
    worst = {}
    for op in _ops(H, family, mat):
        for ci, cfg in enumerate(CONFIGS_S if name == 'S' else CONFIGS):
            for warm in ((1, 0) if op in ('load_n', 'load_m') else (1,)):
                kw = dict(cfg)
                count = kw.pop('count')
                b0 = R.poke(H.lay, 100 + ci, bool(mat), count=count, wide=True, bdiag=H.Bdiag, **kw)
                case = R.Case(H, count, 200 + ci, warm=warm, mat=bool(mat))
                b1, out = L.run([op], b0, case)
                worst[op] = max(worst.get(op, 0.0), R.judge(op, H, b0, case, b1, out))
    print('ratio to the bound', name, family, mat, {k: float('%.3g' % v) for k, v in worst.items()})
    record_deviation('lockstep_kernels', '%s-%s-mat%d' % (name, family, mat), **worst)
    assert max(worst.values()) <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------------- the direct route
# r in {1, 7, 9, 33} at n about 200 (GC = 4), r = 9 at n = 581 (GC = 10 = 8 + 2, n mod 64 = 5), r = 128 (the inversion's LDS above 64 KB); r = 2 at n = 8201
# (cb = 128, GC = 65) runs prod, setl and x only.  The kernels shared with the PCG route (through the view, x with n + r rows) run on D7.
DIRECT_CASES = [(name, family, mat) for name in ('D1', 'D7', 'D9', 'D33', 'D9w', 'D128') for family in ('direct factor', 'direct solve') for mat in (0, 1)] + \
               [('D7', family, mat) for family in ('transposes', 'rows', 'matrices') for mat in (0, 1) if mat or family != 'matrices'] + [('D2x', 'direct solve', 0), ('D2x', 'direct solve', 1)]
CONFIG_BIG = [dict(count=64, rhooff=tuple(range(4, 64)))]                    # r = 128: the references of s and inv are computed for the four lanes that are written


@pytest.mark.parametrize('name,family,mat', DIRECT_CASES, ids=['%s-%s-mat%d' % c for c in DIRECT_CASES])
def test_every_launch_of_the_direct_route_against_its_own_formula(name, family, mat):
    L = live(name)
    H = L.H
    worst = {}
    ops = [op for op in DIRECT_FAMILIES[family] if mat or op not in R.MAT_ONLY]
    if name == 'D2x':
        ops = [op for op in ops if op.startswith('prod') or op.startswith('setl') or op == 'x']
    cfgs = CONFIG_BIG if (name == 'D128' and family == 'direct factor') else (CONFIGS[1:] if name in ('D2x', 'D128') else CONFIGS)
    for op in ops:
        for ci, cfg in enumerate(cfgs):
            kw = dict(cfg)
            count = kw.pop('count')
            b0 = R.poke(H.lay, 300 + ci, bool(mat), count=count, wide=True, bdiag=H.Bdiag, **kw)
            case = R.Case(H, count, 400 + ci, warm=1, mat=bool(mat))
            b1, out = L.run([op], b0, case)
            worst[op] = max(worst.get(op, 0.0), R.judge(op, H, b0, case, b1, out))
            if op == 'inv':
                res, cond = R.judge_inverse(H, b0, b1)
                worst['inv residual'] = max(worst.get('inv residual', 0.0), res)
                worst['cond'] = max(worst.get('cond', 0.0), cond)
    print('ratio to the bound', name, family, mat, {k: float('%.3g' % v) for k, v in worst.items()})
    record_deviation('lockstep_kernels', '%s-%s-mat%d' % (name, family, mat), **worst)
    assert max(v for k, v in worst.items() if k != 'cond') <= 1.0, worst


@pytest.mark.parametrize('name', ['D7', 'D9w'])
def test_prod2_is_two_prods_and_the_own_form_is_the_shared_form_bit_for_bit(name):
    L = live(name)
    H = L.H
    b0 = R.poke(H.lay, 51, True, bdiag=H.Bdiag)
    b0.v('WT')[:] = H.WT.reshape(-1, 1)                      # every lane holds the handle's dense rows
    case = R.Case(H, 64, 52, mat=True)
    two, _ = L.run(['prod_x', 'prod_xs'], b0, case)
    one, _ = L.run(['prod2'], b0, case)
    assert np.array_equal(two.ws.view(np.uint64), one.ws.view(np.uint64)) and not np.array_equal(two.ws, b0.ws)
    shared = R.Blk(b0.lay, b0.ws.copy(), None)
    case0 = R.Case(H, 64, 52)
    sh, _ = L.run(['prod_x', 'prod_xs'], shared, case0)
    sh2, _ = L.run(['prod2'], shared, case0)
    assert np.array_equal(sh.ws.view(np.uint64), sh2.ws.view(np.uint64))
    assert np.array_equal(sh.v('pg').view(np.uint64), two.v('pg').view(np.uint64)) and np.array_equal(sh.v('pg2').view(np.uint64), two.v('pg2').view(np.uint64))


def test_inverse_of_a_lane_with_a_non_positive_pivot_is_all_nan_and_its_neighbours_are_untouched():
    L = live('D7')
    H = L.H
    b0 = R.poke(H.lay, 53, False, bdiag=H.Bdiag)
    b0.v('S')[0, 5] = -1.0
    case = R.Case(H, 64, 54)
    b1, out = L.run(['inv'], b0, case)
    R.judge('inv', H, b0, case, b1, out)
    assert np.isnan(b1.v('S')[:, 5]).all() and not np.isnan(b1.v('S')[:, [4, 6]]).any()
    assert R.judge_inverse(H, b0, b1)[0] <= 1.0


@pytest.mark.parametrize('mat', [0, 1])
def test_closed_gate_and_frozen_lanes_of_the_direct_factor(mat):
    L = live('D9')
    H = L.H
    b0 = R.poke(H.lay, 55, bool(mat), bdiag=H.Bdiag)
    b0.v('iw')[R.IW['WORD'], R.WD['RHOANY']] = 0
    b1, out = L.run(['setrho', 'd0', 's', 'inv'], b0, R.Case(H, 64, 56, mat=bool(mat)))
    assert np.array_equal(b0.ws.view(np.uint64), b1.ws.view(np.uint64)) and (not mat or np.array_equal(b0.mat.view(np.uint64), b1.mat.view(np.uint64)))


@pytest.mark.parametrize('mat', [0, 1])
def test_a_direct_solve_after_entry_calls_is_the_solve_without_them(mat):
    P, q, A, l, u = _problem('D7')
    rng = np.random.default_rng(5)
    nb = 70
    Q = q + 0.05 * rng.standard_normal((nb, len(q))) * (q != 0)
    Ax = np.tile(A.data, (nb, 1)) * (1 + 0.02 * rng.standard_normal((nb, A.nnz)) * (np.abs(A.data) != 1.0)) if mat else None
    H = live('D7').H
    res = []
    for poked in (False, True):
        s = osqp_amd.OSQP(algebra='hip'); s.setup(P, q, A, l, u, verbose=False, **dict(ST, max_iter=4000))
        sv = s._solver
        if poked:
            b0 = R.poke(H.lay, 57, bool(mat), bdiag=H.Bdiag)
            case = R.Case(H, 64, 58, mat=bool(mat))
            ops = (['begin', 'asm_a', 'asm_p', 'norms', 'scale', 'cost', 'cost_apply', 'finish', 'wt', 'vals'] if mat else []) + \
                ['load_n', 'load_m', 'init', 'setrho', 'd0', 's', 'inv', 'prod_x', 'prod_xs', 'setl1', 'initz', 'rhs', 'prod_p', 'h', 'x', 'upd', 'prod2', 'setl0', 'resm', 'resn', 'store_n', 'store_m']
            st, _ = sv.hip_test_lockstep(ops, b0.ws, mat_ws=b0.mat, route=1, **case.kw())
            assert st == 0
        res.append(sv.hip_batch_solve_lockstep_direct(q=Q, Ax=Ax))
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b, equal_nan=True)
    assert (res[0][2][:, 0] == 1).any()


@pytest.mark.parametrize('mat', [0, 1])
def test_closed_gates_leave_both_blocks_bit_unchanged(mat):
    L = live('S')
    H = L.H
    for gate, ops in (('RHOANY', ('minv', 'setrho')), ('CGANY', ('t', 'kp', 'cgupd', 'cgp', 'cgalpha', 'cgbeta'))):
        b0 = R.poke(H.lay, 7, bool(mat), bdiag=H.Bdiag)
        b0.v('iw')[R.IW['WORD'], R.WD[gate]] = 0
        case = R.Case(H, 64, 8, mat=bool(mat))
        b1, out = L.run(list(ops), b0, case)
        assert np.array_equal(b0.ws.view(np.uint64), b1.ws.view(np.uint64)), gate
        assert not mat or np.array_equal(b0.mat.view(np.uint64), b1.mat.view(np.uint64)), gate


@pytest.mark.parametrize('mat', [0, 1])
def test_no_cross_lane_traffic(mat):
    """NaN, +-Inf and 1e308 in the lanes >= count and in the frozen lane: every other lane of both blocks, int state and word block included, is
    bit-identical to the run with benign values there, and passes the judge.  A NaN in one LIVE lane's own r (both runs) arrives in its own RN / RZ partial
    and fold, nowhere else."""
    L = live('S')
    H = L.H
    dead = np.r_[2, np.arange(6, 64)]
    alive = np.setdiff1d(np.arange(64), dead)
    for op in ('rhs', 'kp', 'initz', 't', 'upd', 'resm', 'resn', 'cgupd', 'cgp', 'cginit', 'cgbeta'):
        benign = R.poke(H.lay, 9, bool(mat), count=6, frozen=(2,), bdiag=H.Bdiag)
        benign.v('r')[H.n // 2, 3] = np.nan
        b0 = benign.copy()
        for nm, val in (('x', np.nan), ('xs', np.inf), ('p', -np.inf), ('t', 1e308), ('t2', np.nan), ('Kp', np.nan), ('y', np.inf), ('dx', np.nan), ('dy', 1e308)):
            b0.v(nm)[:, dead] = val
        b0.v('part')[:, :, dead] = np.nan
        case = R.Case(H, 6, 10, mat=bool(mat))
        b1, out = L.run([op], b0, case)
        g1, gout = L.run([op], benign, case)
        end = H.lay.fwd['rec'][0]                                # (block vectors, partials, scalar state: lanes are columns; then the records, lanes are rows)
        assert np.array_equal(b1.ws[:end].reshape(-1, 64)[:, alive].view(np.uint64), g1.ws[:end].reshape(-1, 64)[:, alive].view(np.uint64)), op
        assert np.array_equal(b1.v('rec')[alive].view(np.uint64), g1.v('rec')[alive].view(np.uint64)), op
        assert np.array_equal(b1.v('iw')[:R.IW['WORD'], alive], g1.v('iw')[:R.IW['WORD'], alive]) and np.array_equal(b1.v('iw')[R.IW['WORD']], g1.v('iw')[R.IW['WORD']]), op
        assert not mat or np.array_equal(b1.mat.reshape(-1, 64)[:, alive].view(np.uint64), g1.mat.reshape(-1, 64)[:, alive].view(np.uint64)), op
        assert all(np.array_equal(out[k], gout[k], equal_nan=True) for k in ('x', 'y', 'rec')), op
        R.judge(op, H, b0, case, b1, out, skip=dead)
        if op == 'cgupd':
            assert np.isnan(b1.v('part')[R.PS_RN, :, 3]).sum() == 1 and np.isnan(b1.v('part')[R.PS_RZ, :, 3]).sum() == 1
            assert not np.isnan(b1.v('part')[R.PS_RN][:, [0, 1, 4, 5]]).any()
            b2, out = L.run(['cgbeta'], b1, case)
            R.judge('cgbeta', H, b1, case, b2, out, skip=dead)
            assert np.isnan(b2.v('sc')[R.SC['RN'], 3]) and not np.isnan(b2.v('sc')[R.SC['RN'], [0, 1, 4, 5]]).any()


@pytest.mark.parametrize('mat', [0, 1])
def test_lanes_are_problems(mat):
    """the same inputs in all 64 lanes: every output is bit-identical across lanes"""
    L = live('S')
    H = L.H
    b0 = R.identical_lanes(R.poke(H.lay, 12, bool(mat), bdiag=H.Bdiag))
    case = R.Case(H, 64, 13, mat=bool(mat))
    for k in ('q', 'l', 'u', 'x', 'y'):
        setattr(case, k, np.repeat(getattr(case, k)[:1], 64, axis=0))
    for op in ('load_n', 'load_m', 'minv', 'initz', 'rhs', 't', 'kp', 'upd', 'resm', 'resn', 'setrho', 'cgupd', 'cgp', 'cginit', 'cgalpha', 'cgbeta'):
        b1, out = L.run([op], b0, case)
        assert not np.array_equal(b0.ws, b1.ws), op              # (the op ran: its gate was open)
        end = H.lay.fwd['rec'][0]                                # (everything in front of the records: block vectors, partials, scalar state)
        a = b1.ws[:end].reshape(-1, 64)
        assert np.array_equal(a.view(np.uint64), np.repeat(a[:, :1], 64, axis=1).view(np.uint64)), op
        assert (b1.v('iw')[:R.IW['WORD']] == b1.v('iw')[:R.IW['WORD'], :1]).all(), op


@pytest.mark.parametrize('mat', [0, 1])
def test_scaled_lanes_scale_exactly(mat):
    """lane b's inputs are lane 32's times 2^(b - 32): the outputs of the ops that are homogeneous in them scale exactly"""
    L = live('S')
    H = L.H
    for op in R.HOMOGENEOUS:
        b0 = R.scaled_lanes(R.poke(H.lay, 41, bool(mat), bdiag=H.Bdiag), op)
        b1, out = L.run([op], b0, R.Case(H, 64, 42, mat=bool(mat)))
        R.check_scaled_lanes(b1, op)


def test_entry_rejects_before_anything_runs_and_repeats_bit_for_bit():
    L = live('S')
    H, sv = L.H, L.sv
    b0 = R.poke(H.lay, 21, True, bdiag=H.Bdiag)
    case = R.Case(H, 6, 22, mat=True)
    kw = case.kw()
    for ln in ('q_len', 'l_len', 'u_len', 'x_len', 'y_len', 'rec_len', 'px_len', 'ax_len', 'ws_len', 'mat_len'):
        for d in (-1, 1):
            cur = dict(q_len=6 * 70, l_len=6 * 37, u_len=6 * 37, x_len=6 * 70, y_len=6 * 37, rec_len=72, px_len=case.Px.size, ax_len=case.Ax.size,
                       ws_len=b0.ws.size, mat_len=b0.mat.size)[ln]
            st, out = sv.hip_test_lockstep(['rhs'], b0.ws, mat_ws=b0.mat, lens={ln: cur + d}, **kw)
            assert st == VALIDATION and np.array_equal(out['ws'], b0.ws) and np.array_equal(out['mat_ws'], b0.mat), ln
    for bad in (dict(count=0), dict(count=65), dict(route=2), dict(route=-1)):
        k2 = dict(kw); k2.update(bad)
        if 'count' in bad:
            k2.update(q=None, l=None, u=None, x=None, y=None, rec=None, Px=None, Ax=None)
        st, out = sv.hip_test_lockstep(['rhs'], b0.ws, mat_ws=b0.mat, **k2)
        assert st == VALIDATION and np.array_equal(out['ws'], b0.ws), bad
    st, out = sv.hip_test_lockstep(['rhs'], b0.ws, mat_ws=b0.mat, route=1, **kw)
    assert st == NOT_IMPL and np.array_equal(out['ws'], b0.ws)                     # the direct route declines a handle without long rows
    for ops in (['d0'], ['prod2'], ['wt']):                                        # the direct route's ops do not belong to route 0
        st, out = sv.hip_test_lockstep(ops, b0.ws, mat_ws=b0.mat, **kw)
        assert st == VALIDATION and np.array_equal(out['ws'], b0.ws), ops
    D = live('D7')
    bd = R.poke(D.H.lay, 25, False)
    for ops in (['minv'], ['kp'], ['cginit'], ['wt'], ['vals'], ['norms']):        # no PCG on the direct route; the chunk's own rows need mat
        st, out = D.sv.hip_test_lockstep(ops, bd.ws, route=1, **R.Case(D.H, 6, 26).kw())
        assert st == VALIDATION and np.array_equal(out['ws'], bd.ws), ops
    st, out = D.sv.hip_test_lockstep(['rhs'], bd.ws, route=1, lens=dict(ws_len=bd.ws.size - 64), **R.Case(D.H, 6, 26).kw())
    assert st == VALIDATION
    st, out = D.sv.hip_test_lockstep(['rhs'], np.zeros(R.Layout(D.H.n, D.H.m, D.H.lay.nnzA, D.H.lay.nnzB).ws_doubles), **R.Case(D.H, 6, 26).kw())
    assert st == NOT_IMPL                                                          # and the PCG route declines a Woodbury handle
    for ops in ([], ['rhs'] * 65, [len(R.FWD) + 99], [-1]):
        st, out = sv.hip_test_lockstep(ops, b0.ws, mat_ws=b0.mat, **kw)
        assert st == VALIDATION and np.array_equal(out['ws'], b0.ws), ops
    k3 = dict(kw); k3.update(Px=None, Ax=None)
    st, out = sv.hip_test_lockstep(['norms'], b0.ws, **k3)                         # an op of the matrices of a chunk without mat
    assert st == VALIDATION and np.array_equal(out['ws'], b0.ws)
    T = live('T')
    bt = R.poke(T.H.lay, 23, False)
    st, out = T.sv.hip_test_lockstep(['load_m'], bt.ws, **R.Case(T.H, 6, 24).kw())    # an m-side op on an m = 0 handle
    assert st == VALIDATION and np.array_equal(out['ws'], bt.ws)
    ops = ['rhs', 'cginit', 't', 'kp', 'cgalpha', 'cgupd', 'cgbeta', 'cgp', 'upd', 'resm', 'resn']
    a, oa = L.run(ops, b0, case)
    b, ob = L.run(ops, b0, case)
    assert np.array_equal(a.ws.view(np.uint64), b.ws.view(np.uint64)) and np.array_equal(a.mat.view(np.uint64), b.mat.view(np.uint64))
    assert not np.array_equal(a.ws, b0.ws)


def test_declines_on_a_woodbury_handle():
    import problems
    P, q, A, l, u = problems.portfolio_qp(200, 10)
    s = osqp_amd.OSQP(algebra='hip'); s.setup(P, q, A, l, u, verbose=False, eps_abs=1e-6, eps_rel=1e-6)
    assert s._solver.hip_stats()['woodbury_rows'] > 0
    _, sz = s._solver.hip_test_lockstep_sizes()
    st, out = s._solver.hip_test_lockstep(['rhs'], np.ones(sz['ws_need']))
    assert st == NOT_IMPL and (out['ws'] == 1.0).all()


@pytest.mark.parametrize('mat', [0, 1])
def test_a_solve_after_entry_calls_is_the_solve_without_them(mat):
    """x, y, rec of a lockstep solve (70 problems: a full chunk and a ragged one) on a fresh handle, with and without entry calls in front of it"""
    import scipy.sparse as sp
    P, q, A, l, u = _problem('S')
    rng = np.random.default_rng(5)
    nb, m = 70, len(l)
    Ac = sp.csc_matrix(A); Ac.sort_indices()
    z = A @ rng.standard_normal(len(q))                        # bounds around a point: feasible by construction
    kind = np.arange(m) % 5
    l2 = np.where((kind == 2) | (kind == 3), -1e30, np.where(kind == 1, z, z - 1))
    u2 = np.where((kind == 2) | (kind == 4), 1e30, np.where(kind == 1, z, z + 1))
    Q = q + 0.05 * rng.standard_normal((nb, len(q)))
    Ax = np.tile(Ac.data, (nb, 1)) * (1 + 0.02 * rng.standard_normal((nb, Ac.nnz))) if mat else None
    H = live('S').H
    res = []
    for poked in (False, True):
        s = osqp_amd.OSQP(algebra='hip'); s.setup(P, q, A, l2, u2, verbose=False, **dict(ST, max_iter=4000))
        sv = s._solver
        if poked:
            b0 = R.poke(H.lay, 31, bool(mat), bdiag=H.Bdiag)
            case = R.Case(H, 64, 32, mat=bool(mat))
            ops = (['begin', 'asm_a', 'asm_p', 'norms', 'scale', 'cost', 'cost_apply', 'finish'] if mat else []) + \
                ['load_n', 'load_m', 'init', 'setrho', 'minv', 'initz', 'rhs', 'cginit', 'kp', 'cgupd', 'upd', 'store_n', 'store_m']
            st, _ = sv.hip_test_lockstep(ops, b0.ws, mat_ws=b0.mat, **case.kw())
            assert st == 0
        res.append(sv.hip_batch_solve_lockstep(q=Q, Ax=Ax))
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b, equal_nan=True)
    assert (res[0][2][:, 0] == 1).any()                        # (and the solves are solves)
