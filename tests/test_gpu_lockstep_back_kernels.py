"""GPU tier, kernel level: the kernels osqp-python_amd/csrc/lockstep_hip.hip adds for the BACKWARD PASS and for POLISH (k_ls_adj_* / k_lsm_adj_*, k_ls_pol_* /
k_lsm_pol_*, k_lwa_setl, k_lwa_zero), ONE LAUNCH AT A TIME, against np.longdouble references (tests/lockstep_back_ref.py: layout from the carves, one
reference per op, the decisions in fp64 and every int exact; tests/test_lockstep_back_ref.py proves that machinery on a numpy stand-in of every op and shows
that it notices 29 planted mistakes, at least one per op).  The diagnostic entry osqp_hip_test_lockstep_back pokes a random adjoint block (or forward block and
polish block; and matrix block) into the route's resident blocks, launches the named kernel through the drivers' own launch text (ls_adj_go / ls_pol_go /
LwRun::lwa_go) and hands everything back; the judge checks the op's outputs against  err <= 64 max(e64, k 2^-53) scale  per lane and vector, ints, copies,
transposes and untouched lanes bit for bit, and EVERY other double and int of the blocks and of the caller's arrays bit-unchanged.

Handles (tests/lockstep_ref.py; each with the handle's matrices and with per-problem matrices): T (n = 3, m = 0: the has_m == false paths, nzP < 64), S (n = 70,
m = 37: every op), R (S reordered: pc / pr in the tiles, Pmap / Amap in the gradients), C (n = 4100, m = 130, G = 256: the grid-stride and row-pass ops), D7 and
D9w (the direct route: through the view, over n + r rows, k_lwa_*).  Lane sets, each with a frozen lane (IW_DONE): count = 64, count = 6; on S also count = 1 (in polish mode its lane
takes part) and count = 63; polish with IW_POL = 0, 1, 2 in one chunk; pol_begin on a chunk with no lane solved, with every lane solved and with a mix.  On top of the seeded block the poked edges of lockstep_back_ref.poke_edges: bounds at and beyond
+-1e30, z exactly at l / at u / inside and l == u with y of either sign and 0, nact = n - 1, n, n + 1, steps at min_steps and max_steps, an error of exactly
gain * best, a NaN error, worse at its limit, a done lane, g = 0 = r, g = 0 < r, a singular lane, the residual just below / at / just above
OSQP_HIP_ADJOINT_TOL, absent gy / l / u / dl / du / arec, accepted / rejected on either residual / at equality of the accept rule with check_dualgap 0 and 1.  After the judge, lockstep_back_ref.check_edges asserts on
the launch's own output that each edge LANDED on this handle: the pattern it must produce (status 0 0 2, done and worse per lane, 0 3 2 0 3 3, accept -- reject).

Worst ratio to the bound per family and handle as measured on the MI355X (a record, not a tolerance: the assertion is ratio <= 1; the per-op figures go to
util.record_deviation's file and DESIGN.md section 6), handle's matrices / per-problem matrices:
  adjoint transposes  T 0.014 / 0.014   S 0.014 / 0.013   R 0.014 / 0.013   D7 0.015 / 0.015   D9w 0.015 / 0.015
                      (the worst is adj_load_n; adj_grad_p <= 0.010, adj_grad_a <= 0.012; adj_load_m, adj_out_n, adj_out_m are copies and clamps: exact)
  adjoint rows        T 0.014 / 0.014   S 0.015 / 0.015   R 0.015 / 0.015   C 0.015 / 0.015   D7 0.015 / 0.015   D9w 0.014 / 0.015
                      (the worst are the elementwise adj_unscale and adj_class's bounds; the sums: adj_resm <= 0.013, adj_resn <= 0.011; every row code exact)
  adjoint state       exact on every handle (adj_init, adj_decide, adj_final: every int, word, best error and record column bit-equal to the fp64 rule)
  polish rows         T exact   S 0.0017 / 0.0019   R 0.0016 / 0.0011   C 0.0054 / 0.0054   D7 0.011 / 0.010   D9w 0.012 / 0.014
                      (pol_cone; pol_class and pol_end are copies and selects: exact; on D7 / D9w with k_lwa_setl into x as the direct polish launches it)
  polish state        T 0.017 / 0.023   S 0.0045 / 0.0067   R 0.0045 / 0.0048   D7 0.0027 / 0.0025   D9w 0.00056 / 0.00042
                      (pol_accept's objective and gap; pol_begin, pol_decide, the accept decisions, IW_POL and the words exact)
  direct rows         D7 0.0096 / 0.0096   D9w 0.0040 / 0.0040      (k_lwa_setl into x and into x~; k_lwa_zero zeroes exactly n + r rows of x, x~, dx)
No check failed on the GPU: no kernel body was changed.  (One of the issue's example mistakes cannot show in any output and is therefore not planted:
pol_class taking an equality row as UPPER-active stores the same l = u = z, since the two bounds are equal; what is planted instead leaves such a row
inactive.  A gradient clamp that reads entry nz instead of nz - 1 changes no stored entry either -- the clamped columns are never stored; planted instead:
a store gate that admits column nz, and a store loop that stops after four problems.)"""
import warnings

import numpy as np
import pytest

from osqp_amd import ext_hip
from util import record_deviation

import lockstep_ref as R
import lockstep_back_ref as B
from test_gpu_lockstep_kernels import live, _problem

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
VALIDATION = ext_hip.osqp_error_type.OSQP_DATA_VALIDATION_ERROR
NOT_IMPL = ext_hip.osqp_error_type.OSQP_FUNC_NOT_IMPLEMENTED
SECS = 0.125
FAMILIES = {
    'adjoint transposes': ('adj_load_n', 'adj_load_m', 'adj_out_n', 'adj_out_m', 'adj_grad_p', 'adj_grad_a'),
    'adjoint rows': ('adj_class', 'adj_unscale', 'adj_resm', 'adj_resn'),
    'adjoint state': ('adj_init', 'adj_decide', 'adj_final'),
    'polish rows': ('pol_class', 'pol_cone', 'pol_end'),
    'polish state': ('pol_begin', 'pol_decide', 'pol_accept'),
    'direct rows': ('lwa_setl_x', 'lwa_setl_xs', 'lwa_zero'),
}
# the optional arrays an op branches on: every combination the issue names
ABSENT = {'adj_load_m': ((), ('gy',), ('l', 'u')), 'adj_class': ((), ('gy',)), 'adj_out_m': ((), ('dl',), ('du',)), 'adj_final': ((), ('arec',)),
          'adj_grad_p': (('dA',),), 'adj_grad_a': (('dP',),)}
CONFIGS = [dict(count=64, frozen=(7,)), dict(count=6, frozen=(2,))]      # every lane set has a frozen lane (IW_DONE) and, in polish mode, IW_POL = 0, 1, 2
CONFIGS_S = CONFIGS + [dict(count=1), dict(count=63, frozen=(5,))]


class Back:
    """a handle of the forward kernel test with what the backward references need, and the entry"""
    def __init__(self, name):
        self.L = live(name)
        self.sv, self.route = self.L.sv, self.L.route
        P, q, A, l, u = _problem(name)
        self.H = B.back_handle(self.L.H, P, A, l, u)
        self.lay = {mode: B.BackLayout(self.H.lay, mode) for mode in ('adjoint', 'polish')}
        st, sz = self.sv.hip_test_lockstep_back(['adj_init'], np.zeros(1))
        assert st == VALIDATION                                               # (the sizes come back from a rejected call)
        d = 'd' if self.route else ''
        assert self.lay['adjoint'].ws_doubles == sz[d + 'adj_need'] and self.lay['polish'].split == sz[d + 'ws_need'] and self.lay['polish'].pol_doubles == sz['pol_need']
        assert self.H.lay.mat_doubles == sz[d + 'mat_need'] and (sz['n'], sz['m'], sz['nzP'], sz['nzA'], sz['r']) == (self.H.n, self.H.m, len(self.H.Pe[0]), len(self.H.Ae[0]), self.H.r)
        self.P = None

    def call(self, ops, b0, case, **kw):
        lay = b0.lay
        if lay.mode == 'polish':
            args = dict(ws=b0.ws[:lay.split], pol_ws=b0.ws[lay.split:])
        else:
            args = dict(ws=b0.ws)
        args.update(case.kw(), route=self.route)
        args.update(kw)
        return self.sv.hip_test_lockstep_back(ops, mat_ws=b0.mat, secs=SECS, **args)

    def run(self, ops, b0, case):
        st, out = self.call(ops, b0, case)
        assert st == 0, (ops, st)
        ws = out['ws'] if b0.lay.mode == 'adjoint' else np.concatenate([out['ws'], out['pol_ws']])
        self.P = B.Params.from_entry(out, self.sv.get_settings(), SECS)
        return B.BBlk(b0.lay, ws, out['mat_ws']), out

    def params(self, mode):
        """the scalars of a mode, from a call that runs (the references do not restate them)"""
        lay = self.lay[mode]
        b0 = B.bpoke(lay, 1, False)
        self.run(['adj_init' if mode == 'adjoint' else 'pol_begin'], b0, B.BCase(self.H, 6, 2, mode))
        return self.P


_back = {}


def back(name):
    if name not in _back:
        _back[name] = Back(name)
    return _back[name]


def _family_ops(K, family):
    mode = 'polish' if family.startswith('polish') else 'adjoint'
    ops = [op for op in FAMILIES[family] if op in B.back_ops(K.H, mode)]
    return mode, ops + (['lwa_setl_x'] if (K.H.r and family == 'polish rows') else [])      # (the direct polish launches k_lwa_setl into x in front of the cone)


CASES = [(name, family, mat) for name in ('T', 'S', 'R', 'C', 'D7', 'D9w') for family in FAMILIES for mat in (0, 1)
         if (name != 'C' or family in ('adjoint rows', 'polish rows')) and (family != 'direct rows' or name.startswith('D'))]


@pytest.mark.parametrize('name,family,mat', CASES, ids=['%s-%s-mat%d' % (n, f.replace(' ', '_'), m) for n, f, m in CASES])
def test_every_launch_against_its_own_formula(name, family, mat):
    K = back(name)
    H = K.H
    mode, ops = _family_ops(K, family)
    P0 = K.params(mode)
    worst = {}
    for op in ops:
        for ci, cfg in enumerate(CONFIGS_S if name == 'S' else CONFIGS):
            for none in ABSENT.get(op, ((),)):
                for gap in ((0, 1) if op == 'pol_accept' else (None,)):
                    for variant in B.VARIANTS.get(op, (None,)):
                        kw = dict(cfg)
                        count = kw.pop('count')
                        if count == 1 and mode == 'polish':
                            kw['pol'] = {0: 2 if op == 'pol_end' else 1}      # (a chunk of one problem whose lane takes part)
                        b0 = B.bpoke(K.lay[mode], 500 + ci, bool(mat), count=count, bdiag=H.Bdiag, **kw)
                        case = B.BCase(H, count, 600 + ci, mode, none)
                        P = B.Params(**dict(P0.__dict__, check_dualgap=P0.check_dualgap if gap is None else gap))
                        B.poke_edges(op, H, b0, case, P, variant)
                        if gap is not None:
                            K.L.s.update_settings(check_dualgap=bool(gap))
                        try:
                            b1, out = K.run([op], b0, case)
                        finally:
                            if gap is not None:
                                K.L.s.update_settings(check_dualgap=False)
                        assert K.P.check_dualgap == P.check_dualgap
                        worst[op] = max(worst.get(op, 0.0), B.bjudge(op, H, b0, case, b1, out, P))
                        B.check_edges(op, H, b0, case, b1, out, P, variant)      # (the edge landed: the pattern it must produce, on this handle)
    print('ratio to the bound', name, family, mat, {k: float('%.3g' % v) for k, v in worst.items()})
    record_deviation('lockstep_back_kernels', '%s-%s-mat%d' % (name, family, mat), **worst)
    assert max(worst.values()) <= 1.0, worst


def test_the_entry_reports_the_recurrences_scalars():
    K = back('S')
    st = K.sv.get_settings()
    P = K.params('adjoint')
    assert (P.gain, P.max_steps, P.min_steps, P.adjoint_tol) == (0.9, 60, 1 + st.polish_refine_iter, 1e-6) and 1e-6 <= P.rho0 <= 1e6
    Q = K.params('polish')
    assert (Q.pol_max_steps, Q.pol_min_steps, Q.pol_rho) == (30, 1 + st.polish_refine_iter, P.rho0)


@pytest.mark.parametrize('mat', [0, 1])
def test_lwa_zero_zeroes_exactly_n_plus_r_rows_of_three_vectors(mat):
    K = back('D7')
    H, lay = K.H, K.lay['adjoint']
    b0 = B.bpoke(lay, 31, bool(mat), bdiag=H.Bdiag)
    b1, out = K.run(['lwa_zero'], b0, B.BCase(H, 64, 32))
    changed = np.nonzero(b0.ws.view(np.uint64) != b1.ws.view(np.uint64))[0]
    rows = (H.n + H.r) * 64
    assert changed.size == 3 * rows and changed[0] == lay.fwd['x'][0] and changed[-1] == lay.fwd['dx'][0] + rows - 1 and (b1.ws[changed] == 0.0).all()


@pytest.mark.parametrize('mat', [0, 1])
def test_polish_kernels_store_nothing_in_a_lane_that_does_not_take_part(mat):
    """IW_POL = 0 in every lane: pol_class, pol_cone, pol_accept (words apart) and pol_end leave all blocks bit-unchanged"""
    K = back('S')
    H, lay = K.H, K.lay['polish']
    b0 = B.bpoke(lay, 33, bool(mat), bdiag=H.Bdiag, pol={k: 0 for k in range(64)})
    b0.v('iw')[R.IW['WORD'], [R.WD['POLACC'], R.WD['POLREJ']]] = 0
    b1, out = K.run(['pol_class', 'pol_cone', 'pol_accept', 'pol_end'], b0, B.BCase(H, 64, 34, 'polish'))
    assert np.array_equal(b0.ws.view(np.uint64), b1.ws.view(np.uint64)) and (not mat or np.array_equal(b0.mat.view(np.uint64), b1.mat.view(np.uint64)))


def test_entry_rejects_before_anything_runs_and_repeats_bit_for_bit():
    K = back('S')
    H = K.H
    for mode, good, other in (('adjoint', 'adj_init', 'pol_begin'), ('polish', 'pol_begin', 'adj_init')):
        b0 = B.bpoke(K.lay[mode], 41, True, count=6, bdiag=H.Bdiag)
        case = B.BCase(H, 6, 42, mode)
        same = lambda out: np.array_equal(out['ws'], b0.ws[:out['ws'].size]) and np.array_equal(out['mat_ws'], b0.mat) and \
            all(np.array_equal(out[k], getattr(case, k)) for k in case.IO) and (mode == 'adjoint' or np.array_equal(out['pol_ws'], b0.ws[K.lay[mode].split:]))
        size = lambda a: 0 if a is None else a.size
        fwd = b0.ws.size if mode == 'adjoint' else K.lay[mode].split
        cur = dict(sx_len=size(case.sx), sy_len=size(case.sy), gx_len=size(case.gx), gy_len=size(case.gy), l_len=size(case.l), u_len=size(case.u), dq_len=size(case.dq),
                   dl_len=size(case.dl), du_len=size(case.du), dp_len=size(case.dP), da_len=size(case.dA), arec_len=size(case.arec), x_len=size(case.x), y_len=size(case.y),
                   rec_len=size(case.rec), ws_len=fwd, mat_len=b0.mat.size, pol_len=b0.ws.size - fwd)
        for ops in ([other], ['lwa_zero'], ['lwa_setl_x'], [], [good] * 65, [len(B.BACK_OPS)], [-1]):      # the other mode's op, the direct route's ops, nops, the enum
            st, out = K.call(ops, b0, case)
            assert st == VALIDATION and same(out), (mode, ops)
        lens = ('sx_len', 'sy_len', 'gx_len', 'gy_len', 'l_len', 'u_len', 'dq_len', 'dl_len', 'du_len', 'dp_len', 'da_len', 'arec_len', 'ws_len', 'mat_len') if mode == 'adjoint' \
            else ('x_len', 'y_len', 'rec_len', 'ws_len', 'mat_len', 'pol_len')
        for ln in lens:
            for d in (-1, 1):
                st, out = K.call([good], b0, case, lens={ln: cur[ln] + d})
                assert st == VALIDATION and same(out), (mode, ln)
        for bad in (dict(count=0), dict(count=65), dict(route=2), dict(mode=2)):
            st, out = K.call([good], b0, case, **bad)
            assert st == VALIDATION and same(out), bad
        st, out = K.call([good], b0, case, route=1)                              # the direct route declines a handle without long rows
        assert st == NOT_IMPL and same(out)
        a, oa = K.run([good], b0, case)
        b, ob = K.run([good], b0, case)
        assert np.array_equal(a.ws.view(np.uint64), b.ws.view(np.uint64)) and not np.array_equal(a.ws, b0.ws)
    # the arrays of the other mode, an output op without its array
    b0 = B.bpoke(K.lay['adjoint'], 43, False, count=6)
    case = B.BCase(H, 6, 44)
    st, out = K.call(['adj_init'], b0, case, x=np.zeros((6, H.n)))
    assert st == VALIDATION and np.array_equal(out['ws'], b0.ws)
    for op, none in (('adj_out_n', ('dq',)), ('adj_out_m', ('dl', 'du')), ('adj_grad_p', ('dP',)), ('adj_grad_a', ('dA',))):
        st, out = K.call([op], b0, B.BCase(H, 6, 44, 'adjoint', none))
        assert st == VALIDATION and np.array_equal(out['ws'], b0.ws), op
    # m = 0: every m-side op and the gradient of A are declined
    T = back('T')
    for mode, ops in (('adjoint', ('adj_load_m', 'adj_class', 'adj_resm', 'adj_out_m', 'adj_grad_a')), ('polish', ('pol_cone',))):
        bt = B.bpoke(T.lay[mode], 45, False, count=6)
        for op in ops:
            st, out = T.call([op], bt, B.BCase(T.H, 6, 46, mode))
            assert st == VALIDATION and np.array_equal(out['ws'], bt.ws[:out['ws'].size]), op
    # the PCG route declines a Woodbury handle, in both modes
    D = back('D7')
    for mode in ('adjoint', 'polish'):
        lay0 = B.BackLayout(R.Layout(D.H.n, D.H.m, D.H.lay.nnzA, D.H.lay.nnzB), mode)
        bd = B.bpoke(lay0, 47, False, count=6)
        st, out = D.call(['adj_init' if mode == 'adjoint' else 'pol_begin'], bd, B.BCase(D.H, 6, 48, mode), route=0)
        assert st == NOT_IMPL and np.array_equal(out['ws'], bd.ws[:out['ws'].size]), mode


@pytest.mark.parametrize('mat', [0, 1])
def test_a_backward_pass_and_a_polished_solve_after_entry_calls_are_the_ones_without_them(mat):
    import osqp_amd
    import scipy.sparse as sp
    from test_gpu_lockstep_kernels import ST
    P, q, A, l, u = _problem('S')
    rng = np.random.default_rng(5)
    nb, n, m = 70, len(q), len(l)
    Ac = sp.csc_matrix(A); Ac.sort_indices()
    z = A @ rng.standard_normal(n)
    kind = np.arange(m) % 5
    l2 = np.where((kind == 2) | (kind == 3), -1e30, np.where(kind == 1, z, z - 1))
    u2 = np.where((kind == 2) | (kind == 4), 1e30, np.where(kind == 1, z, z + 1))
    Q = q + 0.05 * rng.standard_normal((nb, n))
    Ax = np.tile(Ac.data, (nb, 1)) * (1 + 0.02 * rng.standard_normal((nb, Ac.nnz))) if mat else None
    K = back('S')
    H = K.H
    res = []
    for poked in (False, True):
        s = osqp_amd.OSQP(algebra='hip'); s.setup(P, q, A, l2, u2, verbose=False, **dict(ST, max_iter=4000, polishing=True))
        sv = s._solver
        if poked:
            for mode, ops in (('polish', ['pol_begin', 'pol_class', 'pol_decide', 'pol_cone', 'pol_accept', 'pol_end']),
                              ('adjoint', ['adj_load_n', 'adj_load_m', 'adj_class', 'adj_init', 'adj_decide', 'adj_unscale', 'adj_resm', 'adj_resn', 'adj_final', 'adj_out_n', 'adj_out_m',
                                           'adj_grad_p', 'adj_grad_a'])):
                b0 = B.bpoke(K.lay[mode], 51, bool(mat), bdiag=H.Bdiag)
                args = dict(ws=b0.ws[:K.lay[mode].split], pol_ws=b0.ws[K.lay[mode].split:]) if mode == 'polish' else dict(ws=b0.ws)
                st, _ = sv.hip_test_lockstep_back(ops, mat_ws=b0.mat, **args, **B.BCase(H, 64, 52, mode).kw())
                assert st == 0
        x, y, rec = sv.hip_batch_solve_lockstep(q=Q, Ax=Ax)
        g = sv.hip_batch_adjoint_lockstep(np.nan_to_num(x), np.nan_to_num(y), np.ones_like(x), dy=0.5 * np.ones_like(y), Ax=Ax)
        rec[:, 9] = 0.0                                          # (polish seconds: a clock)
        res.append((x, y, rec) + tuple(g[k] for k in sorted(g)))
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b, equal_nan=True)
    assert (res[0][2][:, 8] != 0).any()                          # (and polish ran)
