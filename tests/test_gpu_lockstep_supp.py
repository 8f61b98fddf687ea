"""GPU tier, kernel level: k_ls_supp (osqp-python_amd/csrc/lockstep_hip.hip; settings.check_dualgap), ONE LAUNCH through osqp_hip_test_lockstep's op
'supp', on handles of tests/test_gpu_lockstep_kernels.py's set: S (n = 70, m = 37, G = 5: ragged strips, every row class) with the handle's matrices and
with per-problem matrices, D7 (the direct route, m = 207, G = 13: the dense rows are rows of l, u, y like the others) both ways, C (m = 130 at G = 256: most waves
have no row).  A full chunk (count = 64) and a ragged one (count = 6, a frozen lane).  The poked block has rows with one and with both sides infinite and
equality rows; y takes both signs and, planted here, exact zeros.

The judge is tests/gap_ref.py judge_supp (tests/test_batch_gap_rules.py shows that it passes a stand-in and catches four planted mistakes): every
workgroup's partial in slot PS_PKP and the folded sum against the np.longdouble sum of the same terms, bound gamma_k sum |terms| with k counted from the
kernel's own order -- a term passes through 1 rounding of its product, at most ceil(m / 4 G) adds in its lane (rows 4 g + w, + 4 G, ..), 3 adds over the
four waves: k = 4 + ceil(m / 4 G) for a partial; ceil(G / 4) + 3 more through the fold.  S: k = 6 / 11, D7: 8 / 15, C: 5 / 72.  The assertion is ratio <= 1.
Everything else in the work block, the matrix block and the caller's arrays is bit-unchanged, two calls give the same bits, and the kernel's bits are the
stand-in's: the result depends on (m, G) alone, not on the chunk's fill.

Measured on the MI355X, worst ratio to the bound (a record, not a tolerance): S 0.42 / 0.33, D7 0.30 / 0.29, C 0.46 / 0.35 (shared / per-problem matrices;
DESIGN.md section 6 "Duality gap on the batch routes")."""
import warnings

import numpy as np
import pytest

import gap_ref as G
import lockstep_ref as R
from test_gpu_lockstep_kernels import live
from util import record_deviation

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
CONFIGS = [dict(count=64), dict(count=6, frozen=(2,))]
CASES = [(name, mat) for name in ('S', 'D7', 'C') for mat in (0, 1)]


@pytest.mark.parametrize('name,mat', CASES, ids=['%s-mat%d' % c for c in CASES])
def test_one_launch_against_the_long_double_sum(name, mat):
    L = live(name)
    H = L.H
    worst = 0.0
    parts = []
    for ci, cfg in enumerate(CONFIGS):
        kw = dict(cfg)
        count = kw.pop('count')
        b0 = R.poke(H.lay, 700 + ci, bool(mat), count=count, wide=True, bdiag=H.Bdiag, **kw)
        rng = np.random.default_rng(710 + ci)
        y = b0.v('y')
        y[rng.random(y.shape) < 0.15] = 0.0
        l, u = b0.v('l'), b0.v('u')
        assert (y > 0).any() and (y < 0).any() and (y == 0).any()
        assert ((l < -1e29) & (u > 1e29)).any() and ((l < -1e29) & (u < 1e29)).any() and ((l > -1e29) & (u > 1e29)).any() and (l == u).any()
        case = R.Case(H, count, 720 + ci, warm=1, mat=bool(mat))
        b1, out = L.run(['supp'], b0, case)
        part = b1.v('part')[R.PS_PKP]
        worst = max(worst, G.judge_supp(part, l, u, y, H.G))
        assert np.array_equal(part.view(np.uint64), G.standin_supp(l, u, y, H.G).view(np.uint64))      # the kernel's order is the stand-in's
        assert not np.array_equal(part, b0.v('part')[R.PS_PKP])
        # everything else: bit-unchanged
        keep = b0.copy()
        keep.v('part')[R.PS_PKP] = part
        assert np.array_equal(keep.ws.view(np.uint64), b1.ws.view(np.uint64))
        assert not mat or np.array_equal(b0.mat.view(np.uint64), b1.mat.view(np.uint64))
        for key, src in (('x', case.x), ('y', case.y), ('rec', case.rec)):
            assert np.array_equal(np.asarray(out[key]).ravel().view(np.uint64), np.ascontiguousarray(src).ravel().view(np.uint64)), key
        b2, _ = L.run(['supp'], b0, case)
        assert np.array_equal(b1.ws.view(np.uint64), b2.ws.view(np.uint64))
        parts.append(part)
    print('ratio to the bound', name, mat, worst, 'roundings', G.supp_roundings(H.m, H.G))
    record_deviation('lockstep_kernels', '%s-supp-mat%d' % (name, mat), supp=worst)


def test_the_sum_of_a_lane_does_not_depend_on_the_fill():
    """the same column of l, u, y in lane 3 of a full chunk and of a chunk of four: the same partials, bit for bit"""
    L = live('S')
    H = L.H
    res = []
    for count, seed in ((64, 730), (4, 731)):
        b0 = R.poke(H.lay, seed, False, count=count, bdiag=H.Bdiag)
        if res:
            for nm in ('l', 'u', 'y'):
                b0.v(nm)[:, 3] = res[0][1].v(nm)[:, 3]
        b1, _ = L.run(['supp'], b0, R.Case(H, count, seed + 10, warm=1))
        res.append((b1.v('part')[R.PS_PKP][:, 3].copy(), b0))
    assert np.array_equal(res[0][0].view(np.uint64), res[1][0].view(np.uint64)) and np.abs(res[0][0]).max() > 0


def test_the_entry_takes_the_op_where_a_solve_launches_it():
    """'supp' belongs to both routes, with and without per-problem matrices; like the other m-side kernels it needs m > 0 (T has no row)"""
    from osqp_amd import ext_hip
    L = live('T')
    _, sz = L.sv.hip_test_lockstep_sizes()
    st, _ = L.sv.hip_test_lockstep(['supp'], np.zeros(sz['ws_need']))
    assert st == ext_hip.osqp_error_type.OSQP_DATA_VALIDATION_ERROR
