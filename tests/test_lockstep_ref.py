"""CPU tier of the lockstep kernel tests (tests/lockstep_ref.py: layout, references, the judge): the machinery proved on the numpy stand-in of the entry
(lockstep_ref.Standin: plain fp64 loops over the same block layout with the kernels' strips, unroll, tail and fold orders), on handles built in numpy
alone -- T (n = 3, m = 0) and S (n = 70, m = 37) of the GPU tier and the direct route's r = 7 handle, shared and per-problem matrices.  The reference of
EVERY op of the entry passes its own bound there, the exact checks pass, and EVERY planted mistake below makes the corresponding check fail: a judge that
does not notice them proves nothing on the GPU.  The entry's host side is built and run here as a stand-alone program under ASan / UBSan."""
import numpy as np
import pytest

import lockstep_ref as R
from hostsim_util import hostsim

def _handle(name):
    if name == 'D7':                                         # the direct route: r = 7 long rows, n = 206
        P, q, A, l, u = R.problem_D(*R.DIRECT_HANDLES['D7'])
        return R.Handle.synthetic(P, A, seed=3, direct=True)
    P, q, A, l, u = R.problem_T() if name == 'T' else R.problem_S()
    return R.Handle.synthetic(P, A, seed=3)


@pytest.fixture(scope='module', params=['T', 'S', 'D7'])
def H(request):
    return _handle(request.param)


@pytest.fixture(scope='module')
def HD():
    return _handle('D7')


@pytest.fixture(scope='module')
def HS():
    return _handle('S')


def _ops(H, mat):
    return R.route_ops(H, mat)


def _run(H, op, mat, bug=None, count=R.W, seed=11, warm=1, edit=None, **flags):
    b0 = R.poke(H.lay, seed, mat, count=count, bdiag=H.Bdiag, **flags)
    if edit:
        edit(b0)
    case = R.Case(H, count, seed + 1, warm=warm, mat=mat)
    b1, io = R.Standin(H, bug).call([op], b0, case)
    return b0, case, b1, io


@pytest.mark.parametrize('mat', [0, 1])
def test_every_reference_passes_its_own_bound_on_the_standin(H, mat):
    for op in _ops(H, mat):
        for count, flags in ((64, {}), (6, dict(frozen=(2,), cgoff=(1, 4), rhooff=(0, 3)))):
            b0, case, b1, io = _run(H, op, mat, count=count, wide=True, **flags)
            ratio = R.judge(op, H, b0, case, b1, io)
            assert ratio <= 1.0, (op, count, ratio)
            if op == 'inv':
                assert R.judge_inverse(H, b0, b1)[0] <= 1.0


def test_layout_comes_from_the_carve_and_views_do_not_overlap(HS):
    lay = HS.lay
    b = R.poke(lay, 1, True)
    seen = np.zeros(lay.ws_doubles, int)
    for nm in R.FWD:
        o, c = lay.fwd[nm]
        seen[o:o + c] += 1
    assert seen.max() == 1 and lay.G == 5 and b.v('x').shape == (70, 64) and b.v('z').shape == (37, 64) and b.v('part').shape == (32, 5, 64) and b.v('iw').shape == (12, 64)
    assert lay.fwd['y'][0] == lay.fwd['z'][0] + 37 * 64          # the vector behind z: where a store one row past z lands


PLANTED = [('strip_loses_last_row', 'minv', 0, 'ratio|exact lanes'), ('tail_drops_last_of_5', 'initz', 0, 'ratio'), ('fold_skips_last_partial', 'cginit', 0, 'ratio|iw row|word'),
           ('minv_without_rho_term', 'minv', 0, 'ratio'), ('store_to_frozen_lane', 'rhs', 0, 'exact lanes'), ('store_one_row_past', 'initz', 0, 'outside its outputs'),
           ('lane_reads_next_lane', 'kp', 0, 'ratio'), ('lane_reads_next_lane', 'load_n', 1, 'ratio'), ('norms_without_clamp', 'norms', 1, 'ratio')]


@pytest.mark.parametrize('bug,op,mat,what', PLANTED, ids=['%s-%s' % (b, o) for b, o, _, _ in PLANTED])
def test_checks_notice_a_planted_mistake(HS, bug, op, mat, what):
    b0, case, b1, io = _run(HS, op, mat, count=6, frozen=(2,), wide=True)
    assert R.judge(op, HS, b0, case, b1, io) <= 1.0                   # the same call without the mistake passes
    b0, case, b1, io = _run(HS, op, mat, bug=bug, count=6, frozen=(2,), wide=True)
    with pytest.raises(AssertionError, match=what):
        R.judge(op, HS, b0, case, b1, io)


def test_a_mistake_in_the_last_row_of_a_strip_needs_a_strip_longer_than_one_row():
    """S has rpw = ceil(70 / 20) = 4 on the n side: the planted strip mistake exists there.  T (rpw = 1) cannot show it -- which is why S is a handle."""
    assert R.strips(70, 5)[1] == 4 and R.strips(3, 1)[1] == 1 and [len(g) for g in R.strips(70, 5)[0]] == [16, 16, 16, 16, 6]


@pytest.mark.parametrize('gate,ops', [('RHOANY', ('minv', 'setrho')), ('CGANY', ('t', 'kp', 'cgupd', 'cgp', 'cgalpha', 'cgbeta'))])
def test_a_closed_gate_leaves_the_block_bit_unchanged(HS, gate, ops):
    def close(b):
        b.v('iw')[R.IW['WORD'], R.WD[gate]] = 0
    for op in ops:
        b0, case, b1, io = _run(HS, op, 0, edit=close)
        assert np.array_equal(b0.ws.view(np.uint64), b1.ws.view(np.uint64)), op
        assert R.judge(op, HS, b0, case, b1, io) == 0.0


def test_no_cross_lane_traffic_on_the_standin_and_the_judge_sees_it(HS):
    """NaN, +-Inf and 1e308 planted in the lanes >= count and in a frozen lane: every other lane is bit-identical to the benign run; with the lane mistake
    planted it is not."""
    dead = np.r_[2, np.arange(6, 64)]
    for op in ('rhs', 'kp', 'initz', 'cgupd'):
        outs = []
        for bug in (None, 'lane_reads_next_lane'):
            res = []
            for evil in (False, True):
                def edit(b):
                    if evil:
                        for nm, val in (('x', np.nan), ('xs', np.inf), ('p', -np.inf), ('t', 1e308), ('r', np.nan), ('Kp', np.nan)):
                            b.v(nm)[:, dead] = val
                b0, case, b1, io = _run(HS, op, 0, bug=bug, count=6, frozen=(2,), edit=edit)
                live = np.setdiff1d(np.arange(64), dead)
                res.append(np.concatenate([b1.v(nm)[:, live].ravel() for nm in ('r', 'p', 'Kp', 'z', 't', 'xs')] + [b1.v('part')[:, :, live].ravel()]))
            outs.append(np.array_equal(res[0].view(np.uint64), res[1].view(np.uint64)))
        assert outs[0] and (op != 'kp' or not outs[1]), (op, outs)


def test_lanes_are_problems_on_the_standin(HS):
    """the same inputs in all 64 lanes: every output is bit-identical across lanes"""
    for op in ('minv', 'rhs', 'kp', 'initz', 't', 'cgupd', 'cgp', 'setrho'):
        b0 = R.identical_lanes(R.poke(HS.lay, 11, False, bdiag=HS.Bdiag))
        assert b0.v('iw')[R.IW['WORD'], R.WD['CGANY']] == 1 and b0.v('iw')[R.IW['WORD'], R.WD['RHOANY']] == 1      # (the gates are open: the ops run)
        b1, io = R.Standin(HS).call([op], b0, R.Case(HS, 64, 12))
        assert not np.array_equal(b0.ws, b1.ws), op
        a = b1.ws[:HS.lay.fwd['sc'][0]].reshape(-1, 64)
        assert np.array_equal(a.view(np.uint64), np.repeat(a[:, :1], 64, axis=1).view(np.uint64)), op


def test_scaled_lanes_scale_exactly_on_the_standin_and_a_lane_mistake_does_not(HS):
    for op in R.HOMOGENEOUS:
        b0 = R.scaled_lanes(R.poke(HS.lay, 17, False, bdiag=HS.Bdiag), op)
        case = R.Case(HS, 64, 18)
        R.check_scaled_lanes(R.Standin(HS).call([op], b0, case)[0], op)
    b0 = R.scaled_lanes(R.poke(HS.lay, 17, False, bdiag=HS.Bdiag), 'kp')
    with pytest.raises(AssertionError):
        R.check_scaled_lanes(R.Standin(HS, 'lane_reads_next_lane').call(['kp'], b0, R.Case(HS, 64, 18))[0], 'kp')


def test_direct_handle_has_the_edges_it_is_there_for(HD):
    assert (HD.r, HD.n, HD.lay.GC, HD.lay.cb) == (7, 206, 4, 64) and len(HD.Av[1]) == HD.m and HD.islong.sum() == 7 and (HD.wtpos >= 0).sum() == 6 * 201 + 200


def test_checks_notice_lw_prod_reading_row_r_at_the_two_edge(HD):
    """r = 7: the wave that holds row 6 has no second row; a kernel that reads and stores one anyway reads row 0 of the next column and stores into the next block"""
    b0, case, b1, io = _run(HD, 'prod_x', 1, count=6, frozen=(2,))
    assert R.judge('prod_x', HD, b0, case, b1, io) <= 1.0
    b0, case, b1, io = _run(HD, 'prod_x', 1, bug='prod_two_edge_reads_row_r', count=6, frozen=(2,))
    with pytest.raises(AssertionError, match='ratio|outside its outputs'):
        R.judge('prod_x', HD, b0, case, b1, io)


def test_inverse_of_a_lane_with_a_non_positive_pivot_is_all_nan_and_its_neighbours_are_untouched(HD):
    def edit(b):
        b.v('S')[0, 5] = -1.0
    b0, case, b1, io = _run(HD, 'inv', 0, edit=edit)
    R.judge('inv', HD, b0, case, b1, io)
    assert np.isnan(b1.v('S')[:, 5]).all() and not np.isnan(b1.v('S')[:, [4, 6]]).any()
    worst, cond = R.judge_inverse(HD, b0, b1)
    assert worst <= 1.0 and cond <= R.S_COND


def test_prod2_is_two_prods_and_the_own_form_is_the_shared_one_on_the_standin(HD):
    b0 = R.poke(HD.lay, 5, True, bdiag=HD.Bdiag)
    b0.v('WT')[:] = HD.WT.reshape(-1, 1)                      # every lane holds the handle's dense rows
    case = R.Case(HD, 64, 6, mat=True)
    two, _ = R.Standin(HD).call(['prod_x', 'prod_xs'], b0, case)
    one, _ = R.Standin(HD).call(['prod2'], b0, case)
    assert np.array_equal(two.ws.view(np.uint64), one.ws.view(np.uint64))
    shared = R.Blk(b0.lay, b0.ws.copy(), None)
    sh, _ = R.Standin(HD).call(['prod_x'], shared, R.Case(HD, 64, 6))
    assert np.array_equal(sh.v('pg').view(np.uint64), two.v('pg').view(np.uint64))


def test_the_standin_has_every_op_of_the_entry():
    from osqp_amd import _lib
    assert tuple(R.STANDIN_OPS) == tuple(_lib.LOCKSTEP_OPS) and all(hasattr(R.Ref, 'op_' + op) and hasattr(R.Standin, 'k_' + op) for op in R.STANDIN_OPS)


def test_entry_probe_under_the_host_sanitizers(tmp_path):
    """tests/hostsim/ls_entry_probe.cpp, a stand-alone program: every validation branch of Engine::test_lockstep and the lengths it hands down, built with
    -fsanitize=address,undefined and run as its own process (nothing is loaded into python)."""
    import os
    import subprocess
    root = R.ROOT
    csrc = os.path.join(root, 'osqp-python_amd', 'csrc')
    exe = str(tmp_path / 'ls_entry_probe')
    subprocess.check_call(['g++', '-std=c++17', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-DHOSTSIM_LS_ENTRY_PROBE', '-o', exe,
                           os.path.join(root, 'tests', 'hostsim', 'ls_entry_probe.cpp'), os.path.join(root, 'tests', 'hostsim', 'backend_host.cpp')] +
                          [os.path.join(csrc, f) for f in ('engine.cpp', 'engine_setup.cpp', 'engine_api.cpp', 'api.cpp')])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and 'all checks passed' in r.stdout, r.stdout[-2000:]


def test_the_host_simulator_has_no_lockstep_kernels():
    """The simulator does not define be::test_lockstep: the entry reports the sizes, answers OSQP_FUNC_NOT_IMPLEMENTED and writes nothing."""
    P, q, A, l, u = R.problem_S()
    with hostsim():
        import osqp_amd
        from osqp_amd import ext_hip
        m = osqp_amd.OSQP(algebra='hip')
        m.setup(P, q, A, np.where(np.isinf(l), -1e30, l), np.where(np.isinf(u), 1e30, u), verbose=False)
        st0, sz = m._solver.hip_test_lockstep_sizes()
        ws = np.full(sz['ws_need'], 3.0)
        st, out = m._solver.hip_test_lockstep(['rhs'], ws)
    assert sz['n'] == 70 and sz['m'] == 37 and sz['G'] == 5 and sz['ws_need'] == R.Layout(70, 37, sz['nnzA'], sz['nnzB']).ws_doubles
    assert st0 == st == ext_hip.osqp_error_type.OSQP_FUNC_NOT_IMPLEMENTED and (out['ws'] == 3.0).all()
