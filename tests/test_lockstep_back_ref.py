"""CPU tier of the kernel tests of the lockstep BACKWARD PASS and POLISH (tests/lockstep_back_ref.py: layout, references, the judge): the machinery proved on
the numpy stand-in of the entry osqp_hip_test_lockstep_back (lockstep_back_ref.BackStandin), on handles built in numpy alone -- T (n = 3, m = 0), S (n = 70,
m = 37) and the direct route's r = 7 handle, shared and per-problem matrices, at count = 64, 6 and 1, each with a frozen lane or a lane that takes part.  The reference of EVERY op passes its own bound there with the issue's poked
edges in place, the exact checks pass, and EVERY planted mistake below -- at least one per op -- makes the corresponding check fail."""
import numpy as np
import pytest

import lockstep_ref as R
import lockstep_back_ref as B

P0 = B.Params()


def _handle(name):
    direct = name == 'D7'
    P, q, A, l, u = R.problem_D(*R.DIRECT_HANDLES['D7']) if direct else (R.problem_T() if name == 'T' else R.problem_S())
    H = R.Handle.synthetic(P, A, seed=3, direct=direct)
    return B.back_handle(H, P, A, np.maximum(l, -1e30), np.minimum(u, 1e30))


_H = {}


def handle(name):
    if name not in _H:
        _H[name] = _handle(name)
    return _H[name]


def _mode(op):
    return 'polish' if op in B.POL_OPS else 'adjoint'


def _run(H, op, mat, bug=None, count=R.W, seed=11, none=(), mode=None, frozen=(), P=P0, edges=True, variant=None, pol=None):
    mode = mode or _mode(op)
    lay = B.BackLayout(H.lay, mode)
    b0 = B.bpoke(lay, seed, mat, count=count, frozen=frozen, bdiag=H.Bdiag, pol=pol)
    case = B.BCase(H, count, seed + 1, mode, none)
    if edges:
        B.poke_edges(op, H, b0, case, P, variant)
    b1, io = B.BackStandin(H, P, bug).call([op], b0, case)
    return b0, case, b1, io


@pytest.mark.parametrize('mat', [0, 1])
@pytest.mark.parametrize('name', ['T', 'S', 'D7'])
@pytest.mark.parametrize('mode', ['adjoint', 'polish'])
def test_every_reference_passes_its_own_bound_on_the_standin(name, mode, mat):
    H = handle(name)
    for op in B.back_ops(H, mode):
        for count, frozen in ((64, (7,)), (6, (2,)), (1, ())):
            for gap in ((0, 1) if op == 'pol_accept' else (0,)):
                for variant in B.VARIANTS.get(op, (None,)):
                    P = B.Params(check_dualgap=gap)
                    pol = {0: 2 if op == 'pol_end' else 1} if count == 1 else None      # (a chunk of one problem whose lane takes part)
                    b0, case, b1, io = _run(H, op, mat, count=count, frozen=frozen, mode=mode, P=P, variant=variant, pol=pol)
                    assert B.bjudge(op, H, b0, case, b1, io, P) <= 1.0, (op, count)
                    B.check_edges(op, H, b0, case, b1, io, P, variant)


def test_optional_arrays_absent():
    """gy, l, u absent: zero / the handle's own bounds; dl only, du only; a null arec: adj_final writes nothing anywhere"""
    H = handle('S')
    for op, none in (('adj_load_m', ('gy',)), ('adj_load_m', ('l', 'u')), ('adj_class', ('gy',)), ('adj_out_m', ('dl',)), ('adj_out_m', ('du',)), ('adj_final', ('arec',))):
        b0, case, b1, io = _run(H, op, 0, count=6, none=none)
        assert B.bjudge(op, H, b0, case, b1, io, P0) <= 1.0, (op, none)
    b0, case, b1, io = _run(H, 'adj_final', 0, count=6, none=('arec',))
    assert np.array_equal(b0.ws.view(np.uint64), b1.ws.view(np.uint64))


def test_layout_comes_from_the_carves():
    H = handle('S')
    la, lp = B.BackLayout(H.lay, 'adjoint'), B.BackLayout(H.lay, 'polish')
    assert [la.fwd[k][1] for k in B.ADJV] == [70 * 64] * 3 + [37 * 64] * 3 + [37 * 32] and la.fwd['ax'][0] == H.lay.ws_doubles
    assert [lp.fwd[k][1] for k in B.POLV] == [70 * 64] + [37 * 64] * 4 and lp.fwd['sx'][0] == lp.split == H.lay.ws_doubles and lp.pol_doubles == 64 * (70 + 4 * 37) + 64
    b = B.bpoke(la, 1, False)
    assert b.v('code').shape == (37, 64) and set(np.unique(b.v('code'))) == {0, 1, 2}
    D = handle('D7')
    ld = B.BackLayout(D.lay, 'adjoint')
    assert ld.fwd['ax'][0] == D.lay.ws_doubles and ld.fwd['x'][1] == (D.n + 7) * 64 and 'Kp' not in ld.fwd


def test_the_edges_are_where_the_issue_puts_them():
    H = handle('S')
    b0, case, b1, io = _run(H, 'adj_init', 0, count=6)
    assert list(b1.v('iw')[R.IW['STATUS'], :3]) == [0, 0, 2] and list(b1.v('sc')[R.SC['NACT'], :3]) == [69.0, 70.0, 71.0]
    b0, case, b1, io = _run(H, 'adj_decide', 0)
    iw = b1.v('iw')
    assert list(iw[R.IW['DONE'], :7]) == [1, 1, 0, 0, 1, 1, 0] and list(iw[R.IW['WORSE'], :7]) == [0, 0, 1, 1, 2, 0, 0]      # lane 2: exactly gain * best is no progress
    assert iw[R.IW['WORD'], R.WD['LIVE']] == (iw[R.IW['DONE']] == 0).sum() and iw[R.IW['WORD'], R.WD['PCGSUM']] == iw[R.IW['PCG']].sum()
    b0, case, b1, io = _run(H, 'adj_final', 0)
    assert list(io['arec'][:6, 0]) == [0.0, 3.0, 2.0, 0.0, 3.0, 3.0] and list(io['arec'][:3, 2]) == [0.0, np.inf, np.inf]
    b0, case, b1, io = _run(H, 'adj_class', 0)
    assert list(b1.v('code')[:8, 3]) == [0, 0, 0, 2, 1, 2, 2, 1]      # z at l, at u, inside: inactive with y = 0; l == u: by the sign of y, y = 0 upper; y against the bound
    for gap in (0, 1):
        P = B.Params(check_dualgap=gap)
        b0, case, b1, io = _run(H, 'pol_accept', 0, P=P)
        assert list(b1.v('rec')[:4, 8]) == [1.0, -1.0, -1.0, -1.0] and list(b1.v('iw')[R.IW['POL'], :4]) == [1, 2, 2, 2]
        assert (b1.v('rec')[0, 11] != b0.v('rec')[0, 11]) == bool(gap)
    b0, case, b1, io = _run(H, 'pol_cone', 0)
    assert (b1.v('y')[1::4, 1] == 0.0).all() and (b1.v('y')[2::4, 1] < 0).all() and (b1.v('y')[3::4, 1] > 0).all()
    b0, case, b1, io = _run(H, 'pol_begin', 0, count=6)
    assert b1.v('iw')[R.IW['WORD'], R.WD['LIVE']] == (b0.v('iw')[R.IW['STATUS'], :6] == 1).sum()


#           mistake, op, handle, count, what the judge must say
PLANTED = [('load_n_without_dinv', 'adj_load_n', 'S', 64, 'ratio'), ('load_m_dead_lane_upper_sign', 'adj_load_m', 'S', 6, 'exact lanes'),
           ('class_without_equality_override', 'adj_class', 'S', 64, 'code'), ('init_singular_at_equality', 'adj_init', 'S', 64, 'iw row|word'),
           ('decide_keeps_worse', 'adj_decide', 'S', 64, 'iw row'), ('decide_one_step_late', 'adj_decide', 'S', 64, 'iw row|word'),
           ('unscale_keeps_y_on_code0', 'adj_unscale', 'S', 64, 'exact lanes'), ('resm_counts_code0', 'adj_resm', 'S', 64, 'ratio|exact lanes'),
           ('resn_without_sigma', 'adj_resn', 'S', 64, 'ratio'), ('final_inverted_at_g0', 'adj_final', 'S', 64, 'arec'), ('final_tol_inclusive', 'adj_final', 'S', 64, 'arec'),
           ('out_n_reads_ax', 'adj_out_n', 'S', 6, 'exact lanes'), ('out_m_sides_swapped', 'adj_out_m', 'S', 6, 'exact lanes'),
           ('grad_p_without_half', 'adj_grad_p', 'S', 6, 'ratio'), ('grad_a_ry_ay_exchanged', 'adj_grad_a', 'S', 6, 'ratio'),
           ('grad_store_loop_stops_at_4', 'adj_grad_p', 'S', 6, 'ratio'), ('grad_store_gate_admits_nz', 'adj_grad_a', 'S', 6, 'ratio'),
           ('setl_one_row_early', 'lwa_setl_x', 'D7', 64, 'ratio|outside'), ('setl_one_row_early', 'lwa_setl_xs', 'D7', 64, 'ratio|outside'), ('zero_one_row_past', 'lwa_zero', 'D7', 64, 'outside its outputs'),
           ('begin_polishes_dead_lane', 'pol_begin', 'S', 6, 'iw row|word'), ('begin_rhoany_always_1', 'pol_begin', 'S', 64, 'word 2'), ('polclass_equality_not_forced', 'pol_class', 'S', 64, 'exact lanes'),
           ('class_stores_unpolished_lane', 'pol_class', 'S', 64, 'exact lanes'), ('decide_keeps_worse', 'pol_decide', 'S', 64, 'iw row'),
           ('cone_keeps_u', 'pol_cone', 'S', 64, 'exact lanes'), ('accept_writes_rejected_rc3', 'pol_accept', 'S', 64, 'exact lanes'),
           ('accept_at_equality', 'pol_accept', 'S', 64, 'iw row|word'), ('end_restores_accepted', 'pol_end', 'S', 64, 'exact lanes')]


@pytest.mark.parametrize('bug,op,name,count,what', PLANTED, ids=['%s-%s' % (b, o) for b, o, _, _, _ in PLANTED])
def test_checks_notice_a_planted_mistake(bug, op, name, count, what):
    H = handle(name)
    variant = 'none' if bug == 'begin_rhoany_always_1' else None      # (the empty ballot: the only state in which the word is 0)
    b0, case, b1, io = _run(H, op, 0, count=count, variant=variant)
    assert B.bjudge(op, H, b0, case, b1, io, P0) <= 1.0                  # the same call without the mistake passes
    b0, case, b1, io = _run(H, op, 0, bug=bug, count=count, variant=variant)
    with pytest.raises(AssertionError, match=what):
        B.bjudge(op, H, b0, case, b1, io, P0)


def test_every_op_with_an_output_has_a_planted_mistake_and_the_standin_has_every_op():
    from osqp_amd import _lib
    assert tuple(B.BACK_OPS) == tuple(_lib.LOCKSTEP_BACK_OPS)
    assert all(hasattr(B.BackRef, 'op_' + op) and hasattr(B.BackStandin, 'k_' + op) for op in B.BACK_OPS)
    assert {op for _, op, _, _, _ in PLANTED} == set(B.BACK_OPS)


def test_the_struct_mirror_has_the_size_and_the_offsets_of_the_header(tmp_path):
    """OSQPHipLockstepBackTest against its ctypes mirror: sizeof and the offset of every field, from a C program that includes the header"""
    import ctypes
    import os
    import subprocess
    from osqp_amd import _lib
    names = [f[0] for f in _lib.LockstepBackTestStruct._fields_]
    src = tmp_path / 'mirror.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "osqp_hip.h"\nint main(void) {\n  printf("%zu", sizeof(OSQPHipLockstepBackTest));\n' +
                   ''.join('  printf(" %%zu", offsetof(OSQPHipLockstepBackTest, %s));\n' % k for k in names) + '  return 0;\n}\n')
    exe = str(tmp_path / 'mirror')
    subprocess.check_call(['gcc', '-I', os.path.join(R.ROOT, 'include'), '-o', exe, str(src)])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [ctypes.sizeof(_lib.LockstepBackTestStruct)] + [getattr(_lib.LockstepBackTestStruct, k).offset for k in names]


def test_entry_probe_under_the_host_sanitizers(tmp_path):
    """tests/hostsim/ls_back_entry_probe.cpp, a stand-alone program: the validation branches of Engine::test_lockstep_back in both modes, the lengths it hands
    down and its copies of the blocks, built with -fsanitize=address,undefined and run as its own process (nothing is loaded into python)."""
    import os
    import subprocess
    root = R.ROOT
    csrc = os.path.join(root, 'osqp-python_amd', 'csrc')
    exe = str(tmp_path / 'ls_back_entry_probe')
    subprocess.check_call(['g++', '-std=c++17', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-DHOSTSIM_LS_ENTRY_PROBE', '-o', exe,
                           os.path.join(root, 'tests', 'hostsim', 'ls_back_entry_probe.cpp'), os.path.join(root, 'tests', 'hostsim', 'backend_host.cpp')] +
                          [os.path.join(csrc, f) for f in ('engine.cpp', 'engine_setup.cpp', 'engine_api.cpp', 'api.cpp')])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and 'all checks passed' in r.stdout, r.stdout[-2000:]


def test_the_host_simulator_has_no_such_kernels():
    """The simulator does not define be::test_lockstep_back: the entry reports the sizes, answers OSQP_FUNC_NOT_IMPLEMENTED and writes nothing."""
    from hostsim_util import hostsim
    P, q, A, l, u = R.problem_S()
    with hostsim():
        import osqp_amd
        from osqp_amd import ext_hip
        m = osqp_amd.OSQP(algebra='hip')
        m.setup(P, q, A, np.where(np.isinf(l), -1e30, l), np.where(np.isinf(u), 1e30, u), verbose=False)
        st, out = m._solver.hip_test_lockstep_back(['adj_init'], np.full(10, 3.0))
    H = handle('S')
    assert st == ext_hip.osqp_error_type.OSQP_FUNC_NOT_IMPLEMENTED and (out['ws'] == 3.0).all()
    assert (out['n'], out['m'], out['G']) == (70, 37, 5) and out['pol_need'] == B.BackLayout(H.lay, 'polish').pol_doubles
