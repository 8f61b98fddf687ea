"""GPU tier, kernel level: the PCG forms of osqp-python_amd/csrc/pcg_hip.hip a few ADMM iterations at a time -- k_kb, k_k1 / k_k2 / k_kv, the fused pair
k_k2f / k_k1f, k_ka, the slot kernels k_slot_b / k_slot_a, the one-launch F1 form k_slot1<D, MIX> and the K form k_slotk -- against the long-double recurrence
of tests/pcg_ref.py (reference, fp64 twin, bound and judge; tests/test_pcg_ref.py proves them on the CPU and shows the judge rejecting twelve planted
mistakes).  The diagnostic entry osqp_hip_test_admm pokes scaled iterates into a set-up handle, runs `iters` ADMM iterations with a PCG cap through the
handle's own launch path and peeks every vector, the PCG statistics, the last PCG's scalars and its gamma / alpha (/ beta) history.

Forms are forced through OSQPHipPolicy and every case asserts the form it landed on (0 three-kernel, 1 fused pair enqueued by the host, 2 slot
two-kernel, 3 F1 with its replica count D and the mix flag, 4 K form): a case on another form fails.  Per handle: the (iters, cap) pairs of pcg_ref.RUNS at
tolerance 0 from a seeded normal draw, two stop-rule runs whose PCG counts must equal the reference's exactly, a run after osqp_update_rho and a run after
a matrix-value update by index (k_precond, k_f1_refresh, k_kf_values).  Every peeked vector and scalar within its bound; all forms on the same data agree
pairwise within 2 x the bound wherever the kernels state the same recurrence (the extrapolation weight after a PCG that was cut off at its cap differs
BY DESIGN between the forms the host enqueues and the slot forms -- pcg_hip.hip, the comment above cutoff_theta -- so on runs of two or more iterations
the pairs are taken inside each of the two families); a repeated run is bit-identical; graph = 0 and graph = 1 are bit-identical.

m = 0: the PCG path takes an unconstrained problem in the forms the host enqueues and in the slot two-kernel form (A has no row block: every A-phase
workgroup idles and the B phases do the work); the F1 plan and the K form need constraints (Engine::plan_f1, Engine::prepare_kf) and are not asked for.

The F1 shapes start from tests/test_gpu_f1.py's replica shapes and go down to the smallest sizes Engine::plan_f1 still accepts with the same replica count
(it needs at least kGrid / 4 = 256 row blocks of at least 128 entries), with n and m no multiple of 256; the sizes reached are pcg_ref.CASES'.
"""
import ctypes
import os
import warnings

import numpy as np
import pytest

import osqp_amd
import pcg_ref as R

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
SIGMA, ALPHA = 1e-6, 1.6

BASE = dict(woodbury=0, small_direct=0, reorder=0, window=1, graph=1, kform=0)
FORM_POLICY = {0: dict(pcg_fused=0, slots=0, f1=0), 1: dict(pcg_fused=1, slots=0, f1=0), 2: dict(pcg_fused=1, slots=1, f1=0),
               3: dict(pcg_fused=1, slots=1, f1=1), 4: dict(pcg_fused=1, slots=1, f1=0, kform=1)}
VARIANT = {'': {}, 'window0': dict(window=0), 'reorder2': dict(reorder=2), 'graph0': dict(graph=0)}
F012 = ('random_50x100', 'banded_1537x2999', 'lasso_60x300', 'unstructured_3000', 'unconstrained_50')
F1 = ('f1_D1', 'f1_D2', 'f1_D3', 'f1_D4', 'f1_mix')
# (shape, form, variant): forms 0, 1, 2 on their five shapes and on the banded one again without windows; F1 on its shapes (+ one reordered handle); the K form;
# and, for the pairwise comparison on the same data, the two-kernel forms on one F1 shape and on the K form's shape
CASES = ([(s, f, '') for s in F012 for f in (0, 1, 2)] + [('banded_1537x2999', f, 'window0') for f in (0, 1, 2)] +
         [(s, 3, '') for s in F1] + [('f1_D2', 3, 'reorder2')] + [('kform_333', 4, '')] +
         [('f1_D2', 0, ''), ('f1_D2', 2, ''), ('kform_333', 0, ''), ('kform_333', 2, '')])
GRAPH0 = [('banded_1537x2999', 0), ('banded_1537x2999', 1), ('banded_1537x2999', 2), ('f1_D2', 3), ('kform_333', 4)]


def shape_names():
    return tuple(dict.fromkeys(c[0] for c in CASES))


def case_id(c):
    return '%s-form%d%s' % (c[0], c[1], '-' + c[2] if c[2] else '')


_handles, _states, _outs, _worst = {}, {}, {}, {}


def make_handle(shape, form, variant='', P=None, A=None):
    """a fresh handle of the case: the form's policy as the thread's default while osqp_setup runs"""
    from osqp_amd import _lib
    h = _lib.handle()
    P0, q, A0, l, u = R.problem(shape)
    pol = _lib.PolicyStruct()
    h.osqp_hip_default_policy(ctypes.byref(pol))
    for k, v in {**BASE, **FORM_POLICY[form], **VARIANT[variant]}.items():
        setattr(pol, k, v)
    h.osqp_hip_set_default_policy(ctypes.byref(pol))
    try:
        m = osqp_amd.OSQP(algebra='hip')
        none = A0.shape[0] == 0
        m.setup(P0 if P is None else P, q, None if none else (A0 if A is None else A), None if none else l, None if none else u, **R.SETTINGS)
    finally:
        h.osqp_hip_set_default_policy(None)
    return m


def state_for(m, shape, which, P=None, A=None):
    """the runs of the handle's current state, shared by every handle with the same scaling and rho (bit for bit)"""
    P0, q, A0, l, u = R.problem(shape)
    s = R.scaled_of(m._solver, P0 if P is None else P, q, A0 if A is None else A, l, u, SIGMA, ALPHA)
    st, out = m._solver.hip_test_admm(np.zeros(s.n), np.zeros(s.m), np.zeros(s.m), np.zeros(s.n), 1, 0)
    assert st == 0
    D, E, c = m._solver.hip_scaling()
    key = (shape, which, D.tobytes(), E.tobytes(), c, out['rho'].tobytes(), s.theta)
    if key not in _states:
        _states[key] = R.StateRuns(s, out['rho'], R.SEED)
    return _states[key]


def expect_form(out, shape, form, where, strict=True):
    assert out['form'] == form, 'the handle runs the %s form, not the %s form (%s)' % (R.FORM_NAME.get(out['form']), R.FORM_NAME[form], where)
    if form == 3:
        D, mix = R.F1_EXPECT[shape]
        D = D if strict else None                                  # (a permuted problem has other row blocks: any replica count)
        assert out['f1_mix'] == mix and 1 <= out['f1_D'] <= 4 and (D is None or out['f1_D'] == D), 'F1 with D = %d, mix = %d (%s)' % (out['f1_D'], out['f1_mix'], where)
    else:
        assert out['f1_D'] == 0 and out['f1_mix'] == 0


def outs_of(shape, form, variant=''):
    """Everything one handle has to do, once: the base state's runs judged against the reference (kept for the comparisons between handles), then the run
    after osqp_update_rho and the run after a matrix-value update by index."""
    key = (shape, form, variant)
    if key in _outs:
        return _outs[key]
    where = case_id(key)
    fam = R.FORM_FAMILY[form]
    worst = _worst.setdefault((form, variant), R.Worst())
    m = make_handle(shape, form, variant)
    sv = m._solver

    def entry(*a):
        st, out = sv.hip_test_admm(*a)
        if st == 0:
            expect_form(out, shape, form, where, strict=variant != 'reorder2')
        return st, out
    base = state_for(m, shape, 'base')
    got = R.check_state(entry, base, fam, worst, where, form=form)
    launches = {(r.iters, r.cap, r.tol_abs): o['launches'] for r, o in got.items()}
    for (iters, cap, tol), ln in launches.items():
        if tol == 0.0:                                         # what the form enqueues for a chunk at tolerance 0 (slot forms: one begin + the pairs + one spare pair)
            want = {0: iters * (2 + 3 * cap), 1: iters * (3 + 2 * cap) if cap else iters * 2}.get(form)
            if form >= 2:
                per = {2: 2.0 * (cap + 2), 3: cap + 2.0, 4: cap + 3.0}[form]
                want = 1 + 2 * (int(np.ceil(0.5 * iters * per)) + 1)
            if form != 1:
                assert ln == want, 'launches %d, expected %d (%s, iters %d cap %d)' % (ln, want, where, iters, cap)
    if base.s.m:
        m.update_settings(rho=R.RHO_UPDATE)
        R.check_state(entry, state_for(m, shape, 'rho'), fam, worst, where + ' after osqp_update_rho', form=form, pairs=((3, 3),), stop=False, repeat=False)
    P0, q, A0, l, u = R.problem(shape)
    Px, pi, Ax, ai, P2, A2 = R.updated_matrices(P0, A0)
    if base.s.m:
        m.update(Px=Px, Px_idx=pi, Ax=Ax, Ax_idx=ai)
    else:
        m.update(Px=Px, Px_idx=pi)
    R.check_state(entry, state_for(m, shape, 'mat', P2, A2), fam, worst, where + ' after a matrix update by index', form=form, pairs=((3, 3),), stop=False, repeat=False)
    _outs[key] = (base, got)
    _report()
    return _outs[key]


def _report():
    """the worst measured ratio to the bound per form and per output -> pcg_kernel_entry.txt in the directory OSQP_HIP_TEST_REPORT_DIR names (default: the
    git-ignored prof_out/ of the tree; a copy of a run's file is kept under profiles/).  Best effort: a read-only tree must not fail a test."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = os.environ.get('OSQP_HIP_TEST_REPORT_DIR') or os.path.join(root, 'prof_out')
    try:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, 'pcg_kernel_entry.txt'), 'w') as f:
            f.write('Kernel-level tests of the PCG forms (tests/test_gpu_pcg_kernels.py): worst ratio of the measured error to the bound\n'
                    '64 max(e64, max(n, m) 2^-53) scale of tests/pcg_ref.py, per form and per output, over every shape, run and state of the form\n\n')
            keys = R.N_OUT + R.M_OUT + ('rn0', 'gamma', 'alpha', 'beta')
            f.write('%-28s' % 'form' + ''.join('%9s' % k for k in keys) + '\n')
            for (form, variant), w in sorted(_worst.items()):
                f.write('%-28s' % ('%d %s%s' % (form, R.FORM_NAME[form], ' ' + variant if variant else '')) + ''.join(('%9.4f' % w[k]) if k in w else '%9s' % '-' for k in keys) + '\n')
            f.write('\nshapes (n, m): ' + ', '.join('%s (%d, %d)' % (nm, len(R.problem(nm)[1]), len(R.problem(nm)[3])) for nm in shape_names()) + '\n')
    except OSError:
        pass


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_form_against_the_long_double_recurrence(case):
    base, got = outs_of(*case)
    assert len(got) == len(R.RUNS) + len(R.STOP_RUNS)
    w = _worst[(case[1], case[2])]
    print('%s: worst ratio to the bound so far %s' % (case_id(case), {k: round(v, 4) for k, v in w.items()}))


@pytest.mark.parametrize('shape', shape_names())
def test_all_forms_on_the_same_data_agree_pairwise(shape):
    """within 2 x the bound.  Across the two families the pairs are taken on the runs of one ADMM iteration, where every form states the same recurrence; on
    the longer runs inside each family (pcg_ref.py: the extrapolation weight after a PCG that was cut off at its cap)."""
    cases = [c for c in CASES if c[0] == shape]
    res = [(c, outs_of(*c)) for c in cases]
    pairs = 0
    for a in range(len(res)):
        for b in range(a + 1, len(res)):
            (ca, (sa, ga)), (cb, (sb, gb)) = res[a], res[b]
            if sa is not sb:                                       # (a reordered handle may carry another rounding of the cost scale: its own reference)
                continue
            for run in ga:
                if run in gb:                                      # the same reference run: iters = 1, or the same family
                    R.agree(ga[run], gb[run], run, '%s and %s' % (case_id(ca), case_id(cb)), shape)
                    pairs += 1
    assert pairs > 0 or len(res) == 1


@pytest.mark.parametrize('shape,form', GRAPH0, ids=lambda v: str(v))
def test_eager_launches_equal_graph_replay_bit_for_bit(shape, form):
    _, g1 = outs_of(shape, form, '')
    _, g0 = outs_of(shape, form, 'graph0')
    by_key = {(r.iters, r.cap, r.tol_abs): o for r, o in g0.items()}
    for run, out in g1.items():
        R.same_bits(out, by_key[(run.iters, run.cap, run.tol_abs)], 'graph = 1 and graph = 0', '%s form %d, %s' % (shape, form, run.label()), run.ref['used'][-1])


@pytest.mark.parametrize('shape,form', [('banded_1537x2999', 2), ('f1_D2', 3)], ids=lambda v: str(v))
def test_a_solve_after_the_entry_is_the_solve_of_a_fresh_handle(shape, form):
    """The entry leaves its iterates in the handle; with warm_starting = 0 the next osqp_solve cold-starts: bit for bit the solve of a fresh handle."""
    m = make_handle(shape, form)
    s = R.scaled_of(m._solver, *R.problem(shape), SIGMA, ALPHA)
    st, out = m._solver.hip_test_admm(*R.starts(s, R.SEED), 3, 4)
    assert st == 0 and out['form'] == form
    r1 = m.solve()
    r2 = make_handle(shape, form).solve()
    assert r1.info.status_val == r2.info.status_val and r1.info.iter == r2.info.iter and r1.info.iter > 100      # (whatever the status: the same solve)
    assert np.array_equal(r1.x, r2.x) and np.array_equal(r1.y, r2.y)


def test_entry_refuses_a_woodbury_handle_and_bad_arguments():
    import problems
    P, q, A, l, u = problems.portfolio_qp(200, 10)
    m = osqp_amd.OSQP(algebra='hip'); m.setup(P, q, A, l, u, verbose=False)
    if int(m._solver.hip_stats()['woodbury_rows']) > 0:
        st, out = m._solver.hip_test_admm(np.zeros(len(q)), np.zeros(len(l)), np.zeros(len(l)), np.zeros(len(q)), 1, 1)
        assert st == R.NOT_IMPLEMENTED and all(np.isnan(out[k]).all() for k in R.N_OUT + R.M_OUT)
    m2 = make_handle('random_50x100', 2)
    z = (np.zeros(50), np.zeros(100), np.zeros(100), np.zeros(50))
    for bad in (dict(iters=0), dict(iters=9), dict(cap=17), dict(tol_abs=-1.0), dict(lens=dict(n_len=51)), dict(cap=1, lens=dict(hist_len=2))):
        st, out = m2._solver.hip_test_admm(*z, **bad)
        assert st == R.VALIDATION and all(np.isnan(out[k]).all() for k in R.N_OUT + R.M_OUT), bad
