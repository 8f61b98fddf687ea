"""CPU tier: the direct lockstep route with per-problem matrices, Python side, through the host simulator -- the width checks of
hip_batch_solve_lockstep_direct(Px=, Ax=) run before the C call, a well-formed call reaches the engine (which has no lockstep kernels in the simulator
and declines, the nbatch == 0 query included), the record of the last such call has its eight fields, the new C symbols carry the documented argument
lists (and the three existing direct symbols still theirs), and the torch layer starts with its new counter at 0."""
import numpy as np
import pytest
import scipy.sparse as sp

import osqp_amd
import problems
from osqp_amd import _lib, ext_hip
from hostsim_util import hostsim

NOT_IMPL = ext_hip.osqp_error_type.OSQP_FUNC_NOT_IMPLEMENTED


@pytest.mark.parametrize('problem', ['random', 'portfolio'])
def test_direct_mat_checks_widths_and_reaches_the_engine(problem):
    P, q, A, l, u = problems.random_qp(30, 50, density=0.15, seed=5) if problem == 'random' else problems.portfolio_qp(300, 3)
    n, m, B = P.shape[0], A.shape[0], 4
    nzP, nzA = sp.triu(P, format='csc').nnz, sp.csc_matrix(A).nnz
    with hostsim():
        s = osqp_amd.OSQP(algebra='hip')
        s.setup(P, q, A, l, u, verbose=False)
        solver = s._solver
        assert (solver.nnz_P, solver.nnz_A) == (nzP, nzA)
        good = dict(q=np.tile(q, (B, 1)), l=np.tile(l, (B, 1)), u=np.tile(u, (B, 1)), Px=np.ones((B, nzP)), Ax=np.ones((B, nzA)))
        widths = dict(q=n, l=m, u=m, Px=nzP, Ax=nzA)
        for name in good:
            bad = dict(good)
            bad[name] = np.zeros((B, widths[name] + 1))
            with pytest.raises(ValueError, match=r'^%s: expected %d problems of width %d' % (name, B, widths[name])):
                solver.hip_batch_solve_lockstep_direct(**bad)
        with pytest.raises(ValueError, match=r'^Ax: expected'):                     # nbatch below the arrays' rows
            solver.hip_batch_solve_lockstep_direct(Ax=good['Ax'], nbatch=B - 1)
        for kw in (good, dict(Px=good['Px']), dict(Ax=good['Ax']), dict(q=good['q'], Ax=good['Ax'])):      # right widths: the engine is reached and declines here
            with pytest.raises(ValueError) as e:
                solver.hip_batch_solve_lockstep_direct(**kw)
            assert e.value.code == NOT_IMPL
        for kw in (dict(Px_ptr=None, Ax_ptr=1), dict(Px_ptr=1, Ax_ptr=None)):       # the applicability query of the device entry (nothing is dereferenced)
            with pytest.raises(ValueError) as e:
                solver.hip_batch_solve_lockstep_direct_device(0, None, None, None, None, None, None, **kw)
            assert e.value.code == NOT_IMPL
        rec = solver.lockstep_direct_mat_last_record()
        assert tuple(rec) == ext_hip.OSQPSolver.LOCKSTEP_DIRECT_MAT_LAST_FIELDS and len(rec) == 8
        assert tuple(rec)[-2:] == ('matrix_block_bytes', 'prepare_gpu_ms')
        assert all(v == 0 for v in rec.values())                                    # no such call has run
        assert all(v == 0 for v in solver.lockstep_direct_last_record().values())   # nor has the direct route's own record moved
        assert all(v == 0 for v in solver.lockstep_mat_last_record().values())
        for name, nargs in (('osqp_hip_batch_solve_lockstep_direct_mat', 11), ('osqp_hip_batch_solve_lockstep_direct_mat_device', 12),
                            ('osqp_hip_lockstep_direct_mat_last_record', 2),
                            ('osqp_hip_batch_solve_lockstep_direct', 9), ('osqp_hip_batch_solve_lockstep_direct_device', 10), ('osqp_hip_lockstep_direct_last_record', 2)):
            fn = getattr(solver._lib, name)                                         # (AttributeError: the symbol is not in the library)
            assert len(fn.argtypes) == nargs == len(_lib.PROTOTYPES[name][1])
        for name in ('osqp_hip_batch_solve_lockstep_direct_mat', 'osqp_hip_batch_solve_lockstep_direct_mat_device'):      # the argument order of the lockstep route's entries
            assert _lib.PROTOTYPES[name][1] == _lib.PROTOTYPES[name.replace('_direct', '')][1]


def test_the_torch_layer_counts_the_new_calls_from_zero():
    from osqp_amd.nn.torch import OSQP as Layer
    idx = (np.array([0]), np.array([0]))
    layer = Layer(idx, (1, 1), idx, (1, 1), large_batch='lockstep_direct')
    assert layer.large_batch == 'lockstep_direct' and layer.mat_lockstep_direct_launches == 0 and layer.mat_lockstep_launches == 0
