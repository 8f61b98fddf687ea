"""CPU tier: the lockstep route with per-problem matrices (osqp_hip_batch_solve_lockstep_mat) through the host simulator -- the width checks of
hip_batch_solve_lockstep(Px=, Ax=) run before the C call, a well-formed call reaches the engine (which has no lockstep kernels and no device
assembly in the simulator and declines), the record and the scaling query answer as before a first call, and the four C symbols carry the
documented argument lists."""
import numpy as np
import pytest

import osqp_amd
import problems
from osqp_amd import _lib, ext_hip
from hostsim_util import hostsim

E = ext_hip.osqp_error_type


def test_lockstep_mat_checks_widths_and_reaches_the_engine():
    P, q, A, l, u = problems.random_qp(30, 50, density=0.15, seed=5)
    n, m, B = P.shape[0], A.shape[0], 4
    with hostsim():
        s = osqp_amd.OSQP(algebra='hip')
        s.setup(P, q, A, l, u, verbose=False)
        solver = s._solver
        nzP, nzA = solver.nnz_P, solver.nnz_A
        assert nzP > 0 and nzA > 0
        good = dict(Px=np.ones((B, nzP)), Ax=np.ones((B, nzA)), q=np.tile(q, (B, 1)), l=np.tile(l, (B, 1)), u=np.tile(u, (B, 1)), x0=np.zeros((B, n)), y0=np.zeros((B, m)))
        widths = dict(Px=nzP, Ax=nzA, q=n, l=m, u=m, x0=n, y0=m)
        for name in good:
            bad = dict(good)
            bad[name] = np.zeros((B, widths[name] + 1))
            with pytest.raises(ValueError, match=r'^%s: expected %d problems of width %d' % (name, B, widths[name])):
                solver.hip_batch_solve_lockstep(**bad)
        with pytest.raises(ValueError, match=r'^Px: expected'):                    # nbatch below the arrays' rows
            solver.hip_batch_solve_lockstep(Px=good['Px'], nbatch=B - 1)
        for kw in (good, dict(Px=good['Px']), dict(Ax=good['Ax']), dict(Ax=good['Ax'], q=good['q'])):      # right widths: the engine is reached and declines here
            with pytest.raises(ValueError) as e:
                solver.hip_batch_solve_lockstep(**kw)
            assert e.value.code == E.OSQP_FUNC_NOT_IMPLEMENTED
        with pytest.raises(ValueError) as e:                                        # the applicability query of the device entry
            solver.hip_batch_solve_lockstep_device(0, None, None, None, None, None, None, Px_ptr=0, Ax_ptr=0)
        assert e.value.code == E.OSQP_FUNC_NOT_IMPLEMENTED
        rec = solver.lockstep_mat_last_record()
        assert tuple(rec) == ext_hip.OSQPSolver.LOCKSTEP_MAT_LAST_FIELDS and len(rec) == 8
        assert tuple(rec) == ('chunks', 'width', 'admm_iters_max', 'pcg_iters', 'kernel_launches', 'gpu_ms', 'matrix_block_bytes', 'prepare_gpu_ms')
        assert all(v == 0 for v in rec.values())                                    # no such call has run
        with pytest.raises(ValueError) as e:
            solver.lockstep_mat_scaling(0)
        assert e.value.code == E.OSQP_DATA_NOT_INITIALIZED
        for name, nargs in (('osqp_hip_batch_solve_lockstep_mat', 11), ('osqp_hip_batch_solve_lockstep_mat_device', 12),
                            ('osqp_hip_lockstep_mat_last_record', 2), ('osqp_hip_lockstep_mat_scaling', 5)):
            fn = getattr(solver._lib, name)                                         # (AttributeError: the symbol is not in the library)
            assert len(fn.argtypes) == nargs == len(_lib.PROTOTYPES[name][1])
