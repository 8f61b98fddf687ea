"""CPU tier: the direct lockstep adjoint with per-problem matrices, Python side, through the host simulator -- the width checks of
hip_batch_adjoint_lockstep_direct(Px=, Ax=) run before the C call, a well-formed call and the applicability query reach the engine (which has no lockstep
kernels in the simulator and declines), the record of the last such call has its eight named fields, all zero, the other records have not moved, and the
three C symbols carry the documented argument lists."""
import numpy as np
import pytest

import osqp_amd
import problems
from osqp_amd import _lib, ext_hip
from hostsim_util import hostsim


def test_lockstep_direct_mat_adjoint_checks_widths_and_reaches_the_engine():
    P, q, A, l, u = problems.random_qp(30, 50, density=0.15, seed=5)
    n, m, B = P.shape[0], A.shape[0], 4
    with hostsim():
        s = osqp_amd.OSQP(algebra='hip')
        s.setup(P, q, A, l, u, verbose=False)
        solver = s._solver
        nzP, nzA = solver.nnz_P, solver.nnz_A
        assert nzP > 0 and nzA > 0
        good = dict(x=np.zeros((B, n)), y=np.zeros((B, m)), dx=np.ones((B, n)), dy=np.ones((B, m)), l=np.tile(l, (B, 1)), u=np.tile(u, (B, 1)),
                    Px=np.ones((B, nzP)), Ax=np.ones((B, nzA)))
        widths = dict(x=n, y=m, dx=n, dy=m, l=m, u=m, Px=nzP, Ax=nzA)
        for name in ('Px', 'Ax', 'y', 'dx', 'dy', 'l', 'u'):                        # a wrong width is refused before the C call, with the other entries' message
            bad = dict(good)
            bad[name] = np.zeros((B, widths[name] + 1))
            with pytest.raises(ValueError, match=r'^%s: expected %d problems of width %d' % (name, B, widths[name])):
                solver.hip_batch_adjoint_lockstep_direct(**bad)
        for name in ('Px', 'Ax'):                                                   # ... and so is a wrong number of problems, with the other side absent
            other = 'Ax' if name == 'Px' else 'Px'
            bad = dict(good, **{name: np.zeros((B + 1, widths[name])), other: None})
            with pytest.raises(ValueError, match=r'^%s: expected %d problems of width %d' % (name, B, widths[name])):
                solver.hip_batch_adjoint_lockstep_direct(**bad)
        for kw in (good, dict(good, Px=None), dict(good, Ax=None), dict(x=good['x'], y=good['y'], dx=good['dx'], Ax=good['Ax']), dict(good, want=('dq', 'dA'))):
            with pytest.raises(ValueError) as e:                                    # right widths: the call reaches the engine, which declines here
                solver.hip_batch_adjoint_lockstep_direct(**kw)
            assert e.value.code == ext_hip.osqp_error_type.OSQP_FUNC_NOT_IMPLEMENTED
        for kw in (dict(Px_ptr=0, Ax_ptr=0), dict(Px_ptr=0), dict(Ax_ptr=0)):       # the applicability query of the device entry
            with pytest.raises(ValueError) as e:
                solver.hip_batch_adjoint_lockstep_direct_device(0, None, None, None, **kw)
            assert e.value.code == ext_hip.osqp_error_type.OSQP_FUNC_NOT_IMPLEMENTED
        rec = solver.lockstep_direct_mat_adjoint_last_record()
        assert tuple(rec) == ext_hip.OSQPSolver.LOCKSTEP_DIRECT_MAT_ADJOINT_LAST_FIELDS and len(rec) == 8
        assert tuple(rec) == ('chunks', 'width', 'steps_max', 'inversions', 'kernel_launches', 'gpu_ms', 'matrix_block_bytes', 'prepare_gpu_ms')
        assert all(v == 0 for v in rec.values())                                    # no such call has run
        for other in (solver.lockstep_last_record(), solver.lockstep_direct_last_record(), solver.lockstep_direct_mat_last_record(), solver.lockstep_adjoint_last_record(),
                      solver.lockstep_mat_adjoint_last_record(), solver.lockstep_direct_adjoint_last_record()):
            assert all(v == 0 for v in other.values())                              # nor have the other routes' records moved
        for name, nargs in (('osqp_hip_batch_adjoint_lockstep_direct_mat', 16), ('osqp_hip_batch_adjoint_lockstep_direct_mat_device', 17),
                            ('osqp_hip_lockstep_direct_mat_adjoint_last_record', 2)):
            fn = getattr(solver._lib, name)                                         # (AttributeError: the symbol is not in the library)
            assert len(fn.argtypes) == nargs == len(_lib.PROTOTYPES[name][1])
