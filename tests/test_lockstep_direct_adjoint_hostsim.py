"""CPU tier: the direct lockstep adjoint's Python side through the host simulator -- the width checks of hip_batch_adjoint_lockstep_direct run before the C
call, a well-formed call and the applicability query reach the engine (which has no lockstep kernels in the simulator and declines), the record of the
last call has its eight named fields, all zero, the forward records have not moved, and the three C symbols carry the documented argument lists."""
import numpy as np
import pytest

import osqp_amd
import problems
from osqp_amd import _lib, ext_hip
from hostsim_util import hostsim


def test_lockstep_direct_adjoint_checks_widths_and_reaches_the_engine():
    P, q, A, l, u = problems.random_qp(30, 50, density=0.15, seed=5)
    n, m, B = P.shape[0], A.shape[0], 4
    with hostsim():
        s = osqp_amd.OSQP(algebra='hip')
        s.setup(P, q, A, l, u, verbose=False)
        solver = s._solver
        good = dict(x=np.zeros((B, n)), y=np.zeros((B, m)), dx=np.ones((B, n)), dy=np.ones((B, m)), l=np.tile(l, (B, 1)), u=np.tile(u, (B, 1)))
        widths = dict(x=n, y=m, dx=n, dy=m, l=m, u=m)
        for name in ('y', 'dx', 'dy', 'l', 'u'):
            bad = dict(good)
            bad[name] = np.zeros((B, widths[name] + 1))
            with pytest.raises(ValueError, match=r'^%s: expected %d problems of width %d' % (name, B, widths[name])):
                solver.hip_batch_adjoint_lockstep_direct(**bad)
        bad = dict(good, x=np.zeros((B, n + 1)))
        with pytest.raises(ValueError, match=r'^x: expected %d problems of width %d' % (B, n)):
            solver.hip_batch_adjoint_lockstep_direct(**bad)
        for name in ('x', 'y', 'dx'):                                               # the three required arrays
            with pytest.raises(ValueError, match='x, y and dx are required'):
                solver.hip_batch_adjoint_lockstep_direct(**dict(good, **{name: None}))
        for kw in (good, dict(x=good['x'], y=good['y'], dx=good['dx']), dict(good, want=('dq',))):      # right widths: the call reaches the engine, which declines here
            with pytest.raises(ValueError) as e:
                solver.hip_batch_adjoint_lockstep_direct(**kw)
            assert e.value.code == ext_hip.osqp_error_type.OSQP_FUNC_NOT_IMPLEMENTED
        with pytest.raises(ValueError) as e:                                        # the applicability query of the device entry
            solver.hip_batch_adjoint_lockstep_direct_device(0, None, None, None)
        assert e.value.code == ext_hip.osqp_error_type.OSQP_FUNC_NOT_IMPLEMENTED
        rec = solver.lockstep_direct_adjoint_last_record()
        assert tuple(rec) == ext_hip.OSQPSolver.LOCKSTEP_DIRECT_ADJOINT_LAST_FIELDS and len(rec) == 8
        assert tuple(rec) == ('chunks', 'width', 'steps_max', 'inversions', 'kernel_launches', 'gpu_ms', 'workspace_bytes', 'reserved')
        assert all(v == 0 for v in rec.values())                                    # no direct lockstep adjoint call has run
        for other in (solver.lockstep_last_record(), solver.lockstep_direct_last_record(), solver.lockstep_adjoint_last_record()):
            assert all(v == 0 for v in other.values())                              # nor have the other routes' records moved
        for name, nargs in (('osqp_hip_batch_adjoint_lockstep_direct', 14), ('osqp_hip_batch_adjoint_lockstep_direct_device', 15),
                            ('osqp_hip_lockstep_direct_adjoint_last_record', 2)):
            fn = getattr(solver._lib, name)                                         # (AttributeError: the symbol is not in the library)
            assert len(fn.argtypes) == nargs == len(_lib.PROTOTYPES[name][1])
