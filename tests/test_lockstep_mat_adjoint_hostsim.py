"""CPU tier: the lockstep adjoint with per-problem matrices (osqp_hip_batch_adjoint_lockstep_mat) through the host simulator -- the width checks of
hip_batch_adjoint_lockstep(Px=, Ax=) run before the C call, a well-formed call reaches the engine (which has no lockstep kernels and no device
assembly in the simulator and declines), the record answers as before a first call, and the three C symbols carry the documented argument lists."""
import numpy as np
import pytest

import osqp_amd
import problems
from osqp_amd import _lib, ext_hip
from hostsim_util import hostsim

E = ext_hip.osqp_error_type


def test_lockstep_mat_adjoint_checks_widths_and_reaches_the_engine():
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
        for name in ('y', 'dx', 'dy', 'l', 'u', 'Px', 'Ax'):                       # (x fixes the number of problems)
            bad = dict(good)
            bad[name] = np.zeros((B, widths[name] + 1))
            with pytest.raises(ValueError, match=r'^%s: expected %d problems of width %d' % (name, B, widths[name])):
                solver.hip_batch_adjoint_lockstep(**bad)
        with pytest.raises(ValueError, match=r'^Px: expected %d problems of width %d' % (B, nzP)):      # fewer rows than problems
            solver.hip_batch_adjoint_lockstep(**dict(good, Px=np.ones((B - 1, nzP))))
        base = {k: good[k] for k in ('x', 'y', 'dx')}
        for kw in (good, dict(base, Px=good['Px']), dict(base, Ax=good['Ax']), dict(base, Ax=good['Ax'], l=good['l'], want=('dq',))):      # right widths: the engine declines here
            with pytest.raises(ValueError) as e:
                solver.hip_batch_adjoint_lockstep(**kw)
            assert e.value.code == E.OSQP_FUNC_NOT_IMPLEMENTED
        with pytest.raises(ValueError) as e:                                        # the applicability query of the device entry
            solver.hip_batch_adjoint_lockstep_device(0, None, None, None, Px_ptr=0, Ax_ptr=0)
        assert e.value.code == E.OSQP_FUNC_NOT_IMPLEMENTED
        rec = solver.lockstep_mat_adjoint_last_record()
        assert tuple(rec) == ext_hip.OSQPSolver.LOCKSTEP_MAT_ADJOINT_LAST_FIELDS and len(rec) == 8
        assert tuple(rec) == ('chunks', 'width', 'steps_max', 'pcg_iters', 'kernel_launches', 'gpu_ms', 'matrix_block_bytes', 'prepare_gpu_ms')
        assert all(v == 0 for v in rec.values())                                    # no such call has run
        for name, nargs in (('osqp_hip_batch_adjoint_lockstep_mat', 16), ('osqp_hip_batch_adjoint_lockstep_mat_device', 17),
                            ('osqp_hip_lockstep_mat_adjoint_last_record', 2)):
            fn = getattr(solver._lib, name)                                         # (AttributeError: the symbol is not in the library)
            assert len(fn.argtypes) == nargs == len(_lib.PROTOTYPES[name][1])
