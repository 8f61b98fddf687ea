"""CPU tier: the lockstep batch route's Python side through the host simulator -- the width checks of hip_batch_solve_lockstep run before the C
call, a well-formed call reaches the engine (which has no lockstep kernels in the simulator and declines), and the three C symbols carry the
documented argument lists."""
import numpy as np
import pytest

import osqp_amd
import problems
from osqp_amd import _lib, ext_hip
from hostsim_util import hostsim


def test_lockstep_checks_widths_and_reaches_the_engine():
    P, q, A, l, u = problems.random_qp(30, 50, density=0.15, seed=5)
    n, m, B = P.shape[0], A.shape[0], 4
    with hostsim():
        s = osqp_amd.OSQP(algebra='hip')
        s.setup(P, q, A, l, u, verbose=False)
        solver = s._solver
        good = dict(q=np.tile(q, (B, 1)), l=np.tile(l, (B, 1)), u=np.tile(u, (B, 1)), x0=np.zeros((B, n)), y0=np.zeros((B, m)))
        widths = dict(q=n, l=m, u=m, x0=n, y0=m)
        for name in good:
            bad = dict(good)
            bad[name] = np.zeros((B, widths[name] + 1))
            with pytest.raises(ValueError, match=r'^%s: expected %d problems of width %d' % (name, B, widths[name])):
                solver.hip_batch_solve_lockstep(**bad)
        with pytest.raises(ValueError, match=r'^l: expected'):                     # nbatch below the arrays' rows
            solver.hip_batch_solve_lockstep(l=good['l'], u=good['u'], nbatch=B - 1)
        for kw in (good, dict(q=good['q']), dict(l=good['l'], u=good['u'])):       # right widths: the call reaches the engine, which declines here
            with pytest.raises(ValueError) as e:
                solver.hip_batch_solve_lockstep(**kw)
            assert e.value.code == ext_hip.osqp_error_type.OSQP_FUNC_NOT_IMPLEMENTED
        with pytest.raises(ValueError) as e:                                        # the applicability query of the device entry
            solver.hip_batch_solve_lockstep_device(0, None, None, None, None, None, None)
        assert e.value.code == ext_hip.osqp_error_type.OSQP_FUNC_NOT_IMPLEMENTED
        rec = solver.lockstep_last_record()
        assert tuple(rec) == ext_hip.OSQPSolver.LOCKSTEP_LAST_FIELDS and len(rec) == 8
        assert all(v == 0 for v in rec.values())                                    # no lockstep call has run
        for name, nargs in (('osqp_hip_batch_solve_lockstep', 9), ('osqp_hip_batch_solve_lockstep_device', 10), ('osqp_hip_lockstep_last_record', 2)):
            fn = getattr(solver._lib, name)                                         # (AttributeError: the symbol is not in the library)
            assert len(fn.argtypes) == nargs == len(_lib.PROTOTYPES[name][1])
