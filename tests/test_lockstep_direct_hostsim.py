"""CPU tier: the direct lockstep route's Python side through the host simulator -- the width checks of hip_batch_solve_lockstep_direct run before the C
call, a well-formed call reaches the engine (which has no lockstep kernels in the simulator and declines, the nbatch == 0 query included), the record
of the last call has its eight fields, and the three C symbols carry the documented argument lists."""
import numpy as np
import pytest

import osqp_amd
import problems
from osqp_amd import _lib, ext_hip
from hostsim_util import hostsim


@pytest.mark.parametrize('problem', ['random', 'portfolio'])
def test_lockstep_direct_checks_widths_and_reaches_the_engine(problem):
    P, q, A, l, u = problems.random_qp(30, 50, density=0.15, seed=5) if problem == 'random' else problems.portfolio_qp(300, 3)
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
                solver.hip_batch_solve_lockstep_direct(**bad)
        with pytest.raises(ValueError, match=r'^l: expected'):                     # nbatch below the arrays' rows
            solver.hip_batch_solve_lockstep_direct(l=good['l'], u=good['u'], nbatch=B - 1)
        for kw in (good, dict(q=good['q']), dict(l=good['l'], u=good['u'])):       # right widths: the call reaches the engine, which declines here
            with pytest.raises(ValueError) as e:
                solver.hip_batch_solve_lockstep_direct(**kw)
            assert e.value.code == ext_hip.osqp_error_type.OSQP_FUNC_NOT_IMPLEMENTED
        with pytest.raises(ValueError) as e:                                        # the applicability query of the device entry
            solver.hip_batch_solve_lockstep_direct_device(0, None, None, None, None, None, None)
        assert e.value.code == ext_hip.osqp_error_type.OSQP_FUNC_NOT_IMPLEMENTED
        rec = solver.lockstep_direct_last_record()
        assert tuple(rec) == ext_hip.OSQPSolver.LOCKSTEP_DIRECT_LAST_FIELDS and len(rec) == 8
        assert all(v == 0 for v in rec.values())                                    # no direct lockstep call has run
        assert all(v == 0 for v in solver.lockstep_last_record().values())          # nor has the lockstep route's record moved
        for name, nargs in (('osqp_hip_batch_solve_lockstep_direct', 9), ('osqp_hip_batch_solve_lockstep_direct_device', 10), ('osqp_hip_lockstep_direct_last_record', 2)):
            fn = getattr(solver._lib, name)                                         # (AttributeError: the symbol is not in the library)
            assert len(fn.argtypes) == nargs == len(_lib.PROTOTYPES[name][1])


def test_the_torch_layer_knows_the_third_value():
    from osqp_amd.nn.torch import OSQP as Layer
    idx = (np.array([0]), np.array([0]))
    for mode in ('loop', 'lockstep', 'lockstep_direct'):
        assert Layer(idx, (1, 1), idx, (1, 1), large_batch=mode).large_batch == mode
    with pytest.raises(ValueError):
        Layer(idx, (1, 1), idx, (1, 1), large_batch='direct')
