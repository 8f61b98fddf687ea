"""CPU tier: the return code of every lockstep entry point for nbatch = -1, 0, 4 and for x = NULL at nbatch = 4, by raw ctypes calls through the host
simulator, and that a declined call moves no record.

The simulator has no lockstep kernels, so every route declines and the code says in which ORDER an entry checks: the validation prologues of the solve
and the adjoint entries differ, and each keeps its own order.
  solve, host arrays     batch_enter: nbatch <= 0 or x / y / rec NULL -> OSQP_DATA_VALIDATION_ERROR, then the route -> OSQP_FUNC_NOT_IMPLEMENTED
  solve, device arrays   batch_enter with the query: nbatch == 0 asks the route -> OSQP_FUNC_NOT_IMPLEMENTED; then as above
  adjoint, host arrays   nbatch <= 0 or x / y / dx NULL -> OSQP_DATA_VALIDATION_ERROR, then the route
  adjoint, device arrays nbatch < 0 -> OSQP_DATA_VALIDATION_ERROR, then the route -> OSQP_FUNC_NOT_IMPLEMENTED, before nbatch == 0 and before the arguments"""
import itertools

import numpy as np

import osqp_amd
import problems
from osqp_amd import _lib, ext_hip
from hostsim_util import hostsim

BAD, DECLINED = int(ext_hip.osqp_error_type.OSQP_DATA_VALIDATION_ERROR), int(ext_hip.osqp_error_type.OSQP_FUNC_NOT_IMPLEMENTED)
# (direction, arrays) -> codes for (nbatch = -1, nbatch = 0, nbatch = 4, nbatch = 4 with x NULL)
EXPECTED = {('solve', 'host'): (BAD, BAD, DECLINED, BAD),
            ('solve', 'device'): (BAD, DECLINED, DECLINED, BAD),
            ('adjoint', 'host'): (BAD, BAD, DECLINED, BAD),
            ('adjoint', 'device'): (BAD, DECLINED, DECLINED, DECLINED)}
RECORDS = ('lockstep_last_record', 'lockstep_polish_last_record', 'lockstep_mat_last_record', 'lockstep_direct_last_record', 'lockstep_direct_mat_last_record',
           'lockstep_adjoint_last_record', 'lockstep_mat_adjoint_last_record', 'lockstep_direct_adjoint_last_record', 'lockstep_direct_mat_adjoint_last_record')


def test_every_lockstep_entry_answers_in_its_own_order_and_moves_no_record():
    P, q, A, l, u = problems.random_qp(30, 50, density=0.15, seed=5)
    n, m, B = P.shape[0], A.shape[0], 4
    with hostsim():
        s = osqp_amd.OSQP(algebra='hip')
        s.setup(P, q, A, l, u, verbose=False)
        solver = s._solver
        lib, nzP, nzA = solver._lib, solver.nnz_P, solver.nnz_A
        arr = {k: np.zeros((B, w)) for k, w in dict(q=n, l=m, u=m, x=n, y=m, rec=solver.BATCH_REC, dx=n, dy=m, dP=nzP, dq=n, dA=nzA, dl=m, du=m,
                                                    arec=solver.ADJOINT_REC, Px=nzP, Ax=nzA).items()}
        arr['u'] += 1.0
        arr['Px'] += 1.0
        arr['Ax'] += 1.0
        names = {'solve': ('q', 'l', 'u', 'x', 'y', 'rec'), 'adjoint': ('l', 'u', 'x', 'y', 'dx', 'dy', 'dP', 'dq', 'dA', 'dl', 'du', 'arec')}
        seen = 0
        for direction, route, mat, arrays in itertools.product(('solve', 'adjoint'), ('', '_direct'), ('', '_mat'), ('host', 'device')):
            entry = 'osqp_hip_batch_%s_lockstep%s%s%s' % (direction, route, mat, '_device' if arrays == 'device' else '')
            fn = getattr(lib, entry)

            def call(nbatch, x_null=False):
                # host entries take double pointers, device entries addresses: nothing is read before an entry has answered here
                conv = (lambda a: a.ctypes.data_as(_lib.c_double_p)) if arrays == 'host' else (lambda a: a.ctypes.data)
                args = [None if (k == 'x' and x_null) else conv(arr[k]) for k in (('Px', 'Ax') if mat else ()) + names[direction]]
                tail = ([0] if direction == 'solve' else []) + ([None] if arrays == 'device' else [])      # warm, stream
                return int(fn(solver._p, nbatch, *args, *tail))
            got = (call(-1), call(0), call(B), call(B, x_null=True))
            assert got == EXPECTED[direction, arrays], (entry, got)
            seen += 1
        assert seen == 16
        for name in RECORDS:                                                       # a declined call moves no record
            rec = getattr(solver, name)()
            assert len(rec) == 8 and all(v == 0 for v in rec.values()), (name, rec)
