"""CPU tier: the public interface of the dense KKT mode (include/osqp_hip.h osqp_hip_dense_kkt) -- the symbols, what a backend
without the mode answers (the host simulator), and that the mode came as stand-alone entry points: OSQPHipPolicy and OSQPHipStats keep their size.
The mode itself is tests/test_gpu_dense_kkt.py and tests/test_gpu_dense_kkt_kernels.py."""
import ctypes
import os
import subprocess
import warnings

import numpy as np

import osqp_amd
import problems
from osqp_amd import _lib
from backend_param import engine

warnings.simplefilter('ignore')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_IMPLEMENTED = 10                                     # OSQP_FUNC_NOT_IMPLEMENTED
ST = dict(eps_abs=1e-6, eps_rel=1e-6, max_iter=20000, adaptive_rho_interval=50, check_termination=25, verbose=False)


def test_the_entry_points_are_declared_and_exported():
    for name in ('osqp_hip_dense_kkt', 'osqp_hip_dense_kkt_last_record', 'osqp_hip_test_dense_kkt'):
        assert name in _lib.PROTOTYPES
    with engine('hostsim') as h:                         # (_bind has bound every prototype: AttributeError on a missing export)
        assert h.osqp_hip_dense_kkt.argtypes[1] is ctypes.c_int
        assert h.osqp_hip_dense_kkt_last_record.restype is ctypes.c_int
    header = open(os.path.join(ROOT, 'include', 'osqp_hip.h')).read()
    assert '#define OSQP_HIP_DENSE_KKT_MAX_N %d' % _lib.DENSE_KKT_MAX_N in header
    assert '#define OSQP_HIP_DENSE_KKT_REC %d' % len(_lib.DENSE_KKT_REC) in header


def test_host_simulator_declines_and_the_handle_stays_untouched():
    P, q, A, l, u = problems.banded_qp(40, window=10, seed=3)
    with engine('hostsim'):
        a = osqp_amd.OSQP(algebra='hip'); a.setup(P, q, A, l, u, **ST)
        b = osqp_amd.OSQP(algebra='hip'); b.setup(P, q, A, l, u, **ST)
        assert a._solver.hip_dense_kkt(True) == NOT_IMPLEMENTED
        rec = a._solver.hip_dense_kkt_record()
        assert set(rec) == set(_lib.DENSE_KKT_REC) and all(v == 0 for v in rec.values())
        st, out = a._solver.hip_test_dense_kkt('probe')
        assert st == NOT_IMPLEMENTED
        assert a._solver.hip_dense_kkt(False) == 0       # switching off what is off: nothing to do
        ra, rb = a.solve(), b.solve()
        assert ra.info.status_val == rb.info.status_val == 1 and ra.info.iter == rb.info.iter
        assert np.array_equal(ra.x, rb.x) and np.array_equal(ra.y, rb.y)
        assert all(v == 0 for v in a._solver.hip_dense_kkt_record().values())


def test_policy_and_stats_structs_keep_their_size(tmp_path):
    """The mode has no field in OSQPHipPolicy / OSQPHipStats: the C structs are as large as the ctypes mirrors, whose field lists this pull request did
    not touch, and the mirrors still end with the fields they ended with."""
    src = tmp_path / 'sizes.c'
    src.write_text('#include <stdio.h>\n#include "osqp_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(OSQPHipPolicy), sizeof(OSQPHipStats), sizeof(OSQPHipDenseKktTest)); return 0; }\n')
    exe = tmp_path / 'sizes'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), '-o', str(exe), str(src)])
    pol, stats, dk = (int(v) for v in subprocess.check_output([str(exe)]).split())
    assert pol == ctypes.sizeof(_lib.PolicyStruct) and stats == ctypes.sizeof(_lib.StatsStruct) and dk == ctypes.sizeof(_lib.DenseKktTestStruct)
    assert _lib.PolicyStruct._fields_[-1][0] == 'adjoint_woodbury' and len(_lib.PolicyStruct._fields_) == 47
    assert _lib.StatsStruct._fields_[-1][0] == 'batch_wave_split' and len(_lib.StatsStruct._fields_) == 29
