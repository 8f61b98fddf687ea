"""CPU tier: OSQPHipPolicy::adjoint_woodbury (include/osqp_hip.h), the switch that lets a handle with a Woodbury-corrected preconditioner take the
PCG route of the adjoint derivatives -- through the host simulator, ctypes and a stub handle; the route itself is tests/test_gpu_adjoint_woodbury.py.

  * the field's default is 0, it round-trips through set_policy / get_policy on a live handle, and it is read from the environment per handle;
  * OSQPHipPolicy in the header and its ctypes mirror have the same size and the field sits at the same offset, last;
  * the host simulator has no adjoint kernels: with the field at 1 it still answers OSQP_FUNC_NOT_IMPLEMENTED, and the front-end's
    NotImplementedError names the switch;
  * the torch layer's woodbury_backward=True sets the field once per handle it creates, before the first solve (stub handle, as
    test_torch_layer_routes.py); the default layer never touches the policy."""
import ctypes
import os
import subprocess
import types
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import osqp_amd
import problems
from osqp_amd import _lib
from osqp_amd.nn.torch import OSQP as Layer

warnings.simplefilter('ignore')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NI = int(osqp_amd.SolverError.OSQP_FUNC_NOT_IMPLEMENTED)
SOLVED = int(osqp_amd.SolverStatus.OSQP_SOLVED)


def _handle():
    P, q, A, l, u = problems.banded_qp(400, window=30, seed=4)
    m = osqp_amd.OSQP()
    m.setup(P, q, A, l, u, verbose=False, eps_abs=1e-6, eps_rel=1e-6)
    return m


def test_default_is_off_and_the_field_round_trips_on_a_live_handle():
    from hostsim_util import hostsim
    with hostsim() as h:
        assert h.osqp_hip_backend() == b'hostsim'
        p = _lib.PolicyStruct()
        p.adjoint_woodbury = 7
        h.osqp_hip_default_policy(ctypes.byref(p))
        assert p.adjoint_woodbury == 0
        m = _handle()
        assert m._solver.get_policy()['adjoint_woodbury'] == 0
        assert m.solve().info.status_val == SOLVED
        before = m._solver.get_policy()
        m._solver.set_policy(adjoint_woodbury=1)            # not a [setup] field: a live handle takes it
        after = m._solver.get_policy()
        assert after['adjoint_woodbury'] == 1
        assert {k: v for k, v in after.items() if k != 'adjoint_woodbury'} == {k: v for k, v in before.items() if k != 'adjoint_woodbury'}
        m._solver.set_policy(rho_window=3)                  # another field leaves it alone
        assert m._solver.get_policy()['adjoint_woodbury'] == 1
        m._solver.set_policy(adjoint_woodbury=0)
        assert m._solver.get_policy()['adjoint_woodbury'] == 0


def test_environment_is_read_per_handle(monkeypatch):
    from hostsim_util import hostsim
    with hostsim():
        monkeypatch.delenv('OSQP_HIP_ADJOINT_WOODBURY', raising=False)
        m0 = _handle()
        monkeypatch.setenv('OSQP_HIP_ADJOINT_WOODBURY', '1')
        m1 = _handle()
        monkeypatch.setenv('OSQP_HIP_ADJOINT_WOODBURY', 'yes')      # anything but 0 = on
        m2 = _handle()
        monkeypatch.setenv('OSQP_HIP_ADJOINT_WOODBURY', '0')
        m3 = _handle()
        assert [m._solver.get_policy()['adjoint_woodbury'] for m in (m0, m1, m2, m3)] == [0, 1, 1, 0]


def test_the_struct_mirror_has_the_size_of_the_header_and_the_field_is_last(tmp_path):
    src = tmp_path / 'policy.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "osqp_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu", sizeof(OSQPHipPolicy), offsetof(OSQPHipPolicy, adjoint_woodbury), offsetof(OSQPHipPolicy, batch_wave)); return 0; }\n')
    exe = str(tmp_path / 'policy')
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), '-o', exe, str(src)])
    size, off, off_prev = (int(v) for v in subprocess.check_output([exe]).split())
    assert size == ctypes.sizeof(_lib.PolicyStruct)
    assert off == _lib.PolicyStruct.adjoint_woodbury.offset and off_prev == _lib.PolicyStruct.batch_wave.offset
    assert _lib.PolicyStruct._fields_[-1][0] == 'adjoint_woodbury' and off == max(getattr(_lib.PolicyStruct, k).offset for k, _ in _lib.PolicyStruct._fields_)


def test_the_host_simulator_keeps_declining_and_the_message_names_the_switch():
    from hostsim_util import hostsim
    with hostsim():
        m = _handle()
        m._solver.set_policy(adjoint_woodbury=1)
        r = m.solve()
        assert r.info.status_val == SOLVED
        assert m._solver.adjoint_derivative_compute(r.x, None) == NI
        with pytest.raises(NotImplementedError, match='adjoint_woodbury') as e:
            m.adjoint_derivative_compute(dx=r.x)
        assert 'OSQP_HIP_ADJOINT_WOODBURY' in str(e.value)
        assert m._solver.get_policy()['adjoint_woodbury'] == 1


# ---- the torch layer on a stub handle (the pattern of test_torch_layer_routes.py: no library call)
N = M = 2


class _StubExt:
    def __init__(self, log):
        self.log = log

    def set_policy(self, **fields):
        self.log.append(('set_policy', dict(fields)))

    def hip_batch_solve(self, q=None, l=None, u=None, x0=None, y0=None, nbatch=None, Px=None, Ax=None):
        self.log.append(('hip_batch_solve', None))
        raise ValueError(str(NI))


class _StubOSQP:
    log = None

    def __init__(self, algebra='hip'):
        self._solver = _StubExt(self.log)

    def setup(self, P, q, A, l, u, **kw):
        self.log.append(('setup', None))

    def update(self, **kw):
        self.log.append(('update', None))

    def solve(self):
        self.log.append(('solve', None))
        info = types.SimpleNamespace(status_val=SOLVED, iter=25, obj_val=1.5)
        return types.SimpleNamespace(x=np.ones(N), y=-np.ones(M), info=info)


@pytest.mark.parametrize('on', [False, True])
def test_woodbury_backward_sets_the_field_once_per_handle_before_the_first_solve(monkeypatch, on):
    log = []
    monkeypatch.setattr(osqp_amd, 'OSQP', type('Stub', (_StubOSQP,), dict(log=log)))
    idx = (np.arange(N), np.arange(N))
    layer = Layer(idx, (N, N), idx, (M, N), woodbury_backward=True) if on else Layer(idx, (N, N), idx, (M, N))
    assert layer.woodbury_backward is on
    vals = (1.0 + np.arange(N), np.ones((3, N)), 1.0 + np.arange(M), -np.ones(M), np.ones((3, M)))
    ts = [torch.tensor(v, dtype=torch.float64) for v in vals]
    for _ in range(2):                                      # the second forward reuses the handle
        layer(*ts)
    names = [c[0] for c in log]
    assert layer.setup_count == 1 and names.count('setup') == 1 and names.count('solve') == 6
    if on:
        assert [c for c in log if c[0] == 'set_policy'] == [('set_policy', {'adjoint_woodbury': 1})]
        assert names.index('setup') < names.index('set_policy') < names.index('hip_batch_solve') < names.index('solve')
    else:
        assert 'set_policy' not in names
    # another device: another handle, the field set on it as well
    layer._device = 'elsewhere'
    layer(*ts)
    assert layer.setup_count == 2 and [c[0] for c in log].count('set_policy') == (2 if on else 0)
