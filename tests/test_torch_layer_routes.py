"""CPU tier: the route table of the torch layer (osqp_amd/nn/torch.py, module docstring) on a stub handle -- no GPU, no library call.

The stub stands in for ``osqp_amd.OSQP``: its ``_solver`` offers every host entry the table names, records each call as (name, Px given, Ax given),
answers OSQP_FUNC_NOT_IMPLEMENTED for a scripted set of entries and otherwise returns arrays of the right shape with status solved.  The ladder
never looks at values, so n = m = 2, a batch of 3 and diagonal P and A are enough.  The expected sequences below are written out from the table
(world size 1); the device-tensor columns are covered on the GPU tier (test_gpu_torch_layer_device_routes.py)."""
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import osqp_amd
from osqp_amd.nn.torch import OSQP as Layer

NI = int(osqp_amd.SolverError.OSQP_FUNC_NOT_IMPLEMENTED)
SOLVED = int(osqp_amd.SolverStatus.OSQP_SOLVED)
N = M = 2
NB = 3
MODES = ('loop', 'lockstep', 'lockstep_direct')
MATRICES = {'shared': (False, False), 'P_val': (True, False), 'A_val': (False, True), 'both': (True, True)}
FORWARD = {'loop': None, 'lockstep': 'hip_batch_solve_lockstep', 'lockstep_direct': 'hip_batch_solve_lockstep_direct'}
BACKWARD = {'loop': None, 'lockstep': 'hip_batch_adjoint_lockstep', 'lockstep_direct': 'hip_batch_adjoint_lockstep_direct'}
DECLINES = {'nothing': lambda batch: (), 'one workgroup': lambda batch: batch[:1], 'every batch entry': lambda batch: batch}
COUNTERS = ('setup_count', 'adjoint_launches', 'mat_batch_launches', 'mat_lockstep_launches', 'mat_lockstep_direct_launches',
            'mat_lockstep_adjoint_launches', 'mat_lockstep_direct_adjoint_launches')
WIDTHS = {'dP': N, 'dq': N, 'dA': M, 'dl': M, 'du': M}
OFFSET = {'dP': 1000.0, 'dq': 2000.0, 'dA': 3000.0, 'dl': 4000.0, 'du': 5000.0}


def _grad(key, b):
    """What the stub answers for gradient `key` of batch element b (engine order)."""
    return OFFSET[key] + 10.0 * b + np.arange(WIDTHS[key])


class StubExt:
    """The ext_hip solver of a handle: the batch entries and the single-handle adjoint entries."""
    nnz_P, nnz_A, n, m = N, M, N, M

    def __init__(self, log, script):
        self.log, self.script = log, script
        self.at = 0

    def _enter(self, name, Px=None, Ax=None):
        self.log.append((name, Px is not None, Ax is not None))
        if name in self.script.get('decline', ()):
            raise ValueError(str(NI))
        if name in self.script.get('error', {}):
            raise ValueError(self.script['error'][name])

    def _solve(self, name, q, l, u, Px, Ax, nbatch):
        self._enter(name, Px, Ax)
        B = len(q) if nbatch is None else nbatch
        assert q.shape == (B, N) and l.shape == (B, M) and u.shape == (B, M)
        assert (Px is None or Px.shape == (B, N)) and (Ax is None or Ax.shape == (B, M))
        rec = np.zeros((B, 12)); rec[:, 0] = SOLVED
        if 'unsolved' in self.script:
            rec[self.script['unsolved'], 0] = 4
        return np.arange(B * N, dtype=float).reshape(B, N), -np.arange(B * M, dtype=float).reshape(B, M), rec

    def hip_batch_solve(self, q=None, l=None, u=None, x0=None, y0=None, nbatch=None, Px=None, Ax=None):
        return self._solve('hip_batch_solve', q, l, u, Px, Ax, nbatch)

    def hip_batch_solve_lockstep(self, q=None, l=None, u=None, x0=None, y0=None, nbatch=None, Px=None, Ax=None):
        return self._solve('hip_batch_solve_lockstep', q, l, u, Px, Ax, nbatch)

    def hip_batch_solve_lockstep_direct(self, q=None, l=None, u=None, x0=None, y0=None, nbatch=None, Px=None, Ax=None):
        return self._solve('hip_batch_solve_lockstep_direct', q, l, u, Px, Ax, nbatch)

    def _adjoint(self, name, x, y, dx, dy, l, u, Px, Ax, want):
        self._enter(name, Px, Ax)
        B = len(x)
        assert x.shape == dx.shape == (B, N) and y.shape == l.shape == u.shape == (B, M) and dy is None
        res = {k: np.stack([_grad(k, b) for b in range(B)]) for k in want}
        res['rec'] = np.zeros((B, 4))
        if 'unsolved_adjoint' in self.script and name != 'hip_batch_adjoint':
            res['rec'][self.script['unsolved_adjoint']] = (3, 1, 0.5, 7)
        return res

    def hip_batch_adjoint(self, x, y, dx, dy=None, l=None, u=None, Px=None, Ax=None, want=('dP', 'dq', 'dA', 'dl', 'du')):
        return self._adjoint('hip_batch_adjoint', x, y, dx, dy, l, u, Px, Ax, want)

    def hip_batch_adjoint_lockstep(self, x, y, dx, dy=None, l=None, u=None, want=('dP', 'dq', 'dA', 'dl', 'du'), Px=None, Ax=None):
        return self._adjoint('hip_batch_adjoint_lockstep', x, y, dx, dy, l, u, Px, Ax, want)

    def hip_batch_adjoint_lockstep_direct(self, x, y, dx, dy=None, l=None, u=None, want=('dP', 'dq', 'dA', 'dl', 'du'), Px=None, Ax=None):
        return self._adjoint('hip_batch_adjoint_lockstep_direct', x, y, dx, dy, l, u, Px, Ax, want)

    def _no_device_entry(self, *a, **kw):
        raise AssertionError('host tensors went to a device entry')
    hip_batch_adjoint_lockstep_device = hip_batch_adjoint_lockstep_direct_device = _no_device_entry

    def adjoint_derivative_compute_at(self, x, y, dx):
        self.log.append(('adjoint_derivative_compute_at', False, False))
        assert x.shape == dx.shape == (N,) and y.shape == (M,)
        self.at += 1
        return NI if 'adjoint_derivative_compute_at' in self.script.get('decline', ()) else 0

    def adjoint_last_record(self):
        self.log.append(('adjoint_last_record', False, False))
        return dict(status=0, active_rows=1, residual=0.0, steps=5)

    def adjoint_derivative_get_mat(self, dP, dA):
        self.log.append(('adjoint_derivative_get_mat', False, False))
        dP.x[:], dA.x[:] = _grad('dP', self.at - 1), _grad('dA', self.at - 1)
        return 0

    def adjoint_derivative_get_vec(self, dq, dl, du):
        self.log.append(('adjoint_derivative_get_vec', False, False))
        dq[:], dl[:], du[:] = _grad('dq', self.at - 1), _grad('dl', self.at - 1), _grad('du', self.at - 1)
        return 0


class StubOSQP:
    """osqp_amd.OSQP as the layer uses it: setup / update / solve, ._solver, .ext.CSC and ._derivative_cache."""
    log, script = None, None            # set per test (_stub)
    ext = types.SimpleNamespace(CSC=lambda M: types.SimpleNamespace(x=np.zeros(M.nnz)))

    def __init__(self, algebra='hip'):
        self._solver = StubExt(self.log, self.script)
        self.solves = 0

    def setup(self, P, q, A, l, u, **kw):
        self.log.append(('setup', False, False))
        self._derivative_cache = {'P': sp.triu(P, format='csc'), 'A': sp.csc_matrix(A)}

    def update(self, **kw):
        self.log.append(('update', kw.get('Px') is not None, kw.get('Ax') is not None))

    def solve(self):
        self.log.append(('solve', False, False))
        self.solves += 1
        info = types.SimpleNamespace(status_val=SOLVED, iter=25, obj_val=1.5)
        return types.SimpleNamespace(x=np.full(N, float(self.solves)), y=np.full(M, -float(self.solves)), info=info)


@pytest.fixture
def stub(monkeypatch):
    def make(**script):
        cls = type('Stub', (StubOSQP,), dict(log=[], script=script))
        monkeypatch.setattr(osqp_amd, 'OSQP', cls)
        return cls.log
    return make


def _layer(**kw):
    idx = (np.arange(N), np.arange(N))
    return Layer(idx, (N, N), idx, (M, N), **kw)


def _inputs(p2d, a2d, grad=False):
    """P_val, q (batched), A_val, l (shared), u (batched): per-element matrix rows differ, so the per-element loop re-uploads them."""
    rows = lambda two_d, w: (1.0 + np.arange(NB)[:, None] + np.arange(w)) if two_d else 1.0 + np.arange(w)
    vals = (rows(p2d, N), np.ones((NB, N)), rows(a2d, M), -np.ones(M), np.ones((NB, M)))
    return [torch.tensor(v, dtype=torch.float64, requires_grad=grad) for v in vals]


def _c(name, p=False, a=False):
    return (name, p, a)


def _loop_calls(mat):
    """_loop: update(q, l, u) + solve() per element, after update(Px, Ax) where the element's matrices are not the handle's (element 0's are)."""
    out = []
    for b in range(NB):
        out += ([_c('update', True, True)] if mat and b else []) + [_c('update'), _c('solve')]
    return out


def _backward_loop_calls(mat, upto=NB):
    out = []
    for b in range(upto):
        out += ([_c('update', True, True)] if mat and b else []) + [_c('update'), _c('adjoint_derivative_compute_at'), _c('adjoint_last_record'),
                                                                    _c('adjoint_derivative_get_mat'), _c('adjoint_derivative_get_vec')]
    return out


def _counters(layer):
    return {k: getattr(layer, k, 0) for k in COUNTERS}


def _expect_counters(**kw):
    return dict({k: 0 for k in COUNTERS}, setup_count=1, **kw)


@pytest.mark.parametrize('declines', list(DECLINES))
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('matrices', list(MATRICES))
def test_forward(stub, matrices, mode, declines):
    p, a = MATRICES[matrices]
    mat = p or a
    declined = DECLINES[declines](['hip_batch_solve'] + [FORWARD[m] for m in MODES if FORWARD[m]])
    log = stub(decline=declined)
    layer = _layer(large_batch=mode)
    # the table: the one-workgroup kernel, then the route large_batch names, then the loop
    calls, counters, raises, last = [_c('setup'), _c('hip_batch_solve', p, a)], {}, False, 'batch'
    if mat and not declined:
        counters['mat_batch_launches'] = 1
    if declined:
        route = FORWARD[mode]
        if route is None:
            calls += _loop_calls(mat); last = 'loop'
        else:
            calls.append(_c(route, p, a)); last = 'batch'
            if route not in declined:
                if mat:
                    counters['mat_lockstep_launches' if mode == 'lockstep' else 'mat_lockstep_direct_launches'] = 1
            elif mat and mode == 'lockstep_direct':              # per-element matrices, 'lockstep_direct' declining: on to the loop
                calls += _loop_calls(mat); last = 'loop'
            else:                                                # shared matrices, and per-element 'lockstep': the decline comes out
                raises = True
    ts = _inputs(p, a)
    if raises:
        with pytest.raises(ValueError) as e:
            layer(*ts)
        assert str(e.value) == str(NI)
    else:
        x = layer(*ts)
        assert x.shape == (NB, N) and x.dtype == torch.float64
        want_x = np.arange(NB * N, dtype=float).reshape(NB, N) if last == 'batch' else np.repeat(1.0 + np.arange(NB), N).reshape(NB, N)
        assert np.array_equal(x.numpy(), want_x)
        assert layer.last_dual is not None and np.array_equal(np.asarray(layer.last_dual), -want_x)
        assert layer.last_rec.shape == (NB, 12 if last == 'batch' else 8) and (layer.last_rec[:, 0] == SOLVED).all()
    assert log == calls
    assert _counters(layer) == _expect_counters(**counters)


@pytest.mark.parametrize('declines', list(DECLINES))
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('matrices', list(MATRICES))
def test_backward(stub, matrices, mode, declines):
    p, a = MATRICES[matrices]
    mat = p or a
    declined = DECLINES[declines](['hip_batch_adjoint'] + [BACKWARD[m] for m in MODES if BACKWARD[m]])
    log = stub(decline=declined)
    layer = _layer(large_backward=mode)
    ts = _inputs(p, a, grad=True)
    x = layer(*ts)
    assert x.grad_fn is not None and layer.last_dual is not None
    assert log == [_c('setup'), _c('hip_batch_solve', p, a)]
    del log[:]
    g = torch.arange(NB * N, dtype=torch.float64).reshape(NB, N)
    x.backward(g)
    # the table: the batch adjoint kernel, then the route large_backward names, then the loop; every decline goes on
    calls, counters, last = [_c('hip_batch_adjoint', p, a)], dict(adjoint_launches=1), 'batch'
    if declined:
        counters['adjoint_launches'] = 0
        route = BACKWARD[mode]
        if route is not None:
            calls.append(_c(route, p, a))
            if route not in declined:
                counters['adjoint_launches'] = 1
                if mat:
                    counters['mat_lockstep_adjoint_launches' if mode == 'lockstep' else 'mat_lockstep_direct_adjoint_launches'] = 1
        if route is None or route in declined:
            calls += _backward_loop_calls(mat); last = 'loop'
            counters['adjoint_launches'] = NB
    if mat:
        counters['mat_batch_launches'] = 1
    assert log == calls
    assert _counters(layer) == _expect_counters(**counters)
    rec = np.asarray(layer.last_adjoint_rec)
    assert rec.shape == (NB, 4) and (rec[:, 0] == 0).all() and (rec[:, 1] == (1 if last == 'loop' else 0)).all()
    p_map = layer._p_map(N)
    for key, t, two_d in zip(('dP', 'dq', 'dA', 'dl', 'du'), ts, (p, True, a, False, True)):
        full = np.stack([_grad(key, b) for b in range(NB)])
        if key == 'dP':
            full = full[:, p_map]
        want = full if two_d else full.sum(0)               # an input shared by the batch receives the batch sum
        assert t.grad.shape == t.shape and np.array_equal(t.grad.numpy(), want), key


def test_forward_unsolved_element_raises(stub):
    """Status other than solved: RuntimeError naming the first such element, after last_rec was set."""
    log = stub(unsolved=[1, 2])
    layer = _layer()
    with pytest.raises(RuntimeError, match=r'^Unable to solve QP, status: 4 \(batch element 1\)$'):
        layer(*_inputs(False, False))
    assert log == [_c('setup'), _c('hip_batch_solve')] and layer.last_rec[2, 0] == 4


def test_forward_other_errors_are_not_declines(stub):
    """Only OSQP_FUNC_NOT_IMPLEMENTED moves the ladder on; any other ValueError of an entry comes out as it is."""
    log = stub(error={'hip_batch_solve': 'q: expected 3 problems of width 2'})
    layer = _layer(large_batch='lockstep')
    with pytest.raises(ValueError, match='^q: expected 3 problems of width 2$'):
        layer(*_inputs(False, False))
    assert log == [_c('setup'), _c('hip_batch_solve')]


@pytest.mark.parametrize('mode', ['lockstep', 'lockstep_direct'])
def test_backward_unsolved_adjoint_system_raises(stub, mode):
    """A nonzero status in the record of the lockstep adjoint: RuntimeError with the per-element route's text, last_adjoint_rec kept, the call counted."""
    stub(decline=['hip_batch_adjoint'], unsolved_adjoint=1)
    layer = _layer(large_backward=mode)
    x = layer(*_inputs(False, False, grad=True))
    err = int(osqp_amd.SolverError.OSQP_LINSYS_SOLVER_INIT_ERROR)
    with pytest.raises(RuntimeError, match=r'^adjoint derivatives of batch element 1: error %d \(status 3, residual 5.000e-01\)$' % err):
        x.sum().backward()
    assert layer.adjoint_launches == 1 and np.asarray(layer.last_adjoint_rec)[1, 0] == 3


def test_backward_loop_on_a_declining_handle_raises(stub):
    """The last entry has nowhere to go on to: NotImplementedError, the one call counted."""
    log = stub(decline=['hip_batch_adjoint', 'hip_batch_adjoint_lockstep', 'adjoint_derivative_compute_at'])
    layer = _layer(large_backward='lockstep')
    x = layer(*_inputs(False, False, grad=True))
    del log[:]
    with pytest.raises(NotImplementedError, match='backward is not available on this handle'):
        x.sum().backward()
    assert log == [_c('hip_batch_adjoint'), _c('hip_batch_adjoint_lockstep'), _c('update'), _c('adjoint_derivative_compute_at'), _c('adjoint_last_record')]
    assert layer.adjoint_launches == 1
