"""GPU tier: the device-tensor columns of the torch layer's route table (osqp_amd/nn/torch.py, module docstring; the host columns and every decline
are walked on a stub in test_torch_layer_routes.py).  ROCm tensors go through forward and backward; which route ran is read from the handle's own
records -- ``chunks`` of the eight lockstep ``*_last_record`` entries: up for the route taken, unchanged for all others -- and from the layer's
counters.  A call with per-element matrices moves its ``_mat_`` record AND the record of its route (test_gpu_lockstep_mat.py: "last_shared",
test_gpu_lockstep_direct_mat.py: "the direct route's own record moves too"), a call with shared matrices only the latter.  The same call on host
tensors goes to the same engine entry family in every case here (host entry and ``_device`` entry of one route, or the host entry for both), so x
and every gradient must be bit-equal between the two.

Shapes: banded_qp(400, window=40), the smallest standard shape past the one-workgroup kernel (test_gpu_batch_lockstep.py); portfolio_qp(600, 4), the
Woodbury handle with a diagonal K0 that only the direct route takes (test_gpu_lockstep_direct.py); banded_qp(40, window=8), which fits one workgroup.
A batch of 3.  Per-element matrices are the shared values times (1 + 0.01 b): x / (1 + 0.01 b) of a feasible x stays feasible, P stays definite."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import problems

pytestmark = pytest.mark.gpu
warnings.simplefilter('ignore')
NB = 3
EPS = 1e-6
RECORDS = ('lockstep_last_record', 'lockstep_mat_last_record', 'lockstep_direct_last_record', 'lockstep_direct_mat_last_record',
           'lockstep_adjoint_last_record', 'lockstep_mat_adjoint_last_record', 'lockstep_direct_adjoint_last_record', 'lockstep_direct_mat_adjoint_last_record')
COUNTERS = ('setup_count', 'adjoint_launches', 'mat_batch_launches', 'mat_lockstep_launches', 'mat_lockstep_direct_launches',
            'mat_lockstep_adjoint_launches', 'mat_lockstep_direct_adjoint_launches')


class Problem:
    def __init__(self, P, q, A, l, u, seed=13):
        self.P, self.A = sp.csc_matrix(P), sp.csc_matrix(A)
        self.P.sort_indices(); self.A.sort_indices()
        rng = np.random.default_rng(seed)
        self.Q = np.stack([q + 0.05 * b * rng.standard_normal(len(q)) for b in range(NB)])
        self.L, self.U = np.tile(l, (NB, 1)), np.tile(u, (NB, 1))
        scale = 1 + 0.01 * np.arange(NB)[:, None]
        self.Pv, self.Av = self.P.data * scale, self.A.data * scale

    def layer(self, **kw):
        from osqp_amd.nn.torch import OSQP as Layer
        pco, aco = self.P.tocoo(), self.A.tocoo()
        return Layer((pco.row, pco.col), self.P.shape, (aco.row, aco.col), self.A.shape, eps_rel=EPS, eps_abs=EPS, max_iter=200000, **kw)

    def tensors(self, device, per_element):
        import torch
        vals = [self.Pv if per_element else self.P.data, self.Q, self.Av if per_element else self.A.data, self.L, self.U]
        return [torch.tensor(np.array(v), dtype=torch.float64, device=device, requires_grad=True) for v in vals]


@pytest.fixture(scope='module')
def probs():
    return dict(large=Problem(*problems.banded_qp(400, window=40)), woodbury=Problem(*problems.portfolio_qp(600, 4)),
                small=Problem(*problems.banded_qp(40, window=8)))


def _chunks(layer):
    ext = layer._solver._solver
    return {name: getattr(ext, name)()['chunks'] for name in RECORDS}


def _moved(before, after):
    return {name for name in RECORDS if after[name] != before[name]}


def _run(prob, device, per_element, mode):
    """Forward and backward of one fresh layer with large_batch = large_backward = mode: x, the gradients, which records moved in each pass, the counters."""
    layer = prob.layer(large_batch=mode, large_backward=mode)
    ts = prob.tensors(device, per_element)
    x = layer(*ts)
    assert x.device == ts[1].device and x.shape == (NB, prob.P.shape[0])
    zero = dict.fromkeys(RECORDS, 0)                   # a handle's records before its first call
    after_forward = _chunks(layer)
    (0.5 * (x ** 2).sum()).backward()
    after_backward = _chunks(layer)
    for t in ts:
        assert t.grad is not None and t.grad.device == t.device and t.grad.shape == t.shape
    grads = [t.grad.cpu().numpy() for t in ts]
    assert all(np.isfinite(g).all() for g in grads) and all(np.abs(g).max() > 0 for g in grads)
    return (x.detach().cpu().numpy(), grads, _moved(zero, after_forward), _moved(after_forward, after_backward), after_backward,
            {k: getattr(layer, k) for k in COUNTERS})


# (problem, per-element matrices, large_batch = large_backward): the record the forward moves, the record the backward moves (with per-element
# matrices: that `_mat_` record and the route's own), the counters
CASES = {
    'small shared':              ('small', False, 'lockstep', None, None, dict(adjoint_launches=1)),
    'small per element':         ('small', True, 'lockstep', None, None, dict(adjoint_launches=1, mat_batch_launches=1)),
    'large shared loop':         ('large', False, 'loop', None, None, dict(adjoint_launches=NB)),
    'large shared lockstep':     ('large', False, 'lockstep', 'lockstep_last_record', 'lockstep_adjoint_last_record', dict(adjoint_launches=1)),
    'large per element lockstep': ('large', True, 'lockstep', 'lockstep_mat_last_record', 'lockstep_mat_adjoint_last_record',
                                   dict(adjoint_launches=1, mat_lockstep_launches=1, mat_lockstep_adjoint_launches=1)),
    'woodbury shared direct':    ('woodbury', False, 'lockstep_direct', 'lockstep_direct_last_record', 'lockstep_direct_adjoint_last_record', dict(adjoint_launches=1)),
    'woodbury per element direct': ('woodbury', True, 'lockstep_direct', 'lockstep_direct_mat_last_record', 'lockstep_direct_mat_adjoint_last_record',
                                    dict(adjoint_launches=1, mat_lockstep_direct_launches=1, mat_lockstep_direct_adjoint_launches=1)),
}


@pytest.mark.parametrize('case', list(CASES))
def test_device_tensors_take_the_route_of_the_table(probs, case):
    name, per_element, mode, forward_record, backward_record, counters = CASES[case]
    out = {device: _run(probs[name], device, per_element, mode) for device in ('cuda', 'cpu')}
    for device, (x, grads, forward_moved, backward_moved, chunks, counted) in out.items():
        route = lambda record: {record, record.replace('_mat_', '_')} if record else set()
        assert forward_moved == route(forward_record), (device, forward_moved)
        assert backward_moved == route(backward_record), (device, backward_moved)
        assert all(chunks[r] == 1 for r in route(forward_record) | route(backward_record)), (device, chunks)
        assert counted == dict(dict.fromkeys(COUNTERS, 0), setup_count=1, **counters), (device, counted)
    (xd, gd), (xh, gh) = out['cuda'][:2], out['cpu'][:2]
    assert np.array_equal(xd, xh), np.abs(xd - xh).max()
    for key, a, b in zip(('P_val', 'q_val', 'A_val', 'l_val', 'u_val'), gd, gh):
        assert np.array_equal(a, b), (key, np.abs(a - b).max())
