"""The reference's torch layer (/root/reference/src/osqp/nn/torch.py:22-290) on the MI355X engine.

The reference keeps one ``osqp.OSQP`` object per batch element alive across forward calls (nn/torch.py:113-140, 200-224) and fans the elements out
over joblib threads.  Here ONE persistent engine handle plays that role: set up once (``setup_count``), afterwards only ``update()``d when the matrix
values change, and a forward or a backward is one call of a batch entry of that handle wherever one takes the problem.  Which entry is the route table
below, and ``_FORWARD`` / ``_BACKWARD`` are that table as data: ``_walk`` tries the entries of a row in order.  NI: the entry raised ValueError with the
engine's not-implemented code (the problem does not fit one workgroup, or the handle is not on that route); any other error of an entry comes out as it is.

Forward (nn/torch.py:113-230), one rank.  P_val and A_val 1-D: shared by the batch; 2-D: per element (:128-157, 184-217).

  matrices     q, l, u        entries tried in order, by ``large_batch``                                                  counter
  shared       host arrays    hip_batch_solve; on NI 'loop': _loop | 'lockstep': hip_batch_solve_lockstep (NI raises)      none
                              | 'lockstep_direct': hip_batch_solve_lockstep_direct (NI raises)
  shared       ROCm tensors   hip_batch_solve_device (zero-copy, torch's current stream); on NI 'loop': the row above,     none
                              which asks hip_batch_solve again | 'lockstep': hip_batch_solve_lockstep_device (NI raises)
                              | 'lockstep_direct': hip_batch_solve_lockstep_direct_device (NI raises)
  per element  either, as     hip_batch_solve(Px, Ax);                                                                     mat_batch_launches
               host arrays    on NI 'loop': _loop                                                                          none
                              | 'lockstep': hip_batch_solve_lockstep(Px, Ax) (NI raises)                                   mat_lockstep_launches
                              | 'lockstep_direct': hip_batch_solve_lockstep_direct(Px, Ax); on NI: _loop                   mat_lockstep_direct_launches

  Two asymmetries, kept as they grew: with shared matrices a handle that 'lockstep_direct' declines raises, with per-element matrices it goes on to
  _loop; and per-element 'lockstep' raises where per-element 'lockstep_direct' goes on.
  _loop is the reference's own route: update(Px, Ax, q, l, u) + solve() per element on the handle (:136-157).  A batch element that is not solved
  raises RuntimeError (:158-162).  ``last_dual`` keeps the duals, ``last_rec`` the per-element record of a forward that ran on host arrays.
  ``polishing=True`` is passed to ``setup``: the handle polishes every solved problem on whichever route takes it ('lockstep_direct' included).
  With ``torch.distributed`` initialised (world size > 1) the batch entries above do not apply: shared matrices are block-partitioned over the ranks
  and the rows all-gathered (``osqp_amd.sharded``, host or device), on NI _loop; per-element matrices take _loop.

Backward (nn/torch.py:233-290): when an input requires grad, ``forward`` runs as a ``torch.autograd.Function`` on the (x, y) the forward kept.

  gradient       entries tried in order, by ``large_backward``; every NI goes on
  host tensor    hip_batch_adjoint; 'lockstep': hip_batch_adjoint_lockstep | 'lockstep_direct': hip_batch_adjoint_lockstep_direct; _backward_loop
  ROCm tensor    the same entries with the suffix _device (zero-copy, torch's current stream); _backward_loop

  The lockstep entries are given Px / Ax only for a 2-D side.  ``adjoint_launches`` rises by 1 per call made and by 1 per element in _backward_loop
  (the single-handle adjoint at the forward's (x, y), which raises NotImplementedError on a handle it does not take -- one with a Woodbury-corrected
  preconditioner, unless the layer was made with ``woodbury_backward=True``, which sets OSQPHipPolicy::adjoint_woodbury on every handle it creates;
  ``large_backward='lockstep_direct'`` keeps precedence where it applies); ``mat_lockstep_adjoint_launches``
  / ``mat_lockstep_direct_adjoint_launches`` by 1 when that call was given matrices.  ``last_adjoint_rec`` keeps the record per element (ext_hip
  ADJOINT_FIELDS); an element whose adjoint system a lockstep entry did not solve raises RuntimeError.  The gradients are shaped like the inputs: an
  input shared by the batch (1-D) gets the batch sum, and dP holds for every entry of P_val (the full symmetric pattern P_idx) the value
  (r_i x_j + r_j x_i) / 2 of its position, the same in either triangle.  A ``torch.distributed`` job (world size > 1) raises NotImplementedError.
"""
import numpy as np
import scipy.sparse as spa
import torch
from torch.nn import Module

import osqp_amd
from osqp_amd import sharded

NEXT, RAISE = 'next', 'raise'      # what NI from an entry does: on to the next entry of the row, or out of the layer
ONE, MANY = 'one', 'many'          # an entry for one rank only / for a torch.distributed job only (None: either)

# A row of the route table: (entry, counters it bumps, the large_batch / large_backward it needs or None, ranks, what NI does).
_FORWARD = {   # (per-element matrices, q / l / u as ROCm tensors); per-element matrices always go through the host entries
    (False, False): [('hip_batch_solve', (), None, ONE, NEXT),
                     ('solve_batch_sharded', (), None, MANY, NEXT),
                     ('hip_batch_solve_lockstep', (), 'lockstep', ONE, RAISE),
                     ('hip_batch_solve_lockstep_direct', (), 'lockstep_direct', ONE, RAISE),
                     ('_loop', (), None, None, RAISE)],
    (False, True): [('hip_batch_solve_device', (), None, ONE, NEXT),
                    ('solve_batch_sharded_device', (), None, MANY, NEXT),
                    ('hip_batch_solve_lockstep_device', (), 'lockstep', ONE, RAISE),
                    ('hip_batch_solve_lockstep_direct_device', (), 'lockstep_direct', ONE, RAISE)],      # nothing left: the row of host arrays
    (True, False): [('hip_batch_solve', ('mat_batch_launches',), None, ONE, NEXT),
                    ('hip_batch_solve_lockstep', ('mat_lockstep_launches',), 'lockstep', ONE, RAISE),
                    ('hip_batch_solve_lockstep_direct', ('mat_lockstep_direct_launches',), 'lockstep_direct', ONE, NEXT),
                    ('_loop', (), None, None, RAISE)],
}
_BACKWARD = {  # per-element matrices; the entries are the host ones, a ROCm gradient takes their _device forms
    mat: [('hip_batch_adjoint', ('adjoint_launches',), None, ONE, NEXT),
          ('hip_batch_adjoint_lockstep', ('adjoint_launches',) + (('mat_lockstep_adjoint_launches',) if mat else ()), 'lockstep', ONE, NEXT),
          ('hip_batch_adjoint_lockstep_direct', ('adjoint_launches',) + (('mat_lockstep_direct_adjoint_launches',) if mat else ()), 'lockstep_direct', ONE, NEXT),
          ('_backward_loop', (), None, ONE, RAISE)]
    for mat in (False, True)}


def _np(t):
    return t.detach().cpu().double().numpy()


def _distributed():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def _declined(e):
    """True for the ValueError of an entry that declines (the table's NI); every other one is raised again."""
    if str(e) != str(int(osqp_amd.SolverError.OSQP_FUNC_NOT_IMPLEMENTED)):
        raise e
    return True


def _batch_shape(params):
    """Which of (P_val, q_val, A_val, l_val, u_val) are per element (2-D), and the batch size."""
    batched = [p.ndimension() == 2 for p in params]
    return batched, max([p.size(0) for p, b in zip(params, batched) if b], default=1)


def _dev_index(t):
    return (t.device.index or 0) if t.is_cuda else (torch.cuda.current_device() if torch.cuda.is_available() else 0)


def _forward_rows(a, nb, k):
    return a if a.ndim == 2 else np.broadcast_to(a, (nb, k))                          # nn/torch.py:184-188


def _host_rows(t, nb, k):
    return np.broadcast_to(np.asarray(_np(torch.as_tensor(t)), dtype=float).reshape(-1, k), (nb, k))


def _device_rows(t, dev, nb, k):
    return torch.as_tensor(t).detach().to(device=dev, dtype=torch.float64).reshape(-1, k).expand(nb, k).contiguous()


def _check_solved(status):
    """status: the status column of a forward's record, a numpy array or a host tensor."""
    bad = np.nonzero(np.asarray(status) != int(osqp_amd.SolverStatus.OSQP_SOLVED))[0]
    if bad.size:
        raise RuntimeError('Unable to solve QP, status: %d (batch element %d)' % (int(status[bad[0]]), int(bad[0])))


class OSQP(Module):
    def __init__(self, P_idx, P_shape, A_idx, A_shape, eps_rel=1e-5, eps_abs=1e-5, verbose=False, max_iter=10000, algebra='hip', solver_type='indirect', large_batch='loop', large_backward='loop', polishing=False, check_dualgap=False, woodbury_backward=False):
        super().__init__()
        if large_batch not in ('loop', 'lockstep', 'lockstep_direct'):
            raise ValueError("large_batch: 'loop', 'lockstep' or 'lockstep_direct'")
        if large_backward not in ('loop', 'lockstep', 'lockstep_direct'):
            raise ValueError("large_backward: 'loop', 'lockstep' or 'lockstep_direct'")
        self.large_backward = large_backward   # backward of such a batch: the single-handle adjoint per element ('loop'), or one call of the lockstep adjoint / its direct form for Woodbury handles
        self.large_batch = large_batch   # shared matrices too large for the batch kernel: one element after the other ('loop'), the lockstep route, or its direct form for Woodbury handles ('lockstep_direct')
        self.P_idx, self.P_shape, self.A_idx, self.A_shape = P_idx, P_shape, A_idx, A_shape
        self.eps_rel, self.eps_abs, self.verbose, self.max_iter = eps_rel, eps_abs, verbose, max_iter
        self.algebra, self.solver_type = algebra, solver_type
        self.polishing = bool(polishing)   # settings.polishing of the handle this layer sets up (default off: every forward as before)
        self.check_dualgap = bool(check_dualgap)   # settings.check_dualgap of that handle: every batch route then tests the duality gap per element (last_rec column 11)
        self.woodbury_backward = bool(woodbury_backward)   # OSQPHipPolicy::adjoint_woodbury = 1 on every handle this layer sets up: the 'loop' backward then differentiates on handles with a Woodbury-corrected preconditioner too (default off: such a handle raises NotImplementedError as before)
        self.n, self.m = P_shape[0], A_shape[0]
        self._solver = None          # the persistent handle (reference: the `solvers` list kept across forwards)
        self._Pv = self._Av = None   # matrix values currently on the handle
        self._device = None
        self._triu_pick = None       # positions of the upper-triangle entries of P inside P_val
        self.setup_count = 0         # number of osqp_setup calls made by this layer (1 after any number of same-structure forwards)
        self.last_dual = None
        self.adjoint_launches = 0    # launches of the adjoint kernel made by this layer's backward passes (one per backward; one per element where the batch kernel does not hold the problem)
        self.last_adjoint_rec = None # (nb, 4) record of the last backward: status, active rows, residual, reserved (ext_hip ADJOINT_FIELDS)
        self._grad_maps = None
        self.mat_batch_launches = 0      # calls of the one-workgroup kernel with per-element matrices made by this layer's forwards
        self.mat_lockstep_launches = 0   # calls of the lockstep route with per-element matrices made by this layer's forwards (large_batch='lockstep')
        self.last_rec = None         # per-element record of the last forward that ran on host arrays (ext_hip BATCH_FIELDS where a batch route made it: status_polish is column 8, duality_gap column 11)
        self.mat_lockstep_direct_launches = 0   # calls of the direct lockstep route with per-element matrices made by this layer's forwards (large_batch='lockstep_direct')
        self.mat_lockstep_adjoint_launches = 0   # calls of the lockstep adjoint with per-element matrices made by this layer's backwards (large_backward='lockstep')
        self.mat_lockstep_direct_adjoint_launches = 0   # calls of the direct lockstep adjoint with per-element matrices made by this layer's backwards (large_backward='lockstep_direct')

    # ------------------------------------------------------------------ the persistent handle
    def _matrices(self, P_val, A_val):
        P = spa.csc_matrix((P_val, self.P_idx), shape=self.P_shape)
        A = spa.csc_matrix((A_val, self.A_idx), shape=self.A_shape)
        return P, A

    def _handle(self, P_val, A_val, q0, l0, u0, device=0):
        """The set-up solver for these matrix values: created on first use, afterwards only update()d (nn/torch.py:136-140)."""
        if self._solver is None or self._device != device:
            P, A = self._matrices(P_val, A_val)
            if self._triu_pick is None:
                tag = spa.triu(self._matrices(np.arange(1, len(P_val) + 1, dtype=float), A_val)[0], format='csc')
                self._triu_pick = tag.data.astype(int) - 1
            s = osqp_amd.OSQP(algebra=self.algebra)
            s.setup(P, q0, A, l0, u0, solver_type=self.solver_type, verbose=self.verbose, eps_abs=self.eps_abs, eps_rel=self.eps_rel,
                    max_iter=self.max_iter, warm_starting=False, device=device, **({'polishing': True} if self.polishing else {}),
                    **({'check_dualgap': True} if self.check_dualgap else {}))
            if self.woodbury_backward:
                s._solver.set_policy(adjoint_woodbury=1)
            self._solver, self._device = s, device
            self._Pv, self._Av = np.array(P_val, dtype=float), np.array(A_val, dtype=float)
            self.setup_count += 1
        elif not (np.array_equal(self._Pv, P_val) and np.array_equal(self._Av, A_val)):
            self._solver.update(Px=np.asarray(P_val, dtype=float)[self._triu_pick], Ax=np.asarray(A_val, dtype=float))
            self._Pv, self._Av = np.array(P_val, dtype=float), np.array(A_val, dtype=float)
        return self._solver

    def _per_element(self, Pn, An, batched):
        """(Px, Ax) of a batch entry: the upper triangle of a 2-D P_val, a 2-D A_val, None for a shared side."""
        return (Pn[:, self._triu_pick] if batched[0] else None), (An if batched[2] else None)

    def _walk(self, routes, mode, world, call):
        """The one ladder of forward and backward: call(entry) for the entries of `routes` that apply to `mode` (large_batch / large_backward) and to
        `world`, in order, until one does not decline; its counters are bumped here and nowhere else.  Returns (entry, what call returned), or
        (None, None) where every entry that applies declined and was allowed to."""
        for entry, counters, needs, ranks, on_decline in routes:
            if needs not in (None, mode) or (ranks is not None and (ranks == ONE) != (world == 1)):
                continue
            try:
                out = call(entry)
            except ValueError as e:
                if on_decline == RAISE:
                    raise
                _declined(e)
                continue
            for c in counters:
                setattr(self, c, getattr(self, c) + 1)
            return entry, out
        return None, None

    # ------------------------------------------------------------------ forward
    def forward(self, P_val, q_val, A_val, l_val, u_val):
        params = (P_val, q_val, A_val, l_val, u_val)
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return _OSQPFunction.apply(self, *params)
        return self._solve(*params)

    def _walk_forward(self, routes, world, call):
        """_walk for a forward, whose call(entry) returns (x, y, rec): keeps the duals and returns (x, rec); None where _walk found no entry."""
        entry, out = self._walk(routes, self.large_batch, world, call)
        if entry is None:
            return None
        x, y, rec = out
        if y is not None:
            self.last_dual = y
        return x, rec

    def _solve(self, P_val, q_val, A_val, l_val, u_val):
        params = [P_val, q_val, A_val, l_val, u_val]
        for p in params:
            assert p.ndimension() <= 2, 'Unexpected number of dimensions'
        dtype, device = q_val.dtype, q_val.device
        batched, nb = _batch_shape(params)
        mat = batched[0] or batched[2]
        Pn, An = _np(P_val), _np(A_val)                                                # (small: the matrix VALUES, once per forward)
        rank, world = _distributed()
        if not mat and q_val.is_cuda:                                                  # data on the GPU: zero-copy (one rank, or this rank's share)
            out = self._forward_device(Pn, An, q_val, l_val, u_val, nb, rank, world)
            if out is not None:
                return out if any(batched) else out.squeeze(0)
        qn, ln, un = _forward_rows(_np(q_val), nb, self.n), _forward_rows(_np(l_val), nb, self.m), _forward_rows(_np(u_val), nb, self.m)
        dev_index = _dev_index(q_val)
        if not mat:
            s = self._handle(Pn, An, qn[0], ln[0], un[0], device=dev_index)
        elif world == 1:
            # (the handle's OWN matrices matter only for the side that is shared; a batched side keeps what the handle holds -- no re-assembly per forward)
            have = self._solver is not None and self._device == dev_index
            s = self._handle((self._Pv if have else Pn[0]) if batched[0] else Pn, (self._Av if have else An[0]) if batched[2] else An, qn[0], ln[0], un[0], device=dev_index)

        def call(entry):
            if entry == '_loop':
                return self._loop(Pn, qn, An, ln, un, nb, batched, dev_index)
            if entry == 'solve_batch_sharded':
                dev = device if q_val.is_cuda else None
                table, xl, yl, (lo, hi) = sharded.solve_batch_sharded(s, q=qn, l=ln, u=un, rank=rank, world=world, device=dev)
                x = sharded.gather_rows(xl, nb, device=dev)
                rec = np.zeros((nb, 8)); rec[:, 0:5] = table[:, 1:6]
                return x, None, rec
            Px, Ax = self._per_element(Pn, An, batched)
            return getattr(s._solver, entry)(q=qn, l=ln, u=un, Px=Px, Ax=Ax, nbatch=nb)
        x, rec = self._walk_forward(_FORWARD[mat, False], world, call)
        self.last_rec = rec
        _check_solved(rec[:, 0])
        out = torch.as_tensor(x, dtype=dtype, device=device)
        return out if any(batched) else out.squeeze(0)

    def _forward_device(self, Pn, An, q_val, l_val, u_val, nb, rank=0, world=1):
        """q, l, u stay where they are (float64, contiguous, (nb, .) on q_val's device); x comes back as a device tensor, None where the device row
        of the table is used up.  In a distributed job (world > 1) this rank solves its contiguous share by device pointer and the shares meet in two
        all_gathers of device tensors (records, solutions) -- no host copy of q, l, u or x (sharded.solve_batch_sharded_device)."""
        dev = q_val.device
        exp = lambda t, k: t.detach().to(device=dev, dtype=torch.float64).expand(nb, k).contiguous()
        qd, ld, ud = exp(q_val, self.n), exp(l_val, self.m), exp(u_val, self.m)
        if self._solver is None or self._device != (dev.index or 0):                   # first forward only: the handle's own q, l, u
            s = self._handle(Pn, An, qd[0].cpu().numpy(), ld[0].cpu().numpy(), ud[0].cpu().numpy(), device=dev.index or 0)
        else:
            s = self._handle(Pn, An, None, None, None, device=dev.index or 0)

        def call(entry):
            if entry == 'solve_batch_sharded_device':
                table, xl, yl, (lo, hi) = sharded.solve_batch_sharded_device(s, q=qd, l=ld, u=ud, rank=rank, world=world)
                _check_solved(table[:, 1].to('cpu'))                                    # 8 bytes per problem: the statuses
                y = sharded.gather_rows_device(yl, nb)
                return sharded.gather_rows_device(xl, nb), y, None
            x = torch.empty((nb, self.n), dtype=torch.float64, device=dev)
            y = torch.empty((nb, self.m), dtype=torch.float64, device=dev)
            rec = torch.empty((nb, 12), dtype=torch.float64, device=dev)    # OSQP_HIP_BATCH_REC
            getattr(s._solver, entry)(nb, qd.data_ptr(), ld.data_ptr(), ud.data_ptr(), x.data_ptr(), y.data_ptr(), rec.data_ptr(),
                                      warm=False, stream=torch.cuda.current_stream(dev).cuda_stream)
            _check_solved(rec[:, 0].to('cpu'))                                          # (waits for the stream)
            return x, y, rec
        out = self._walk_forward(_FORWARD[False, True], world, call)
        return None if out is None else out[0].to(q_val.dtype)

    def _loop(self, Pn, qn, An, ln, un, nb, batched, dev_index=0):
        """Per-element matrices (or a problem too large for the batch kernel): the single-QP engine, one element after the
        other on the persistent handle -- update(Px, Ax, q, l, u) + solve(), as nn/torch.py:136-157."""
        x = np.zeros((nb, self.n)); y = np.zeros((nb, self.m)); rec = np.zeros((nb, 8))
        for i in range(nb):
            Pv = Pn[i] if batched[0] else Pn
            Av = An[i] if batched[2] else An
            s = self._handle(Pv, Av, qn[i], ln[i], un[i], device=dev_index)
            s.update(q=qn[i], l=ln[i], u=un[i])
            r = s.solve()
            x[i] = r.x
            y[i] = r.y
            rec[i, 0], rec[i, 1], rec[i, 2] = r.info.status_val, r.info.iter, r.info.obj_val
        return x, y, rec

    # ------------------------------------------------------------------ backward
    def _p_map(self, nP):
        """P_val position -> position of its upper-triangle twin in the engine's dP (upper triangle of P, CSC order)."""
        if self._grad_maps is None:
            rows, cols = (np.asarray(a).astype(np.int64) for a in self.P_idx)
            tr, tc = np.minimum(rows, cols), np.maximum(rows, cols)
            where = {(int(tr[k]), int(tc[k])): t for t, k in enumerate(self._triu_pick)}
            self._grad_maps = np.array([where[(int(tr[k]), int(tc[k]))] for k in range(nP)], dtype=np.int64)
        return self._grad_maps

    def _backward_loop(self, Pn, An, ln, un, X, Y, g, nb, batched, want):
        """Backward of a batch the batch adjoint kernel does not hold (the forward's _loop): the single-handle adjoint (the PCG route for large QPs)
        once per element at the (x, y) the forward kept -- osqp_hip_adjoint_compute_at: the element's matrices and bounds go onto the handle, no
        solve is repeated.  Every call is counted in adjoint_launches."""
        widths = {'dP': len(self._triu_pick), 'dq': self.n, 'dA': An.shape[-1], 'dl': self.m, 'du': self.m}
        res = {k: np.zeros((nb, widths[k])) for k in want}
        res['rec'] = np.zeros((nb, 4))
        NI = int(osqp_amd.SolverError.OSQP_FUNC_NOT_IMPLEMENTED)
        for i in range(nb):
            s = self._handle(Pn[i] if batched[0] else Pn, An[i] if batched[2] else An, None, ln[i], un[i], device=self._device)
            s.update(l=ln[i], u=un[i])      # (leaves the last element's bounds on the handle and its status reset: every forward updates all data before it solves)
            ext = s._solver
            st = ext.adjoint_derivative_compute_at(X[i], Y[i], np.ascontiguousarray(g[i], dtype=float))
            self.adjoint_launches += 1
            rec = ext.adjoint_last_record()
            res['rec'][i] = (rec['status'], rec['active_rows'], rec['residual'], rec['steps'])
            if st == NI:
                raise NotImplementedError('osqp_amd.nn.torch.OSQP: backward is not available on this handle (Woodbury-corrected preconditioner: woodbury_backward=True takes it; include/osqp_hip.h)')
            if st:
                raise RuntimeError('adjoint derivatives of batch element %d: error %d (status %d, residual %.3e)' % (i, int(st), rec['status'], rec['residual']))
            dP, dA = s.ext.CSC(s._derivative_cache['P'].copy()), s.ext.CSC(s._derivative_cache['A'].copy())
            st = ext.adjoint_derivative_get_mat(dP, dA)
            dq, dl, du = np.empty(self.n), np.zeros(self.m), np.zeros(self.m)
            st = st or ext.adjoint_derivative_get_vec(dq, dl, du)
            if st:
                raise RuntimeError('adjoint derivatives of batch element %d: error %d' % (i, int(st)))
            for k, v in (('dP', dP.x), ('dA', dA.x), ('dq', dq), ('dl', dl), ('du', du)):
                if k in res: res[k][i] = v
        return {k: torch.as_tensor(v) for k, v in res.items()}

    def _adjoint_call(self, ext, saved, Pn, An, x, y, g, nb, batched, want):
        """The one marshalling of a batch adjoint: launch(entry) calls that host entry of `ext` on host arrays or, for a gradient on the GPU, its
        _device form by device pointer on torch's current stream (zero-copy), and returns the gradients named in `want` and 'rec' as tensors."""
        P_val, q_val, A_val, l_val, u_val = saved
        if not g.is_cuda:
            Px, Ax = self._per_element(Pn, An, batched)
            xn, yn, gn, ln, un = (_host_rows(t, nb, k) for t, k in ((x, self.n), (y, self.m), (g, self.n), (l_val, self.m), (u_val, self.m)))
            return lambda entry: {k: torch.as_tensor(v) for k, v in getattr(ext, entry)(xn, yn, gn, None, l=ln, u=un, Px=Px, Ax=Ax, want=want).items()}
        dev = g.device
        xd, yd, gd, ld, ud = (_device_rows(t, dev, nb, k) for t, k in ((x, self.n), (y, self.m), (g, self.n), (l_val, self.m), (u_val, self.m)))
        Pxd = _device_rows(P_val, dev, nb, Pn.shape[-1])[:, torch.as_tensor(self._triu_pick, device=dev)].contiguous() if batched[0] else None
        Axd = _device_rows(A_val, dev, nb, An.shape[-1]) if batched[2] else None
        widths = {'dP': len(self._triu_pick), 'dq': self.n, 'dA': An.shape[-1], 'dl': self.m, 'du': self.m}
        res = {k: torch.empty((nb, widths[k]), dtype=torch.float64, device=dev) for k in want}
        res['rec'] = torch.empty((nb, 4), dtype=torch.float64, device=dev)             # OSQP_HIP_ADJOINT_REC
        ptr = lambda t: None if t is None else t.data_ptr()

        def launch(entry):
            getattr(ext, entry + '_device')(nb, x_ptr=ptr(xd), y_ptr=ptr(yd), dx_ptr=ptr(gd), dy_ptr=None, l_ptr=ptr(ld), u_ptr=ptr(ud), Px_ptr=ptr(Pxd), Ax_ptr=ptr(Axd),
                                            dP_ptr=ptr(res.get('dP')), dq_ptr=ptr(res.get('dq')), dA_ptr=ptr(res.get('dA')), dl_ptr=ptr(res.get('dl')), du_ptr=ptr(res.get('du')),
                                            rec_ptr=ptr(res['rec']), stream=torch.cuda.current_stream(dev).cuda_stream)
            return res
        return launch

    def _backward(self, saved, x, y, dl_dx, needs):
        P_val, q_val, A_val, l_val, u_val = params = list(saved)
        batched, nb = _batch_shape(params)
        if _distributed()[1] > 1:
            raise NotImplementedError('osqp_amd.nn.torch.OSQP: backward in a torch.distributed job (world size > 1) is not implemented')
        if y is None:
            raise NotImplementedError('osqp_amd.nn.torch.OSQP: backward needs the duals of the forward, which this forward did not keep')
        Pn, An = _np(P_val), _np(A_val)
        # the handle's own values of a SHARED side are what the forward solved with (an intermediate forward may have replaced them)
        s = self._handle(self._Pv if batched[0] else Pn, self._Av if batched[2] else An, None, None, None, device=self._device)
        p_map = self._p_map(Pn.shape[-1])      # (A_val is in the CSC order of A, as the forward takes it)
        want = tuple(k for k, need in zip(('dP', 'dq', 'dA', 'dl', 'du'), needs) if need)
        g = dl_dx.detach().reshape(-1, self.n)
        if g.shape[0] != nb:
            g = g.expand(nb, self.n)
        launch = self._adjoint_call(s._solver, saved, Pn, An, x, y, g, nb, batched, want)

        def call(entry):
            if entry != '_backward_loop':
                return launch(entry)
            # outside the batch kernel (the forward ran _loop): the single-handle adjoint per element
            return self._backward_loop(Pn, An, _host_rows(l_val, nb, self.m), _host_rows(u_val, nb, self.m), _host_rows(x, nb, self.n), _host_rows(y, nb, self.m),
                                       _np(g).reshape(nb, self.n), nb, batched, want)
        entry, res = self._walk(_BACKWARD[batched[0] or batched[2]], self.large_backward, 1, call)
        self.last_adjoint_rec = res['rec']
        if 'lockstep' in entry:                            # an element whose adjoint system was not solved raises as _backward_loop does
            rec = res['rec'].cpu().numpy()
            bad = np.nonzero(rec[:, 0] != 0)[0]
            if bad.size:
                i = int(bad[0])
                raise RuntimeError('adjoint derivatives of batch element %d: error %d (status %d, residual %.3e)'
                                   % (i, int(osqp_amd.SolverError.OSQP_LINSYS_SOLVER_INIT_ERROR), int(rec[i, 0]), rec[i, 2]))
        if 'dP' in res:                                    # engine order (upper triangle, CSC) -> the order of P_val, either triangle the same value
            res['dP'] = res['dP'][:, torch.as_tensor(p_map, device=res['dP'].device)]
        grads = []
        for key, p, b in zip(('dP', 'dq', 'dA', 'dl', 'du'), params, batched):
            if key not in res:
                grads.append(None)
                continue
            v = res[key] if b else res[key].sum(0)
            grads.append(v.to(device=p.device, dtype=p.dtype).reshape(p.shape))
        return tuple(grads)


class _OSQPFunction(torch.autograd.Function):
    """forward = the layer's solve; backward = one launch of the adjoint kernel on what the forward kept (x, the duals, the inputs)."""

    @staticmethod
    def forward(ctx, layer, P_val, q_val, A_val, l_val, u_val):
        layer.last_dual = None
        out = layer._solve(P_val.detach(), q_val.detach(), A_val.detach(), l_val.detach(), u_val.detach())
        ctx.layer, ctx.dual = layer, layer.last_dual
        ctx.save_for_backward(P_val, q_val, A_val, l_val, u_val, out)
        return out

    @staticmethod
    def backward(ctx, dl_dx):
        *saved, out = ctx.saved_tensors
        return (None,) + ctx.layer._backward(saved, out, ctx.dual, dl_dx, ctx.needs_input_grad[1:])
