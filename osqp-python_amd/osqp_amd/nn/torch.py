"""Forward pass of the reference's torch layer (/root/reference/src/osqp/nn/torch.py:22-230) on the MI355X engine.

The reference keeps one ``osqp.OSQP`` object per batch element alive ACROSS forward calls -- the first call sets them up, every
later call only ``update()``s and ``solve()``s them (nn/torch.py:113-140, 200-224) -- and fans the elements out over joblib
threads.  Here one persistent engine handle plays that role:

  * P_val and A_val shared by the whole batch (1-D tensors): the handle is set up ONCE (``setup_count`` counts it); later
    forwards re-upload the matrix values only if they changed (``osqp_update_data_mat``: device-side re-assembly) and solve
    the whole batch with ONE kernel launch (one workgroup per problem: the reference's update(q,l,u)+solve() per element).
    q / l / u that live on the GPU (torch ROCm tensors) are handed over ZERO-COPY by device pointer on torch's current
    stream (``osqp_hip_batch_solve_device``) and the solution is produced on the device;
  * with ``torch.distributed`` initialised (world size > 1) the batch is block-partitioned over the ranks, every rank solves its
    share on its own GPU, and the rows are all-gathered (``osqp_amd.sharded``) -- the multi-GPU form of the reference's thread pool;
  * per-element P_val / A_val (2-D tensors, :128-157, 184-217): the SAME single launch -- every workgroup reads its own element's matrix values, assembled
    and equilibrated per element by a launch in front of it (osqp_hip_batch_solve_mat); only a problem too large for one workgroup falls back to the
    single-QP handle, one element after the other -- or, with ``large_batch='lockstep'``, goes to the lockstep route (osqp_hip_batch_solve_lockstep:
    64 problems at a time on block vectors, any size; host tensors through the host entry, ROCm tensors zero-copy through the device entry), or, with
    ``large_batch='lockstep_direct'``, to its direct form for a Woodbury handle with a diagonal K0 (osqp_hip_batch_solve_lockstep_direct: the
    factor-model portfolio QP, which the lockstep route declines); a handle the chosen route declines raises as ``'lockstep'`` always has.
    With ``large_batch='lockstep'`` (one rank) a forward with 2-D P_val and / or A_val that the single launch declines makes ONE call of the lockstep
    route with per-element matrices (osqp_hip_batch_solve_lockstep_mat; ``mat_lockstep_launches`` counts them) in place of the per-element loop; its
    backward is the per-element loop unless ``large_backward='lockstep'`` (below).
    With ``large_batch='lockstep_direct'`` (one rank) such a forward on a Woodbury handle with a diagonal K0 makes ONE call of the direct route with per-element
    matrices (osqp_hip_batch_solve_lockstep_direct_mat: every element scaled and solved on its own P_val / A_val; ``mat_lockstep_direct_launches`` counts
    them; host and ROCm tensors alike through the host entry); a handle that entry declines goes on to the per-element loop as before.  The backward of such a
    forward is the per-element loop, which raises NotImplementedError on a Woodbury handle, unless ``large_backward='lockstep_direct'`` (below).
  * ``polishing=True`` (default False: every forward as before) is passed to ``setup``: the handle polishes every solved problem, on whichever route the
    forward takes -- the one-workgroup kernel, the per-element loop, the lockstep route with shared or with per-element matrices (there the polish runs
    on the device inside the one call; ``lockstep_polish_last_record`` of the handle counts attempted / accepted / rejected).  The adjoint classifies the
    active rows from (x, y), and a polished point gives a clean active set.  With ``large_batch='lockstep_direct'`` the route does not polish.

Like the reference, a batch element that is not solved raises RuntimeError (:158-162).

Backward (the reference's :233-290): when an input requires grad, ``forward`` runs as a ``torch.autograd.Function`` and the returned tensor carries a
grad_fn.  ``backward(dl_dx)`` makes ONE launch of the adjoint kernel for the whole batch (``osqp_hip_batch_adjoint``; ``adjoint_launches`` counts
them) on the solution and duals the forward kept, and returns (dP, dq, dA, dl, du) shaped like the inputs: an input shared by the batch (1-D) gets
the sum over the batch, as autograd's ``expand`` would give.  dP holds, for every entry of P_val (the full symmetric pattern P_idx), the value
(r_i x_j + r_j x_i) / 2 of its position -- the same in either triangle.  Gradients arriving on the GPU go through the device-pointer entry point
on torch's current stream, zero-copy.  ``last_adjoint_rec`` keeps the kernel's record per element (status, active rows, residual).  A problem the
batch kernel cannot hold (its forward ran one element after the other on the handle) is differentiated the same way: the single-handle adjoint
(``osqp_hip_adjoint_compute_at``: the PCG route for large QPs, at the (x, y) the forward kept) once per element, ``adjoint_launches`` counting every call, shared inputs receiving
the batch sum -- or, with ``large_backward='lockstep'`` (default ``'loop'``: unchanged) and shared P_val / A_val, ONE call of the lockstep adjoint for the whole batch
(``osqp_hip_batch_adjoint_lockstep``; ``adjoint_launches`` rises by 1; an element whose adjoint system was not solved raises RuntimeError as the
per-element route does), or, with ``large_backward='lockstep_direct'``, ONE call of its direct form on a Woodbury handle with a diagonal K0
(``osqp_hip_batch_adjoint_lockstep_direct``: the backward of ``large_batch='lockstep_direct'``; a handle the route declines goes on to the per-element
loop, as with ``'lockstep'``).  With ``large_backward='lockstep'`` and 2-D P_val and / or A_val that the batch adjoint kernel declines, the backward is
ONE call of the lockstep adjoint with per-element matrices (``osqp_hip_batch_adjoint_lockstep_mat``: every element's adjoint system on its own matrices
and scaling; ``adjoint_launches`` rises by 1 and ``mat_lockstep_adjoint_launches`` counts these calls; host tensors through the host entry, ROCm tensors
zero-copy through the device entry) in place of update(Px, Ax) + the single-handle adjoint per element; a handle that entry declines goes on to the
per-element loop.  With ``large_backward='lockstep_direct'`` and 2-D P_val and / or A_val the backward is likewise ONE call of the direct lockstep adjoint
with per-element matrices (``osqp_hip_batch_adjoint_lockstep_direct_mat``: every element's adjoint system on its own matrices, dense rows and scaling by the
Woodbury formula -- the backward of ``large_batch='lockstep_direct'`` with per-element factor models; ``adjoint_launches`` rises by 1 and
``mat_lockstep_direct_adjoint_launches`` counts these calls; host tensors through the host entry, ROCm tensors zero-copy through the device entry on torch's
current stream); a handle the route declines goes on to the per-element loop.  A ``torch.distributed`` job (world size > 1) raises NotImplementedError in backward.  With no input requiring grad,
forward behaves exactly as before.
"""
import numpy as np
import scipy.sparse as spa
import torch
from torch.nn import Module

import osqp_amd
from osqp_amd import sharded


def _np(t):
    return t.detach().cpu().double().numpy()


def _distributed():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


class OSQP(Module):
    def __init__(self, P_idx, P_shape, A_idx, A_shape, eps_rel=1e-5, eps_abs=1e-5, verbose=False, max_iter=10000, algebra='hip', solver_type='indirect', large_batch='loop', large_backward='loop', polishing=False):
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
        self.mat_lockstep_launches = 0   # calls of the lockstep route with per-element matrices made by this layer's forwards (large_batch='lockstep')
        self.last_rec = None         # per-element record of the last forward that ran on host arrays (ext_hip BATCH_FIELDS where a batch route made it: status_polish is column 8)
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
                    max_iter=self.max_iter, warm_starting=False, device=device, **({'polishing': True} if self.polishing else {}))
            self._solver, self._device = s, device
            self._Pv, self._Av = np.array(P_val, dtype=float), np.array(A_val, dtype=float)
            self.setup_count += 1
        elif not (np.array_equal(self._Pv, P_val) and np.array_equal(self._Av, A_val)):
            self._solver.update(Px=np.asarray(P_val, dtype=float)[self._triu_pick], Ax=np.asarray(A_val, dtype=float))
            self._Pv, self._Av = np.array(P_val, dtype=float), np.array(A_val, dtype=float)
        return self._solver

    # ------------------------------------------------------------------ forward
    def forward(self, P_val, q_val, A_val, l_val, u_val):
        params = (P_val, q_val, A_val, l_val, u_val)
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return _OSQPFunction.apply(self, *params)
        return self._solve(*params)

    def _solve(self, P_val, q_val, A_val, l_val, u_val):
        params = [P_val, q_val, A_val, l_val, u_val]
        for p in params:
            assert p.ndimension() <= 2, 'Unexpected number of dimensions'
        dtype, device = q_val.dtype, q_val.device
        batched = [p.ndimension() == 2 for p in params]
        nb = max([p.size(0) for p, b in zip(params, batched) if b], default=1)
        shared = not batched[0] and not batched[2]
        Pn, An = _np(P_val), _np(A_val)                                                # (small: the matrix VALUES, once per forward)
        rank, world = _distributed()
        if shared and q_val.is_cuda:                                                   # data on the GPU: zero-copy (one rank, or this rank's share)
            out = self._forward_device(Pn, An, q_val, l_val, u_val, nb, rank, world)
            if out is not None:
                return out if any(batched) else out.squeeze(0)
        bc = lambda a, k: a if a.ndim == 2 else np.broadcast_to(a, (nb, k))          # nn/torch.py:184-188
        qn, ln, un = bc(_np(q_val), self.n), bc(_np(l_val), self.m), bc(_np(u_val), self.m)
        if shared:                                                                      # shared matrices: batched kernel
            dev_index = (device.index or 0) if q_val.is_cuda else (torch.cuda.current_device() if torch.cuda.is_available() else 0)
            s = self._handle(Pn, An, qn[0], ln[0], un[0], device=dev_index)
            try:
                if world > 1:
                    table, xl, yl, (lo, hi) = sharded.solve_batch_sharded(s, q=qn, l=ln, u=un, rank=rank, world=world,
                                                                         device=device if q_val.is_cuda else None)
                    x = sharded.gather_rows(xl, nb, device=device if q_val.is_cuda else None)
                    rec = np.zeros((nb, 8)); rec[:, 0:5] = table[:, 1:6]
                else:
                    x, y, rec = s._solver.hip_batch_solve(q=qn, l=ln, u=un)
                    self.last_dual = y
            except ValueError as e:                                                    # only "does not fit one workgroup's LDS" falls back
                if str(e) != str(int(osqp_amd.SolverError.OSQP_FUNC_NOT_IMPLEMENTED)):
                    raise
                if self.large_batch == 'lockstep' and world == 1:                      # any size, 64 problems at a time (osqp_hip_batch_solve_lockstep)
                    x, y, rec = s._solver.hip_batch_solve_lockstep(q=qn, l=ln, u=un)
                    self.last_dual = y
                elif self.large_batch == 'lockstep_direct' and world == 1:             # a Woodbury handle with a diagonal K0 (osqp_hip_batch_solve_lockstep_direct)
                    x, y, rec = s._solver.hip_batch_solve_lockstep_direct(q=qn, l=ln, u=un)
                    self.last_dual = y
                else:
                    x, rec = self._loop(Pn, qn, An, ln, un, nb, batched, dev_index)
        else:
            dev_index = (device.index or 0) if q_val.is_cuda else (torch.cuda.current_device() if torch.cuda.is_available() else 0)
            x = rec = None
            if world == 1:                                                              # per-element matrices: one launch (osqp_hip_batch_solve_mat)
                # (the handle's OWN matrices matter only for the side that is shared; a batched side keeps what the handle holds -- no re-assembly per forward)
                have = self._solver is not None and self._device == dev_index
                s = self._handle((self._Pv if have else Pn[0]) if batched[0] else Pn, (self._Av if have else An[0]) if batched[2] else An, qn[0], ln[0], un[0], device=dev_index)
                try:
                    x, y, rec = s._solver.hip_batch_solve(q=qn, l=ln, u=un, Px=(Pn[:, self._triu_pick] if batched[0] else None), Ax=(An if batched[2] else None), nbatch=nb)
                    self.last_dual = y
                    self.mat_batch_launches = getattr(self, 'mat_batch_launches', 0) + 1
                except ValueError as e:
                    if str(e) != str(int(osqp_amd.SolverError.OSQP_FUNC_NOT_IMPLEMENTED)):
                        raise
                    x = rec = None
                    if self.large_batch == 'lockstep':                                  # any size, every element on its own matrices: ONE call (osqp_hip_batch_solve_lockstep_mat)
                        x, y, rec = s._solver.hip_batch_solve_lockstep(q=qn, l=ln, u=un, Px=(Pn[:, self._triu_pick] if batched[0] else None), Ax=(An if batched[2] else None), nbatch=nb)
                        self.last_dual = y
                        self.mat_lockstep_launches += 1
                    elif self.large_batch == 'lockstep_direct':                         # a Woodbury handle with a diagonal K0, every element on its own matrices: ONE call (osqp_hip_batch_solve_lockstep_direct_mat)
                        try:
                            x, y, rec = s._solver.hip_batch_solve_lockstep_direct(q=qn, l=ln, u=un, Px=(Pn[:, self._triu_pick] if batched[0] else None), Ax=(An if batched[2] else None), nbatch=nb)
                            self.last_dual = y
                            self.mat_lockstep_direct_launches += 1
                        except ValueError as e2:                                        # a handle that entry declines: the per-element loop, as before
                            if str(e2) != str(int(osqp_amd.SolverError.OSQP_FUNC_NOT_IMPLEMENTED)):
                                raise
                            x = rec = None
            if x is None:
                x, rec = self._loop(Pn, qn, An, ln, un, nb, batched, dev_index)
        self.last_rec = rec
        bad = np.nonzero(rec[:, 0] != int(osqp_amd.SolverStatus.OSQP_SOLVED))[0]
        if bad.size:
            raise RuntimeError('Unable to solve QP, status: %d (batch element %d)' % (int(rec[bad[0], 0]), int(bad[0])))
        out = torch.as_tensor(x, dtype=dtype, device=device)
        return out if any(batched) else out.squeeze(0)

    def _forward_device(self, Pn, An, q_val, l_val, u_val, nb, rank=0, world=1):
        """q, l, u stay where they are (float64, contiguous, (nb, .) on q_val's device); x comes back as a device tensor.  In a
        distributed job (world > 1) this rank solves its contiguous share by device pointer and the shares meet in two all_gathers of
        device tensors (records, solutions) -- no host copy of q, l, u or x (sharded.solve_batch_sharded_device)."""
        dev = q_val.device
        exp = lambda t, k: t.detach().to(device=dev, dtype=torch.float64).expand(nb, k).contiguous()
        qd, ld, ud = exp(q_val, self.n), exp(l_val, self.m), exp(u_val, self.m)
        if self._solver is None or self._device != (dev.index or 0):                   # first forward only: the handle's own q, l, u
            s = self._handle(Pn, An, qd[0].cpu().numpy(), ld[0].cpu().numpy(), ud[0].cpu().numpy(), device=dev.index or 0)
        else:
            s = self._handle(Pn, An, None, None, None, device=dev.index or 0)
        if world > 1:
            try:
                table, xl, yl, (lo, hi) = sharded.solve_batch_sharded_device(s, q=qd, l=ld, u=ud, rank=rank, world=world)
            except ValueError as e:
                if str(e) != str(int(osqp_amd.SolverError.OSQP_FUNC_NOT_IMPLEMENTED)):
                    raise
                return None
            st = table[:, 1].to('cpu')                                                  # 8 bytes per problem: the statuses
            bad = torch.nonzero(st != int(osqp_amd.SolverStatus.OSQP_SOLVED)).flatten()
            if bad.numel():
                raise RuntimeError('Unable to solve QP, status: %d (batch element %d)' % (int(st[bad[0]]), int(bad[0])))
            self.last_dual = sharded.gather_rows_device(yl, nb)
            return sharded.gather_rows_device(xl, nb).to(q_val.dtype)
        x = torch.empty((nb, self.n), dtype=torch.float64, device=dev)
        y = torch.empty((nb, self.m), dtype=torch.float64, device=dev)
        rec = torch.empty((nb, 12), dtype=torch.float64, device=dev)    # OSQP_HIP_BATCH_REC
        stream = torch.cuda.current_stream(dev).cuda_stream
        try:
            s._solver.hip_batch_solve_device(nb, qd.data_ptr(), ld.data_ptr(), ud.data_ptr(), x.data_ptr(), y.data_ptr(), rec.data_ptr(),
                                             warm=False, stream=stream)
        except ValueError as e:
            if str(e) != str(int(osqp_amd.SolverError.OSQP_FUNC_NOT_IMPLEMENTED)):
                raise
            if self.large_batch not in ('lockstep', 'lockstep_direct'):
                return None                                                            # does not fit one workgroup's LDS
            entry = s._solver.hip_batch_solve_lockstep_device if self.large_batch == 'lockstep' else s._solver.hip_batch_solve_lockstep_direct_device
            entry(nb, qd.data_ptr(), ld.data_ptr(), ud.data_ptr(), x.data_ptr(), y.data_ptr(), rec.data_ptr(),
                                                      warm=False, stream=stream)
        st = rec[:, 0].to('cpu')                                                        # (waits for the stream)
        bad = torch.nonzero(st != int(osqp_amd.SolverStatus.OSQP_SOLVED)).flatten()
        if bad.numel():
            raise RuntimeError('Unable to solve QP, status: %d (batch element %d)' % (int(st[bad[0]]), int(bad[0])))
        self.last_dual = y
        return x.to(q_val.dtype)

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
        self.last_dual = y
        return x, rec

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
                raise NotImplementedError('osqp_amd.nn.torch.OSQP: backward is not available on this handle (Woodbury-corrected preconditioner; include/osqp_hip.h)')
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

    def _backward_lockstep(self, ext, l_val, u_val, x, y, g, nb, want, P_val=None, A_val=None):
        """Backward of a shared-matrix batch past the batch adjoint kernel, with large_backward='lockstep' or 'lockstep_direct': one call of the lockstep
        adjoint (or of its direct form) for the whole batch (cuda tensors: zero-copy through the device entry on torch's current stream).  An element whose adjoint system was not solved raises as
        _backward_loop does.  None: this handle is not on the route (the caller goes on to the per-element loop).
        P_val / A_val (2-D): per-element matrices -- the same one call through osqp_hip_batch_adjoint_lockstep_mat[_device] or, with 'lockstep_direct',
        osqp_hip_batch_adjoint_lockstep_direct_mat[_device]."""
        mat = P_val is not None or A_val is not None
        widths = {'dP': len(self._triu_pick), 'dq': self.n, 'dA': ext.nnz_A, 'dl': self.m, 'du': self.m}
        direct = self.large_backward == 'lockstep_direct'
        host_entry = ext.hip_batch_adjoint_lockstep_direct if direct else ext.hip_batch_adjoint_lockstep
        device_entry = ext.hip_batch_adjoint_lockstep_direct_device if direct else ext.hip_batch_adjoint_lockstep_device
        try:
            if g.is_cuda:
                dev = g.device
                f64 = lambda t, k: torch.as_tensor(t).detach().to(device=dev, dtype=torch.float64).reshape(-1, k).expand(nb, k).contiguous()
                xd, yd, gd, ld, ud = f64(x, self.n), f64(y, self.m), f64(g, self.n), f64(l_val, self.m), f64(u_val, self.m)
                res = {k: torch.empty((nb, widths[k]), dtype=torch.float64, device=dev) for k in want}
                res['rec'] = torch.empty((nb, 4), dtype=torch.float64, device=dev)     # OSQP_HIP_ADJOINT_REC
                ptr = lambda t: None if t is None else t.data_ptr()
                Pxd = None if P_val is None else f64(P_val, P_val.shape[-1])[:, torch.as_tensor(self._triu_pick, device=dev)].contiguous()
                Axd = None if A_val is None else f64(A_val, A_val.shape[-1])
                matkw = dict(Px_ptr=ptr(Pxd), Ax_ptr=ptr(Axd)) if mat else {}
                device_entry(nb, xd.data_ptr(), yd.data_ptr(), gd.data_ptr(), None, ld.data_ptr(), ud.data_ptr(),
                             ptr(res.get('dP')), ptr(res.get('dq')), ptr(res.get('dA')), ptr(res.get('dl')), ptr(res.get('du')),
                             res['rec'].data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream, **matkw)
            else:
                bc = lambda a, k: np.broadcast_to(np.asarray(a, dtype=float).reshape(-1, k), (nb, k))
                matkw = dict(Px=None if P_val is None else _np(P_val)[:, self._triu_pick], Ax=None if A_val is None else _np(A_val)) if mat else {}
                res = host_entry(bc(_np(torch.as_tensor(x)), self.n), bc(_np(torch.as_tensor(y)), self.m), bc(_np(g), self.n), None,
                                 l=bc(_np(l_val), self.m), u=bc(_np(u_val), self.m), want=want, **matkw)
                res = {k: torch.as_tensor(v) for k, v in res.items()}
        except ValueError as e:
            if str(e) != str(int(osqp_amd.SolverError.OSQP_FUNC_NOT_IMPLEMENTED)):
                raise
            return None
        self.adjoint_launches += 1
        if direct:
            self.mat_lockstep_direct_adjoint_launches += int(mat)
        else:
            self.mat_lockstep_adjoint_launches += int(mat)
        rec = res['rec'].cpu().numpy()
        bad = np.nonzero(rec[:, 0] != 0)[0]
        if bad.size:
            i = int(bad[0])
            self.last_adjoint_rec = res['rec']
            raise RuntimeError('adjoint derivatives of batch element %d: error %d (status %d, residual %.3e)'
                               % (i, int(osqp_amd.SolverError.OSQP_LINSYS_SOLVER_INIT_ERROR), int(rec[i, 0]), rec[i, 2]))
        return res

    def _backward(self, saved, x, y, dl_dx, needs):
        P_val, q_val, A_val, l_val, u_val = saved
        params = [P_val, q_val, A_val, l_val, u_val]
        batched = [p.ndimension() == 2 for p in params]
        nb = max([p.size(0) for p, b in zip(params, batched) if b], default=1)
        if _distributed()[1] > 1:
            raise NotImplementedError('osqp_amd.nn.torch.OSQP: backward in a torch.distributed job (world size > 1) is not implemented')
        if y is None:
            raise NotImplementedError('osqp_amd.nn.torch.OSQP: backward needs the duals of the forward, which this forward did not keep')
        s = self._solver
        Pn, An = _np(P_val), _np(A_val)
        # the handle's own values of a SHARED side are what the forward solved with (an intermediate forward may have replaced them)
        self._handle(self._Pv if batched[0] else Pn, self._Av if batched[2] else An, None, None, None, device=self._device)
        p_map = self._p_map(Pn.shape[-1])      # (A_val is in the CSC order of A, as the forward takes it)
        want = tuple(k for k, need in zip(('dP', 'dq', 'dA', 'dl', 'du'), needs) if need)
        g = dl_dx.detach().reshape(-1, self.n)
        if g.shape[0] != nb:
            g = g.expand(nb, self.n)
        try:
            if g.is_cuda:
                dev = g.device
                f64 = lambda t, k: torch.as_tensor(t).detach().to(device=dev, dtype=torch.float64).reshape(-1, k).expand(nb, k).contiguous()
                xd, yd, gd, ld, ud = f64(x, self.n), f64(y, self.m), f64(g, self.n), f64(l_val, self.m), f64(u_val, self.m)
                Pxd = f64(P_val, Pn.shape[-1])[:, torch.as_tensor(self._triu_pick, device=dev)].contiguous() if batched[0] else None
                Axd = f64(A_val, An.shape[-1]) if batched[2] else None
                widths = {'dP': len(self._triu_pick), 'dq': self.n, 'dA': An.shape[-1], 'dl': self.m, 'du': self.m}
                res = {k: torch.empty((nb, widths[k]), dtype=torch.float64, device=dev) for k in want}
                res['rec'] = torch.empty((nb, 4), dtype=torch.float64, device=dev)     # OSQP_HIP_ADJOINT_REC
                ptr = lambda t: None if t is None else t.data_ptr()
                s._solver.hip_batch_adjoint_device(nb, xd.data_ptr(), yd.data_ptr(), gd.data_ptr(), None, ld.data_ptr(), ud.data_ptr(), ptr(Pxd), ptr(Axd),
                                                   ptr(res.get('dP')), ptr(res.get('dq')), ptr(res.get('dA')), ptr(res.get('dl')), ptr(res.get('du')),
                                                   res['rec'].data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
            else:
                bc = lambda a, k: np.broadcast_to(np.asarray(a, dtype=float).reshape(-1, k), (nb, k))
                res = s._solver.hip_batch_adjoint(bc(_np(torch.as_tensor(x)), self.n), bc(_np(torch.as_tensor(y)), self.m), bc(_np(g), self.n), None,
                                                  l=bc(_np(l_val), self.m), u=bc(_np(u_val), self.m),
                                                  Px=Pn[:, self._triu_pick] if batched[0] else None, Ax=An if batched[2] else None, want=want)
                res = {k: torch.as_tensor(v) for k, v in res.items()}
            self.adjoint_launches += 1
        except ValueError as e:
            if str(e) != str(int(osqp_amd.SolverError.OSQP_FUNC_NOT_IMPLEMENTED)):
                raise
            res = None
            if self.large_backward in ('lockstep', 'lockstep_direct') and not batched[0] and not batched[2]:
                res = self._backward_lockstep(s._solver, l_val, u_val, x, y, g, nb, want)      # shared matrices, any size: ONE call (osqp_hip_batch_adjoint_lockstep[_direct])
            elif self.large_backward in ('lockstep', 'lockstep_direct'):                        # per-element matrices, any size: ONE call (osqp_hip_batch_adjoint_lockstep[_direct]_mat)
                res = self._backward_lockstep(s._solver, l_val, u_val, x, y, g, nb, want, P_val if batched[0] else None, A_val if batched[2] else None)
        if res is None:
            # outside the batch kernel (the forward ran _loop): the single-handle adjoint per element
            bc = lambda a, k: np.broadcast_to(np.asarray(a, dtype=float).reshape(-1, k), (nb, k))
            res = self._backward_loop(Pn, An, bc(_np(l_val), self.m), bc(_np(u_val), self.m), bc(_np(torch.as_tensor(x)), self.n), bc(_np(torch.as_tensor(y)), self.m),
                                      _np(g).reshape(nb, self.n), nb, batched, want)
        self.last_adjoint_rec = res['rec']
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
