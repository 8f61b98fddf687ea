"""'Extension module' of the hip algebra: the object surface that /root/reference/src/bindings.cpp.in gives the
reference front-end (constants, enums, CSC, OSQPSettings, OSQPInfo, OSQPSolution, OSQPSolver ...), re-authored as a
thin ctypes shim over the C ABI of libosqp_hip.so (include/osqp_hip.h).  Checklist: SURVEY.md Appendix B.
"""
import ctypes as C
from enum import IntEnum

import numpy as np
import scipy.sparse as spa

from . import _lib

OSQP_USE_FLOAT = 0          # bindings.cpp.in:327-331
OSQP_USE_LONG = 0           # bindings.cpp.in:333-337
OSQP_INFTY = 1e30           # bindings.cpp.in:340


class osqp_linsys_solver_type(IntEnum):      # bindings.cpp.in:343-346
    OSQP_DIRECT_SOLVER = 1
    OSQP_INDIRECT_SOLVER = 2


class osqp_status_type(IntEnum):             # bindings.cpp.in:349-361
    OSQP_SOLVED = 1
    OSQP_SOLVED_INACCURATE = 2
    OSQP_PRIMAL_INFEASIBLE = 3
    OSQP_PRIMAL_INFEASIBLE_INACCURATE = 4
    OSQP_DUAL_INFEASIBLE = 5
    OSQP_DUAL_INFEASIBLE_INACCURATE = 6
    OSQP_MAX_ITER_REACHED = 7
    OSQP_TIME_LIMIT_REACHED = 8
    OSQP_NON_CVX = 9
    OSQP_SIGINT = 10
    OSQP_UNSOLVED = 11


class osqp_error_type(IntEnum):              # bindings.cpp.in:364-375
    OSQP_NO_ERROR = 0
    OSQP_DATA_VALIDATION_ERROR = 1
    OSQP_SETTINGS_VALIDATION_ERROR = 2
    OSQP_LINSYS_SOLVER_INIT_ERROR = 3
    OSQP_NONCVX_ERROR = 4
    OSQP_MEM_ALLOC_ERROR = 5
    OSQP_WORKSPACE_NOT_INIT_ERROR = 6
    OSQP_ALGEBRA_LOAD_ERROR = 7
    OSQP_CODEGEN_DEFINES_ERROR = 8
    OSQP_DATA_NOT_INITIALIZED = 9
    OSQP_FUNC_NOT_IMPLEMENTED = 10


class osqp_precond_type(IntEnum):            # bindings.cpp.in:378-381
    OSQP_NO_PRECONDITIONER = 0
    OSQP_DIAGONAL_PRECONDITIONER = 1


class osqp_capabilities_type(IntEnum):       # bindings.cpp.in:395-400
    OSQP_CAPABILITY_DIRECT_SOLVER = 0x01
    OSQP_CAPABILITY_INDIRECT_SOLVER = 0x02
    OSQP_CAPABILITY_CODEGEN = 0x04
    OSQP_CAPABILITY_UPDATE_MATRICES = 0x08
    OSQP_CAPABILITY_DERIVATIVES = 0x10


# .export_values() on the first, second and fourth enum (bindings.cpp.in:346,361,381)
for _e in (osqp_linsys_solver_type, osqp_status_type, osqp_precond_type):
    globals().update(_e.__members__)


OSQP_HIP_ADJOINT_TOL = 1e-6      # include/osqp_hip.h: an adjoint residual below this is status 0


def _ptr(a, typ):
    return None if a is None else a.ctypes.data_as(typ)


def _rows(a, name, B, width):
    """`a` as (B, width) float64 in C order -- the C side reads exactly B * width entries; None stays None."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.size != B * width or (a.ndim > 1 and a.shape[-1] != width):
        raise ValueError('%s: expected %d problems of width %d, got shape %s' % (name, B, width, a.shape))
    return a.reshape(B, width)


class CSC:
    """bindings.cpp.in:12-62: zero-copy int32/f64 views of a SciPy CSC matrix."""

    def __init__(self, A):
        if not spa.isspmatrix_csc(A):
            A = spa.csc_matrix(A)
        self.m, self.n = int(A.shape[0]), int(A.shape[1])
        self.p = np.ascontiguousarray(A.indptr, dtype=np.int32)
        self.i = np.ascontiguousarray(A.indices, dtype=np.int32)
        self.x = np.ascontiguousarray(A.data, dtype=np.float64)
        self.nzmax = int(A.nnz)
        self.nz = -1

    def _struct(self):
        return _lib.CscStruct(self.m, self.n, _ptr(self.p, _lib.c_int_p), _ptr(self.i, _lib.c_int_p),
                              _ptr(self.x, _lib.c_double_p), self.nzmax, self.nz)


class OSQPSettings(_lib.SettingsStruct):
    """bindings.cpp.in:405-447.  The 29 fields are class attributes (ctypes descriptors), which is what the front-end
    enumerates to discover legal keyword settings (interface.py:318-322)."""
    pass


def osqp_set_default_settings(settings):       # bindings.cpp.in:449
    _lib.handle().osqp_set_default_settings(C.byref(settings))


def osqp_capabilities():                       # bindings.cpp.in:402
    return int(_lib.handle().osqp_capabilities())


def osqp_hip_capabilities():
    """osqp_capabilities() plus what this engine adds to the reference's list: OSQP_CAPABILITY_DERIVATIVES (the adjoint kernel)."""
    return int(_lib.handle().osqp_hip_capabilities())


def _info_property(name, typ, writable):
    def get(self):
        v = getattr(self._s.contents, name)
        return v.decode() if isinstance(v, bytes) else v

    def set_(self, v):
        setattr(self._s.contents, name, v)

    return property(get, set_ if writable else None)


class OSQPInfo:
    """bindings.cpp.in:473-492 (obj_val and dual_obj_val are read-write, :478-479)."""

    def __init__(self, struct_ptr):
        self._s = struct_ptr


for _n, _t in _lib.INFO_FIELDS:
    setattr(OSQPInfo, _n, _info_property(_n, _t, _n in ('obj_val', 'dual_obj_val')))


class OSQPSolution:
    """bindings.cpp.in:64-105: each access returns a fresh copy of the solver's host array."""

    def __init__(self, struct_ptr, m, n):
        self._s, self._m, self._n = struct_ptr, m, n

    def _arr(self, p, k):
        return np.ctypeslib.as_array(p, shape=(k,)).copy() if k > 0 else np.zeros(0)

    x = property(lambda self: self._arr(self._s.contents.x, self._n))
    y = property(lambda self: self._arr(self._s.contents.y, self._m))
    prim_inf_cert = property(lambda self: self._arr(self._s.contents.prim_inf_cert, self._m))
    dual_inf_cert = property(lambda self: self._arr(self._s.contents.dual_inf_cert, self._n))


def _vec(a, dtype=np.float64):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


class OSQPSolver:
    """bindings.cpp.in:107-323, :495-512."""

    def __init__(self, P, q, A, l, u, m, n, settings):
        self._lib = _lib.handle()
        self._p = _lib.SolverP()
        self.m, self.n = int(m), int(n)
        for a in (q, l, u):                              # .noconvert() at bindings.cpp.in:497
            if not (isinstance(a, np.ndarray) and a.dtype == np.float64):
                raise TypeError('q, l, u must be float64 numpy arrays')
        q, l, u = _vec(q), _vec(l), _vec(u)
        Ps, As = P._struct(), A._struct()
        self.nnz_P, self.nnz_A = P.nzmax, A.nzmax          # widths of hip_batch_solve's Px / Ax (P as given: its upper triangle)
        status = self._lib.osqp_setup(C.byref(self._p), C.byref(Ps), _ptr(q, _lib.c_double_p), C.byref(As),
                                      _ptr(l, _lib.c_double_p), _ptr(u, _lib.c_double_p), self.m, self.n, C.byref(settings))
        if status:
            self._p = None
            raise ValueError(str(status))                # bindings.cpp.in:153-156
        self._solution = OSQPSolution(self._p.contents.solution, self.m, self.n)
        self._info = OSQPInfo(self._p.contents.info)

    def __del__(self):
        if getattr(self, '_p', None):
            self._lib.osqp_cleanup(self._p)              # bindings.cpp.in:159-161
            self._p = None

    solution = property(lambda self: self._solution)
    info = property(lambda self: self._info)

    def get_settings(self):
        s = OSQPSettings()
        C.memmove(C.byref(s), self._p.contents.settings, C.sizeof(s))
        return s

    def solve(self):                                     # ctypes drops the GIL for the call (cf. bindings.cpp.in:196-201)
        status = self._lib.osqp_solve(self._p)
        if status:                                       # a device / allocation failure inside the solve: never a silent stale result
            raise RuntimeError('osqp_solve failed with osqp_error_type %d' % status)
        return status

    def warm_start(self, x=None, y=None):
        x, y = _vec(x), _vec(y)
        return self._lib.osqp_warm_start(self._p, _ptr(x, _lib.c_double_p), _ptr(y, _lib.c_double_p))

    def update_data_vec(self, q=None, l=None, u=None):
        q, l, u = _vec(q), _vec(l), _vec(u)
        return self._lib.osqp_update_data_vec(self._p, _ptr(q, _lib.c_double_p), _ptr(l, _lib.c_double_p), _ptr(u, _lib.c_double_p))

    def hip_update_data_vec_device(self, q_ptr=None, l_ptr=None, u_ptr=None, stream=None):
        """osqp_hip_update_data_vec_device: raw device addresses (int or None = unchanged) of UNSCALED float64 vectors on this
        solver's GPU, e.g. torch_tensor.data_ptr(); ordered after the work queued on `stream` (hipStream_t handle as int)."""
        return self._lib.osqp_hip_update_data_vec_device(self._p, q_ptr, l_ptr, u_ptr, stream)

    def hip_warm_start_device(self, x_ptr=None, y_ptr=None, stream=None):
        return self._lib.osqp_hip_warm_start_device(self._p, x_ptr, y_ptr, stream)

    def update_data_mat(self, P_x=None, P_i=None, A_x=None, A_i=None):        # bindings.cpp.in:240-281
        P_x, A_x = _vec(P_x), _vec(A_x)
        P_i, A_i = _vec(P_i, np.int32), _vec(A_i, np.int32)
        P_n = len(P_i) if P_i is not None else (len(P_x) if P_x is not None else 0)
        A_n = len(A_i) if A_i is not None else (len(A_x) if A_x is not None else 0)
        return self._lib.osqp_update_data_mat(self._p, _ptr(P_x, _lib.c_double_p), _ptr(P_i, _lib.c_int_p), P_n,
                                              _ptr(A_x, _lib.c_double_p), _ptr(A_i, _lib.c_int_p), A_n)

    def update_settings(self, settings):
        status = self._lib.osqp_update_settings(self._p, C.byref(settings))
        if status:
            raise ValueError(str(status))                # bindings.cpp.in:204-209
        return status

    def update_rho(self, rho_new):
        return self._lib.osqp_update_rho(self._p, float(rho_new))

    # ---- adjoint derivatives (bindings.cpp.in:283-319): the C call's osqp_error_type is returned, as the pybind layer does ----
    def adjoint_derivative_compute(self, dx=None, dy=None):
        dx, dy = _vec(dx), _vec(dy)
        for a, k, name in ((dx, self.n, 'dx'), (dy, self.m, 'dy')):
            if a is not None and a.size != k:
                raise ValueError('%s: expected %d entries, got %d' % (name, k, a.size))
        return self._lib.osqp_adjoint_derivative_compute(self._p, _ptr(dx, _lib.c_double_p), _ptr(dy, _lib.c_double_p))

    def adjoint_derivative_compute_at(self, x, y, dx, dy=None):
        """osqp_hip_adjoint_compute_at: the adjoint at a solution (x, y) the caller kept, with the data now on the handle; returns the error code."""
        x, y, dx, dy = _vec(x), _vec(y), _vec(dx), _vec(dy)
        for a, k, name in ((x, self.n, 'x'), (y, self.m, 'y'), (dx, self.n, 'dx'), (dy, self.m, 'dy')):
            if a is not None and a.size != k:
                raise ValueError('%s: expected %d entries, got %d' % (name, k, a.size))
        dp = _lib.c_double_p
        return self._lib.osqp_hip_adjoint_compute_at(self._p, _ptr(x, dp), _ptr(y, dp), _ptr(dx, dp), _ptr(dy, dp))

    # OSQP_HIP_ADJOINT_LAST_REC doubles of osqp_hip_adjoint_last_record
    ADJOINT_LAST_FIELDS = ('status', 'active_rows', 'residual', 'steps', 'recurrence_s', 'gradient_s', 'total_s', 'pcg_iters')

    def adjoint_last_record(self):
        """osqp_hip_adjoint_last_record as a dict (ADJOINT_LAST_FIELDS): what the last adjoint_derivative_compute of this handle found."""
        rec = np.zeros(len(self.ADJOINT_LAST_FIELDS))
        st = self._lib.osqp_hip_adjoint_last_record(self._p, _ptr(rec, _lib.c_double_p))
        if st:
            raise ValueError(str(int(st)))
        out = dict(zip(self.ADJOINT_LAST_FIELDS, rec.tolist()))
        for k in ('status', 'active_rows', 'steps', 'pcg_iters'):
            out[k] = int(out[k])
        return out

    def adjoint_derivative_get_mat(self, dP, dA):
        """dP, dA: CSC objects carrying the patterns of P's upper triangle and of A; their x arrays are filled."""
        Ps, As = dP._struct(), dA._struct()
        return self._lib.osqp_adjoint_derivative_get_mat(self._p, C.byref(Ps), C.byref(As))

    def adjoint_derivative_get_vec(self, dq, dl, du):
        for a, k in ((dq, self.n), (dl, self.m), (du, self.m)):
            if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.size == k):
                raise TypeError('dq, dl, du must be contiguous float64 numpy arrays of length n, m, m')
        return self._lib.osqp_adjoint_derivative_get_vec(self._p, _ptr(dq, _lib.c_double_p), _ptr(dl, _lib.c_double_p), _ptr(du, _lib.c_double_p))

    # ---- out of scope (codegen): the engine reports OSQP_FUNC_NOT_IMPLEMENTED ----
    def codegen(self, output_dir, file_prefix, defines):
        return self._lib.osqp_codegen(self._p, None, None, None)

    # ---- engine extensions ----
    PRECONDITIONERS = {0: 'none', 1: 'jacobi', 2: 'jacobi + woodbury (dense rows, system inverted in one workgroup\'s LDS)',
                       3: 'jacobi + woodbury (dense rows, dense system formed and inverted on the fp64 matrix cores)'}      # OSQP_HIP_PRECOND_*

    def hip_stats(self):
        s = _lib.StatsStruct()
        self._lib.osqp_hip_get_stats(self._p, C.byref(s))
        return {k: getattr(s, k) for k, _ in s._fields_}

    def hip_preconditioner(self):
        """What this handle's PCG is preconditioned with right now, in words (OSQPHipStats::preconditioner)."""
        st = self.hip_stats()
        name = self.PRECONDITIONERS[int(st['preconditioner'])]
        if int(st['preconditioner']) == 3:
            cd = int(st.get('woodbury_dual_cols', 0))
            name += (', column space (%d x %d)' % (cd, cd)) if cd else ', row space'
        return name

    def get_policy(self):
        """This handle's engine policy (include/osqp_hip.h OSQPHipPolicy) as a dict."""
        p = _lib.PolicyStruct()
        self._lib.osqp_hip_get_policy(self._p, C.byref(p))
        return {k: getattr(p, k) for k, _ in p._fields_}

    def set_policy(self, **fields):
        """Change fields of this handle's policy, e.g. set_policy(small_direct=0, rho_window=0).  [setup] fields keep their value."""
        p = _lib.PolicyStruct()
        self._lib.osqp_hip_get_policy(self._p, C.byref(p))
        for k, v in fields.items():
            if k not in dict(p._fields_):
                raise ValueError('unknown policy field %r' % k)
            setattr(p, k, v)
        st = self._lib.osqp_hip_set_policy(self._p, C.byref(p))
        if st:
            raise ValueError(str(st))

    def hip_time_kernel(self, which, reps=50):
        ms = C.c_double()
        st = self._lib.osqp_hip_time_kernel(self._p, int(which), int(reps), C.byref(ms))
        if st:
            raise ValueError(str(st))
        return ms.value

    def hip_trace_read(self, count=1024 * 16):
        buf = (C.c_ulonglong * count)()
        st = self._lib.osqp_hip_trace_read(self._p, buf, count)
        if st:
            raise ValueError(str(st))
        return np.frombuffer(buf, dtype=np.uint64).copy()

    def hip_test_spmv(self, which, vec):
        vec = _vec(vec)
        out = np.empty(self.m if which == 0 else self.n)
        self._lib.osqp_hip_test_spmv(self._p, int(which), _ptr(vec, _lib.c_double_p), _ptr(out, _lib.c_double_p))
        return out

    def hip_test_dense(self, op, C_buf, A=None, B=None, M=0, N=0, K=0, alpha=1.0, beta=0.0, a_strides=(0, 0), b_strides=(0, 0), c_strides=(0, 1), offsets=(0, 0, 0)):
        """One routine of the dense fp64 kernels on flat float64 buffers (osqp_hip_test_dense; op 0: gemm, 1: gemm_sym, 2: spd_inverse).  a_strides = (as_i, as_k),
        b_strides = (bs_k, bs_j), c_strides = (cs_i, cs_j) in elements, offsets = (a_off, b_off, c_off).  Returns (status, the C buffer after the call, minpiv)."""
        A, B = (None if a is None else np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (A, B))
        out = np.array(C_buf, dtype=np.float64).ravel()                # (a copy: the caller's canvas stays as it was)
        t = _lib.DenseTestStruct(int(op), int(M), int(N), int(K), float(alpha), float(beta), int(a_strides[0]), int(a_strides[1]), int(b_strides[0]), int(b_strides[1]),
                                 int(c_strides[0]), int(c_strides[1]), int(offsets[0]), int(offsets[1]), int(offsets[2]),
                                 0 if A is None else A.size, 0 if B is None else B.size, out.size,
                                 _ptr(A, _lib.c_double_p), _ptr(B, _lib.c_double_p), _ptr(out, _lib.c_double_p), 0.0)
        st = int(self._lib.osqp_hip_test_dense(self._p, C.byref(t)))
        return st, out, float(t.minpiv)

    def hip_test_band(self, n, bw, band, perm, rhs=None, x=None, threads=256, guard=0, pivot_floor=0.0):
        """The padded band of the batch path's direct solve on one matrix (osqp_hip_test_band): band[c (bw + 1) + k] = K[c + k][c], perm [n], rhs [nrhs, n],
        x = the canvas the solutions are written into (nrhs n + 16 doubles; default: NaN).  Every length is passed as it is: the entry validates.
        Returns (status, x canvas after the call, image, dinv, bad)."""
        band = np.ascontiguousarray(band, dtype=np.float64).ravel()
        perm = np.ascontiguousarray(perm, dtype=np.int32).ravel()
        rhs = np.zeros((0, max(int(n), 0))) if rhs is None else np.ascontiguousarray(rhs, dtype=np.float64)
        nrhs = rhs.shape[0] if rhs.ndim == 2 else 1
        rhs = rhs.ravel()
        out = np.full(nrhs * max(int(n), 0) + 16, np.nan) if x is None else np.array(x, dtype=np.float64).ravel()      # (a copy: the caller's canvas stays as it was)
        image = np.full(8 + (max(int(n), 0) + 7) // 8 * 8 * (max(int(bw), 0) + 8) + 64, np.nan)                        # band_doubles(n, bw), csrc/band_ldl.h
        dinv = np.full(max(int(n), 0), np.nan)
        t = _lib.BandTestStruct(int(n), int(bw), int(threads), int(guard), int(nrhs), float(pivot_floor), band.size, perm.size, rhs.size, out.size, image.size, dinv.size,
                                _ptr(band, _lib.c_double_p), _ptr(perm, _lib.c_int_p), _ptr(rhs, _lib.c_double_p), _ptr(out, _lib.c_double_p),
                                _ptr(image, _lib.c_double_p), _ptr(dinv, _lib.c_double_p), 0)
        st = int(self._lib.osqp_hip_test_band(self._p, C.byref(t)))
        return st, out, image, dinv, int(t.bad)

    def hip_test_woodbury(self, r, x0=None, refactor=1, parity=0, direct=0, order=None, lens=None):
        """The Woodbury correction of this handle on one right-hand side (osqp_hip_test_woodbury): optionally wb_factor, then wb_apply(parity, direct) on
        r [n] (direct: x~ starts from x0 [n]).  order: of the dense system (default: from hip_stats()).  Every output is a NaN canvas of its count + 16;
        lens = {field: length} overrides a length as it is passed (the entry validates).  Returns (status, dict) with the canvases u, xs, dinv0, S, Sinv,
        rho, idx (int32, -1) as the call left them and form, order, rows, exact, info, done, iters, gamma, rnorm."""
        n, m = self.n, self.m
        if order is None:
            s = self.hip_stats()
            order = int(s['woodbury_dual_cols']) or int(s['woodbury_rows'])
        r = np.ascontiguousarray(r, dtype=np.float64).ravel()
        x0 = np.zeros(0) if x0 is None else np.ascontiguousarray(x0, dtype=np.float64).ravel()
        cnt = dict(u=n + 16, xs=n + 16, dinv0=n + 16, S=order * order + 16, Sinv=order * order + 16, rho=m + 16)
        out = {k: np.full(v, np.nan) for k, v in cnt.items()}
        out['idx'] = np.full(order + 16, -1, dtype=np.int32)
        ln = dict(r_len=r.size, x0_len=x0.size, u_len=cnt['u'], xs_len=cnt['xs'], dinv0_len=cnt['dinv0'], s_len=cnt['S'], sinv_len=cnt['Sinv'], rho_len=cnt['rho'], idx_len=order + 16)
        ln.update(lens or {})
        t = _lib.WoodburyTestStruct(int(refactor), int(parity), int(direct), *[int(ln[k]) for k in ('r_len', 'x0_len', 'u_len', 'xs_len', 'dinv0_len', 's_len', 'sinv_len', 'rho_len', 'idx_len')],
                                    _ptr(r, _lib.c_double_p), _ptr(x0, _lib.c_double_p), *[_ptr(out[k], _lib.c_double_p) for k in ('u', 'xs', 'dinv0', 'S', 'Sinv', 'rho')],
                                    _ptr(out['idx'], _lib.c_int_p))
        st = int(self._lib.osqp_hip_test_woodbury(self._p, C.byref(t)))
        out.update(form=int(t.form), order=int(t.order), rows=int(t.rows), exact=int(t.exact), info=(int(t.info[0]), int(t.info[1])), done=int(t.done), iters=int(t.iters),
                   gamma=float(t.gamma), rnorm=float(t.rnorm))
        return st, out

    def hip_test_admm(self, x, z, y, xt, iters=1, cap=0, tol_rel=0.0, tol_abs=0.0, lens=None):
        """`iters` ADMM iterations of the PCG path from the SCALED iterates x [n], z [m], y [m], xt [n] (x~) through this handle's own launch path
        (osqp_hip_test_admm: POKE, RUN, PEEK; every PCG capped at `cap` iterations, stopped at max(tol_rel ||rhs||, tol_abs)).  lens = {field: length}
        overrides a length as it is passed (the entry validates).  Returns (status, dict): the NaN canvases x, z, y, xt, zt, dx, dy, v, t0, xg, rho, Minv
        and hist [3, cap] (gamma, alpha, beta) as the call left them, and form, f1_D, f1_mix, launches, stat_sum, stat_max, stat_unconv, stat_n,
        pcg_iters, pcg_done, tol_now, rn0.  The handle's iterates stay as the run left them."""
        n, m = self.n, self.m
        ins = [np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (x, z, y, xt)]
        size = dict(x=n, z=m, y=m, xt=n, zt=m, dx=n, dy=m, v=m, t0=m, xg=n, rho=m, Minv=n, hist=3 * max(int(cap), 0))
        out = {k: np.full(size[k], np.nan) for k in _lib.ADMM_TEST_OUT}
        ln = dict(n_len=n, m_len=m, hist_len=size['hist'])
        ln.update(lens or {})
        t = _lib.AdmmTestStruct(int(iters), int(cap), float(tol_rel), float(tol_abs), int(ln['n_len']), int(ln['m_len']), int(ln['hist_len']),
                                *[_ptr(a if a.size else None, _lib.c_double_p) for a in ins],
                                *[_ptr(out[k] if out[k].size else None, _lib.c_double_p) for k in _lib.ADMM_TEST_OUT])
        st = int(self._lib.osqp_hip_test_admm(self._p, C.byref(t)))
        out['hist'] = out['hist'].reshape(3, -1)
        out.update({k: int(getattr(t, k)) for k in ('form', 'f1_D', 'f1_mix', 'launches', 'stat_sum', 'stat_max', 'stat_unconv', 'stat_n', 'pcg_iters', 'pcg_done')})
        out.update(tol_now=float(t.tol_now), rn0=float(t.rn0))
        return st, out

    def hip_res_names(self):
        """The order of the residual block (backend.h ResId) as a list of names: 'R_PRI_U', ... (osqp_hip_res_name)."""
        names = []
        while True:
            s = self._lib.osqp_hip_res_name(len(names))
            if s is None:
                return names
            names.append(s.decode())

    def hip_test_boundary(self, x, dx, xt, z, y, dy, zt, mode=0, need=0, thr=0.0, unscaled=0, iter=0, at_check=1, chunk_done=1, status_in=0, groups=1, keep=0,
                          lens=None):
        """The chunk boundary on the SCALED vectors x, dx, xt [n] and z, y, dy, zt [m] (osqp_hip_test_boundary: POKE, RUN, PEEK).  mode 0: the residual
        pass, the second-stage kernels of the infeasibility tests for the bits of `need` (1 primal, 2 dual, with thr / unscaled), the fetch.  mode 1: the
        device-driven boundary group, `groups` times, on a state block with the caller's iter / at_check / chunk_done / status_in.  lens = {field: length}
        overrides a length as it is passed (the entry validates).  Returns (status, dict): the NaN canvases res (a dict by name: 'R_PRI_U', ...; 'res_vec'
        is the array), rho, rho_inv, v, t0, ztg, xg, xsp, Minv as the call left them, tol_rel, tol_abs, launches, form and, in mode 1, dev / host: dicts
        of the state block's fields as the device left them and as the host's rules give them."""
        n, m = self.n, self.m
        ins = [np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (x, dx, xt, z, y, dy, zt)]
        size = dict(res=_lib.RES_COUNT, rho=m, rho_inv=m, v=m, t0=m, ztg=m, xg=n, xsp=n, Minv=n)
        out = {k: np.full(size[k], np.nan) for k in _lib.BOUNDARY_TEST_OUT}
        ln = dict(n_len=n, m_len=m, res_len=_lib.RES_COUNT)
        ln.update(lens or {})
        t = _lib.BoundaryTestStruct(int(mode), int(need), int(unscaled), int(groups), int(keep), int(iter), int(at_check), int(chunk_done), int(status_in), float(thr),
                                    int(ln['n_len']), int(ln['m_len']), int(ln['res_len']),
                                    *[_ptr(a if a.size else None, _lib.c_double_p) for a in ins],
                                    *[_ptr(out[k] if out[k].size else None, _lib.c_double_p) for k in _lib.BOUNDARY_TEST_OUT])
        st = int(self._lib.osqp_hip_test_boundary(self._p, C.byref(t)))
        out['res_vec'] = out['res']
        out['res'] = dict(zip(self.hip_res_names(), out['res_vec']))
        out.update(tol_rel=float(t.tol_rel), tol_abs=float(t.tol_abs), launches=int(t.launches), form=int(t.form))
        for side in ('dev', 'host'):
            c = getattr(t, side)
            d = {k: int(getattr(c, k)) for k in _lib.BOUNDARY_CTL_INTS + ('inf_unscaled',)}
            d.update({k: float(getattr(c, k)) for k in _lib.BOUNDARY_CTL_DOUBLES})
            d['budget'] = (int(c.budget[0]), int(c.budget[1]))
            out[side] = d
        return st, out

    def hip_get_reordering(self):
        """osqp_hip_get_reordering: (perm_cols [n], perm_rows [m]) -- the caller's index of the engine's k-th variable / constraint (the identity
        unless the handle works on a permuted copy)."""
        pc, pr = np.zeros(self.n, np.int32), np.zeros(max(self.m, 1), np.int32)
        st = int(self._lib.osqp_hip_get_reordering(self._p, _ptr(pc, _lib.c_int_p), _ptr(pr, _lib.c_int_p)))
        if st:
            raise ValueError('osqp_hip_get_reordering failed: %d' % st)
        return pc, pr[:self.m]

    def hip_test_lockstep_sizes(self):
        """The sizes osqp_hip_test_lockstep reports (n, m, nnzA, nnzB, nzP, nzA, G, ws_need, mat_need and, where the direct route takes the handle, r, GC, cb,
        nv, dws_need, dmat_need), from a call that is rejected: nothing runs."""
        t = _lib.LockstepTestStruct()
        st = int(self._lib.osqp_hip_test_lockstep(self._p, C.byref(t)))
        return st, {k: int(getattr(t, k)) for k in ('n', 'm', 'nnzA', 'nnzB', 'nzP', 'nzA', 'G', 'ws_need', 'mat_need', 'r', 'GC', 'cb', 'nv', 'dws_need', 'dmat_need')}

    def hip_test_lockstep(self, ops, ws, mat_ws=None, count=64, warm=0, q=None, l=None, u=None, x=None, y=None, rec=None, Px=None, Ax=None,
                          route=0, handle=False, maps=False, view=False, lens=None):
        """Single launches of the lockstep kernels on the caller's blocks (osqp_hip_test_lockstep): ops = names of _lib.LOCKSTEP_OPS / LOCKSTEP_MORE_OPS (or raw ints), one kernel
        launch each; ws / mat_ws: the whole work / matrix block (mat_ws given: the per-problem-matrix kernels).  q, l, u, Px, Ax: (count, width) or None;
        x, y, rec: (count, width), default zeros.  route = 1: the direct route (ws / mat_ws are then that route's blocks).  handle / maps / view: also return the
        engine's CSR and scalings / assembly maps / the direct route's view of A and dense rows.  Every array is copied: the caller's
        stay as they were.  lens = {field: length} overrides a length as it is passed (the entry validates).  Returns (status, dict)."""
        _, sz = self.hip_test_lockstep_sizes()
        n, m = sz['n'], sz['m']
        mat = mat_ws is not None
        code = lambda o: _lib.LOCKSTEP_MORE_OPS[o] if o in _lib.LOCKSTEP_MORE_OPS else _lib.LOCKSTEP_OPS.index(o)
        codes = np.array([code(o) if isinstance(o, str) else int(o) for o in ops], dtype=np.int32)
        f64 = lambda a: None if a is None else np.array(a, dtype=np.float64).ravel()
        count = int(count)
        cz = max(count, 0)
        out = dict(ws=f64(ws), mat_ws=f64(mat_ws), x=np.zeros(cz * n) if x is None else f64(x), y=np.zeros(cz * m) if y is None else f64(y),
                   rec=np.zeros(cz * self.BATCH_REC) if rec is None else f64(rec))
        ins = dict(q=f64(q), l=f64(l), u=f64(u), Px=f64(Px), Ax=f64(Ax))
        size = lambda a: 0 if a is None else a.size
        ln = dict(q_len=size(ins['q']), l_len=size(ins['l']), u_len=size(ins['u']), x_len=out['x'].size, y_len=out['y'].size, rec_len=out['rec'].size,
                  px_len=size(ins['Px']), ax_len=size(ins['Ax']), ws_len=out['ws'].size, mat_len=size(out['mat_ws']))
        ln.update({k: 0 for k in _lib.LOCKSTEP_TEST_LENS if k not in ln})
        ia = {k: None for k in ('A_rowptr', 'A_col', 'B_rowptr', 'B_col', 'Pm1', 'Pm2', 'pvmap', 'AmA', 'AmB', 'avmap', 'Bdiag', 'Av_rowptr', 'Av_col', 'vsrc', 'wtpos', 'rows', 'islong')}
        da = {k: None for k in ('A_val', 'B_val', 'D', 'Dinv', 'E', 'Einv', 'Praw', 'Araw', 'Av_val', 'WT')}
        if handle:
            ln.update(arp_len=m + 1, anz_len=sz['nnzA'], brp_len=n + 1, bnz_len=sz['nnzB'], n_len=n, m_len=m)
            ia.update(A_rowptr=np.zeros(m + 1, np.int32), A_col=np.zeros(sz['nnzA'], np.int32), B_rowptr=np.zeros(n + 1, np.int32), B_col=np.zeros(sz['nnzB'], np.int32))
            da.update(A_val=np.zeros(sz['nnzA']), B_val=np.zeros(sz['nnzB']), D=np.zeros(n), Dinv=np.zeros(n), E=np.zeros(m), Einv=np.zeros(m))
        if maps:
            ln.update(pmap_len=sz['nzP'], amap_len=sz['nzA'], bdiag_len=n)
            ia.update({k: np.zeros(sz['nzP'], np.int32) for k in ('Pm1', 'Pm2', 'pvmap')}, **{k: np.zeros(sz['nzA'], np.int32) for k in ('AmA', 'AmB', 'avmap')}, Bdiag=np.zeros(n, np.int32))
            da.update(Praw=np.zeros(sz['nzP']), Araw=np.zeros(sz['nzA']))
        if view:
            nv, nr = sz['nv'], n * sz['r']
            ln.update(avrp_len=m + 1, av_len=nv, wt_len=nr, rows_len=sz['r'], islong_len=m)
            ia.update(Av_rowptr=np.zeros(m + 1, np.int32), Av_col=np.zeros(nv, np.int32), vsrc=np.zeros(nv, np.int32), wtpos=np.zeros(nr, np.int32), rows=np.zeros(sz['r'], np.int32), islong=np.zeros(m, np.int32))
            da.update(Av_val=np.zeros(nv), WT=np.zeros(nr))
        for k in [k for k, v in list(ia.items()) + list(da.items()) if v is not None and v.size == 0]:      # (an empty group is "not wanted")
            (ia if k in ia else da)[k] = None
        ln.update(lens or {})
        dp, ip = _lib.c_double_p, _lib.c_int_p
        t = _lib.LockstepTestStruct(int(route), int(mat), count, int(warm), codes.size, _ptr(codes, ip), *[int(ln[k]) for k in _lib.LOCKSTEP_TEST_LENS],
                                    _ptr(ins['q'], dp), _ptr(ins['l'], dp), _ptr(ins['u'], dp), _ptr(out['x'], dp), _ptr(out['y'], dp), _ptr(out['rec'], dp),
                                    _ptr(ins['Px'], dp), _ptr(ins['Ax'], dp), _ptr(out['ws'], dp), _ptr(out['mat_ws'], dp),
                                    *[_ptr(ia[k], ip) for k in ('A_rowptr', 'A_col', 'B_rowptr', 'B_col')], *[_ptr(da[k], dp) for k in ('A_val', 'B_val', 'D', 'Dinv', 'E', 'Einv')],
                                    *[_ptr(ia[k], ip) for k in ('Pm1', 'Pm2', 'pvmap', 'AmA', 'AmB', 'avmap', 'Bdiag')], _ptr(da['Praw'], dp), _ptr(da['Araw'], dp),
                                    *[_ptr(ia[k], ip) for k in ('Av_rowptr', 'Av_col', 'vsrc', 'wtpos', 'rows', 'islong')], _ptr(da['Av_val'], dp), _ptr(da['WT'], dp))
        st = int(self._lib.osqp_hip_test_lockstep(self._p, C.byref(t)))
        out.update(ia)
        out.update(da)
        out.update(sz, c=float(t.c), x=out['x'].reshape(cz, n), y=out['y'].reshape(cz, m), rec=out['rec'].reshape(cz, self.BATCH_REC))
        return st, out

    def hip_test_lockstep_back(self, ops, ws, mode='adjoint', mat_ws=None, pol_ws=None, count=64, route=0, secs=0.0, lens=None, **arrays):
        """Single launches of the lockstep kernels of the backward pass (mode 'adjoint') and of polish (mode 'polish') on the caller's blocks
        (osqp_hip_test_lockstep_back): ops = names of _lib.LOCKSTEP_BACK_OPS (or raw ints), one kernel launch each; ws: the whole adjoint work block, or the
        forward block with pol_ws the whole polish block; mat_ws given: the per-problem-matrix twins.  arrays: sx sy gx gy l u (in), dq dl du dP dA arec
        (adjoint, in and out), x y rec (polish), each (count, width) or None.  Every array is copied.  lens = {field: length} overrides a length as it is
        passed (the entry validates).  Returns (status, dict): the blocks, the arrays, the sizes and, after a call that ran, the scalars of the mode."""
        names = _lib.LOCKSTEP_BACK_IN + _lib.LOCKSTEP_BACK_IO
        assert set(arrays) <= set(names), arrays.keys()
        codes = np.array([_lib.LOCKSTEP_BACK_OPS.index(o) if isinstance(o, str) else int(o) for o in ops], dtype=np.int32)
        f64 = lambda a: None if a is None else np.array(a, dtype=np.float64).ravel()
        shapes = {k: np.shape(v) for k, v in arrays.items() if v is not None}
        out = {k: f64(arrays.get(k)) for k in names}
        out.update(ws=f64(ws), mat_ws=f64(mat_ws), pol_ws=f64(pol_ws))
        ln = {k: (0 if out[a] is None else out[a].size) for k, a in zip(_lib.LOCKSTEP_BACK_LENS, names)}
        ln.update(lens or {})
        dp = _lib.c_double_p
        t = _lib.LockstepBackTestStruct(int(mode == 'polish') if isinstance(mode, str) else int(mode), int(route), int(mat_ws is not None), int(count), codes.size,
                                        _ptr(codes, _lib.c_int_p), float(secs), *[int(ln[k]) for k in _lib.LOCKSTEP_BACK_LENS], *[_ptr(out[k], dp) for k in names])
        st = int(self._lib.osqp_hip_test_lockstep_back(self._p, C.byref(t)))
        for k, shp in shapes.items():
            out[k] = out[k].reshape(shp)
        out.update({k: int(getattr(t, k)) for k in _lib.LOCKSTEP_BACK_SIZES})
        out.update({k: getattr(t, k) for k in _lib.LOCKSTEP_BACK_SCALARS})
        return st, out

    def hip_set_rho_eq_factor(self, factor):
        return self._lib.osqp_hip_set_rho_eq_factor(self._p, float(factor))

    def hip_dense_kkt(self, on=True):
        """Dense KKT mode of this handle (osqp_hip_dense_kkt): on -- form and invert K = P + sigma I + A' diag(rho) A on the device and solve every ADMM
        iteration's linear system exactly by one dense product; off -- free it.  Returns the status (0, or OSQP_FUNC_NOT_IMPLEMENTED where the mode declines
        the handle, which is then left untouched)."""
        return int(self._lib.osqp_hip_dense_kkt(self._p, int(bool(on))))

    def hip_dense_kkt_record(self):
        """osqp_hip_dense_kkt_last_record as a dict (keys: _lib.DENSE_KKT_REC): state 0 off / 1 direct / 2 refused for the current rho, order,
        factorisations of the last solve and their ms, probe value and smallest pivot of the last inversion, device bytes, factorisations since enabling."""
        rec = np.zeros(len(_lib.DENSE_KKT_REC))
        st = int(self._lib.osqp_hip_dense_kkt_last_record(self._p, _ptr(rec, _lib.c_double_p)))
        if st:
            raise RuntimeError('osqp_hip_dense_kkt_last_record failed with status %d' % st)
        out = dict(zip(_lib.DENSE_KKT_REC, (float(v) for v in rec)))
        for k in ('state', 'order', 'solve_factorisations', 'factorisations'):
            out[k] = int(out[k])
        return out

    def hip_test_dense_kkt(self, op, r=None, xg=None, lens=None):
        """The dense KKT mode's kernels on this handle (osqp_hip_test_dense_kkt; SCALED problem, the ENGINE's numbering).  op 'form': K [n, n] as formed,
        before the inversion, and the rho vector [m]; 'apply': x~ = xg + K^-1 r and u = K^-1 r for r, xg [n]; 'probe': the probe value.  Outputs are NaN
        canvases of their count + 16; lens = {field: length} overrides a length as it is passed (the entry validates).  Returns (status, dict) with the
        canvases K, rho, xs, u as the call left them and state, order, done, iters, probe, minpiv."""
        n, m = self.n, self.m
        code = _lib.DENSE_KKT_OPS.index(op) if isinstance(op, str) else int(op)
        f64 = lambda a: np.zeros(0) if a is None else np.ascontiguousarray(a, dtype=np.float64).ravel()
        r, xg = f64(r), f64(xg)
        cnt = dict(K=n * n + 16 if code == 0 else 0, rho=m + 16 if code == 0 else 0, xs=n + 16 if code == 1 else 0, u=n + 16 if code == 1 else 0)
        out = {k: np.full(v, np.nan) for k, v in cnt.items()}
        ln = dict(r_len=r.size, xg_len=xg.size, k_len=cnt['K'], rho_len=cnt['rho'], xs_len=cnt['xs'], u_len=cnt['u'])
        ln.update(lens or {})
        dp = _lib.c_double_p
        t = _lib.DenseKktTestStruct(code, *[int(ln[k]) for k in ('r_len', 'xg_len', 'k_len', 'rho_len', 'xs_len', 'u_len')],
                                    _ptr(r if r.size else None, dp), _ptr(xg if xg.size else None, dp), *[_ptr(out[k] if out[k].size else None, dp) for k in ('K', 'rho', 'xs', 'u')])
        st = int(self._lib.osqp_hip_test_dense_kkt(self._p, C.byref(t)))
        out.update(state=int(t.state), order=int(t.order), done=int(t.done), iters=int(t.iters), probe=float(t.probe), minpiv=float(t.minpiv))
        return st, out

    BATCH_FIELDS = ('status_val', 'iter', 'obj_val', 'prim_res', 'dual_res', 'rho', 'rho_updates', 'pcg_iters', 'status_polish', 'polish_time', 'rho_estimate', 'duality_gap')
    BATCH_REC = len(BATCH_FIELDS)        # OSQP_HIP_BATCH_REC

    def hip_batch_solve(self, q=None, l=None, u=None, x0=None, y0=None, nbatch=None, Px=None, Ax=None):
        """Solve a batch of QPs sharing this solver's P, A and settings (osqp_hip_batch_solve).  q: (B, n), l/u: (B, m).
        Px (B, nnz(triu P)) / Ax (B, nnz(A)): per-problem matrix values in the CSC order given at setup (osqp_hip_batch_solve_mat: the reference's
        per-element P_val / A_val, nn/torch.py:128-157) -- still one launch.  Returns x (B, n), y (B, m), rec (B, BATCH_REC) with columns BATCH_FIELDS
        (duality_gap: 0 unless settings.check_dualgap, which every batch route honours per problem; dual_obj_val = obj_val - duality_gap)."""
        return self._lockstep_host(self._lib.osqp_hip_batch_solve, q, l, u, x0, y0, nbatch, Px, Ax, mat_entry=self._lib.osqp_hip_batch_solve_mat)

    def hip_batch_solve_device(self, nbatch, q_ptr, l_ptr, u_ptr, x_ptr, y_ptr, rec_ptr, warm=False, stream=None, Px_ptr=None, Ax_ptr=None):
        """osqp_hip_batch_solve_device: raw device addresses (int or None) of float64 arrays laid out as in hip_batch_solve;
        rec: (B, BATCH_REC).  Enqueued on `stream` (hipStream_t handle as int; None: the solver's stream, synchronous).
        Px_ptr / Ax_ptr: per-problem matrix values on the device (osqp_hip_batch_solve_mat_device)."""
        if Px_ptr is not None or Ax_ptr is not None:
            st = self._lib.osqp_hip_batch_solve_mat_device(self._p, int(nbatch), Px_ptr, Ax_ptr, q_ptr, l_ptr, u_ptr, x_ptr, y_ptr, rec_ptr, int(bool(warm)), stream)
        else:
            st = self._lib.osqp_hip_batch_solve_device(self._p, int(nbatch), q_ptr, l_ptr, u_ptr, x_ptr, y_ptr, rec_ptr, int(bool(warm)), stream)
        if st:
            raise self._batch_error(st)

    def hip_batch_solve_lockstep(self, q=None, l=None, u=None, x0=None, y0=None, nbatch=None, Px=None, Ax=None):
        """hip_batch_solve for problems of ANY size (osqp_hip_batch_solve_lockstep): 64 problems at a time on block vectors.
        Same arguments, same checks, same returns: x (B, n), y (B, m), rec (B, BATCH_REC).  With the setting polishing every SOLVED
        problem is polished on the device (rec[:, 8] = 1 kept, -1 rejected; lockstep_polish_last_record).
        Px (B, nnz(triu P)) / Ax (B, nnz(A)): per-problem matrix values in the CSC order given at setup (osqp_hip_batch_solve_lockstep_mat): every
        problem is scaled as a solver set up with its data alone and, with the setting polishing, polished on its own matrices as above
        (lockstep_mat_last_record: the ADMM part; lockstep_polish_last_record: polish; lockstep_mat_scaling)."""
        return self._lockstep_host(self._lib.osqp_hip_batch_solve_lockstep, q, l, u, x0, y0, nbatch, Px, Ax)

    def _lockstep_host(self, entry, q, l, u, x0, y0, nbatch, Px=None, Ax=None, mat_entry=None):
        """The host-array call of a batch solve, the one-launch route's or a lockstep route's (`entry`: its C entry point; `mat_entry`: the one that takes
        Px / Ax, the lockstep route's by default): widths checked here, then the engine."""
        arrs = [a for a in (q, l, u, x0, y0, Px, Ax) if a is not None]
        B = int(nbatch) if nbatch is not None else int(np.asarray(arrs[0]).shape[0])
        q, l, u = _rows(q, 'q', B, self.n), _rows(l, 'l', B, self.m), _rows(u, 'u', B, self.m)
        warm = x0 is not None or y0 is not None      # a missing one starts from zero, like warm_start(x=None) / (y=None) of a single solver
        # (l, u are clamped to +-OSQP_INFTY inside the kernel, like interface.py:334-337)
        x = np.zeros((B, self.n)) if x0 is None else _rows(x0, 'x0', B, self.n).copy()
        y = np.zeros((B, self.m)) if y0 is None else _rows(y0, 'y0', B, self.m).copy()
        rec = np.zeros((B, self.BATCH_REC))
        dp = _lib.c_double_p
        args = (_ptr(q, dp), _ptr(l, dp), _ptr(u, dp), _ptr(x, dp), _ptr(y, dp), _ptr(rec, dp), int(warm))
        if Px is not None or Ax is not None:
            Px, Ax = _rows(Px, 'Px', B, self.nnz_P), _rows(Ax, 'Ax', B, self.nnz_A)
            st = (mat_entry or self._lib.osqp_hip_batch_solve_lockstep_mat)(self._p, B, _ptr(Px, dp), _ptr(Ax, dp), *args)
        else:
            st = entry(self._p, B, *args)
        if st:
            raise self._batch_error(st)
        return x, y, rec

    def _device_call(self, stem, nbatch, Px_ptr, Ax_ptr, *args):
        """The device-array call of a lockstep route: `<stem>_mat_device` when a matrix pointer is given, `<stem>_device` otherwise."""
        if Px_ptr is not None or Ax_ptr is not None:
            st = getattr(self._lib, stem + '_mat_device')(self._p, int(nbatch), Px_ptr, Ax_ptr, *args)
        else:
            st = getattr(self._lib, stem + '_device')(self._p, int(nbatch), *args)
        if st:
            raise self._batch_error(st)

    def _last_record(self, entry_name, fields):
        """One of the engine's *_last_record entries as a dict over `fields`: counts as int, timings and the reserved slot as float."""
        rec = np.zeros(len(fields))
        st = getattr(self._lib, entry_name)(self._p, _ptr(rec, _lib.c_double_p))
        if st:
            raise ValueError(str(int(st)))
        return {k: v if k in ('gpu_ms', 'seconds', 'prepare_gpu_ms', 'reserved') else int(v) for k, v in zip(fields, rec.tolist())}

    def hip_batch_solve_lockstep_device(self, nbatch, q_ptr, l_ptr, u_ptr, x_ptr, y_ptr, rec_ptr, warm=False, stream=None, Px_ptr=None, Ax_ptr=None):
        """osqp_hip_batch_solve_lockstep_device: raw device addresses (int or None) laid out as in hip_batch_solve_lockstep; the work goes on `stream`
        (None: the solver's) and the call returns when the results are there.  nbatch == 0: does the route apply?
        Px_ptr / Ax_ptr: per-problem matrix values on the device (osqp_hip_batch_solve_lockstep_mat_device)."""
        self._device_call('osqp_hip_batch_solve_lockstep', nbatch, Px_ptr, Ax_ptr, q_ptr, l_ptr, u_ptr, x_ptr, y_ptr, rec_ptr, int(bool(warm)), stream)

    # OSQP_HIP_LOCKSTEP_MAT_LAST_REC doubles of osqp_hip_lockstep_mat_last_record
    LOCKSTEP_MAT_LAST_FIELDS = ('chunks', 'width', 'admm_iters_max', 'pcg_iters', 'kernel_launches', 'gpu_ms', 'matrix_block_bytes', 'prepare_gpu_ms')

    def lockstep_mat_last_record(self):
        """osqp_hip_lockstep_mat_last_record as a dict (LOCKSTEP_MAT_LAST_FIELDS): what the last lockstep call with per-problem matrices of this handle
        did; zeros before the first."""
        return self._last_record('osqp_hip_lockstep_mat_last_record', self.LOCKSTEP_MAT_LAST_FIELDS)

    def lockstep_mat_scaling(self, b):
        """osqp_hip_lockstep_mat_scaling: (D, E, c) of problem b of the last chunk the last lockstep call with per-problem matrices processed, numbered
        like hip_scaling().  ValueError with code OSQP_DATA_NOT_INITIALIZED before the first call or for b outside that chunk."""
        D, E, c = np.zeros(self.n), np.zeros(self.m), C.c_double()
        st = self._lib.osqp_hip_lockstep_mat_scaling(self._p, int(b), _ptr(D, _lib.c_double_p), _ptr(E, _lib.c_double_p), C.byref(c))
        if st:
            raise self._batch_error(st)
        return D, E, c.value

    # OSQP_HIP_LOCKSTEP_LAST_REC doubles of osqp_hip_lockstep_last_record
    LOCKSTEP_LAST_FIELDS = ('chunks', 'width', 'admm_iters_max', 'pcg_iters', 'kernel_launches', 'gpu_ms', 'workspace_bytes', 'reserved')

    def lockstep_last_record(self):
        """osqp_hip_lockstep_last_record as a dict (LOCKSTEP_LAST_FIELDS): what the last lockstep call of this handle did; zeros before the first."""
        return self._last_record('osqp_hip_lockstep_last_record', self.LOCKSTEP_LAST_FIELDS)

    # OSQP_HIP_LOCKSTEP_POLISH_LAST_REC doubles of osqp_hip_lockstep_polish_last_record
    LOCKSTEP_POLISH_LAST_FIELDS = ('attempted', 'accepted', 'rejected', 'steps_max', 'pcg_iters', 'kernel_launches', 'gpu_ms', 'workspace_bytes')

    def lockstep_polish_last_record(self):
        """osqp_hip_lockstep_polish_last_record as a dict (LOCKSTEP_POLISH_LAST_FIELDS): the polish part of the last lockstep call of this handle
        (settings.polishing) -- hip_batch_solve_lockstep, or hip_batch_solve_lockstep_direct on a polishing handle (pcg_iters is 0 there); zeros before the
        first call and after a call without polishing (a direct call on a handle that never polished leaves it as it was)."""
        return self._last_record('osqp_hip_lockstep_polish_last_record', self.LOCKSTEP_POLISH_LAST_FIELDS)

    def hip_batch_solve_lockstep_direct(self, q=None, l=None, u=None, x0=None, y0=None, nbatch=None, Px=None, Ax=None):
        """hip_batch_solve_lockstep for the handles it declines (osqp_hip_batch_solve_lockstep_direct): a Woodbury-corrected handle in the small mode
        whose K0 is diagonal (the factor-model portfolio QP) -- the Woodbury formula per problem in place of the PCG.  Same arguments, checks and
        returns; every other handle raises with OSQP_FUNC_NOT_IMPLEMENTED.
        Px (B, nnz(triu P)) / Ax (B, nnz(A)): per-problem matrix values in the CSC order given at setup (osqp_hip_batch_solve_lockstep_direct_mat); either
        alone is allowed, the other side takes the handle's current values.  Every problem is scaled and solved as a solver set up with its data alone
        (lockstep_direct_mat_last_record).
        settings.polishing: every problem that ends OSQP_SOLVED is polished (record columns 8 and 9: status_polish 1 / -1, the chunk's polish seconds), on
        its own matrices where Px / Ax are given; lockstep_polish_last_record has the polish part of the call, lockstep_direct_last_record the ADMM part."""
        return self._lockstep_host(self._lib.osqp_hip_batch_solve_lockstep_direct, q, l, u, x0, y0, nbatch, Px, Ax, mat_entry=self._lib.osqp_hip_batch_solve_lockstep_direct_mat)

    def hip_batch_solve_lockstep_direct_device(self, nbatch, q_ptr, l_ptr, u_ptr, x_ptr, y_ptr, rec_ptr, warm=False, stream=None, Px_ptr=None, Ax_ptr=None):
        """osqp_hip_batch_solve_lockstep_direct_device: raw device addresses (int or None) laid out as in hip_batch_solve_lockstep; the work goes on
        `stream` (None: the solver's) and the call returns when the results are there.  nbatch == 0: does the route apply?
        Px_ptr / Ax_ptr: per-problem matrix values on the device (osqp_hip_batch_solve_lockstep_direct_mat_device)."""
        self._device_call('osqp_hip_batch_solve_lockstep_direct', nbatch, Px_ptr, Ax_ptr, q_ptr, l_ptr, u_ptr, x_ptr, y_ptr, rec_ptr, int(bool(warm)), stream)

    # OSQP_HIP_LOCKSTEP_DIRECT_MAT_LAST_REC doubles of osqp_hip_lockstep_direct_mat_last_record
    LOCKSTEP_DIRECT_MAT_LAST_FIELDS = ('chunks', 'width', 'admm_iters_max', 'factorisations', 'kernel_launches', 'gpu_ms', 'matrix_block_bytes', 'prepare_gpu_ms')

    def lockstep_direct_mat_last_record(self):
        """osqp_hip_lockstep_direct_mat_last_record as a dict (LOCKSTEP_DIRECT_MAT_LAST_FIELDS): what the last direct lockstep call with per-problem
        matrices of this handle did; zeros before the first."""
        return self._last_record('osqp_hip_lockstep_direct_mat_last_record', self.LOCKSTEP_DIRECT_MAT_LAST_FIELDS)

    # OSQP_HIP_LOCKSTEP_DIRECT_LAST_REC doubles of osqp_hip_lockstep_direct_last_record
    LOCKSTEP_DIRECT_LAST_FIELDS = ('chunks', 'width', 'admm_iters_max', 'factorisations', 'kernel_launches', 'gpu_ms', 'workspace_bytes', 'seconds')

    def lockstep_direct_last_record(self):
        """osqp_hip_lockstep_direct_last_record as a dict (LOCKSTEP_DIRECT_LAST_FIELDS): what the last direct lockstep call of this handle did; zeros
        before the first."""
        return self._last_record('osqp_hip_lockstep_direct_last_record', self.LOCKSTEP_DIRECT_LAST_FIELDS)

    ADJOINT_FIELDS = ('status', 'active_rows', 'residual', 'reserved')
    ADJOINT_REC = len(ADJOINT_FIELDS)    # OSQP_HIP_ADJOINT_REC
    ADJOINT_TOL = 1e-6                   # OSQP_HIP_ADJOINT_TOL

    def hip_batch_adjoint(self, x, y, dx, dy=None, l=None, u=None, Px=None, Ax=None, want=('dP', 'dq', 'dA', 'dl', 'du')):
        """Adjoint derivatives of a batch of solved QPs (osqp_hip_batch_adjoint: one launch).  x, dx: (B, n); y, dy: (B, m), dy None = 0;
        l / u (B, m), Px (B, nnz(triu P)), Ax (B, nnz(A)): what the batch was solved with, None = this solver's own values.
        Returns a dict with the arrays named in `want` -- dP (B, nnz(triu P)) and dA (B, nnz(A)) in the CSC order given at setup, dq (B, n),
        dl, du (B, m) -- and 'rec' (B, ADJOINT_REC) with columns ADJOINT_FIELDS."""
        return self._adjoint_host(self._lib.osqp_hip_batch_adjoint, x, y, dx, dy, l, u, want, Px, Ax, always_mat=True)

    def hip_batch_adjoint_device(self, nbatch, x_ptr, y_ptr, dx_ptr, dy_ptr=None, l_ptr=None, u_ptr=None, Px_ptr=None, Ax_ptr=None,
                                 dP_ptr=None, dq_ptr=None, dA_ptr=None, dl_ptr=None, du_ptr=None, rec_ptr=None, stream=None):
        """osqp_hip_batch_adjoint_device: raw device addresses (int or None) of float64 arrays laid out as in hip_batch_adjoint; enqueued on `stream`
        (hipStream_t handle as int; None: the solver's stream, synchronous).  nbatch == 0 only asks whether the problem fits."""
        st = self._lib.osqp_hip_batch_adjoint_device(self._p, int(nbatch), Px_ptr, Ax_ptr, l_ptr, u_ptr, x_ptr, y_ptr, dx_ptr, dy_ptr,
                                                     dP_ptr, dq_ptr, dA_ptr, dl_ptr, du_ptr, rec_ptr, stream)
        if st:
            raise self._batch_error(st)

    LOCKSTEP_ADJOINT_FIELDS = ('status', 'active_rows', 'residual', 'steps')      # the OSQP_HIP_ADJOINT_REC doubles per problem on the lockstep route

    def hip_batch_adjoint_lockstep(self, x, y, dx, dy=None, l=None, u=None, want=('dP', 'dq', 'dA', 'dl', 'du'), Px=None, Ax=None):
        """hip_batch_adjoint for problems of ANY size (osqp_hip_batch_adjoint_lockstep): shared P / A, 64 problems at a time on block vectors, every
        adjoint system by the recurrence of the single-handle PCG route.  Same arguments, same checks, same returns; the columns of 'rec' are
        LOCKSTEP_ADJOINT_FIELDS.
        Px (B, nnz(triu P)) / Ax (B, nnz(A)): per-problem matrix values in the CSC order given at setup (osqp_hip_batch_adjoint_lockstep_mat): every
        problem's adjoint system on its own matrices and scaling -- the backward of hip_batch_solve_lockstep(Px=, Ax=) (lockstep_mat_adjoint_last_record)."""
        return self._adjoint_host(self._lib.osqp_hip_batch_adjoint_lockstep, x, y, dx, dy, l, u, want, Px, Ax)

    def _adjoint_host(self, entry, x, y, dx, dy, l, u, want, Px=None, Ax=None, mat_entry=None, always_mat=False):
        """The host-array call of a batch adjoint, the one-launch route's or a lockstep route's (`entry`: its C entry point; `mat_entry`: the one with
        per-problem matrices, None: the PCG route's; `always_mat`: `entry` itself takes Px / Ax, given or not): widths checked here, then the engine."""
        if x is None or y is None or dx is None:
            raise ValueError('x, y and dx are required')
        x = np.ascontiguousarray(x, dtype=np.float64)
        B = 1 if x.ndim == 1 else int(x.shape[0])
        x, y, dx, dy, l, u = (_rows(a, nm, B, w) for a, nm, w in ((x, 'x', self.n), (y, 'y', self.m), (dx, 'dx', self.n), (dy, 'dy', self.m), (l, 'l', self.m), (u, 'u', self.m)))
        widths = {'dP': self.nnz_P, 'dq': self.n, 'dA': self.nnz_A, 'dl': self.m, 'du': self.m}
        out = {k: (np.zeros((B, widths[k])) if k in want else None) for k in widths}
        rec = np.zeros((B, self.ADJOINT_REC))
        dp = _lib.c_double_p
        outs = (_ptr(out['dP'], dp), _ptr(out['dq'], dp), _ptr(out['dA'], dp), _ptr(out['dl'], dp), _ptr(out['du'], dp), _ptr(rec, dp))
        if always_mat or Px is not None or Ax is not None:
            Px, Ax = _rows(Px, 'Px', B, self.nnz_P), _rows(Ax, 'Ax', B, self.nnz_A)
            st = (entry if always_mat else mat_entry or self._lib.osqp_hip_batch_adjoint_lockstep_mat)(self._p, B, _ptr(Px, dp), _ptr(Ax, dp), _ptr(l, dp), _ptr(u, dp), _ptr(x, dp), _ptr(y, dp),
                                                                              _ptr(dx, dp), _ptr(dy, dp), *outs)
        else:
            st = entry(self._p, B, _ptr(l, dp), _ptr(u, dp), _ptr(x, dp), _ptr(y, dp), _ptr(dx, dp), _ptr(dy, dp), *outs)
        if st:
            raise self._batch_error(st)
        res = {k: v for k, v in out.items() if v is not None}
        res['rec'] = rec
        return res

    def hip_batch_adjoint_lockstep_device(self, nbatch, x_ptr, y_ptr, dx_ptr, dy_ptr=None, l_ptr=None, u_ptr=None,
                                          dP_ptr=None, dq_ptr=None, dA_ptr=None, dl_ptr=None, du_ptr=None, rec_ptr=None, stream=None, Px_ptr=None, Ax_ptr=None):
        """osqp_hip_batch_adjoint_lockstep_device: raw device addresses (int or None) laid out as in hip_batch_adjoint_lockstep; the work goes on `stream`
        (None: the solver's) and the call returns when the results are there.  nbatch == 0: does the route apply?
        Px_ptr / Ax_ptr: per-problem matrix values on the device (osqp_hip_batch_adjoint_lockstep_mat_device)."""
        self._device_call('osqp_hip_batch_adjoint_lockstep', nbatch, Px_ptr, Ax_ptr, l_ptr, u_ptr, x_ptr, y_ptr, dx_ptr, dy_ptr, dP_ptr, dq_ptr, dA_ptr, dl_ptr, du_ptr, rec_ptr, stream)

    # OSQP_HIP_LOCKSTEP_MAT_ADJOINT_LAST_REC doubles of osqp_hip_lockstep_mat_adjoint_last_record
    LOCKSTEP_MAT_ADJOINT_LAST_FIELDS = ('chunks', 'width', 'steps_max', 'pcg_iters', 'kernel_launches', 'gpu_ms', 'matrix_block_bytes', 'prepare_gpu_ms')

    def lockstep_mat_adjoint_last_record(self):
        """osqp_hip_lockstep_mat_adjoint_last_record as a dict (LOCKSTEP_MAT_ADJOINT_LAST_FIELDS): what the last lockstep adjoint call with per-problem
        matrices of this handle did; zeros before the first."""
        return self._last_record('osqp_hip_lockstep_mat_adjoint_last_record', self.LOCKSTEP_MAT_ADJOINT_LAST_FIELDS)

    # OSQP_HIP_LOCKSTEP_ADJOINT_LAST_REC doubles of osqp_hip_lockstep_adjoint_last_record
    LOCKSTEP_ADJOINT_LAST_FIELDS = ('chunks', 'width', 'steps_max', 'pcg_iters', 'kernel_launches', 'gpu_ms', 'workspace_bytes', 'reserved')

    def lockstep_adjoint_last_record(self):
        """osqp_hip_lockstep_adjoint_last_record as a dict (LOCKSTEP_ADJOINT_LAST_FIELDS): what the last lockstep adjoint call of this handle did; zeros before the first."""
        return self._last_record('osqp_hip_lockstep_adjoint_last_record', self.LOCKSTEP_ADJOINT_LAST_FIELDS)

    def hip_batch_adjoint_lockstep_direct(self, x, y, dx, dy=None, l=None, u=None, want=('dP', 'dq', 'dA', 'dl', 'du'), Px=None, Ax=None):
        """hip_batch_adjoint_lockstep for the handles it declines (osqp_hip_batch_adjoint_lockstep_direct): the backward pass of
        hip_batch_solve_lockstep_direct, on the handles that call accepts -- the recurrence's linear solve is the Woodbury formula per problem, S inverted
        once.  Same arguments, same checks, same returns; every other handle raises ValueError with OSQP_FUNC_NOT_IMPLEMENTED.
        Px (B, nnz(triu P)) / Ax (B, nnz(A)): per-problem matrix values in the CSC order given at setup (osqp_hip_batch_adjoint_lockstep_direct_mat): every
        problem's adjoint system on its own matrices, dense rows and scaling -- the backward of hip_batch_solve_lockstep_direct(Px=, Ax=)
        (lockstep_direct_mat_adjoint_last_record)."""
        return self._adjoint_host(self._lib.osqp_hip_batch_adjoint_lockstep_direct, x, y, dx, dy, l, u, want, Px, Ax,
                                  mat_entry=self._lib.osqp_hip_batch_adjoint_lockstep_direct_mat)

    def hip_batch_adjoint_lockstep_direct_device(self, nbatch, x_ptr, y_ptr, dx_ptr, dy_ptr=None, l_ptr=None, u_ptr=None,
                                                 dP_ptr=None, dq_ptr=None, dA_ptr=None, dl_ptr=None, du_ptr=None, rec_ptr=None, stream=None, Px_ptr=None, Ax_ptr=None):
        """osqp_hip_batch_adjoint_lockstep_direct_device: raw device addresses (int or None) laid out as in hip_batch_adjoint_lockstep; the work goes on
        `stream` (None: the solver's) and the call returns when the results are there.  nbatch == 0: does the route apply?
        Px_ptr / Ax_ptr: per-problem matrix values on the device (osqp_hip_batch_adjoint_lockstep_direct_mat_device)."""
        self._device_call('osqp_hip_batch_adjoint_lockstep_direct', nbatch, Px_ptr, Ax_ptr, l_ptr, u_ptr, x_ptr, y_ptr, dx_ptr, dy_ptr, dP_ptr, dq_ptr, dA_ptr, dl_ptr, du_ptr, rec_ptr, stream)

    # OSQP_HIP_LOCKSTEP_DIRECT_MAT_ADJOINT_LAST_REC doubles of osqp_hip_lockstep_direct_mat_adjoint_last_record
    LOCKSTEP_DIRECT_MAT_ADJOINT_LAST_FIELDS = ('chunks', 'width', 'steps_max', 'inversions', 'kernel_launches', 'gpu_ms', 'matrix_block_bytes', 'prepare_gpu_ms')

    def lockstep_direct_mat_adjoint_last_record(self):
        """osqp_hip_lockstep_direct_mat_adjoint_last_record as a dict (LOCKSTEP_DIRECT_MAT_ADJOINT_LAST_FIELDS): what the last direct lockstep adjoint
        call with per-problem matrices of this handle did; zeros before the first."""
        return self._last_record('osqp_hip_lockstep_direct_mat_adjoint_last_record', self.LOCKSTEP_DIRECT_MAT_ADJOINT_LAST_FIELDS)

    # OSQP_HIP_LOCKSTEP_DIRECT_ADJOINT_LAST_REC doubles of osqp_hip_lockstep_direct_adjoint_last_record
    LOCKSTEP_DIRECT_ADJOINT_LAST_FIELDS = ('chunks', 'width', 'steps_max', 'inversions', 'kernel_launches', 'gpu_ms', 'workspace_bytes', 'reserved')

    def lockstep_direct_adjoint_last_record(self):
        """osqp_hip_lockstep_direct_adjoint_last_record as a dict (LOCKSTEP_DIRECT_ADJOINT_LAST_FIELDS): what the last direct lockstep adjoint call of this
        handle did; zeros before the first."""
        return self._last_record('osqp_hip_lockstep_direct_adjoint_last_record', self.LOCKSTEP_DIRECT_ADJOINT_LAST_FIELDS)

    def _batch_error(self, st):
        """ValueError(str(code)) as the pybind layer raises for a failed call (callers compare str(e) with the code); `.reason` says why
        the batch kernel declined: OSQP_FUNC_NOT_IMPLEMENTED = the QP does not fit one workgroup's LDS, or this handle works on a
        reordered copy of the problem (OSQPHipPolicy::reorder = 2; the automatic mode never reorders a problem the batch kernel takes)."""
        e = ValueError(str(st))
        e.code = int(st)
        e.reason = ('the handle works on a reordered copy of the problem (OSQPHipPolicy::reorder): the batch kernel takes the caller\'s numbering only'
                    if self.hip_stats().get('reordered') else 'the batch kernel declined (code %d): the QP does not fit one workgroup\'s LDS, or an argument is invalid' % int(st))
        return e

    def hip_scaling(self):
        D, E, c = np.empty(self.n), np.empty(self.m), C.c_double()
        self._lib.osqp_hip_get_scaling(self._p, _ptr(D, _lib.c_double_p), _ptr(E, _lib.c_double_p), C.byref(c))
        return D, E, c.value
