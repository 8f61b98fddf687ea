"""Kernel-level references of the lockstep kernels of the BACKWARD PASS and of POLISH (osqp-python_amd/csrc/lockstep_hip.hip "adjoint derivatives of a chunk",
"polish of a chunk", k_lwa_setl / k_lwa_zero), ONE LAUNCH AT A TIME: every op of the diagnostic entry osqp_hip_test_lockstep_back has a reference here that maps
the uploaded blocks, the caller's arrays and the handle's arrays to the expected blocks and arrays.  The machinery is tests/lockstep_ref.py's -- Layout, Blk,
poke, Handle, Ref's helpers, spmm, strips, put, nanmax_reduce, compare (THE BOUND: err <= 64 max(e64, k 2^-53) scale per lane and output vector) and the
Standin's row passes, tiles and folds -- imported, not copied.  Nothing runs a recurrence: every case is one launch from a poked state.

WHERE THINGS SIT comes from the carve log (tests/hostsim/policy_probe.cpp): the adjoint block is the forward's followed by lockstep_carve_adjoint's
  ADJV   ax gdx rx | ay gdy ry | code (m x 64 int32, packed)
and the polish block, lockstep_carve_polish's  POLV  x | y z l u, is appended to the forward block HERE (names sx sy sz sl su, BackLayout.split: where the
caller cuts the two apart), so that "every other double is bit-unchanged" covers it with the same text.

The elementwise rules are restated from their headers: step_rules.h adjoint_active, polish_active, normal_cone, in_x, in_q, clamp_lower, clamp_upper;
term_rules.h recurrence_err_rhs, recurrence_err_polish, recurrence_ends, term_info, polish_accept, term_dual_obj, batch_record_gap.  The DECISIONS (a row's
code, the end of a recurrence, accept / reject, status 0 / 3) are comparisons of stored values, of max-folds of stored values, or of ONE correctly rounded
product / quotient of them: the references evaluate them in fp64, as the kernels do, and every int they produce is compared exactly.
The scalars of the recurrences (gain, min_steps, max_steps, rho0, pol_rho, pol_min_steps, pol_max_steps, adjoint_tol, check_dualgap) are not restated:
they come out of the entry (Params.from_entry); the CPU tier passes a Params of its own to the stand-in and the references alike.

EXACT (bit comparisons): every int (code, iw rows, words), copies and transposes (ax gdx ay gdy, out_n, out_m, polish's save and restore), the lanes and rows
an op must not touch, every other double and int of all blocks, every caller array the op does not write."""
import numpy as np

import lockstep_ref as R
from lockstep_ref import W, LD, INFTY, SC, IW, WD, PS_M0, PS_N0, KREC

ADJV = ('ax', 'gdx', 'rx', 'ay', 'gdy', 'ry', 'code')
POLV = ('sx', 'sy', 'sz', 'sl', 'su')
AS_ACT, AS_RM, AS_GM, AS_RN, AS_GN = R.PS_BN, PS_M0, PS_M0 + 1, PS_M0 + 2, PS_M0 + 3      # enum LsAdjSlot
PS_SUPP = R.PS_PKP
SOLVED = 1
ADJ_REC = 4                                                  # kAdjointRec
ADJ_OPS = ('adj_load_n', 'adj_load_m', 'adj_class', 'adj_init', 'adj_decide', 'adj_unscale', 'adj_resm', 'adj_resn', 'adj_final', 'adj_out_n', 'adj_out_m',
           'adj_grad_p', 'adj_grad_a')
LWA_OPS = ('lwa_setl_x', 'lwa_setl_xs', 'lwa_zero')
POL_OPS = ('pol_begin', 'pol_class', 'pol_decide', 'pol_cone', 'pol_accept', 'pol_end')
BACK_OPS = ADJ_OPS + LWA_OPS + POL_OPS
M_SIDE = ('adj_load_m', 'adj_class', 'adj_resm', 'adj_out_m', 'adj_grad_a', 'pol_cone')
ADJ_IO = ('dq', 'dl', 'du', 'dP', 'dA', 'arec')
POL_IO = ('x', 'y', 'rec')


class Params:
    """the scalars the entry reports (include/osqp_hip.h OSQPHipLockstepBackTest, out) and the settings the accept test reads"""
    def __init__(self, **kw):
        self.__dict__.update(dict(gain=0.9, min_steps=4, max_steps=60, rho0=1e6, pol_rho=1e6, pol_min_steps=4, pol_max_steps=30, adjoint_tol=1e-6, check_dualgap=0,
                                  eps_abs=1e-8, eps_rel=1e-8, secs=0.125), **kw)

    @staticmethod
    def from_entry(out, settings, secs=0.125):
        return Params(**{k: out[k] for k in ('gain', 'min_steps', 'max_steps', 'rho0', 'pol_rho', 'pol_min_steps', 'pol_max_steps', 'adjoint_tol', 'check_dualgap')},
                      eps_abs=settings.eps_abs, eps_rel=settings.eps_rel, secs=secs)


def back_handle(H, P, A, l, u):
    """what the backward references need besides lockstep_ref.Handle: the handle's own bounds in the engine's numbering and, for the gradients, the (row, column)
    of every stored entry of the caller's triu(P) and A -- the CALLER's CSC order, mapped to the engine's numbering through the permutations alone (the
    engine's own entry maps Pi / Pj / Pmap, Ai / Aj / Amap are what the kernel reads and what this checks)"""
    import scipy.sparse as sp
    ipc, ipr = np.empty(H.n, int), np.empty(H.m, int)
    ipc[H.pc] = np.arange(H.n); ipr[H.pr] = np.arange(H.m)
    Pu = sp.triu(P, format='csc'); Pu.sort_indices()
    Ac = sp.csc_matrix(A); Ac.sort_indices()
    H.l0, H.u0 = np.asarray(l, float)[H.pr], np.asarray(u, float)[H.pr]
    H.Pe = (ipc[Pu.indices], ipc[np.repeat(np.arange(H.n), np.diff(Pu.indptr))])
    H.Ae = (ipr[Ac.indices], ipc[np.repeat(np.arange(H.n), np.diff(Ac.indptr))])
    return H


class BackLayout(R.Layout):
    """lockstep_ref.Layout of the same handle with the adjoint's vectors (mode 'adjoint': the block lockstep_layout / lockstep_direct_layout carve with a != NULL)
    or the polish block behind the forward block (mode 'polish')"""
    def __init__(self, lay, mode):
        R.Layout.__init__(self, lay.n, lay.m, lay.nnzA, lay.nnzB, lay.r, lay.nv)
        import ctypes as C
        L = R.layout_lib()
        n, m, r = self.n, self.m, self.r
        cap = L.ll_const(6)
        ranges, info = (C.c_size_t * (2 * cap))(), (C.c_size_t * 3)()
        self.mode, self.split = mode, self.ws_doubles
        fwd = dict(self.fwd)
        if mode == 'adjoint':
            which = 3 if r else 1
            k = L.ll_carve(which, None, n, m, r, self.nnzA, self.nnzB, ranges, info)
            got = [(int(ranges[2 * q]), int(ranges[2 * q + 1])) for q in range(k)]
            assert info[1] and k == len(fwd) + len(ADJV) and got[:len(fwd)] == list(fwd.values())
            fwd.update(zip(ADJV, got[len(self.fwd):]))
            assert fwd['ax'][0] == self.ws_doubles and fwd['code'][1] == (m * W + 1) // 2
            self.ws_doubles = int(L.ll_size(which, n, m, r, self.nnzA, self.nnzB))
        else:
            k = L.ll_carve(4, None, n, m, 0, self.nnzA, self.nnzB, ranges, info)
            assert info[1] and k == len(POLV)
            fwd.update({nm: (self.split + int(ranges[2 * q]), int(ranges[2 * q + 1])) for q, nm in enumerate(POLV)})
            self.pol_doubles = int(L.ll_size(4, n, m, 0, self.nnzA, self.nnzB))
            self.ws_doubles = self.split + self.pol_doubles
        self.fwd = fwd


class BBlk(R.Blk):
    def copy(self):
        return BBlk(self.lay, self.ws.copy(), None if self.mat is None else self.mat.copy())

    def v(self, name):
        if name == 'code':
            o, c = self.lay.fwd['code']
            return self.ws[o:o + c].view(np.int32)[:self.lay.m * W].reshape(self.lay.m, W)
        return R.Blk.v(self, name)

    def get(self, key):
        if isinstance(key, tuple) and key[0] == 'reccol':
            return self.v('rec')[:, key[1]]
        return R.Blk.get(self, key)


def bpoke(lay, seed, mat, count=W, frozen=(), pol=None, bdiag=None):
    """lockstep_ref.poke over the longer block, then what the backward / polish kernels need of it: codes 0 / 1 / 2, non-negative max-type partials, integer
    counts of active rows, a positive best error; polish: IW_POL 0 / 1 / 2 by lane (pol: {lane: value}, default lane % 3), the lanes >= count unsolved and
    not attempted, ordered saved bounds."""
    b0 = R.poke(lay, seed, mat, count=count, frozen=frozen, wide=True, bdiag=bdiag)
    b = BBlk(lay, b0.ws, b0.mat)
    rng = np.random.default_rng(seed + 1000)
    b.v('part')[PS_M0:] = np.abs(b.v('part')[PS_M0:])
    b.v('sc')[SC['BEST']] = np.abs(b.v('sc')[SC['BEST']]) + 1e-3
    iw, lanes = b.v('iw'), np.arange(W)
    if lay.mode == 'adjoint':
        b.v('code')[:] = rng.integers(0, 3, size=(lay.m, W))
        b.v('part')[AS_ACT] = rng.integers(0, 3, size=(lay.G, W))
        b.v('sc')[SC['NACT']] = rng.integers(0, 9, size=W)
        iw[IW['STATUS']] = np.where(lanes % 7 == 3, 2, 0)
    else:
        iw[IW['STATUS']] = np.where(lanes >= count, R.UNSOLVED, iw[IW['STATUS']])
        iw[IW['POL']] = np.where(lanes >= count, 0, lanes % 3)
        for k, v in (pol or {}).items():
            iw[IW['POL'], k] = v
        m = lay.m
        if m:
            sc = R.lane_scales()
            lo = rng.standard_normal((m, W)) * sc
            kind = rng.integers(0, 5, size=(m, W))
            b.v('sl')[:] = np.where((kind == 2) | (kind == 3), -INFTY, lo)
            b.v('su')[:] = np.where(kind == 1, lo, np.where((kind == 2) | (kind == 4), INFTY, lo + (0.1 + rng.random((m, W))) * sc))
    return b


class BCase:
    """the API arrays of a call, the CALLER's numbering.  adjoint: sx gx (count, n), sy gy l u (count, m) in; dq dl du dP dA arec in and out (random: what an op
    does not write must come back).  polish: x y rec.  none: names of optional arrays that are absent."""
    def __init__(self, H, count, seed, mode='adjoint', none=()):
        rng = np.random.default_rng(seed)
        sc = R.lane_scales()[:count, None]
        n, m = H.n, H.m
        self.count, self.mode, self.IO = count, mode, (ADJ_IO if mode == 'adjoint' else POL_IO)
        g = lambda w: rng.standard_normal((count, w)) * sc
        for k in ('sx', 'sy', 'gx', 'gy', 'l', 'u') + ADJ_IO + POL_IO:
            setattr(self, k, None)
        if mode == 'adjoint':
            self.sx, self.gx, self.sy, self.gy = g(n), g(n), g(m), g(m)
            lo = g(m)
            kind = rng.integers(0, 5, size=(count, m))
            self.l = np.where((kind == 2) | (kind == 3), -np.inf, lo)
            self.u = np.where(kind == 1, lo, np.where((kind == 2) | (kind == 4), np.inf, lo + (0.1 + rng.random((count, m))) * sc))
            self.dq, self.dl, self.du, self.dP, self.dA, self.arec = g(n), g(m), g(m), g(len(H.Pe[0])), g(len(H.Ae[0])), g(ADJ_REC)
            for k in none:
                setattr(self, k, None)
        else:
            self.x, self.y, self.rec = g(n), g(m), g(KREC)

    def kw(self):
        names = ('sx', 'sy', 'gx', 'gy', 'l', 'u') + ADJ_IO if self.mode == 'adjoint' else POL_IO
        return dict(count=self.count, mode=self.mode, **{k: getattr(self, k) for k in names if getattr(self, k) is not None})


def recurrence_ends(err, gain, steps, min_steps, max_steps, best, worse):
    """term_rules.h recurrence_ends, per lane, fp64 -> (end, best, worse)"""
    with np.errstate(all='ignore'):
        worse = np.where(~(err < gain * best), worse + 1, 0)
        best = np.where(err < best, err, best)
        end = ((steps >= min_steps) & ((err < 1e-13) | (worse >= 2))) | (steps >= max_steps)
    return end, best, worse


def sel_max(a, b):
    """std::max's select  a < b ? b : a  (a NaN goes where it always went)"""
    return np.where(a < b, b, a)


def polish_accept(pri, dua, pri0, dua0):
    return ((pri < pri0) & (dua < dua0)) | ((pri < pri0) & (dua0 < 1e-10)) | ((dua < dua0) & (pri0 < 1e-10))


class BackRef(R.Ref):
    """op -> {key: (expected, k, exact lanes)} as lockstep_ref.Ref; more keys: 'code' (ints), ('reccol', c): column c of the block's records, ('io', name): a
    caller's array transposed to (width, count), ('ioc', name, c): column c of a caller's array"""
    def __init__(self, H, b0, case, dt, P):
        R.Ref.__init__(self, H, b0, case, dt)
        self.P = P

    def all_exact(self):
        return np.ones(W, bool)

    def mine(self):
        return np.arange(W) < self.c.count

    def f64fold(self, slot, kind):
        """a fold whose result feeds a DECISION: fp64, in the kernel's order for sums (ls_fold: wave w takes g = w, w + 4, ..; then the four in wave order)"""
        p = self.b.v('part')[slot][:self.H.G]
        if kind == 'max':
            return R.nanmax_reduce(p, 0).astype(np.float64)
        acc = [np.zeros(W) for _ in range(4)]
        for g in range(self.H.G):
            acc[g % 4] = acc[g % 4] + p[g]
        return ((acc[0] + acc[1]) + acc[2]) + acc[3]

    # ---- adjoint
    def op_adj_load_n(self):
        H, c, dt = self.H, self.c, self.dt
        ex, z = self.all_exact(), np.zeros((H.n, W), dt)
        ax, gv = self.lanes_in(c.sx, H.pc), self.lanes_in(c.gx, H.pc)
        xt = ax * self.sv('Dinv')                                                # in_x
        q = self.cs()[None, :] * self.sv('D') * gv                                 # in_q: (c D) q
        full = lambda nm, top: np.concatenate([top, self.V(nm)[H.n:]])
        out = {'ax': (ax, 0, ex), 'gdx': (gv, 0, ex), 'q': (q, 2, None), 'x': (full('x', z), 0, ex), 'dx': (full('dx', z), 0, ex)}
        if H.r:                                                                    # the direct route: x~ = Dinv x into the block vector x~, the zeros into p
            out.update({'xs': (full('xs', xt), 1, None), 'p': (z, 0, ex)})
        else:
            out.update({'p': (xt, 1, None), 'xs': (z, 0, ex)})
        return out

    def op_adj_load_m(self):
        H, c, dt = self.H, self.c, self.dt
        ex, mine = self.all_exact(), self.mine()[None, :]
        own = lambda a, a0: self.lanes_in(a, H.pr) if a is not None else np.asarray(a0, dt)[:, None] * np.ones((1, W), dt)
        l = np.where(mine, np.maximum(own(c.l, H.l0), -INFTY), -INFTY)
        u = np.where(mine, np.minimum(own(c.u, H.u0), INFTY), INFTY)
        gdy = self.lanes_in(c.gy, H.pr) if c.gy is not None else np.zeros((H.m, W), dt)
        return {'ay': (self.lanes_in(c.sy, H.pr), 0, ex), 'gdy': (gdy, 0, ex), 'l': (l, 0, ex), 'u': (u, 0, ex)}

    def op_adj_class(self):
        H, c, dt = self.H, self.c, self.dt
        ex = self.all_exact()
        zi = self.sv('Einv') * self.Ax(self.V('xs') if H.r else self.V('p'))
        with np.errstate(all='ignore'):
            z64 = zi.astype(np.float64)
            l, u, y = self.b.v('l'), self.b.v('u'), self.b.v('ay')
            low = z64 - l < -y
            upp = ~low & (u - z64 < y)
            eq = l == u
            low, upp = np.where(eq, y < 0.0, low), np.where(eq, ~(y < 0.0), upp)
        kc = np.where(low, 1, np.where(upp, 2, 0))
        on = kc != 0
        bnd = np.where(on, -(self.sv('E') * self.V('gdy')), 0) if c.gy is not None else np.zeros((H.m, W), dt)
        z0 = np.zeros((H.m, W), dt)
        groups, _ = R.strips(H.m, H.G)
        return {'code': (kc.astype(np.int32), 0, ex), 'l': (np.where(on, bnd, -INFTY), 1, None), 'u': (np.where(on, bnd, INFTY), 1, None), 'z': (bnd, 1, None),
                'zt': (z0, 0, ex), 'y': (z0, 0, ex), 'dy': (z0, 0, ex), ('part', AS_ACT): (R.put(on.astype(dt), groups, 'sum', dt), 0, ex)}

    def state(self, rows):
        return {('iw', IW[k]): self.ints(0, v) for k, v in rows.items()}

    def op_adj_init(self):
        H, dt, P = self.H, self.dt, self.P
        ex = self.all_exact()
        nact = self.f64fold(AS_ACT, 'sum') if H.m > 0 else np.zeros(W)
        mine, sing = self.mine(), nact > float(H.n)
        f = lambda v: (np.full(W, v, dt), 0, ex)
        out = {('sc', SC['RHOBAR']): f(P.rho0), ('sc', SC['EQF']): f(1.0), ('sc', SC['EPSCG']): f(0.0), ('sc', SC['EPSPREV']): f(np.inf), ('sc', SC['BEST']): f(np.inf),
               ('sc', SC['NACT']): (nact.astype(dt), H.G, None)}
        zero = np.zeros(W)
        out.update(self.state(dict(DONE=~mine | sing, STATUS=np.where(mine & sing, 2, 0), RHOUPD=zero, PCG=zero, RELRULE=zero, CGON=zero, RHOCH=zero + 1, STEPS=zero, WORSE=zero)))
        out.update({('word', WD['CGANY']): 0, ('word', WD['LIVE']): int((mine & ~sing).sum()), ('word', WD['RHOANY']): 1, ('word', WD['PCGSUM']): 0, ('word', WD['CGIT']): 0})
        return out

    def decide(self, err, gain, min_steps, max_steps):
        iw, sc = self.b.v('iw'), self.b.v('sc')
        live = ~self.iw('DONE')
        steps = iw[IW['STEPS']] + 1
        end, best, worse = recurrence_ends(err, gain, steps, min_steps, max_steps, sc[SC['BEST']], iw[IW['WORSE']])
        done = np.where(live & end, 1, iw[IW['DONE']])
        out = {('sc', SC['BEST']): (np.where(live, best, sc[SC['BEST']]).astype(self.dt), 1, ~live)}
        out.update(self.state(dict(STEPS=np.where(live, steps, iw[IW['STEPS']]), WORSE=np.where(live, worse, iw[IW['WORSE']]), DONE=done, RHOCH=np.zeros(W))))
        out.update({('word', WD['LIVE']): int((done == 0).sum()), ('word', WD['RHOANY']): 0, ('word', WD['PCGSUM']): int(iw[IW['PCG']].sum())})
        return out

    def op_adj_decide(self):
        P, has_m = self.P, self.H.m > 0
        mx = lambda s: self.f64fold(s, 'max')
        pri, z = (mx(PS_M0 + 3), mx(PS_M0 + 5)) if has_m else (np.zeros(W), np.zeros(W))
        dua, qn = mx(PS_N0 + 3), mx(PS_N0 + 8)
        with np.errstate(all='ignore'):
            err = sel_max(pri, dua) / (sel_max(qn, z) + 1e-30)                     # recurrence_err_rhs
        return self.decide(err, P.gain, P.min_steps, P.max_steps)

    def op_adj_unscale(self):
        H = self.H
        ex = self.all_exact()
        full = self.V('x')
        ys = np.where(self.b.v('code') != 0, self.V('y'), 0)
        return {'rx': (self.sv('D') * full[:H.n], 1, None), 'y': (ys, 0, ex), 'ry': (self.cs(True)[None, :] * self.sv('E') * ys, 2, None)}

    def op_adj_resm(self):
        H, dt = self.H, self.dt
        on = self.b.v('code') != 0
        dy = self.V('gdy')
        with np.errstate(all='ignore'):
            rm = np.where(on, np.abs(dy + self.sv('Einv') * self.Ax(self.V('x'))), 0)
            gm = np.where(on, np.abs(dy), 0)
        groups, _ = R.strips(H.m, H.G)
        k = self.klen(H.Av if H.r else H.A)
        return {('part', AS_RM): (R.put(rm, groups, 'max', dt), k + 1, None), ('part', AS_GM): (R.put(gm, groups, 'max', dt), 0, self.all_exact())}

    def op_adj_resn(self):
        H, dt = self.H, self.dt
        rp, col, _ = H.B
        x, y = self.V('x')[:H.n], self.V('y')
        X = np.concatenate([x, y])
        a0, a1 = R.spmm(rp, col, self.Bv(), X, dt, pick=col < H.n), R.spmm(rp, col, self.Bv(), X, dt, pick=col >= H.n)
        kr = self.cs(True)[None, :] * self.sv('Dinv') * ((a0 - dt(H.sigma) * x) + a1)
        dx = self.V('gdx')
        groups, _ = R.strips(H.n, H.G)
        return {('part', AS_RN): (R.put(np.abs(dx + kr), groups, 'max', dt), self.klen(H.B) + 3, None), ('part', AS_GN): (R.put(np.abs(dx), groups, 'max', dt), 0, self.all_exact())}

    def op_adj_final(self):
        H, c, P = self.H, self.c, self.P
        if c.arec is None:
            return {}
        mx = lambda s: self.f64fold(s, 'max')
        nm = lambda a, b: np.where(np.isnan(a) | np.isnan(b), np.nan, np.maximum(a, b))
        rm, gm = (mx(AS_RM), mx(AS_GM)) if H.m > 0 else (np.zeros(W), np.zeros(W))
        r, g = nm(rm, mx(AS_RN)), nm(gm, mx(AS_GN))
        sing = self.b.v('iw')[IW['STATUS']] == 2
        with np.errstate(all='ignore'):
            resid = np.where(sing, np.inf, np.where(g > 0.0, r / g, np.where(r > 0.0, np.inf, 0.0)))
        status = np.where(sing, 2.0, np.where(resid < P.adjoint_tol, 0.0, 3.0))
        n = c.count
        ex = np.ones(n, bool)
        return {('ioc', 'arec', 0): (status[:n], 0, ex), ('ioc', 'arec', 1): (self.b.v('sc')[SC['NACT']][:n], 0, ex), ('ioc', 'arec', 2): (resid[:n].astype(self.dt), 1, None),
                ('ioc', 'arec', 3): (self.b.v('iw')[IW['STEPS']][:n].astype(float), 0, ex)}

    def op_adj_out_n(self):
        return {('io', 'dq'): (self.out_lanes(self.V('rx'), self.H.pc), 0, np.ones(self.c.count, bool))}

    def op_adj_out_m(self):
        code, ry, ex = self.b.v('code'), self.V('ry'), np.ones(self.c.count, bool)
        out = {}
        for side, nm in ((1, 'dl'), (2, 'du')):
            if getattr(self.c, nm) is not None:
                out[('io', nm)] = (self.out_lanes(np.where(code == side, -ry, 0), self.H.pr), 0, ex)
        return out

    def op_adj_grad_p(self):
        (i, j), n = self.H.Pe, self.c.count
        rx, ax = self.V('rx'), self.V('ax')
        return {('io', 'dP'): ((self.dt(0.5) * (rx[i] * ax[j] + rx[j] * ax[i]))[:, :n], 2, None)}

    def op_adj_grad_a(self):
        (i, j), n = self.H.Ae, self.c.count
        return {('io', 'dA'): ((self.V('ay')[i] * self.V('rx')[j] + self.V('ry')[i] * self.V('ax')[j])[:, :n], 2, None)}

    # ---- the direct route's two
    def lwa_setl(self, nm):
        H = self.H
        full = self.V(nm)
        full[H.n:] = self.V('pg').sum(axis=0)
        return {nm: (full, H.lay.GC, None)}

    def op_lwa_setl_x(self):
        return self.lwa_setl('x')

    def op_lwa_setl_xs(self):
        return self.lwa_setl('xs')

    def op_lwa_zero(self):
        z = np.zeros((self.H.n + self.H.r, W), self.dt)
        return {nm: (z, 0, self.all_exact()) for nm in ('x', 'xs', 'dx')}

    # ---- polish
    def op_pol_begin(self):
        P, dt = self.P, self.dt
        iw, s = self.b.v('iw'), self.V('sc')
        pol = iw[IW['STATUS']] == SOLVED
        ex = self.all_exact()
        out = {('sc', SC['RHOBAR']): (np.where(pol, dt(P.pol_rho), s[SC['RHOBAR']]), 0, ex), ('sc', SC['EQF']): (np.where(pol, dt(1.0), s[SC['EQF']]), 0, ex),
               ('sc', SC['BEST']): (np.where(pol, dt(np.inf), s[SC['BEST']]), 0, ex)}
        zero = np.zeros(W)
        out.update(self.state(dict(POL=pol, DONE=~pol, RHOCH=pol, CGON=zero, PCG=zero, STEPS=zero, WORSE=zero)))
        out.update({('word', WD['CGANY']): 0, ('word', WD['LIVE']): int(pol.sum()), ('word', WD['RHOANY']): int(pol.any()), ('word', WD['CGIT']): 0, ('word', WD['POLACC']): 0,
                    ('word', WD['POLREJ']): 0})
        return out

    def op_pol_class(self):
        H = self.H
        pol = self.b.v('iw')[IW['POL']] != 0
        ex = self.all_exact()
        z, y, l, u = (self.b.v(k) for k in ('z', 'y', 'l', 'u'))
        with np.errstate(all='ignore'):
            low = z - l < -y                                                       # polish_active
            upp = ~low & (u - z < y)
        low = low | (l == u)
        on = low | upp
        bnd = np.where(low, l, u)
        sel = lambda new, name: (np.where(pol[None, :], new, self.b.v(name)).astype(self.dt), 0, ex)
        sx = self.V('sx')
        return {'sx': (np.where(pol[None, :], self.V('x')[:H.n], sx), 0, ex), 'sz': sel(z, 'sz'), 'sy': sel(y, 'sy'), 'sl': sel(l, 'sl'), 'su': sel(u, 'su'),
                'l': sel(np.where(on, bnd, -INFTY), 'l'), 'u': sel(np.where(on, bnd, INFTY), 'u'), 'z': sel(np.where(on, bnd, z), 'z'), 'y': sel(np.where(on, y, 0.0), 'y')}

    def op_pol_decide(self):
        P, has_m = self.P, self.H.m > 0
        mx = lambda s: self.f64fold(s, 'max')
        zero = np.zeros(W)
        pri, ax, z = (mx(PS_M0 + 3), mx(PS_M0 + 4), mx(PS_M0 + 5)) if has_m else (zero, zero, zero)
        dua, px, aty, qn = mx(PS_N0 + 3), mx(PS_N0 + 4), mx(PS_N0 + 5), mx(PS_N0 + 8)
        with np.errstate(all='ignore'):                                            # recurrence_err_polish
            ep, ed = pri / (sel_max(ax, z) + 1e-30), dua / (sel_max(sel_max(aty, px), qn) + 1e-30)
            err = sel_max(ep, ed)
        return self.decide(err, 0.5, P.pol_min_steps, P.pol_max_steps)

    def op_pol_cone(self):
        H = self.H
        pol = self.b.v('iw')[IW['POL']] != 0
        l, u = self.V('sl'), self.V('su')
        t = self.Ax(self.V('x')) + self.V('y')
        zc = np.minimum(np.maximum(t, l), u)                                       # normal_cone
        k = self.klen(H.Av if H.r else H.A) + 1
        keep = lambda new, name, kk, exact: (np.where(pol[None, :], new, self.V(name)), kk, ~pol | exact)
        return {'l': keep(l, 'l', 0, True), 'u': keep(u, 'u', 0, True), 'z': keep(zc, 'z', k, False), 'y': keep(t - zc, 'y', k, False)}

    def op_pol_accept(self):
        H, P, dt = self.H, self.P, self.dt
        has_m, gap_on = H.m > 0, bool(P.check_dualgap)
        zero = np.zeros(W)
        mx, sm = (lambda s: self.f64fold(s, 'max')), (lambda s: self.f64fold(s, 'sum'))
        pri_u, pri_s = (mx(PS_M0), mx(PS_M0 + 3)) if has_m else (zero, zero)
        dua_u, dua_s, xpx, qx = mx(PS_N0), mx(PS_N0 + 3), sm(PS_N0 + 14), sm(PS_N0 + 15)
        supp = sm(PS_SUPP) if (gap_on and has_m) else zero
        c64, ci64 = self.cs().astype(np.float64), self.cs(True).astype(np.float64)
        rec, iw = self.b.v('rec'), self.b.v('iw')
        pol = iw[IW['POL']] != 0
        with np.errstate(all='ignore'):
            prim = zero if not has_m else (pri_u if H.unscaled else pri_s)         # term_info, fp64: what the decision compares
            dual = ci64 * dua_u if H.unscaled else dua_s
            ok = pol & polish_accept(prim, dual, rec[:, 3], rec[:, 4])
            # the values, in dt: the sums folded in dt
            xpx_d, qx_d = self.fold(PS_N0 + 14, 'sum'), self.fold(PS_N0 + 15, 'sum')
            supp_d = self.fold(PS_SUPP, 'sum') if (gap_on and has_m) else np.zeros(W, dt)
            f = self.cs(True) if H.scaling else np.ones(W, dt)
            obj = (dt(0.5) * xpx_d + qx_d) * f
            gap = obj - (dt(-0.5) * xpx_d - supp_d) * f
        col = lambda cnum, new, k: (('reccol', cnum), (np.where(ok, new, rec[:, cnum]).astype(dt), k, ~ok))
        out = dict([col(2, obj, H.G), col(3, prim, 0), col(4, dual, 1)])
        out[('reccol', 8)] = (np.where(ok, 1.0, np.where(pol, -1.0, rec[:, 8])).astype(dt), 0, self.all_exact())
        if gap_on:
            out.update([col(11, gap, H.G)])
        out.update(self.state(dict(POL=np.where(pol & ~ok, 2, iw[IW['POL']]))))
        out.update({('word', WD['POLACC']): int(ok.sum()), ('word', WD['POLREJ']): int((pol & ~ok).sum())})
        return out

    def op_pol_end(self):
        H, P = self.H, self.P
        pv = self.b.v('iw')[IW['POL']]
        pol, back = pv != 0, (pv == 2)[None, :]
        ex = self.all_exact()
        x = self.V('x')
        x[:H.n] = np.where(back, self.V('sx'), x[:H.n])
        return {('reccol', 9): (np.where(pol, self.dt(P.secs), self.V('rec')[:, 9]), 0, ex), 'x': (x, 0, ex), 'y': (np.where(back, self.V('sy'), self.V('y')), 0, ex),
                'z': (np.where(back, self.V('sz'), self.V('z')), 0, ex)}


def bjudge(op, H, b0, case, b1, io1, P, skip=None):
    """lockstep_ref.judge for the ops of this file: the listed outputs against the rule (-> worst ratio), exact lanes and ints bit for bit, and every other
    double and int of the blocks and every caller array the op does not write bit-unchanged.  io1: the caller's arrays after the call."""
    with np.errstate(all='ignore'):
        ref, r64 = BackRef(H, b0, case, LD, P).run(op), BackRef(H, b0, case, np.float64, P).run(op)
    lay = b0.lay
    pos = BBlk(lay, np.arange(lay.ws_doubles, dtype=np.float64), None if b0.mat is None else np.arange(lay.mat_doubles, dtype=np.float64))
    touched = np.zeros(lay.ws_doubles, bool)
    mtouched = None if b0.mat is None else np.zeros(lay.mat_doubles, bool)
    itouched = np.zeros((R.KINT, W), bool)
    iot = {k: np.zeros(np.shape(getattr(case, k)), bool) for k in case.IO if getattr(case, k) is not None}
    worst, problems = 0.0, []
    for key, val in ref.items():
        name = key[0] if isinstance(key, tuple) else key
        if name == 'word':
            itouched[IW['WORD'], key[1]] = True
            got = int(b1.v('iw')[IW['WORD'], key[1]])
            if got != val:
                problems.append('%s word %d: %d, expected %d' % (op, key[1], got, val))
            continue
        want, k, exact = val
        if name == 'iw':
            itouched[key[1]] = True
            if not np.array_equal(b1.v('iw')[key[1]], want):
                problems.append('%s iw row %d: lanes %s differ' % (op, key[1], np.nonzero(b1.v('iw')[key[1]] != want)[0][:8]))
            continue
        if name == 'code':
            o, c = lay.fwd['code']
            touched[o:o + c] = True
            if not np.array_equal(b1.v('code'), want):
                bad = np.nonzero(b1.v('code') != want)
                problems.append('%s code: %d rows differ, first row %d lane %d' % (op, bad[0].size, bad[0][0], bad[1][0]))
            continue
        if name == 'io':
            iot[key[1]][:] = True
            got = np.asarray(io1[key[1]], np.float64).T
        elif name == 'ioc':
            iot[key[1]][:, key[2]] = True
            got = np.asarray(io1[key[1]], np.float64)[:, key[2]]
        else:
            got = b1.get(key)
            where = pos.get(key)
            got = got[:want.shape[0]] if got.ndim == 2 and want.ndim == 2 else got
            where = where[:want.shape[0]] if where.ndim == 2 and want.ndim == 2 else where
            (mtouched if (name in lay.mat and name not in lay.fwd) else touched)[where.astype(np.int64).ravel()] = True
        worst = max(worst, R.compare('%s %s' % (op, key), got, want, r64[key][0], k, exact, skip, problems))
    ir = lay.fwd['iw']
    touched[ir[0]:ir[0] + ir[1]] = True
    bad = np.nonzero((b0.ws.view(np.uint64) != b1.ws.view(np.uint64)) & ~touched)[0]
    if bad.size:
        where = [nm for nm in lay.fwd if lay.fwd[nm][0] <= bad[0] < sum(lay.fwd[nm])]
        problems.append('%s: %d doubles outside its outputs changed, first at %d (%s row %d lane %d)' % (op, bad.size, bad[0], where, (bad[0] - (lay.fwd[where[0]][0] if where else 0)) // W, bad[0] % W))
    ibad = np.nonzero((b0.v('iw') != b1.v('iw')) & ~itouched)
    if ibad[0].size:
        problems.append('%s: ints outside its outputs changed: rows %s lanes %s' % (op, ibad[0][:8], ibad[1][:8]))
    if b0.mat is not None:
        bad = np.nonzero((b0.mat.view(np.uint64) != b1.mat.view(np.uint64)) & ~mtouched)[0]
        if bad.size:
            problems.append('%s: %d doubles of the matrix block outside its outputs changed, first at %d' % (op, bad.size, bad[0]))
    for k, t in iot.items():
        a, b = np.asarray(io1[k], np.float64).reshape(t.shape), np.asarray(getattr(case, k), np.float64)
        if ((a.view(np.uint64) != b.view(np.uint64)) & ~t).any():
            problems.append("%s: the caller's %s changed where the op does not write" % (op, k))
    assert not problems, '\n'.join(problems)
    return worst


def back_ops(H, mode):
    """the ops that belong to a handle's route, to the mode and to the handle (m = 0: what the drivers never launch then)"""
    ops = (ADJ_OPS + LWA_OPS if H.r else ADJ_OPS) if mode == 'adjoint' else (POL_OPS + ('lwa_setl_x',) if H.r else POL_OPS)
    return [op for op in ops if (H.m > 0 or op not in M_SIDE)]


class BackStandin(R.Standin):
    """osqp_hip_test_lockstep_back in plain fp64 numpy for every op (BACK_OPS): lockstep_ref.Standin's row passes, tiles, partials and folds with the new
    kernels' bodies.  bug: one planted mistake (tests/test_lockstep_back_ref.py lists them)."""
    def __init__(self, H, P, bug=None):
        R.Standin.__init__(self, H, bug)
        self.P = P

    def call(self, ops, blk, case):
        b = blk.copy()
        self.io = {k: (None if getattr(case, k) is None else getattr(case, k).copy()) for k in case.IO}
        with np.errstate(all='ignore'):
            for op in ops:
                getattr(self, 'k_' + op)(b, case)
        return b, self.io

    def vals_view(self, b):
        return self.vals(b, 'A')

    # ---- adjoint
    def k_adj_load_n(self, b, c):
        H = self.H
        n = H.n
        dst_p, dst_xs = (b.v('xs'), b.v('p')) if H.r else (b.v('p'), b.v('xs'))      # (the direct route's view kl exchanges the two)
        xv = self.tile_in(c.sx, H.pc, n)
        b.v('ax')[:] = xv; dst_p[:n] = xv if self.bug == 'load_n_without_dinv' else xv * self.sv(b, 'Dinv')
        b.v('x')[:n] = 0.0; dst_xs[:n] = 0.0; b.v('dx')[:n] = 0.0
        gv = self.tile_in(c.gx, H.pc, n)
        b.v('gdx')[:] = gv; b.v('q')[:] = self.cs(b)[None, :] * self.sv(b, 'D') * gv

    def k_adj_load_m(self, b, c):
        H = self.H
        m, mine = H.m, (np.arange(W) < c.count)[None, :]
        b.v('ay')[:] = self.tile_in(c.sy, H.pr, m)
        b.v('gdy')[:] = self.tile_in(c.gy, H.pr, m) if c.gy is not None else 0.0
        lo = self.tile_in(c.l, H.pr, m) if c.l is not None else H.l0[:, None] * np.ones((1, W))
        up = self.tile_in(c.u, H.pr, m) if c.u is not None else H.u0[:, None] * np.ones((1, W))
        b.v('l')[:] = np.where(mine, np.fmax(lo, -INFTY), -INFTY)
        b.v('u')[:] = np.where(mine, np.fmin(up, INFTY), -INFTY if self.bug == 'load_m_dead_lane_upper_sign' else INFTY)

    def k_adj_class(self, b, c):
        H = self.H
        E, Einv = self.sv(b, 'E'), self.sv(b, 'Einv')
        src = b.v('xs') if H.r else b.v('p')
        has_dy = c.gy is not None
        code, l, u, ay, gdy = b.v('code'), b.v('l'), b.v('u'), b.v('ay'), b.v('gdy')
        cnt = [[np.zeros(W) for _ in range(4)] for _ in range(H.G)]
        def load(i, cc, v, acc):
            acc[0] += v * src[cc]
        def row(i, acc, g, w):
            zi = Einv[i] * acc[0]
            low = zi - l[i] < -ay[i]
            upp = ~low & (u[i] - zi < ay[i])
            eq = l[i] == u[i]
            if self.bug != 'class_without_equality_override':
                low, upp = np.where(eq, ay[i] < 0.0, low), np.where(eq, ~(ay[i] < 0.0), upp)
            kc = np.where(low, 1, np.where(upp, 2, 0))
            bnd = np.where(kc != 0, -(E[i] * gdy[i]), 0.0) if has_dy else np.zeros(W)
            code[i] = kc
            l[i] = np.where(kc != 0, bnd, -INFTY); u[i] = np.where(kc != 0, bnd, INFTY)
            b.v('z')[i] = bnd; b.v('zt')[i] = 0.0; b.v('y')[i] = 0.0; b.v('dy')[i] = 0.0
            cnt[g][w] = cnt[g][w] + (kc != 0)
        self.rows(b, 'A', 1, load, row)
        self.put(b, AS_ACT, ['sum'], [[[cnt[g][w]] for w in range(4)] for g in range(H.G)])

    def k_adj_init(self, b, c):
        H, P = self.H, self.P
        nact = self.fold(b.v('part')[AS_ACT], H.G, 'sum') if H.m > 0 else np.zeros(W)
        mine = np.arange(W) < c.count
        sing = (nact >= H.n) if self.bug == 'init_singular_at_equality' else (nact > H.n)
        sc, iw = b.v('sc'), b.v('iw')
        sc[SC['RHOBAR']] = P.rho0; sc[SC['EQF']] = 1.0; sc[SC['EPSCG']] = 0.0; sc[SC['EPSPREV']] = np.inf; sc[SC['BEST']] = np.inf; sc[SC['NACT']] = nact
        iw[IW['DONE']] = ~mine | sing; iw[IW['STATUS']] = np.where(mine & sing, 2, 0)
        for nm, v in (('RHOUPD', 0), ('PCG', 0), ('RELRULE', 0), ('CGON', 0), ('RHOCH', 1), ('STEPS', 0), ('WORSE', 0)):
            iw[IW[nm]] = v
        for nm, v in (('CGANY', 0), ('LIVE', int((mine & ~sing).sum())), ('RHOANY', 1), ('PCGSUM', 0), ('CGIT', 0)):
            iw[IW['WORD'], WD[nm]] = v

    def decide(self, b, err, gain, min_steps, max_steps):
        sc, iw = b.v('sc'), b.v('iw')
        live = iw[IW['DONE']] == 0
        steps = iw[IW['STEPS']] + 1
        best, worse = sc[SC['BEST']].copy(), iw[IW['WORSE']].copy()
        better = err < gain * best
        worse = np.where(~better, worse + (0 if self.bug == 'decide_keeps_worse' else 1), 0)
        best = np.where(err < best, err, best)
        end = ((steps >= min_steps) & ((err < 1e-13) | (worse >= 2))) | (steps >= max_steps + (1 if self.bug == 'decide_one_step_late' else 0))
        iw[IW['STEPS']] = np.where(live, steps, iw[IW['STEPS']]); sc[SC['BEST']] = np.where(live, best, sc[SC['BEST']]); iw[IW['WORSE']] = np.where(live, worse, iw[IW['WORSE']])
        iw[IW['DONE']] = np.where(live & end, 1, iw[IW['DONE']])
        iw[IW['RHOCH']] = 0
        iw[IW['WORD'], WD['LIVE']] = int((iw[IW['DONE']] == 0).sum()); iw[IW['WORD'], WD['RHOANY']] = 0; iw[IW['WORD'], WD['PCGSUM']] = int(iw[IW['PCG']].sum())

    def k_adj_decide(self, b, c):
        H, P, part = self.H, self.P, b.v('part')
        mx = lambda s: self.fold(part[s], H.G, 'max')
        pri, z = (mx(PS_M0 + 3), mx(PS_M0 + 5)) if H.m > 0 else (np.zeros(W), np.zeros(W))
        dua, qn = mx(PS_N0 + 3), mx(PS_N0 + 8)
        self.decide(b, sel_max(pri, dua) / (sel_max(qn, z) + 1e-30), P.gain, P.min_steps, P.max_steps)

    def k_adj_unscale(self, b, c):
        H = self.H
        b.v('rx')[:] = self.sv(b, 'D') * b.v('x')[:H.n]
        ys = b.v('y').copy() if self.bug == 'unscale_keeps_y_on_code0' else np.where(b.v('code') != 0, b.v('y'), 0.0)
        b.v('y')[:] = ys
        b.v('ry')[:] = self.cs(b, True)[None, :] * self.sv(b, 'E') * ys

    def k_adj_resm(self, b, c):
        H = self.H
        Einv, x, code, gdy = self.sv(b, 'Einv'), b.v('x'), b.v('code'), b.v('gdy')
        st = [[[np.zeros(W), np.zeros(W)] for _ in range(4)] for _ in range(H.G)]
        def load(i, cc, v, acc):
            acc[0] += v * x[cc]
        def row(i, acc, g, w):
            on = np.ones(W, bool) if self.bug == 'resm_counts_code0' else code[i] != 0
            s = st[g][w]
            s[0] = np.where(on, R._nanmax(s[0], np.abs(gdy[i] + Einv[i] * acc[0])), s[0]); s[1] = np.where(on, R._nanmax(s[1], np.abs(gdy[i])), s[1])
        self.rows(b, 'A', 1, load, row)
        self.put(b, AS_RM, ['max', 'max'], st)

    def k_adj_resn(self, b, c):
        H = self.H
        n, sigma = H.n, (0.0 if self.bug == 'resn_without_sigma' else H.sigma)
        Dinv, ci, x, y, gdx = self.sv(b, 'Dinv'), self.cs(b, True), b.v('x'), b.v('y'), b.v('gdx')
        st = [[[np.zeros(W), np.zeros(W)] for _ in range(4)] for _ in range(H.G)]
        def load(j, cc, v, acc):
            if cc < n:
                acc[0] += v * x[cc]
            else:
                acc[1] += v * y[cc - n]
        def row(j, acc, g, w):
            kr = ci * Dinv[j] * ((acc[0] - sigma * x[j]) + acc[1])
            s = st[g][w]
            s[0] = R._nanmax(s[0], np.abs(gdx[j] + kr)); s[1] = R._nanmax(s[1], np.abs(gdx[j]))
        self.rows(b, 'B', 2, load, row)
        self.put(b, AS_RN, ['max', 'max'], st)

    def k_adj_final(self, b, c):
        H, P, part = self.H, self.P, b.v('part')
        if c.arec is None:
            return
        mx = lambda s: self.fold(part[s], H.G, 'max')
        rm, gm = (mx(AS_RM), mx(AS_GM)) if H.m > 0 else (np.zeros(W), np.zeros(W))
        r, g = R._nanmax(rm, mx(AS_RN)), R._nanmax(gm, mx(AS_GN))
        for lane in range(c.count):
            sing = b.v('iw')[IW['STATUS'], lane] == 2
            if self.bug == 'final_inverted_at_g0':
                resid = np.inf if sing else (g[lane] / r[lane] if r[lane] > 0.0 else (np.inf if g[lane] > 0.0 else 0.0))
            else:
                resid = np.inf if sing else (r[lane] / g[lane] if g[lane] > 0.0 else (np.inf if r[lane] > 0.0 else 0.0))
            below = resid <= P.adjoint_tol if self.bug == 'final_tol_inclusive' else resid < P.adjoint_tol
            self.io['arec'][lane] = (2.0 if sing else (0.0 if below else 3.0), b.v('sc')[SC['NACT'], lane], resid, b.v('iw')[IW['STEPS'], lane])

    def k_adj_out_n(self, b, c):
        self.tile_out(b.v('ax' if self.bug == 'out_n_reads_ax' else 'rx'), self.H.pc, self.io['dq'], c.count)

    def k_adj_out_m(self, b, c):
        code, ry = b.v('code'), b.v('ry')
        for side, nm in ((1, 'dl'), (2, 'du')):
            if self.io[nm] is not None:
                s = 3 - side if self.bug == 'out_m_sides_swapped' else side
                self.tile_out(np.where(code == s, -ry, 0.0), self.H.pr, self.io[nm], c.count)

    def grad(self, b, c, sym):
        H = self.H
        i, j = H.Pe if sym else H.Ae
        nz = len(i)
        out = self.io['dP' if sym else 'dA']
        ra, ca, rb, cb = (b.v(k) for k in (('rx', 'ax', 'ax', 'rx') if sym else ('ay', 'rx', 'ry', 'ax')))
        if self.bug == 'grad_a_ry_ay_exchanged' and not sym:
            ra, rb = rb, ra
        for e0 in range(0, nz, 64):                              # a workgroup's 64 entries; the tile's columns past nz are clamped reads (entry nz - 1), never stored
            for el in range(64):
                e = min(e0 + el, nz - 1)
                t = ra[i[e]] * ca[j[e]] + cb[j[e]] * rb[i[e]] if sym else ra[i[e]] * ca[j[e]] + rb[i[e]] * cb[j[e]]
                if sym and self.bug != 'grad_p_without_half':
                    t = 0.5 * t
                if e0 + el < nz or (self.bug == 'grad_store_gate_admits_nz' and e0 + el == nz):      # (the mistake's store lands on the next problem's entry 0)
                    flat = out.reshape(-1)
                    for bb in range(c.count if self.bug != 'grad_store_loop_stops_at_4' else min(c.count, 4)):      # (b = wave, wave + 4, ..: every b < count once)
                        if bb * nz + e0 + el < flat.size:
                            flat[bb * nz + e0 + el] = t[bb]

    def k_adj_grad_p(self, b, c):
        self.grad(b, c, True)

    def k_adj_grad_a(self, b, c):
        self.grad(b, c, False)

    # ---- the direct route's two
    def k_lwa_setl_x(self, b, c):
        for a in range(self.H.r):
            b.v('x')[self.H.n + a - (1 if self.bug == 'setl_one_row_early' else 0)] = self.lw_fold(b.v('pg')[:, a])

    def k_lwa_setl_xs(self, b, c):
        for a in range(self.H.r):
            b.v('xs')[self.H.n + a - (1 if self.bug == 'setl_one_row_early' else 0)] = self.lw_fold(b.v('pg')[:, a])

    def k_lwa_zero(self, b, c):
        rows = self.H.n + self.H.r + (1 if self.bug == 'zero_one_row_past' else 0)
        for nm in ('x', 'xs', 'dx'):
            o, _ = b.lay.fwd[nm]
            b.ws[o:o + rows * W] = 0.0

    # ---- polish
    def k_pol_begin(self, b, c):
        P = self.P
        sc, iw = b.v('sc'), b.v('iw')
        pol = iw[IW['STATUS']] == SOLVED
        if self.bug == 'begin_polishes_dead_lane':
            pol = pol | (np.arange(W) == W - 1)
        sc[SC['RHOBAR']] = np.where(pol, P.pol_rho, sc[SC['RHOBAR']]); sc[SC['EQF']] = np.where(pol, 1.0, sc[SC['EQF']]); sc[SC['BEST']] = np.where(pol, np.inf, sc[SC['BEST']])
        iw[IW['POL']] = pol; iw[IW['DONE']] = ~pol; iw[IW['RHOCH']] = pol
        for nm in ('CGON', 'PCG', 'STEPS', 'WORSE'):
            iw[IW[nm]] = 0
        for nm, v in (('CGANY', 0), ('LIVE', int(pol.sum())), ('RHOANY', 1 if self.bug == 'begin_rhoany_always_1' else int(pol.any())), ('CGIT', 0), ('POLACC', 0), ('POLREJ', 0)):
            iw[IW['WORD'], WD[nm]] = v

    def k_pol_class(self, b, c):
        H = self.H
        pol = (b.v('iw')[IW['POL']] != 0)[None, :]
        if self.bug == 'class_stores_unpolished_lane':
            pol = np.ones((1, W), bool)
        keep = lambda name, new: np.where(pol, new, b.v(name))
        z, y, l, u = (b.v(k).copy() for k in ('z', 'y', 'l', 'u'))
        b.v('sx')[:] = keep('sx', b.v('x')[:H.n])
        for nm, v in (('sz', z), ('sy', y), ('sl', l), ('su', u)):
            b.v(nm)[:] = keep(nm, v)
        low = z - l < -y
        upp = ~low & (u - z < y)
        if self.bug != 'polclass_equality_not_forced':       # (an equality row taken as UPPER-active stores the same l = u = z: only a row left inactive shows)
            low = low | (l == u)
        on = low | upp
        bnd = np.where(low, l, u)
        b.v('l')[:] = keep('l', np.where(on, bnd, -INFTY)); b.v('u')[:] = keep('u', np.where(on, bnd, INFTY))
        b.v('z')[:] = keep('z', np.where(on, bnd, z)); b.v('y')[:] = keep('y', np.where(on, y, 0.0))

    def k_pol_decide(self, b, c):
        H, P, part = self.H, self.P, b.v('part')
        mx = lambda s: self.fold(part[s], H.G, 'max')
        zero = np.zeros(W)
        pri, ax, z = (mx(PS_M0 + 3), mx(PS_M0 + 4), mx(PS_M0 + 5)) if H.m > 0 else (zero, zero, zero)
        dua, px, aty, qn = mx(PS_N0 + 3), mx(PS_N0 + 4), mx(PS_N0 + 5), mx(PS_N0 + 8)
        ep, ed = pri / (sel_max(ax, z) + 1e-30), dua / (sel_max(sel_max(aty, px), qn) + 1e-30)
        self.decide(b, sel_max(ep, ed), 0.5, P.pol_min_steps, P.pol_max_steps)

    def k_pol_cone(self, b, c):
        pol = b.v('iw')[IW['POL']] != 0
        x, y, z, l, u, sl, su = (b.v(k) for k in ('x', 'y', 'z', 'l', 'u', 'sl', 'su'))
        def load(i, cc, v, acc):
            acc[0] += v * x[cc]
        def row(i, acc, g, w):
            t = acc[0] + y[i]
            zc = np.fmin(np.fmax(t, sl[i]), su[i])
            l[i] = np.where(pol, sl[i], l[i])
            if self.bug != 'cone_keeps_u':
                u[i] = np.where(pol, su[i], u[i])
            z[i] = np.where(pol, zc, z[i]); y[i] = np.where(pol, t - zc, y[i])
        self.rows(b, 'A', 1, load, row)

    def k_pol_accept(self, b, c):
        H, P, part = self.H, self.P, b.v('part')
        has_m, gap_on = H.m > 0, bool(P.check_dualgap)
        mx, sm = (lambda s: self.fold(part[s], H.G, 'max')), (lambda s: self.fold(part[s], H.G, 'sum'))
        zero = np.zeros(W)
        pri_u, pri_s = (mx(PS_M0), mx(PS_M0 + 3)) if has_m else (zero, zero)
        dua_u, dua_s, xpx, qx = mx(PS_N0), mx(PS_N0 + 3), sm(PS_N0 + 14), sm(PS_N0 + 15)
        supp = sm(PS_SUPP) if (gap_on and has_m) else zero
        ci = self.cs(b, True)
        rec, iw = b.v('rec'), b.v('iw')
        acc = rej = 0
        for lane in range(W):
            if not iw[IW['POL'], lane]:
                continue
            f = ci[lane] if H.scaling else 1.0
            obj = (0.5 * xpx[lane] + qx[lane]) * f
            prim = 0.0 if not has_m else (pri_u[lane] if H.unscaled else pri_s[lane])
            dual = ci[lane] * dua_u[lane] if H.unscaled else dua_s[lane]
            rc = rec[lane]
            if self.bug == 'accept_at_equality':
                ok = (prim <= rc[3] and dual <= rc[4]) or (prim <= rc[3] and rc[4] < 1e-10) or (dual <= rc[4] and rc[3] < 1e-10)
            else:
                ok = (prim < rc[3] and dual < rc[4]) or (prim < rc[3] and rc[4] < 1e-10) or (dual < rc[4] and rc[3] < 1e-10)
            if ok:
                rc[2] = obj; rc[3] = prim; rc[4] = dual; rc[8] = 1.0
                if gap_on:
                    rc[11] = obj - (-0.5 * xpx[lane] - supp[lane]) * f
                acc += 1
            else:
                rc[8] = -1.0; iw[IW['POL'], lane] = 2
                if self.bug == 'accept_writes_rejected_rc3':
                    rc[3] = prim
                rej += 1
        iw[IW['WORD'], WD['POLACC']] = acc; iw[IW['WORD'], WD['POLREJ']] = rej

    def k_pol_end(self, b, c):
        H, P = self.H, self.P
        pv = b.v('iw')[IW['POL']]
        pol = pv != 0
        back = (pol if self.bug == 'end_restores_accepted' else (pv == 2))[None, :]
        b.v('rec')[:, 9] = np.where(pol, P.secs, b.v('rec')[:, 9])
        b.v('x')[:H.n] = np.where(back, b.v('sx'), b.v('x')[:H.n])
        b.v('y')[:] = np.where(back, b.v('sy'), b.v('y')); b.v('z')[:] = np.where(back, b.v('sz'), b.v('z'))


# ---------------------------------------------------------------------------------------------------------------- the poked edges
# States, not random draws: each puts named rows and lanes of a poked block (and case) at an edge of its kernel's rule.  Shared by both tiers.
def edge_adj_class(H, b, c):
    """lane 3: x~ = 0, so z = Einv (A x~) is exactly 0 in every row in any precision; rows cycle through z at l, at u, strictly inside, l == u with y of either
    sign and exactly 0"""
    if H.m == 0:
        return
    (b.v('xs') if H.r else b.v('p'))[:, 3] = 0.0
    rows = np.arange(H.m)
    l = np.array([0.0, -1.0, -1.0, 0.0, 0.0, 0.0, -1.0, 0.0])[rows % 8]
    u = np.array([1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 2.0])[rows % 8]
    y = np.array([0.0, 0.0, 0.0, 0.5, -0.5, 0.0, 0.25, -0.25])[rows % 8]
    b.v('l')[:, 3], b.v('u')[:, 3], b.v('ay')[:, 3] = l, u, y


def edge_adj_init(H, b, count):
    """lanes 0, 1, 2: nact = n - 1, n, n + 1 (integer partials: the sum is exact); lane 1 must stay regular, lane 2 alone becomes status 2"""
    if H.m == 0:
        return
    for lane, v in ((0, H.n - 1), (1, H.n), (2, H.n + 1)):
        b.v('part')[AS_ACT][:, lane] = 0.0
        b.v('part')[AS_ACT][0, lane] = v


def edge_decide(H, b, P, polish):
    """lanes 0 .. 6: steps + 1 == min_steps with a negligible error; steps + 1 == max_steps; an error of exactly gain * best; a NaN error; worse at its limit;
    a done lane; steps + 1 == min_steps - 1 with a negligible error (one step early: must go on).  The denominators are 1: err is the numerator, exactly."""
    part, sc, iw = b.v('part'), b.v('sc'), b.v('iw')
    gain, mn, mx = (0.5, P.pol_min_steps, P.pol_max_steps) if polish else (P.gain, P.min_steps, P.max_steps)
    lanes = np.arange(7)
    for s in (PS_M0 + 3, PS_M0 + 4, PS_M0 + 5, PS_N0 + 3, PS_N0 + 4, PS_N0 + 5, PS_N0 + 8):
        part[s][:, lanes] = 0.0
    part[PS_N0 + 8][0, lanes] = 1.0                                                # qn_s = 1: both measures divide by 1 + 1e-30 = 1
    best = 0.25
    err = np.array([1e-14, 0.2, gain * best, np.nan, 0.3, 0.1, 1e-14])
    part[PS_N0 + 3][0, lanes] = err                                                # dua_s
    if H.m > 0:                                                                    # (a NaN error needs a NaN PRIMAL residual: the selects of both measures drop a NaN dual one)
        part[PS_N0 + 3][0, 3] = 0.0
        part[PS_M0 + 3][0, 3] = np.nan
    sc[SC['BEST'], lanes] = best
    iw[IW['STEPS'], lanes] = [mn - 1, mx - 1, mn + 1, mn + 1, mn + 1, mn + 1, max(mn - 2, 0)]
    iw[IW['WORSE'], lanes] = [0, 0, 0, 0, 1, 0, 0]
    iw[IW['DONE'], lanes] = [0, 0, 0, 0, 0, 1, 0]
    iw[IW['WORD'], WD['LIVE']] = int((iw[IW['DONE']] == 0).sum())


def edge_adj_final(H, b, P):
    """lanes 0 .. 5: g = 0 = r; g = 0 < r; a singular lane; resid one ulp below, exactly at, one ulp above the tolerance (g = 1: resid = r exactly)"""
    part, iw = b.v('part'), b.v('iw')
    lanes = np.arange(6)
    for s in (AS_RM, AS_GM, AS_RN, AS_GN):
        part[s][:, lanes] = 0.0
    tol = P.adjoint_tol
    part[AS_RN][0, lanes] = [0.0, 0.5, 0.1, np.nextafter(tol, 0.0), tol, np.nextafter(tol, 1.0)]
    part[AS_GN][0, lanes] = [0.0, 0.0, 1.0, 1.0, 1.0, 1.0]
    iw[IW['STATUS'], lanes] = [0, 0, 2, 0, 0, 0]


def edge_pol_class(H, b):
    """lane 1 (IW_POL = 1): rows cycle through an equality row (l == u, z off it, y of either sign), an inactive row, a row active below, a row active above, an equality row with z on it and y = 0
    (active by the override alone)"""
    if H.m == 0:
        return
    rows = np.arange(H.m)
    l = np.array([1.0, 1.0, -1.0, 0.0, -1.0, 1.0])[rows % 6]
    u = np.array([1.0, 1.0, 1.0, 2.0, 0.5, 1.0])[rows % 6]
    z = np.array([1.5, 0.5, 0.0, 0.25, 0.25, 1.0])[rows % 6]
    y = np.array([0.5, -0.5, 0.0, -0.5, 0.5, 0.0])[rows % 6]
    for nm, v in (('l', l), ('u', u), ('z', z), ('y', y)):
        b.v(nm)[:, 1] = v


def edge_pol_accept(H, b):
    """lanes 0 .. 3 attempted (IW_POL = 1).  m > 0: accepted; rejected on the primal residual; rejected on the dual residual; at EQUALITY of the rule (the
    record's primal residual is the polished point's, bit for bit: not an improvement).  m = 0, where the primal residual is 0 by definition: accepted with a
    positive recorded primal residual; accepted through the rule's third clause (recorded primal residual 0, the dual one improves); rejected on the dual
    residual; at EQUALITY on the dual side (the record's dual residual is the polished point's: cinv x the stored maximum, ONE correctly rounded product).
    The record's residuals are set from the partials' own maxima."""
    part, rec, iw = b.v('part'), b.v('rec'), b.v('iw')
    lanes = np.arange(4)
    iw[IW['POL'], lanes] = 1
    pslot, dslot = (PS_M0 if H.unscaled else PS_M0 + 3), (PS_N0 if H.unscaled else PS_N0 + 3)
    dua = part[dslot][:, lanes].max(axis=0)
    if H.m > 0:
        pri = part[pslot][:, lanes].max(axis=0)
        rec[lanes, 3] = pri * np.array([2.0, 0.5, 2.0, 1.0])
        rec[lanes, 4] = 1e3 * dua * np.array([2.0, 2.0, 1e-9, 2.0])
    else:
        cinv = (b.v('sc')[SC['CINV'], lanes] if b.mat is not None else np.full(4, H.cinv)) if H.unscaled else np.ones(4)
        rec[lanes, 3] = [1.0, 0.0, 1.0, 0.0]
        rec[lanes, 4] = np.array([1e3, 1e3, 1e-6, 1.0]) * (cinv * dua)


def edge_pol_cone(H, b):
    """lane 1 (IW_POL = 1): the saved bounds cycle through an equality row, a row that ends inactive (A x + y strictly inside: y -> 0 exactly), a row active
    below, a row active above"""
    if H.m == 0:
        return
    rows = np.arange(H.m)
    b.v('sl')[:, 1] = np.array([0.3, -1e6, 1e6, -2e6])[rows % 4]
    b.v('su')[:, 1] = np.array([0.3, 1e6, 2e6, -1e6])[rows % 4]


def edge_adj_load_m(H, b, c):
    """problem 0: bounds at +-1e30 and beyond (clamped to +-OSQP_INFTY); lanes >= count receive -+OSQP_INFTY whatever the block held"""
    if H.m == 0 or c.l is None or c.u is None:
        return
    c.l[0, 0::3], c.l[0, 1::3] = -1e30, -1e35
    c.u[0, 0::3], c.u[0, 1::3] = 1e30, 1e32


def poke_edges(op, H, b, c, P, variant=None):
    """the states the issue names, on top of the seeded block, by op"""
    if op == 'adj_load_m':
        edge_adj_load_m(H, b, c)
    elif op == 'adj_class':
        edge_adj_class(H, b, c)
    elif op == 'adj_init':
        edge_adj_init(H, b, c.count)
    elif op in ('adj_decide', 'pol_decide'):
        edge_decide(H, b, P, op == 'pol_decide')
    elif op == 'adj_final':
        edge_adj_final(H, b, P)
    elif op == 'pol_class':
        edge_pol_class(H, b)
    elif op == 'pol_cone':
        edge_pol_cone(H, b)
    elif op == 'pol_accept':
        edge_pol_accept(H, b)
    elif op == 'pol_begin':
        edge_pol_begin(H, b, c.count, variant)


VARIANTS = {'pol_begin': ('none', 'all', 'mix')}             # ops whose edges are whole-chunk states: one launch per variant


def edge_pol_begin(H, b, count, variant):
    """the chunk's statuses as a whole: 'none' -- no lane solved (the empty ballot: WD_RHOANY = 0, WD_LIVE = 0, no scalar stored); 'all' -- every lane below
    count solved (count = 64: all 64 lanes take part); 'mix' -- the seeded draw with one solved and one unsolved lane for certain"""
    st, lanes = b.v('iw')[IW['STATUS']], np.arange(W)
    if variant == 'none':
        st[:] = np.where(st == SOLVED, 7, st)
    elif variant == 'all':
        st[:] = np.where(lanes < count, SOLVED, R.UNSOLVED)
    elif count >= 2:
        st[0], st[1] = SOLVED, 3


def check_edges(op, H, b0, c, b1, io, P, variant=None):
    """The poked edges LANDED: the pattern each edge must produce, asserted on the launch's own output wherever the edge applies (any handle, either tier).
    The judge has compared the output with the reference already; this says that the state the reference was asked about is the one the issue names."""
    n, m, count = H.n, H.m, c.count
    iw0, iw, sc = b0.v('iw'), b1.v('iw'), b1.v('sc')
    k = min(count, 8)
    if op == 'adj_load_m' and c.l is not None and c.u is not None and m > 0:
        assert b1.v('l')[:, 0].min() == -INFTY and b1.v('u')[:, 0].max() == INFTY and (np.abs(b1.v('l')[:, 0]) <= INFTY).all() and (np.abs(b1.v('u')[:, 0]) <= INFTY).all()
        assert (b1.v('l')[:, count:] == -INFTY).all() and (b1.v('u')[:, count:] == INFTY).all()
    elif op == 'adj_class' and m >= 8:
        assert list(b1.v('code')[:8, 3]) == [0, 0, 0, 2, 1, 2, 2, 1]      # z at l, at u, inside with y = 0: inactive; l == u: by the sign of y, y = 0 upper; y against the bound
    elif op == 'adj_init' and m > 0:
        assert list(sc[SC['NACT'], :3]) == [n - 1.0, n, n + 1.0]
        assert list(iw[IW['STATUS'], :3]) == [0, 0, 2 if count > 2 else 0] and list(iw[IW['DONE'], :3]) == [int(0 >= count), int(1 >= count), 1]
    elif op in ('adj_decide', 'pol_decide') and (P.pol_min_steps if op == 'pol_decide' else P.min_steps) >= 2:
        nan_lane = [0, 1] if m > 0 else [1, 0]                 # (m = 0: no primal residual to be NaN; a NaN dual one is dropped by the selects: the error is 0)
        assert list(iw[IW['DONE'], :7]) == [1, 1, 0, nan_lane[0], 1, 1, 0] and list(iw[IW['WORSE'], :7]) == [0, 0 if op == 'adj_decide' else 1, 1, nan_lane[1], 2, 0, 0]      # (lane 1's error 0.2 is progress under the adjoint's gain 0.9, none under polish's 0.5)
        assert iw[IW['STEPS'], 5] == iw0[IW['STEPS'], 5] and iw[IW['WORD'], WD['LIVE']] == (iw[IW['DONE']] == 0).sum() and iw[IW['WORD'], WD['PCGSUM']] == iw0[IW['PCG']].sum()
    elif op == 'adj_final' and c.arec is not None:
        k = min(count, 6)
        assert list(io['arec'][:k, 0]) == [0.0, 3.0, 2.0, 0.0, 3.0, 3.0][:k] and list(io['arec'][:k, 2][:3]) == [0.0, np.inf, np.inf][:k]
    elif op == 'pol_class' and m >= 6 and iw0[IW['POL'], 1]:
        assert list(b1.v('l')[:6, 1]) == [1.0, 1.0, -INFTY, 0.0, 0.5, 1.0] and list(b1.v('u')[:6, 1]) == [1.0, 1.0, INFTY, 0.0, 0.5, 1.0] and list(b1.v('z')[:6, 1]) == [1.0, 1.0, 0.0, 0.0, 0.5, 1.0]
        assert list(b1.v('y')[:6, 1]) == [0.5, -0.5, 0.0, -0.5, 0.5, 0.0]
    elif op == 'pol_cone' and m >= 4 and iw0[IW['POL'], 1]:
        y = b1.v('y')[:, 1]
        assert (b1.v('z')[0::4, 1] == 0.3).all() and (y[1::4] == 0.0).all() and (y[2::4] < 0).all() and (y[3::4] > 0).all()
        assert np.array_equal(b1.v('l')[:, 1], b0.v('sl')[:, 1]) and np.array_equal(b1.v('u')[:, 1], b0.v('su')[:, 1])
    elif op == 'pol_accept':
        want = [1.0, -1.0, -1.0, -1.0] if m > 0 else [1.0, 1.0, -1.0, -1.0]
        assert list(b1.v('rec')[:4, 8]) == want and list(iw[IW['POL'], :4]) == [1 if v > 0 else 2 for v in want]
        assert (b1.v('rec')[0, 11] != b0.v('rec')[0, 11]) == bool(P.check_dualgap) and b1.v('rec')[3, 3] == b0.v('rec')[3, 3] and b1.v('rec')[3, 4] == b0.v('rec')[3, 4]
    elif op == 'pol_begin':
        live, any_ = int(iw[IW['WORD'], WD['LIVE']]), int(iw[IW['WORD'], WD['RHOANY']])
        if variant == 'none':
            assert (live, any_) == (0, 0) and np.array_equal(b0.v('sc').view(np.uint64), b1.v('sc').view(np.uint64)) and (iw[IW['DONE']] == 1).all() and (iw[IW['POL']] == 0).all()
        elif variant == 'all':
            assert (live, any_) == (count, 1) and (iw[IW['POL'], :count] == 1).all() and (iw[IW['POL'], count:] == 0).all() and (sc[SC['RHOBAR'], :count] == P.pol_rho).all()
        elif count >= 2:
            assert 0 < live < count and any_ == 1 and list(iw[IW['POL'], :2]) == [1, 0]
    elif op in ('adj_grad_p', 'adj_grad_a') and (n, m) == (70, 37):
        assert len(H.Pe[0]) % 64 != 0 and len(H.Ae[0]) % 64 != 0 and len(H.Pe[0]) > 64 and len(H.Ae[0]) > 64      # S: more than one workgroup, a ragged last tile
