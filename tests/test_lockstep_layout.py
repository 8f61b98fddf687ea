"""CPU tier: osqp-python_amd/csrc/lockstep_layout.h -- the one text that says where everything sits in the work blocks of a lockstep chunk
(lockstep_hip.hip's four drivers, Engine::lockstep_mat_scaling) -- behind tests/hostsim/policy_probe.cpp, with the COUNTING cursor: no memory is
touched.  Every carve must end inside its size function, keep its ranges disjoint and 64-double aligned, and put the scalar state where
lockstep_sc_offset says; the size functions must return what they always have (the closed forms are restated below, independently: the records'
workspace_bytes and the committed profiles depend on them)."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

from test_policy_rules import DEPS, OUT, ROOT, SRC

NS, MS, RS = (1, 63, 64, 65, 400, 8193), (0, 1, 64, 65, 800), (1, 2, 128)
FORWARD, ADJOINT, DIRECT, DIRECT_ADJOINT, POLISH, MAT = range(6)
W = 64


@pytest.fixture(scope='module')
def lib():
    if not (os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(f) for f in DEPS)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'include'), '-o', OUT, SRC])
    L = C.CDLL(OUT)
    SP = C.POINTER(C.c_size_t)
    L.ll_carve.argtypes = [C.c_int, C.c_void_p] + [C.c_int] * 5 + [SP, SP]; L.ll_carve.restype = C.c_int
    L.ll_size.argtypes = [C.c_int] * 6; L.ll_size.restype = C.c_size_t
    L.ll_sc_offset.argtypes = [C.c_int] * 2; L.ll_sc_offset.restype = C.c_size_t
    L.ll_const.argtypes = [C.c_int]; L.ll_const.restype = C.c_int
    assert [L.ll_const(k) for k in range(6)] == [W, 32, 16, 12, 11, 12]       # kLsW, kLsSlots, kLsScal, kLsInt, kLsMatScalC, kBatchRec
    return L


def nnz(n, m):
    return 3 * m, 3 * m + 2 * n                  # some nnz(A), nnz(B): the matrix block's carve is linear in them


def carve(lib, which, n, m, r=0):
    """-> (ranges [(offset, doubles)] in carve order, end, fits, offset of the scalar state) from the counting cursor (base = NULL)"""
    cap = lib.ll_const(6)
    ranges, info = (C.c_size_t * (2 * cap))(), (C.c_size_t * 3)()
    k = lib.ll_carve(which, None, n, m, r, *nnz(n, m), ranges, info)
    assert 0 < k <= cap
    return [(ranges[2 * q], ranges[2 * q + 1]) for q in range(k)], info[0], bool(info[1]), info[2]


def size(lib, which, n, m, r=0):
    return lib.ll_size(which, n, m, r, *nnz(n, m))


def cases(which):
    if which in (DIRECT, DIRECT_ADJOINT):
        return [(n, m, r) for n, m, r in itertools.product(NS, MS, RS) if m >= 1]       # (the direct drivers decline m < 1)
    return [(n, m, 0) for n, m in itertools.product(NS, MS)]


# ---- the closed forms as they have been since each route was added, restated
def grid(n, m):
    return min(256, max(1, (max(n, m) + 15) // 16))


def colblocks(n):
    cb = 64 * max(1, ((n + 63) // 64 + 127) // 128)
    return (n + cb - 1) // cb


def ws_doubles(n, m):
    return W * (8 * n + 9 * m + 32 * grid(n, m) + (m + 63) // 64 + 1 + 16 + 12 + 12) + 64


def adjoint_extra(n, m):
    return W * (3 * n + 3 * m + (m + 1) // 2) + 64


def direct_ws_doubles(n, m, r):
    return W * (3 * (n + r) + 4 * n + 9 * m + 32 * grid(n, m) + (m + 63) // 64 + 1 + 16 + 12 + 12 + r * r + 2 * colblocks(n) * r + r + 1) + 64


CLOSED = {
    FORWARD: lambda n, m, r: ws_doubles(n, m),
    ADJOINT: lambda n, m, r: ws_doubles(n, m) + adjoint_extra(n, m),
    DIRECT: direct_ws_doubles,
    DIRECT_ADJOINT: lambda n, m, r: direct_ws_doubles(n, m, r) + adjoint_extra(n, m),
    POLISH: lambda n, m, r: W * (n + 4 * m) + 64,
    MAT: lambda n, m, r: W * (sum(nnz(n, m)) + 2 * n + 2 * m) + 64,
}


@pytest.mark.parametrize('which', range(6))
def test_size_functions_return_what_they_always_have(lib, which):
    for n, m, r in cases(which):
        assert size(lib, which, n, m, r) == CLOSED[which](n, m, r), (n, m, r)
    for n, m in itertools.product(NS, MS):
        tm = (m + 63) // 64
        assert lib.ll_sc_offset(n, m) == W * (8 * n + 9 * m + 32 * grid(n, m) + max(tm, 1)), (n, m)


@pytest.mark.parametrize('which', range(6))
def test_carve_fits_is_disjoint_and_aligned(lib, which):
    for n, m, r in cases(which):
        ranges, end, fits, _ = carve(lib, which, n, m, r)
        assert fits and end <= size(lib, which, n, m, r), (n, m, r)
        assert max(o + c for o, c in ranges) == end
        assert all(o % 64 == 0 for o, _ in ranges), (n, m, r)                   # every block starts at a multiple of 64 doubles
        live = sorted((o, c) for o, c in ranges if c > 0)                        # (m = 0 leaves the m-side ranges empty)
        assert all(a + ca <= b for (a, ca), (b, _) in zip(live, live[1:])), (n, m, r)


@pytest.mark.parametrize('which,forward', [(ADJOINT, FORWARD), (DIRECT_ADJOINT, DIRECT)])
def test_adjoint_vectors_start_at_the_forward_size_function(lib, which, forward):
    for n, m, r in cases(which):
        fwd, fwd_end, _, _ = carve(lib, forward, n, m, r)
        ranges, end, fits, _ = carve(lib, which, n, m, r)
        assert ranges[:len(fwd)] == fwd and len(ranges) == len(fwd) + 7          # x, dx, r_x, y, dy, r_y, the row codes
        assert ranges[len(fwd)][0] == size(lib, forward, n, m, r) >= fwd_end
        assert fits and end <= size(lib, which, n, m, r)
        assert ranges[-1][1] == (m * W + 1) // 2                                  # m x 64 int32 codes


@pytest.mark.parametrize('which', [ADJOINT, DIRECT_ADJOINT])
def test_adjoint_carve_is_ax_gdx_rx_ay_gdy_ry_code_back_to_back(lib, which):
    """lockstep_carve_adjoint as tests/lockstep_back_ref.py names it (ADJV): three n x 64 vectors, three m x 64 vectors, the packed int codes"""
    for n, m, r in cases(which):
        ranges, end, fits, _ = carve(lib, which, n, m, r)
        adj = ranges[-7:]
        assert [c for _, c in adj] == [n * W] * 3 + [m * W] * 3 + [(m * W + 1) // 2], (n, m, r)
        assert all(o + c == o2 for (o, c), (o2, _) in zip(adj, adj[1:])) and sum(adj[-1]) == end <= size(lib, which, n, m, r)


def test_polish_carve_is_x_y_z_l_u_back_to_back(lib):
    """lockstep_carve_polish as tests/lockstep_back_ref.py names it (POLV): the saved x (n x 64), then y, z, l, u (m x 64 each), from offset 0"""
    for n, m, _ in cases(POLISH):
        ranges, end, fits, _ = carve(lib, POLISH, n, m)
        assert ranges == [(0, n * W)] + [(n * W + k * m * W, m * W) for k in range(4)] and fits and end == W * (n + 4 * m) <= size(lib, POLISH, n, m)


def test_scalar_state_sits_at_lockstep_sc_offset_and_c_in_its_row(lib):
    scal, c_row = lib.ll_const(2), lib.ll_const(4)
    for n, m in itertools.product(NS, MS):
        ranges, _, _, sc = carve(lib, FORWARD, n, m)
        assert sc == lib.ll_sc_offset(n, m)
        assert (sc, scal * W) in ranges                                           # the scalar state: kLsScal rows
        assert c_row + 1 < scal                                                   # c and 1 / c (kLsMatScalC, + 1) are rows of it: sc + 11 * 64
        parti = [c for o, c in ranges if o + c == sc and c > 0][-1]
        assert parti == max(1, (m + 63) // 64) * W                                # one row per tile of m; m = 0 still reserves one
    for n, m, r in cases(DIRECT):                                                 # the direct route's own order keeps the block in one piece too
        ranges, _, _, sc = carve(lib, DIRECT, n, m, r)
        assert (sc, scal * W) in ranges and ranges[0] == (0, (n + r) * W)         # x has n + r rows there


def test_m0_reserves_one_parti_row(lib):
    for n in NS:
        ranges, _, _, sc = carve(lib, FORWARD, n, 0)
        assert (sc - W, W) in ranges
