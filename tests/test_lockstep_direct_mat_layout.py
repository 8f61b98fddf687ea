"""CPU tier: the block of a direct lockstep chunk with per-problem matrices (osqp-python_amd/csrc/lockstep_layout.h lockstep_direct_mat_layout /
lockstep_direct_mat_ws_doubles) behind tests/hostsim/direct_mat_layout_probe.cpp, with the COUNTING cursor: no memory is touched.  The carve must end
inside its size function, keep its ranges disjoint and 64-double aligned, begin with the matrix block exactly as ls_mat_block carves it from the same
base, and match the closed form restated here: 64 (nnz(A) + nnz(B) + 2 n + 2 m + n r + nv) + 128 doubles."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'hostsim', 'direct_mat_layout_probe.cpp')
DEPS = [SRC, os.path.join(ROOT, 'osqp-python_amd', 'csrc', 'lockstep_layout.h')]
OUT = os.path.join(ROOT, 'tests', '_build', 'libdirect_mat_layout_probe.so')
NS, MS, RS = (1, 63, 64, 65, 604, 2020, 2127), (1, 64, 65, 605, 2021), (1, 5, 21, 128)
W = 64


@pytest.fixture(scope='module')
def lib():
    if not (os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(f) for f in DEPS)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Wextra', '-shared', '-fPIC', '-o', OUT, SRC])
    L = C.CDLL(OUT)
    SP = C.POINTER(C.c_size_t)
    L.dm_carve.argtypes = [C.c_void_p] + [C.c_int] * 6 + [SP, SP]; L.dm_carve.restype = C.c_int
    L.dm_size.argtypes = [C.c_int] * 6; L.dm_size.restype = C.c_size_t
    L.dm_carve_mat.argtypes = [C.c_int] * 4 + [SP, SP]; L.dm_carve_mat.restype = C.c_int
    L.dm_size_mat.argtypes = [C.c_int] * 4; L.dm_size_mat.restype = C.c_size_t
    L.dm_const.argtypes = [C.c_int]; L.dm_const.restype = C.c_int
    assert L.dm_const(0) == W
    return L


def shape(n, m, r):
    """nnz(A), nnz(B), entries of the view for a factor-model shape: r dense rows over n columns, m - r one-entry rows"""
    nzA = r * n + max(m - r, 0)
    return nzA, nzA + n, max(m - r, 0) + min(r, m)


def carve(lib, n, m, r):
    cap = lib.dm_const(1)
    ranges, info = (C.c_size_t * (2 * cap))(), (C.c_size_t * 4)()
    k = lib.dm_carve(None, n, m, r, *shape(n, m, r), ranges, info)
    assert 0 < k <= cap
    return [(ranges[2 * q], ranges[2 * q + 1]) for q in range(k)], info[0], bool(info[1])


CASES = list(itertools.product(NS, MS, RS))


def test_size_function_matches_the_closed_form(lib):
    for n, m, r in CASES:
        nzA, nzB, nv = shape(n, m, r)
        assert lib.dm_size(n, m, r, nzA, nzB, nv) == W * (nzA + nzB + 2 * n + 2 * m + n * r + nv) + 128, (n, m, r)
        assert lib.dm_size_mat(n, m, nzA, nzB) == W * (nzA + nzB + 2 * n + 2 * m) + 64                  # (what it always was)
    nzA, nzB, nv = shape(2020, 2021, 21)
    assert 512 * 2020 * 21 == 21719040                                                                  # the dense rows at portfolio_qp(2000, 20): 22 MB
    assert 8 * lib.dm_size(2020, 2021, 21, nzA, nzB, nv) < 80e6


def test_carve_fits_is_disjoint_and_aligned(lib):
    for n, m, r in CASES:
        nzA, nzB, nv = shape(n, m, r)
        ranges, end, fits = carve(lib, n, m, r)
        assert fits and end <= lib.dm_size(n, m, r, nzA, nzB, nv), (n, m, r)
        assert max(o + c for o, c in ranges) == end
        assert all(o % 64 == 0 for o, _ in ranges), (n, m, r)
        live = sorted((o, c) for o, c in ranges if c > 0)
        assert all(a + ca <= b for (a, ca), (b, _) in zip(live, live[1:])), (n, m, r)
        assert [c for _, c in ranges[-2:]] == [n * r * W, nv * W]                                        # the dense rows, then the view's values


def test_the_matrix_block_comes_first_as_ls_mat_block_carves_it(lib):
    cap = lib.dm_const(1)
    for n, m, r in CASES:
        nzA, nzB, nv = shape(n, m, r)
        ranges, _, _ = carve(lib, n, m, r)
        mr, mi = (C.c_size_t * (2 * cap))(), (C.c_size_t * 4)()
        k = lib.dm_carve_mat(n, m, nzA, nzB, mr, mi)
        mat = [(mr[2 * q], mr[2 * q + 1]) for q in range(k)]
        assert mi[1] == 1 and k == 6 and ranges[:k] == mat and len(ranges) == k + 2, (n, m, r)
        assert ranges[k][0] == mi[0]                                                                     # the dense rows start where the matrix block's carve ends
