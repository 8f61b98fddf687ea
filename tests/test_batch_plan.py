"""CPU tier: the batch path's launch plan (osqp-python_amd/csrc/batch_plan.cpp, behind tests/hostsim/batch_plan_probe.cpp) and the width checks of
hip_batch_solve, which run before the C call (through the host simulator: its batch entry point declines, the checks come first)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import osqp_amd
import problems
from osqp_amd import ext_hip
from hostsim_util import hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'osqp-python_amd', 'csrc')
SRCS = [os.path.join(ROOT, 'tests', 'hostsim', 'batch_plan_probe.cpp'), os.path.join(CSRC, 'batch_plan.cpp')]
OUT = os.path.join(ROOT, 'tests', '_build', 'libbatch_plan_probe.so')
DEPS = SRCS + [os.path.join(CSRC, 'backend.h'), os.path.join(CSRC, 'band_ldl.h')]
NO_SPEC, SPEC_WORKGROUP, SPEC_WAVE = 0, 1, 2                 # BatchPlan::Spec
FIELDS = ('spec', 'split', 'variant', 'e', 'spec_e', 'spec_w', 'split_w', 'n8', 'wgs', 'wgs_all')


@pytest.fixture(scope='module')
def plan():
    if not (os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(f) for f in DEPS)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-o', OUT] + SRCS)
    L = C.CDLL(OUT)
    L.bpp_plan.argtypes = [C.c_int] * 12 + [C.POINTER(C.c_int)]

    def run(n=120, m=240, nnz=1292, bw=20, nbatch=4096, spectral=1, wave=1, order=1, wv_split=48, wv_cus=16, wide_rounds=1 << 20, cus=256):
        out = (C.c_int * len(FIELDS))()
        L.bpp_plan(n, m, nnz, bw, nbatch, spectral, wave, order, wv_split, wv_cus, wide_rounds, cus, out)
        return dict(zip(FIELDS, out))
    return run


def test_plan_of_the_mpc_batch(plan):
    p = plan()                                # (the MPC batch's shape: n = 120, m = 240, 1292 products)
    assert (p['spec'], p['split'], p['variant'], p['e'], p['spec_e'], p['n8']) == (SPEC_WAVE, 48, 2, 6, 6, 120)
    assert (p['wgs'], p['wgs_all'], p['spec_w'], p['split_w']) == (240, 256, 1, 1)
    assert plan(wave=0)['spec'] == SPEC_WORKGROUP and plan(spectral=0, wave=0)['spec'] == NO_SPEC
    assert plan(wide_rounds=1)['spec_w'] == 2 and plan(wide_rounds=0)['split_w'] == 2


def test_plan_split_rules(plan):
    assert plan(order=0)['split'] == 0                       # no launch order
    assert plan(nbatch=8 * 48 - 1)['split'] == 0             # nbatch < 8 split
    assert plan(nbatch=8 * 48)['split'] == 48
    assert plan(cus=32, wv_cus=16)['split'] == 0             # cus <= 2 wv_cus
    assert plan(cus=33, wv_cus=16)['split'] == 48
    for kw in (dict(order=0), dict(nbatch=300), dict(cus=32)):
        p = plan(**kw)
        assert p['spec'] == SPEC_WAVE and p['wgs'] == p['wgs_all'] == min(kw.get('cus', 256), kw.get('nbatch', 4096))


def test_plan_without_spectral_stage(plan):
    p = plan(nnz=2100)                                       # e256 = 9 > 8: the banded kernel alone, its E = 16 instantiation
    assert (p['spec'], p['variant'], p['e']) == (NO_SPEC, 2, 16)
    assert plan(nnz=500)['spec'] == NO_SPEC                  # too few products for the spectral form's scratch (prod_len < 4 (kBatchSpecN + 2))
    assert plan(bw=-1)['spec'] == NO_SPEC and plan(bw=-1)['variant'] == 3      # no direct form: the PCG kernel with one wave


def test_batch_solve_checks_widths():
    P, q, A, l, u = problems.random_qp(30, 50, density=0.15, seed=5)
    n, m, B = P.shape[0], A.shape[0], 4
    L, U = np.tile(l, (B, 1)), np.tile(u, (B, 1))
    Pfull = (P + sp.triu(P, 1).T).tocsc()
    assert Pfull.nnz > sp.triu(P).nnz
    with hostsim():
        s = osqp_amd.OSQP(algebra='hip')
        s.setup(P, q, A, l, u, verbose=False)
        solver = s._solver
        good = dict(q=np.tile(q, (B, 1)), l=L, u=U, x0=np.zeros((B, n)), y0=np.zeros((B, m)),
                    Px=np.tile(sp.triu(P, format='csc').data, (B, 1)), Ax=np.tile(A.tocsc().data, (B, 1)))
        widths = dict(q=n, l=m, u=m, x0=n, y0=m, Px=sp.triu(P).nnz, Ax=A.nnz)
        for name, a in good.items():
            bad = dict(good)
            bad[name] = np.zeros((B, widths[name] + 1))
            with pytest.raises(ValueError, match=r'^%s: expected %d problems of width %d' % (name, B, widths[name])):
                solver.hip_batch_solve(**bad)
        with pytest.raises(ValueError, match=r'^Px: expected'):                    # the full P instead of its upper triangle
            solver.hip_batch_solve(Px=np.tile(Pfull.data, (B, 1)), Ax=good['Ax'])
        with pytest.raises(ValueError, match=r'^l: expected'):                     # nbatch below the arrays' rows
            solver.hip_batch_solve(l=L, u=U, nbatch=B - 1)
        for kw in (dict(l=L, u=U), dict(Px=good['Px'], Ax=good['Ax'])):          # right widths: the call reaches the engine (which declines here)
            with pytest.raises(ValueError) as e:
                solver.hip_batch_solve(**kw)
            assert e.value.code == ext_hip.osqp_error_type.OSQP_FUNC_NOT_IMPLEMENTED
