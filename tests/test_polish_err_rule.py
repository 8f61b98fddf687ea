"""CPU tier: the error measure of the polish recurrence (osqp-python_amd/csrc/term_rules.h recurrence_err_polish: Engine::run_recurrence on the host,
lockstep_hip.hip k_ls_pol_decide per problem on the device), behind tests/hostsim/polish_err_probe.cpp, on hand-made values.  What is expected restates
the formula:  max(pri / (max(ax, z) + 1e-30), dua / (max(aty, px, qn) + 1e-30))  -- every operation is one rounding, so the values are compared exactly."""
import ctypes as C
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'hostsim', 'polish_err_probe.cpp')
OUT = os.path.join(ROOT, 'tests', '_build', 'libpolish_err_probe.so')
DEPS = [SRC, os.path.join(ROOT, 'osqp-python_amd', 'csrc', 'term_rules.h')]


@pytest.fixture(scope='module')
def lib():
    if not (os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(f) for f in DEPS)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'include'), '-o', OUT, SRC])
    L = C.CDLL(OUT)
    L.pe_err.argtypes = [C.c_double] * 7; L.pe_err.restype = C.c_double
    return L


def ref(pri, ax, z, dua, aty, px, qn):
    return max(pri / (max(ax, z) + 1e-30), dua / (max(max(aty, px), qn) + 1e-30))


#                 pri   ax   z    dua  aty  px   qn
CASES = {
    'primal side decides, A x is the larger product': (3.0, 8.0, 4.0, 1.0, 16.0, 2.0, 1.0),
    'primal side decides, z is the larger product': (3.0, 4.0, 8.0, 1.0, 16.0, 2.0, 1.0),
    "dual side decides, A' y is the largest term": (1.0, 16.0, 2.0, 3.0, 8.0, 4.0, 2.0),
    'dual side decides, P x is the largest term': (1.0, 16.0, 2.0, 3.0, 4.0, 8.0, 2.0),
    'dual side decides, q is the largest term': (1.0, 16.0, 2.0, 3.0, 4.0, 2.0, 8.0),
    'no constraint rows: the primal quotient is 0 / 1e-30': (0.0, 0.0, 0.0, 3.0, 0.0, 7.0, 5.0),
    'equal quotients': (1.0, 2.0, 2.0, 2.0, 4.0, 4.0, 4.0),
    'zero products under a nonzero residual': (1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
}


@pytest.mark.parametrize('name', list(CASES))
def test_error_measure(lib, name):
    v = CASES[name]
    got, exp = lib.pe_err(*v), ref(*v)
    assert got == exp, (got, exp)


def test_each_branch_is_taken(lib):
    """the hand-made expectations, written out: the cases above do select the operand their names say"""
    assert lib.pe_err(*CASES['primal side decides, A x is the larger product']) == 3.0 / (8.0 + 1e-30)
    assert lib.pe_err(*CASES['primal side decides, z is the larger product']) == 3.0 / (8.0 + 1e-30)
    for k in ("dual side decides, A' y is the largest term", 'dual side decides, P x is the largest term', 'dual side decides, q is the largest term'):
        assert lib.pe_err(*CASES[k]) == 3.0 / (8.0 + 1e-30)
    assert lib.pe_err(*CASES['zero products under a nonzero residual']) == 1.0 / 1e-30


def test_all_zeros(lib):
    assert lib.pe_err(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0) == 0.0


def test_nan(lib):
    """The selects are std::max's, which the expression had on the host before it moved here: (a < b) ? b : a keeps a NaN in its FIRST operand and drops one
    in its second.  A NaN primal residual or A x therefore makes the error NaN (no progress for recurrence_ends); a NaN dual residual or z leaves the value
    of the finite operands -- where it always went."""
    nan = float('nan')
    assert math.isnan(lib.pe_err(nan, 2.0, 2.0, 2.0, 4.0, 4.0, 4.0))
    assert math.isnan(lib.pe_err(1.0, nan, 2.0, 2.0, 4.0, 4.0, 4.0))
    assert lib.pe_err(1.0, 2.0, 2.0, nan, 4.0, 4.0, 4.0) == 1.0 / (2.0 + 1e-30)
    assert lib.pe_err(1.0, 2.0, nan, 0.0, 4.0, 4.0, 4.0) == 1.0 / (2.0 + 1e-30)
    for v in ((nan, 2.0, 2.0, 2.0, 4.0, 4.0, 4.0), (1.0, 2.0, 2.0, nan, 4.0, 4.0, 4.0), (1.0, 2.0, 2.0, 2.0, nan, 4.0, 4.0), (1.0, 2.0, 2.0, 2.0, 4.0, 4.0, nan)):
        got, exp = lib.pe_err(*v), ref(*v)                  # (python's max has the same select)
        assert got == exp or (math.isnan(got) and math.isnan(exp)), (v, got, exp)
