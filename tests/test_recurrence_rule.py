"""CPU tier: the progress rule of the recurrence polish and the adjoint derivatives run (osqp-python_amd/csrc/term_rules.h recurrence_ends /
recurrence_err_rhs: Engine::run_recurrence on the host, lockstep_hip.hip k_ls_adj_decide per problem on the device), behind
tests/hostsim/recurrence_probe.cpp, on hand-made error sequences.  What is expected restates the rule from its description: a step that does not bring
the error below gain * best counts as no progress; the recurrence ends after at least min_steps when the error is below 1e-13 or two steps in a row
showed no progress, and at max_steps at the latest."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'hostsim', 'recurrence_probe.cpp')
OUT = os.path.join(ROOT, 'tests', '_build', 'librecurrence_probe.so')
DEPS = [SRC, os.path.join(ROOT, 'osqp-python_amd', 'csrc', 'term_rules.h')]


@pytest.fixture(scope='module')
def lib():
    if not (os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(f) for f in DEPS)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'include'), '-o', OUT, SRC])
    L = C.CDLL(OUT)
    L.rr_run.argtypes = [C.POINTER(C.c_double), C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]; L.rr_run.restype = C.c_int
    L.rr_err.argtypes = [C.c_double] * 4; L.rr_err.restype = C.c_double
    return L


def run(lib, errs, gain=0.9, min_steps=4, max_steps=60):
    best, worse = C.c_double(), C.c_int()
    ended = lib.rr_run((C.c_double * len(errs))(*errs), len(errs), gain, min_steps, max_steps, C.byref(best), C.byref(worse))
    return ended, best.value, worse.value


def ref(errs, gain, min_steps, max_steps):
    best, worse = float('inf'), 0
    for s, e in enumerate(errs, 1):
        worse = 0 if e < gain * best else worse + 1
        best = min(best, e)
        if (s >= min_steps and (e < 1e-13 or worse >= 2)) or s >= max_steps:
            return s, best, worse
    return 0, best, worse


CASES = {
    'minimum steps: a negligible error at step 1 still takes min_steps': ([1e-14, 1e-15, 1e-16, 1e-17, 1e-18], 0.9, 4, 60, 4),
    'minimum steps: two stalls before min_steps end it at min_steps': ([1.0, 1.0, 1.0, 1.0, 1.0], 0.9, 4, 60, 4),
    'two stalls in a row': ([1.0, 0.5, 0.25, 0.125, 0.06, 0.058, 0.057, 0.01], 0.9, 4, 60, 7),
    'one stall, then progress, resets the count': ([1.0, 0.5, 0.25, 0.125, 0.12, 0.05, 0.049, 0.02, 0.019, 0.0185], 0.9, 4, 60, 10),
    'err < 1e-13': ([1.0, 1e-3, 1e-6, 1e-9, 1e-12, 9e-14, 1e-20], 0.9, 4, 60, 6),
    'exactly 1e-13 is not below it': ([1.0, 1e-3, 1e-6, 1e-9, 1e-13, 1e-14], 0.9, 4, 60, 6),
    'the cap': ([0.8 ** k for k in range(70)], 0.9, 4, 60, 60),
    'the cap below min_steps still ends': ([0.5 ** k for k in range(10)], 0.9, 8, 5, 5),
    "polish's gain: a step that does not halve the error is no progress": ([1.0, 0.6, 0.4, 0.1], 0.5, 1, 30, 3),
    'a NaN error is no progress': ([1.0, float('nan'), float('nan'), 0.1], 0.9, 1, 60, 3),
    'never ends within the sequence': ([1.0, 0.5, 0.25], 0.9, 4, 60, 0),
}


@pytest.mark.parametrize('name', list(CASES))
def test_recurrence_rule(lib, name):
    errs, gain, min_steps, max_steps, want = CASES[name]
    got = run(lib, errs, gain, min_steps, max_steps)
    exp = ref(errs, gain, min_steps, max_steps)
    assert exp[0] == want, exp                      # (the hand-made expectation and the restated rule agree)
    assert got[0] == want and got[2] == exp[2], (got, exp)
    assert got[1] == exp[1] or (got[1] != got[1] and exp[1] != exp[1]), (got, exp)


def test_error_measure(lib):
    assert lib.rr_err(2.0, 1.0, 4.0, 8.0) == 2.0 / (8.0 + 1e-30)
    assert lib.rr_err(1.0, 3.0, 4.0, 2.0) == 3.0 / (4.0 + 1e-30)
    assert lib.rr_err(0.0, 0.0, 0.0, 0.0) == 0.0
    assert lib.rr_err(1.0, 1.0, 0.0, 0.0) == 1.0 / 1e-30
