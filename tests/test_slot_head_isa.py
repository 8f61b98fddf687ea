"""CPU tier: the F1 slot kernel's code object, compiled here with the project's own rule for pcg_hip.o (hipcc cross-compiles for gfx950
without a GPU).  For every k_slot1 instantiation: its head arrives in preloaded kernel-argument SGPRs (preload length > 0), no scratch,
four waves per SIMD, and the order of the head: the first block's stream leaves before any scalar load or wait, and the records go out
ahead of the first wait.  A change that silently loses the preload (a by-value struct argument, a dropped Makefile flag), puts a memory
round trip in front of the first request again or pushes the kernel into scratch fails here, before any GPU time."""
import os
import re
import shlex
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'osqp-python_amd')
OUT = os.path.join(ROOT, 'tests', '_build', 'pcg_hip_gfx950.s')
DEPS = [os.path.join(PKG, 'Makefile')] + [os.path.join(PKG, 'csrc', f) for f in ('pcg_hip.hip', 'hip_common.h', 'backend.h', 'policy.h')]


def _compile_command():
    # the command `make` would run for the object (-B: as if out of date, -n: print it only), turned into a device-only assembly listing
    out = subprocess.check_output(['make', '-s', '-B', '-n', '-C', PKG, 'build/obj/pcg_hip.o'], text=True)
    cmd = next(shlex.split(line) for line in out.splitlines() if 'hipcc' in line and 'pcg_hip.hip' in line)
    o = cmd.index('-o')
    del cmd[o:o + 2]
    cmd.remove('-c')
    return cmd + ['--cuda-device-only', '-S', '-o', OUT]


@pytest.fixture(scope='module')
def listing():
    if not (os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(f) for f in DEPS)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.check_call(_compile_command(), cwd=PKG)
    with open(OUT) as f:
        return f.read()


def test_compile_command_carries_the_preload_flag():
    assert '-amdgpu-kernarg-preload-count=16' in _compile_command()


def test_every_slot_kernel_has_a_preloaded_head(listing):
    # one segment per kernel: its descriptor (.amdhsa_kernel ... .end_amdhsa_kernel) and the resource comments that follow it
    parts = re.split(r'^\s*\.amdhsa_kernel\s+', listing, flags=re.M)[1:]
    slots = {p.split(None, 1)[0]: p for p in parts if '7k_slot1I' in p.split(None, 1)[0]}
    assert len(slots) == 16, sorted(slots)                  # D = 1..4 x MIX x WT
    for name, seg in slots.items():
        preload = int(re.search(r'\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)', seg).group(1))
        scratch = int(re.search(r'^; ScratchSize: (\d+)', seg, re.M).group(1))
        occ = int(re.search(r'^; Occupancy: (\d+)', seg, re.M).group(1))
        assert preload > 0, (name, preload)
        assert scratch == 0, (name, scratch)
        assert occ == 4, (name, occ)


def _heads(listing):
    # the instructions of every k_slot1 from its real entry: the 256-byte aligned label behind the compatibility prologue (which loads the
    # arguments for firmware without preloading and branches over the alignment padding)
    out = {}
    for m in re.finditer(r'^(_ZN\S*7k_slot1I\S*):', listing, re.M):
        body = listing[m.end():listing.index('.Lfunc_end', m.end())].splitlines()
        entry = next(k for k, line in enumerate(body) if re.match(r'\s*\.p2align\s+8\b', line))
        out[m.group(1)] = [line.strip() for line in body[entry + 1:]
                           if line.strip() and not line.strip().startswith((';', '.')) and not line.strip().endswith(':')]
    return out


def test_slot_head_issues_the_stream_before_any_wait(listing):
    heads = _heads(listing)
    assert len(heads) == 16, sorted(heads)
    for name, ins in heads.items():
        first_lds = next(k for k, op in enumerate(ins) if op.startswith('global_load_lds_dwordx4'))
        first_wait = next(k for k, op in enumerate(ins) if op.startswith('s_waitcnt') and 'lgkmcnt' in op)
        # nothing fetched (from Dev or anywhere else) and nothing waited for before the first block's stream goes out
        assert not [op for op in ins[:first_lds] if op.startswith(('s_load', 's_buffer_load', 's_waitcnt'))], (name, ins[:first_lds])
        early = [op.split()[0] for op in ins[:first_wait] if op.startswith('s_load')]
        assert 's_load_dwordx8' in early, (name, early)       # the slot record
        mix = re.search(r'k_slot1ILi\dELb([01])ELb[01]E', name).group(1) == '1'
        if not mix:                                           # the forms without far columns (configs[1] among them): the first block record too
            assert 's_load_dwordx16' in early, (name, early)
