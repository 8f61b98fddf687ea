"""CPU tier: the scalar fold of the F1 form's launches in the code object, compiled here with the project's own rule for pcg_hip.o (the command
test_slot_head_isa.py takes from `make -n`, a listing of its own).

f1_fold_finish<true> (f1_iteration) fetches the PCG tolerance, gamma_{k-2} and alpha_{k-2} with scalar loads: as vector loads they queue behind the
launch's partials and its first stream, and the fold ends a round trip late.  What is checked:
  * every k_slot1 and k_f1_probe instantiation: no scratch, four waves per SIMD;
  * k_f1_probe<4, false, true>, which holds phase F alone: between the requests of the previous launch's partials (six global_load_dwordx4) and the
    first s_barrier -- the fold's block reduction -- stands no global_load_dwordx2 and at least three s_load_dwordx2.  The parent's listing has three
    global_load_dwordx2 and no s_load_dwordx2 there, so the marker separates the two builds.  (The marker first meant for this file -- 4 + D
    buffer_load_dwordx2, the first block's window requests, in front of that barrier -- belongs to the form that was measured and dropped, the
    requests ahead of the fold: DESIGN.md section 4.2 "The fold's scalars as scalar loads".)
  * no block loop starts with `s_waitcnt vmcnt(0)` as its first vector-memory wait: such a wait sits out the next block's stream and the previous
    block's stores (the rules above f1_body).  A block loop is a loop of depth 1 that requests a stream (global_load_lds_dwordx4); every k_slot1
    shows five in its listing and every k_f1_probe two, except k_slot1<4, true, false> (three) and k_f1_probe<4, true, false> (one), and each
    kernel is held to its count, so that no loop drops out of the check unseen.  All 32 kernels are checked.  The four kernels with far columns
    and four replicas -- k_slot1<4, true, *>, k_f1_probe<4, true, *> -- have ONE loop with such a wait in the parent's listing too, identical
    there and here: at most that one is let through in those four; the twelve <1..3, true, *> kernels and the sixteen without far columns
    have none and may have none."""
import os
import re
import subprocess

import pytest

import test_slot_head_isa as head

OUT = os.path.join(head.ROOT, 'tests', '_build', 'pcg_hip_fold_gfx950.s')


@pytest.fixture(scope='module')
def listing():
    if not (os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(f) for f in head.DEPS)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        cmd = head._compile_command()
        cmd[cmd.index('-o') + 1] = OUT
        subprocess.check_call(cmd, cwd=head.PKG)
    with open(OUT) as f:
        return f.read()


def _kernels(listing, which):
    """name -> (instructions and labels of the function, its descriptor and resource comments)"""
    desc = {p.split(None, 1)[0]: p for p in re.split(r'^\s*\.amdhsa_kernel\s+', listing, flags=re.M)[1:]}
    out = {}
    for m in re.finditer(r'^(_ZN\S*%s\S*):' % which, listing, re.M):
        body = listing[m.end():listing.index('.Lfunc_end', m.end())].splitlines()
        out[m.group(1)] = ([line.strip() for line in body if line.strip() and not line.strip().startswith(';')], desc[m.group(1)])
    return out


def test_no_scratch_and_four_waves_in_every_instantiation(listing):
    for which, count in (('7k_slot1I', 16), ('10k_f1_probeI', 16)):      # D = 1..4 x MIX x WT
        ks = _kernels(listing, which)
        assert len(ks) == count, sorted(ks)
        for name, (_, seg) in ks.items():
            scratch = int(re.search(r'^; ScratchSize: (\d+)', seg, re.M).group(1))
            occ = int(re.search(r'^; Occupancy: (\d+)', seg, re.M).group(1))
            vgprs = int(re.search(r'^; NumVgprs: (\d+)', seg, re.M).group(1))
            lds = int(re.search(r'^; LDSByteSize: (\d+)', seg, re.M).group(1))
            assert scratch == 0 and occ == 4 and vgprs <= 128 and lds == 39008, (name, scratch, occ, vgprs, lds)


def test_fold_scalars_arrive_as_scalar_loads(listing):
    ks = _kernels(listing, r'10k_f1_probeILi4ELb0ELb1E')
    assert len(ks) == 1, sorted(ks)
    (ins, _), = ks.values()
    parts = [k for k, op in enumerate(ins) if op.startswith('global_load_dwordx4')]
    barrier = next(k for k, op in enumerate(ins) if op.startswith('s_barrier'))
    assert len([k for k in parts if k < barrier]) == 6, parts     # three slots of kGrid partials, two 16-byte loads per lane each
    fold = ins[max(k for k in parts if k < barrier) + 1:barrier]
    vec = [op for op in fold if op.startswith(('global_load', 'buffer_load', 'flat_load'))]
    sca = [op for op in fold if op.startswith('s_load_dwordx2')]
    print('between the partials and the first barrier: vector loads %r, scalar 8-byte loads %d' % (vec, len(sca)))
    assert not vec, vec
    assert len(sca) >= 3, sca


def _block_loops(ins):
    """[(header label, index of the header in ins)] of the depth-1 loops that request a stream.  The members of a loop are read from the compiler's
    block comments: `in Loop: Header=BBn_m` on a member, `Parent Loop BBn_m` on the header of a loop nested in it (whose members name only that inner
    header: followed transitively)."""
    label = re.compile(r'^(\.LBB\d+_\d+):\s*(;.*)?$')
    blocks, cur = [], None                                   # (label, comment, first index, ops)
    for k, op in enumerate(ins):
        m = label.match(op)
        if m:
            cur = [m.group(1), m.group(2) or '', k, []]
            blocks.append(cur)
        elif cur is not None:
            cur[3].append(op)
    out = []
    for lab, com, k, ops in blocks:
        if 'Loop Header: Depth=1' not in com:
            continue
        heads, grew = {lab[2:]}, True                        # BBn_m as the comments name it
        while grew:
            grew = False
            for b in blocks:
                if b[0][2:] not in heads and 'Loop Header' in b[1] and any(re.search(r'Parent Loop %s\b' % re.escape(h), b[1]) for h in heads):
                    heads.add(b[0][2:])
                    grew = True
        members = [b for b in blocks if b[0][2:] in heads or any(re.search(r'Header=%s\b' % re.escape(h), b[1]) for h in heads)]
        if any(op.startswith('global_load_lds_dwordx4') for b in members for op in b[3]):
            out.append((lab, k))
    return out


def test_no_block_loop_starts_with_a_full_vector_memory_wait(listing):
    seen = 0
    for which, least in (('7k_slot1I', 5), ('10k_f1_probeI', 2)):      # k_slot1: the chunk start, F_0, F_k and KA's two sites; the probe: F_0 and F_k
        ks = _kernels(listing, which)
        assert len(ks) == 16, sorted(ks)
        for name, (ins, _) in sorted(ks.items()):
            D, mix, wt = re.search(r'(?:k_slot1|k_f1_probe)ILi(\d)ELb([01])ELb([01])E', name).groups()
            loops = _block_loops(ins)
            waits = [next(op for op in ins[k:] if op.startswith('s_waitcnt') and 'vmcnt' in op) for _, k in loops]
            full = [(lab, w) for (lab, _), w in zip(loops, waits) if re.search(r'vmcnt\(0\)', w)]
            print('%s<%s, %s, %s>: %d block loops, first waits %s' % (which.lstrip('0123456789')[:-1], D, mix == '1', wt == '1', len(loops), ' '.join(waits)))
            seen += len(loops)
            # every kernel's loops are found (a loop that drops out of the census is not checked): the <4, true, false> kernels show fewer in the
            # listing -- 3 and 1 -- and are held to that
            assert len(loops) >= ((3 if which == '7k_slot1I' else 1) if (D, mix, wt) == ('4', '1', '0') else least), (name, loops)
            # the one such wait the parent has as well: one loop of each <4, true, *> kernel; nowhere else
            assert len(full) <= (1 if (D, mix) == ('4', '1') else 0), (name, full)
    print('%d block loops checked' % seen)
