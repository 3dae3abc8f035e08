"""CPU guard on the gfx950 ISA of the E/F step's hot kernels (no GPU needed; skipped without hipcc).

duet_ef.hip is compiled for gfx950 to assembly (device code only, the library's flags) into a temporary directory, and the
kernel-resource remarks and the instruction stream are read as text:

* ScratchSize is 0 for ef_finalize_own and every ef_classify instance: a register array indexed at run time, or a call, puts
  values in scratch memory, and each such value is one more dependent memory round trip;
* ef_finalize_own makes no call (no ``s_swappc``);
* ef_finalize_own's first trip is one trip: between its first ``s_waitcnt vmcnt`` and the barrier that runs first -- the
  ``s_barrier`` after the hash set's clear (the first ``ds_write2st64_b32``; the compiler places the loop latch's barrier, which
  runs later, above it in the text) -- no column or summary load is issued.  The only loads allowed there are the sixteen-byte
  loads of the seed records of a tile's second contig (at most 2 x kPre x 2 of them), which the contig loop fetches again; what
  the tile's first contig needs, records included, left before the first wait.

The matching is plain: a kernel is the text from its label to its ``.Lfunc_end`` marker, and an instruction is recognised by its
mnemonic at the start of a line.
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'duet_amd', 'csrc')
HIPCC = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)

pytestmark = pytest.mark.skipif(HIPCC is None, reason='hipcc not found')

FINALIZE_OWN = '_ZN12_GLOBAL__N_115ef_finalize_ownENS_6ParamsE'
CLASSIFY = ['_ZN12_GLOBAL__N_111ef_classifyILb%dELb%dEEEvNS_6ParamsE' % (v, d) for v in (1, 0) for d in (0, 1)]


@pytest.fixture(scope='module')
def isa(tmp_path_factory):
    out = tmp_path_factory.mktemp('isa')
    asm = str(out / 'duet_ef.s')
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fvisibility=hidden',
           '-Wno-unused-function', '-I' + os.path.join(REPO, 'include'), '--cuda-device-only', '-S',
           '-Rpass-analysis=kernel-resource-usage', os.path.join(CSRC, 'duet_ef.hip'), '-o', asm]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    with open(asm) as f:
        text = f.read()
    return text, r.stderr


def scratch_size(remarks, name):
    m = re.search(r'Function Name: %s \[.*?\n(?:.*\n){0,8}?.*ScratchSize \[bytes/lane\]: (\d+)' % re.escape(name), remarks)
    assert m, 'no resource remark for ' + name
    return int(m.group(1))


def kernel_lines(text, name):
    start = re.search(r'^%s:' % re.escape(name), text, re.M).start()
    end = text.index('.Lfunc_end', start)
    return [l.strip() for l in text[start:end].split('\n')]


@pytest.mark.parametrize('name', [FINALIZE_OWN] + CLASSIFY)
def test_no_scratch(isa, name):
    assert scratch_size(isa[1], name) == 0


def test_finalize_own_makes_no_call(isa):
    assert not any(l.startswith('s_swappc') for l in kernel_lines(isa[0], FINALIZE_OWN))


def test_finalize_own_first_trip_is_one_trip(isa):
    lines = kernel_lines(isa[0], FINALIZE_OWN)
    first_wait = next(i for i, l in enumerate(lines) if re.match(r's_waitcnt\b.*\bvmcnt\(', l))
    clear = next(i for i, l in enumerate(lines) if l.startswith('ds_write2st64_b32'))
    barrier = next(i for i in range(clear, len(lines)) if lines[i].startswith('s_barrier'))
    assert first_wait < clear < barrier
    late = [l for l in lines[first_wait:barrier] if l.startswith('global_load')]
    assert all(l.startswith('global_load_dwordx4') for l in late), late
    assert len(late) <= 8, late
    # ... and that one trip carries the records and the summaries (sixteen-byte and eight-byte loads)
    early = [l for l in lines[:first_wait] if l.startswith('global_load')]
    assert sum(l.startswith('global_load_dwordx4') for l in early) >= 8
    assert sum(l.startswith('global_load_dwordx2') for l in early) >= 2
