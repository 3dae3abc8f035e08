"""CPU guard on the gfx950 ISA of ef_finalize_own_wide, the two-tiles-per-workgroup instance of ef_finalize_own's body (no GPU
needed; skipped without hipcc) -- in the manner of tests/test_isa_hot_kernels.py, with the same compile line:

* ScratchSize is 0 and the kernel makes no call (no ``s_swappc``): the body is shared with ef_finalize_own, and neither the wider
  per-wavefront LDS slots nor own_sort_set's thread-count parameter may bring a stack;
* its first trip is one trip: between the first ``s_waitcnt vmcnt`` and the barrier that runs first -- the ``s_barrier`` behind the
  hash set's clear (the first ``ds_write2st64_b32``) -- no load is issued other than the sixteen-byte loads of the seed records of
  a second contig, which the contig loop fetches again.
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

WIDE = '_ZN12_GLOBAL__N_120ef_finalize_own_wideENS_6ParamsE'


@pytest.fixture(scope='module')
def isa(tmp_path_factory):
    out = tmp_path_factory.mktemp('isa_wide')
    asm = str(out / 'duet_ef.s')
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fvisibility=hidden',
           '-Wno-unused-function', '-I' + os.path.join(REPO, 'include'), '--cuda-device-only', '-S',
           '-Rpass-analysis=kernel-resource-usage', os.path.join(CSRC, 'duet_ef.hip'), '-o', asm]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    with open(asm) as f:
        text = f.read()
    return text, r.stderr


def kernel_lines(text, name):
    start = re.search(r'^%s:' % re.escape(name), text, re.M).start()
    end = text.index('.Lfunc_end', start)
    return [l.strip() for l in text[start:end].split('\n')]


def test_wide_has_no_scratch(isa):
    m = re.search(r'Function Name: %s \[.*?\n(?:.*\n){0,8}?.*ScratchSize \[bytes/lane\]: (\d+)' % re.escape(WIDE), isa[1])
    assert m, 'no resource remark for ' + WIDE
    assert int(m.group(1)) == 0


def test_wide_makes_no_call(isa):
    assert not any(l.startswith('s_swappc') for l in kernel_lines(isa[0], WIDE))


def test_wide_first_trip_is_one_trip(isa):
    lines = kernel_lines(isa[0], WIDE)
    first_wait = next(i for i, l in enumerate(lines) if re.match(r's_waitcnt\b.*\bvmcnt\(', l))
    clear = next(i for i, l in enumerate(lines) if l.startswith('ds_write2st64_b32'))
    barrier = next(i for i in range(clear, len(lines)) if lines[i].startswith('s_barrier'))
    assert first_wait < clear < barrier
    late = [l for l in lines[first_wait:barrier] if l.startswith('global_load')]
    assert all(l.startswith('global_load_dwordx4') for l in late), late
