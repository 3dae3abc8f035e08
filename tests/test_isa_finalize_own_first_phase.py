"""CPU guard on the gfx950 ISA of ef_finalize_own and ef_finalize_own_wide after round 11 (no GPU needed; skipped without hipcc) --
in the manner of tests/test_isa_finalize_own_wide.py, with the same compile line.  Between the first trip's wait (the first
``s_waitcnt vmcnt``) and the barrier that runs first (the ``s_barrier`` behind the hash set's clear, the first
``ds_write2st64_b32``) every wavefront of every workgroup runs the text in between; what the contig loop's body derives from the
thread index alone, mostly for its rare paths, must not stand there.

* at most 260 instructions in that text.  What the phase needs: three LDS writes of the summaries, the seven selects of `live`, the
  contig's bounds on the scalar unit, the table's clear (two writes), two wavefront maxima (twelve DPP steps and their moves), the
  write of the maxima -- about 60; the text also holds the loop's head and the second contig's reload, which the first pass jumps
  over -- eight loads with their clamped addresses, about 70; twice the sum is 260.  The parent had 357 (342 narrow) there;
* none of them computes a lane predicate of own_sort_set's sorting network (``v_bitop3_b32``): the network is the rare path's;
* at most eight ``global_load_dwordx4`` in front of the first wait, no scratch, and at most 144 VGPRs (three wavefronts per SIMD).
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

KERNELS = {'wide': '_ZN12_GLOBAL__N_120ef_finalize_own_wideENS_6ParamsE', 'narrow': '_ZN12_GLOBAL__N_115ef_finalize_ownENS_6ParamsE'}


@pytest.fixture(scope='module')
def isa(tmp_path_factory):
    out = tmp_path_factory.mktemp('isa_first_phase')
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


def remark(remarks, name, what):
    m = re.search(r'Function Name: %s \[.*?\n(?:.*\n){0,12}?.*[^a-zA-Z]%s: (\d+)' % (re.escape(name), re.escape(what)), remarks)
    assert m, 'no %s remark for %s' % (what, name)
    return int(m.group(1))


def first_phase(lines):
    """-> (index of the first vmcnt wait, the instructions from there to the barrier behind the clear)"""
    first_wait = next(i for i, l in enumerate(lines) if re.match(r's_waitcnt\b.*\bvmcnt\(', l))
    clear = next(i for i, l in enumerate(lines) if l.startswith('ds_write2st64_b32'))
    barrier = next(i for i in range(clear, len(lines)) if lines[i].startswith('s_barrier'))
    assert first_wait < clear < barrier
    return first_wait, [l for l in lines[first_wait:barrier] if l and not l.startswith((';', '.'))]


@pytest.mark.parametrize('which', sorted(KERNELS))
def test_nothing_of_the_rare_paths_between_the_first_wait_and_the_first_barrier(isa, which):
    _, ins = first_phase(kernel_lines(isa[0], KERNELS[which]))
    print(which, 'instructions between the first wait and the first barrier:', len(ins))
    assert len(ins) <= 260
    assert not [l for l in ins if l.startswith('v_bitop3_b32')]


@pytest.mark.parametrize('which', sorted(KERNELS))
def test_first_trip_loads_and_registers(isa, which):
    lines = kernel_lines(isa[0], KERNELS[which])
    first_wait, _ = first_phase(lines)
    assert sum(l.startswith('global_load_dwordx4') for l in lines[:first_wait]) <= 8
    assert remark(isa[1], KERNELS[which], r'ScratchSize [bytes/lane]') == 0
    assert remark(isa[1], KERNELS[which], 'VGPRs') <= 144
