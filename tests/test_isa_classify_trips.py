# coding=utf-8
"""CPU guard on the dependent memory trips of ef_classify in the gfx950 ISA (no GPU needed; skipped without hipcc).

A tile's walk needs three trips in front of it -- offsets and candidate scalars, mark indices, tags -- and a wait, a branch or a
late argument load anywhere in between adds one.  duet_ef.hip is compiled as tests/test_isa_hot_kernels.py compiles it (device
code only, the library's flags, to assembly with the kernel-resource remarks) and the text of ef_classify<true, false>, the
instance of host-planned runs over a 16-byte aligned mark array, is read with the same plain matching: the kernel is the text from
its label to its ``.Lfunc_end`` marker, an instruction is recognised by its mnemonic at the start of a line.

The anchors, in the order of the text:

* the first ``s_waitcnt`` that names ``vmcnt`` -- the prologue's wait.  In front of it at least six ``global_load*`` have left: the
  two offsets, four columns and the start flag (this build: nine, with the tile's first and last offset);
* the walk's first ``ds_read_b64`` (consume_range's tag read).  Between the prologue's wait and it no ``s_load*`` stands outside a
  block that a conditional branch jumps over (``s_cbranch_* .LBBn`` up to the label ``.LBBn`` further down): every kernel argument
  came in at entry;
* the staging pass: the first kStageIt = 3 ``global_load_dwordx4`` behind the prologue's wait are the index loads.  They stand in a
  straight line (no label, no branch) without an ``s_waitcnt`` naming ``vmcnt`` between the first and the last; the first
  ``global_load_dwordx2`` behind them is the first gather, the 4 * kStageIt-th the last; no ``global_load_dwordx4`` follows the first
  gather up to the pass's ``s_barrier``; and no ``s_waitcnt vmcnt(0)`` stands between the first index load and the last gather
  (this build waits with vmcnt(2), vmcnt(5) and vmcnt(8): for one index load each);
* the remarks: at most 80 VGPRs (six wavefronts per SIMD) and no scratch memory for each of the four instances."""
import re

import pytest

from tests.test_isa_hot_kernels import CLASSIFY, HIPCC, isa, kernel_lines, scratch_size      # noqa: F401 (isa: the fixture)

pytestmark = pytest.mark.skipif(HIPCC is None, reason='hipcc not found')

STAGE_IT = 3                            # kStageIt
VEC_HOST = CLASSIFY[0]                  # ef_classify<true, false>
VM_WAIT = re.compile(r's_waitcnt\b.*\bvmcnt\(')


def vgprs(remarks, name):
    m = re.search(r'Function Name: %s \[.*?\n(?:.*\n){0,8}?.*[^a-zA-Z]VGPRs: (\d+)' % re.escape(name), remarks)
    assert m, 'no resource remark for ' + name
    return int(m.group(1))


def anchors(lines):
    """-> (prologue's wait, [index loads], [gathers], the pass's barrier, the walk's first tag read) as line indices"""
    wait = next(i for i, l in enumerate(lines) if VM_WAIT.match(l))
    idx = [i for i in range(wait, len(lines)) if lines[i].startswith('global_load_dwordx4')][:STAGE_IT]
    assert len(idx) == STAGE_IT, 'no staging pass of %d sixteen-byte index loads' % STAGE_IT
    gat = [i for i in range(idx[0], len(lines)) if lines[i].startswith('global_load_dwordx2')][:4 * STAGE_IT]
    assert len(gat) == 4 * STAGE_IT
    barrier = next(i for i in range(gat[0], len(lines)) if lines[i].startswith('s_barrier'))
    walk = next(i for i in range(wait, len(lines)) if lines[i].startswith('ds_read_b64'))
    return wait, idx, gat, barrier, walk


def check_prologue(lines):
    wait, _, _, _, walk = anchors(lines)
    early = [l for l in lines[:wait] if l.startswith('global_load')]
    assert len(early) >= 6, early
    assert wait < walk
    skip_to = None                      # inside a block that a conditional branch jumps over: the label it ends at
    for l in lines[wait:walk]:
        if skip_to and l.startswith(skip_to + ':'):
            skip_to = None
        m = re.match(r's_cbranch_\w+\s+(\.LBB\w+)', l)
        if m and not skip_to and any(x.startswith(m.group(1) + ':') for x in lines[lines.index(l):]):
            skip_to = m.group(1)
        assert skip_to or not l.startswith('s_load'), 'a kernel argument is loaded behind the first wait: ' + l


def check_staging(lines):
    wait, idx, gat, barrier, walk = anchors(lines)
    between = lines[idx[0]:idx[-1] + 1]
    assert not any(VM_WAIT.match(l) for l in between), between
    assert not any(l.startswith('.LBB') or l.startswith('s_cbranch') or l.startswith('s_branch') for l in between), between
    assert idx[-1] < gat[0], 'a gather leaves before the last index load'
    assert gat[-1] < barrier < walk
    late = [l for l in lines[gat[0]:barrier] if l.startswith('global_load_dwordx4')]
    assert not late, late
    full = [l for l in lines[idx[0]:gat[-1]] if re.match(r's_waitcnt\b.*\bvmcnt\(0\)', l)]
    assert not full, full


def test_prologue_is_one_trip_and_the_arguments_come_at_entry(isa):
    check_prologue(kernel_lines(isa[0], VEC_HOST))


def test_a_staging_pass_is_index_loads_then_gathers(isa):
    check_staging(kernel_lines(isa[0], VEC_HOST))


@pytest.mark.parametrize('name', CLASSIFY)
def test_registers_allow_six_waves(isa, name):
    assert vgprs(isa[1], name) <= 80
    assert scratch_size(isa[1], name) == 0
