# coding=utf-8
"""CPU guard on the gfx950 ISA of ef_classify_split, both instances (no GPU needed; skipped without hipcc): the properties
tests/test_isa_hot_kernels.py and tests/test_isa_classify_trips.py hold ef_classify to, read off the same compilation with the
same plain matching, with this kernel's own kSplitStageIt = 2 index loads per thread and pass.

* no scratch memory and no call (``s_swappc``);
* registers: a workgroup is 512 threads, eight wavefronts, two on every SIMD; the kernel asks for six wavefronts per SIMD
  (``__launch_bounds__(512, 6)``: three workgroups per CU, ef_classify's occupancy), which 512 / 6 -> 80 VGPRs allow: at most 80;
* the prologue: at least six ``global_load*`` in front of the first ``s_waitcnt`` naming ``vmcnt``, and between that wait and the
  walk's first ``ds_read_b64`` no ``s_load*`` outside a block that a conditional branch jumps over;
* the staging pass of the instance over an aligned mark array: its sixteen-byte index loads in a straight line without a ``vmcnt``
  wait between them, the gathers behind them, and no ``s_waitcnt vmcnt(0)`` before the last gather."""
import pytest

from tests import test_isa_classify_trips as T
from tests.test_isa_hot_kernels import HIPCC, isa, kernel_lines, scratch_size      # noqa: F401 (isa: the fixture)

pytestmark = pytest.mark.skipif(HIPCC is None, reason='hipcc not found')

SPLIT = ['_ZN12_GLOBAL__N_117ef_classify_splitILb%dEEEvNS_6ParamsE' % v for v in (1, 0)]
STAGE_IT = 2                            # kSplitStageIt


@pytest.mark.parametrize('name', SPLIT)
def test_no_scratch_no_call_and_registers_for_six_waves(isa, name):
    assert scratch_size(isa[1], name) == 0
    assert not any(l.startswith('s_swappc') for l in kernel_lines(isa[0], name))
    assert T.vgprs(isa[1], name) <= 80


@pytest.mark.parametrize('name', SPLIT)
def test_prologue_is_one_trip_and_the_arguments_come_at_entry(isa, name, monkeypatch):
    monkeypatch.setattr(T, 'STAGE_IT', STAGE_IT)
    lines = kernel_lines(isa[0], name)
    if name != SPLIT[0]:
        # the scalar staging has no sixteen-byte loads to anchor on: the prologue's wait and the walk's first tag read alone
        wait = next(i for i, l in enumerate(lines) if T.VM_WAIT.match(l))
        walk = next(i for i in range(wait, len(lines)) if lines[i].startswith('ds_read_b64'))
        monkeypatch.setattr(T, 'anchors', lambda _: (wait, [], [], None, walk))
    T.check_prologue(lines)


def test_a_staging_pass_is_index_loads_then_gathers(isa, monkeypatch):
    monkeypatch.setattr(T, 'STAGE_IT', STAGE_IT)
    T.check_staging(kernel_lines(isa[0], SPLIT[0]))
