# coding=utf-8
"""-m gpu: the tag lookup of the kernels behind ef_classify -- ef_finalize's vote from the marks, the array-free walk and the
hash-set route of ef_finalize_own / ef_finalize_own_wide -- on marks without a tag in every spelling (tests/tag_lookup_edges.py;
tests/test_tag_lookup_edge_cases.py shows on the CPU that the cases are what they are named and that a read of the words behind
the table changes calls of every kind).

Every case under every debug word, bit for bit (pred and ps of every candidate, outputs pre-filled with 0xCD) against
oracle.c_oracle.ef of the canonical problem: through duet_ef_run_host, and resident with the mark array 16-byte aligned and
4 bytes off.  The resident table has eight voter tags of the first seed behind it, inside the same allocation: a kernel that
reads the table at n_reads or n_reads + 1 gets a vote from them, not the zeros that DeviceProblem puts there otherwise.

One case of long candidates -- 499,999, 500,000 and 500,001 marks, PC sums on either side of 2^31 and 2^32 -- runs against
oracle/ef_oracle.py, the exact reference.  One input runs behind duet_svim_phase_device (ef_finalize<DYN>), field for field
against the composed C oracles on the canonical marks."""
import numpy as np
import pytest

from duet_amd import _lib
from duet_amd.devmem import DeviceProblem, DeviceSvim
from tests import svim_ref
from tests import tag_lookup_edges as E
from tests.test_gpu_classify_edges import same
from tests.test_gpu_fused_edges import check, device_run, host_run
from tests.test_tag_lookup_edge_cases import c_reference, long_reference

pytestmark = pytest.mark.gpu

# include/duet_ef.h: DUET_DBG_EF_*
OWN_WIDE, OWN_NARROW, FIN_TPB2, FIN_TPB4 = 0x1, 0x2, 0x20, 0x80
HEAVY_ALL, SPLIT_OFF, OWN_OFF, OWN_ALL, OWN_SMALLTAB = 0x80000, 0x200000, 0x800000, 0x1000000, 0x2000000
MODES = (('default', 0),
         ('three_launches', OWN_OFF),
         ('three_launches_two_tiles', OWN_OFF | FIN_TPB2),
         ('three_launches_four_tiles', OWN_OFF | FIN_TPB4),
         ('two_launches_forced', OWN_ALL),
         ('two_launches_set_of_8', OWN_ALL | OWN_SMALLTAB),
         ('own_wide', OWN_WIDE),
         ('own_narrow', OWN_NARROW),
         ('heavy_all', HEAVY_ALL),
         ('split_off', SPLIT_OFF))
SMALL_K = 64


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.set_debug(0)
    c.close()


_resident = {}


def resident(name):
    """the case's arrays on the device, marks 0 and 4 bytes off, the guard words behind the table (the last case's only)"""
    if name not in _resident:
        _resident.clear()
        soa = E.case(name)
        _resident[name] = [(pad, DeviceProblem(soa, 50, 2, misalign_marks=pad, tag_guard=E.guard_words(soa))) for pad in (0, 4)]
    return _resident[name]


@pytest.mark.parametrize('name,mode', [(n, m) for n in E.NAMES for m, _ in MODES])
def test_case_matches_the_oracle_of_the_canonical_problem(ctx, name, mode):
    soa, want = E.case(name), c_reference(name)
    dbg = dict(MODES)[mode]
    if (dbg & OWN_ALL) and soa.n_contigs > SMALL_K:
        pytest.skip('DUET_DBG_EF_OWN_ALL is not defined for more than 64 contigs')
    ctx.set_debug(dbg)
    try:
        same((name, mode, 'host'), ctx.run_host(soa, 50, 2), want)
        for pad, dp in resident(name):
            dp.out_storage.fill_(0xCD)
            dp.run(ctx)
            ctx.check()
            same((name, mode, 'resident, marks %d bytes off' % pad), dp.results(), want)
    finally:
        ctx.set_debug(0)


# ---- long candidates: the 500,000-mark rule, PC sums at 2^31 and 2^32 ---------------------------------------------------------

HEAVY_OFF, FP_DECIDE = 0x100000, 0x400000
LONG_MODES = (('default', 0), ('heavy_all', HEAVY_ALL), ('heavy_off', HEAVY_OFF), ('fp_decide', FP_DECIDE), ('split_off', SPLIT_OFF),
              ('three_launches', OWN_OFF), ('two_launches_set_of_8', OWN_ALL | OWN_SMALLTAB))
_long_resident = {}


@pytest.mark.parametrize('mode', [m for m, _ in LONG_MODES])
def test_long_sums_match_the_exact_oracle(ctx, mode):
    """candidates of 499,999, 500,000 and 500,001 marks and PC sums on either side of 2^31 and 2^32 (tag_lookup_edges._long_sums)
    against oracle/ef_oracle.py, whose sums are Python integers"""
    soa, _, want = long_reference()
    if not _long_resident:
        _resident.clear()
        _long_resident['dp'] = DeviceProblem(soa, 50, 2, tag_guard=E.guard_words(soa))
    dp = _long_resident['dp']
    ctx.set_debug(dict(LONG_MODES)[mode])
    try:
        same((E.LONG, mode, 'host'), ctx.run_host(soa, 50, 2), want)
        dp.out_storage.fill_(0xCD)
        dp.run(ctx)
        ctx.check()
        same((E.LONG, mode, 'resident'), dp.results(), want)
    finally:
        ctx.set_debug(0)


def test_device_planned_instance(ctx):
    c, canon = E.planned()
    want = svim_ref.fused(canon, c.read_tag, c.depth, c.depth_off, c.depth_bin, c.svlen_thres, c.suppread_thres, **c.kw)
    assert want['rc'] == 0 and int((want['pred'] != 0).sum()) > 100
    ds = DeviceSvim(c.marks, c.read_tag, c.depth, c.depth_off, c.depth_bin, c.svlen_thres, c.suppread_thres, **c.kw)
    try:
        for dbg in (0, HEAVY_ALL):
            ctx.set_debug(dbg)
            for wait in (False, True, False):                      # (planned on the device, planned by the host, and again)
                n, out = device_run(ctx, ds, wait)
                check(('tag_lookup_planned', hex(dbg), 'wait' if wait else 'no wait'), c, want, n, out)
        ctx.set_debug(0)
        n, out = host_run(ctx, c)
        check(('tag_lookup_planned', 'host'), c, want, n, out)
    finally:
        ctx.set_debug(0)
