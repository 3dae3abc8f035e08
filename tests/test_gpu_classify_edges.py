# coding=utf-8
"""-m gpu: ef_classify at the smallest shapes where its addressing can go wrong (tests/classify_edges.py; their structure is
checked on the CPU by tests/test_classify_edge_cases.py) -- tile edges where the clamps at C and C - 1 clamp, mark arrays and
tiles that end or begin off a 16-byte boundary, tiles without marks, spans of exactly one staging pass and one mark more, marks
without a tag in every spelling, more group summaries than a tile has slots, contigs that open on a wavefront's edge.

Every case runs through duet_ef_run_host and through resident arrays with the mark array 16-byte aligned (the 16-byte staging)
and 4 bytes off (the scalar staging), under debug words 0, DUET_DBG_EF_HEAVY_ALL (every candidate by the wave-cooperative walk)
and DUET_DBG_EF_OWN_OFF (three launches), bit for bit against oracle.c_oracle.ef.

The device-planned instances of the kernel run behind duet_svim_phase_device without the host round trip: inputs of exactly 1,
256 and 257 candidates, each under a bound (one candidate per mark) several tiles above the count where the marks allow it,
field for field against the composed C oracles as tests/test_gpu_fused_edges.py does it."""
import numpy as np
import pytest

from duet_amd import _lib
from duet_amd.devmem import DeviceProblem, DeviceSvim
from oracle import c_oracle
from tests import classify_edges as E
from tests import svim_fuzz, svim_ref
from tests.test_gpu_fused_edges import check, device_run, host_run

pytestmark = pytest.mark.gpu

HEAVY_ALL, OWN_OFF = 0x80000, 0x800000         # DUET_DBG_EF_HEAVY_ALL, DUET_DBG_EF_OWN_OFF
DEBUG_WORDS = (0, HEAVY_ALL, OWN_OFF)


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.set_debug(0)
    c.close()


def same(tag, got, want):
    for f, g, w in (('pred', got[0], want[0]), ('ps', got[1], want[1])):
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, (tag, f, 'first mismatches at', bad[:5], g[bad[:5]], w[bad[:5]])


@pytest.mark.parametrize('name', E.NAMES)
def test_case_matches_the_oracle(ctx, name):
    soa = E.case(name)
    rc, want_pred, want_ps = c_oracle.ef(E.as_absent(soa), 50, 2)
    assert rc == 0
    want = (want_pred, want_ps)
    resident = [(pad, DeviceProblem(soa, 50, 2, misalign_marks=pad)) for pad in (0, 4)]
    try:
        for dbg in DEBUG_WORDS:
            ctx.set_debug(dbg)
            same((name, hex(dbg), 'host'), ctx.run_host(soa, 50, 2), want)
            for pad, dp in resident:
                dp.out_storage.fill_(0xCD)
                dp.run(ctx)
                ctx.check()
                same((name, hex(dbg), 'resident, marks %d bytes off' % pad), dp.results(), want)
    finally:
        ctx.set_debug(0)


# ---- the device-planned instances ------------------------------------------------------------------------------------------

def _planned(name, seed, sizes):
    """len(sizes) candidates (an SV group of at most part_max marks is one candidate, tests/svim_fuzz.py) on two contigs"""
    G = len(sizes)
    g_contig = np.minimum(np.arange(G) * 2 // max(G, 1), 1) if G > 1 else np.zeros(1, dtype=np.int64)
    return svim_fuzz.build(name, seed, g_contig, sizes, 2 if G > 1 else 1, favour=True)


PLANNED = {
    'planned_1': lambda: _planned('planned_1', 7001, [90]),                                # bound: 90 candidates, one tile
    'planned_256': lambda: _planned('planned_256', 7002, np.resize([5, 6, 7, 9], 256)),    # bound: 1728, seven tiles for one
    'planned_257': lambda: _planned('planned_257', 7003, np.resize([5, 6, 7, 9], 257)),    # bound: 1733, seven tiles for two
}
_planned_made = {}


def planned_case(name):
    if name not in _planned_made:
        c = PLANNED[name]()
        want = svim_ref.fused(c.marks, c.read_tag, c.depth, c.depth_off, c.depth_bin, c.svlen_thres, c.suppread_thres, **c.kw)
        assert want['rc'] == 0
        _planned_made[name] = (c, want)
    return _planned_made[name]


@pytest.mark.parametrize('name,n_cands', (('planned_1', 1), ('planned_256', 256), ('planned_257', 257)))
def test_device_planned_instances(ctx, name, n_cands):
    c, want = planned_case(name)
    assert len(want['pred']) == n_cands
    if n_cands > 1:
        assert (c.M + 255) // 256 >= (n_cands + 255) // 256 + 4                     # the bound is tiles above the count
        assert int((want['pred'] != 0).sum()) > 10
    ds = DeviceSvim(c.marks, c.read_tag, c.depth, c.depth_off, c.depth_bin, c.svlen_thres, c.suppread_thres, **c.kw)
    try:
        for dbg in (0, HEAVY_ALL):
            ctx.set_debug(dbg)
            for wait in (False, True, False):                      # (planned on the device, planned by the host, and again)
                n, out = device_run(ctx, ds, wait)
                check((name, hex(dbg), 'wait' if wait else 'no wait'), c, want, n, out)
        ctx.set_debug(0)
        n, out = host_run(ctx, c)
        check((name, 'host'), c, want, n, out)
    finally:
        ctx.set_debug(0)
