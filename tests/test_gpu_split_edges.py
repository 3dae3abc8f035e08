# coding=utf-8
"""-m gpu: ef_classify_split -- two lanes per candidate on the two-launch path -- at the smallest shapes where its split or its fold
can go wrong (tests/split_edges.py; their structure and the fold itself are checked on the CPU by tests/test_split_edge_cases.py).

Every case runs through duet_ef_run_host and through resident arrays with the mark array 16-byte aligned (the 16-byte staging)
and 4 bytes off (the scalar staging), bit for bit against oracle.c_oracle.ef, under the debug words
  0                       ef_classify_split, candidates above heavy_t by the owner's wavefront;
  DUET_DBG_EF_SPLIT_OFF   ef_classify on the two-launch path;
  DUET_DBG_EF_HEAVY_ALL   ef_classify_split with every candidate walked by its owner's wavefront, the helpers idle;
  DUET_DBG_EF_HEAVY_OFF   ... with every candidate of up to 255 marks on two lanes;
  DUET_DBG_EF_FP_DECIDE   ... with the binary64 decision behind the fold;
  DUET_DBG_EF_OWN_OFF     three launches, ef_classify.
The seed arrays (duet_ef_get_seed_ps) of every contig are compared between 0 and DUET_DBG_EF_SPLIT_OFF."""
import numpy as np
import pytest

from duet_amd import _lib
from duet_amd.devmem import DeviceProblem
from oracle import c_oracle
from tests import split_edges as S

pytestmark = pytest.mark.gpu

SPLIT_OFF, HEAVY_ALL, HEAVY_OFF, FP_DECIDE, OWN_OFF = 0x200000, 0x80000, 0x100000, 0x400000, 0x800000      # include/duet_ef.h
DEBUG_WORDS = (0, SPLIT_OFF, HEAVY_ALL, HEAVY_OFF, FP_DECIDE, OWN_OFF)


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


@pytest.mark.parametrize('name', S.NAMES)
def test_case_matches_the_oracle(ctx, name):
    soa = S.case(name)
    rc, want_pred, want_ps = c_oracle.ef(soa, 50, 2)
    assert rc == 0
    want = (want_pred, want_ps)
    resident = [(pad, DeviceProblem(soa, 50, 2, misalign_marks=pad)) for pad in (0, 4)]
    seeds = {}
    try:
        for dbg in DEBUG_WORDS:
            ctx.set_debug(dbg)
            same((name, hex(dbg), 'host'), ctx.run_host(soa, 50, 2), want)
            for pad, dp in resident:
                dp.out_storage.fill_(0xCD)
                dp.run(ctx)
                ctx.check()
                same((name, hex(dbg), 'resident, marks %d bytes off' % pad), dp.results(), want)
            if dbg in (0, SPLIT_OFF):
                seeds[dbg] = [ctx.seed_ps(k) for k in range(soa.n_contigs)]
    finally:
        ctx.set_debug(0)
    for k, (a, b) in enumerate(zip(seeds[0], seeds[SPLIT_OFF])):
        assert np.array_equal(a, b), (name, 'seed array of contig', k)
