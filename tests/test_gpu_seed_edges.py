# coding=utf-8
"""-m gpu: the three kernels behind ef_classify -- ef_seed_sort, ef_finalize, ef_finalize_own -- at their capacity edges
(tests/seed_edges.py; tests/test_seed_edge_cases.py shows on the CPU that every case has the structure it is named for): exactly
at, one below and one above kOwnKeys, kOwnTab, kOwnWin, the 512 tile records of the first trip, the 3 / 7 / 24 entries of a tile,
kLongCnt / kLongTiles, kFewRuns / kMaxRuns, kSeedTab / 2 and its 32 probes, kSortLds, 1024 / kOneLds and kSmallK -- with the real
capacities, not DUET_DBG_EF_OWN_SMALLTAB's.

Every case in every mode that applies to it, bit for bit: pred and ps of every candidate against oracle.c_oracle.ef, and the seed
arrays the ABI hands out (after a two-launch run: ef_seed_sort on demand) against np.unique of the CPU model's gathered list.  The
outputs are resident and pre-filled with 0xCD, so a candidate nobody writes shows."""
import numpy as np
import pytest

from duet_amd import _lib
from duet_amd.devmem import DeviceProblem
from oracle import c_oracle
from tests import seed_edges as E
from tests.test_gpu_classify_edges import same
from tests.test_seed_edge_cases import seed_list

pytestmark = pytest.mark.gpu

# include/duet_ef.h: DUET_DBG_EF_FIN_TPB2 / _NO_SEED_HASH / _FIN_TPB4 / _OWN_OFF / _OWN_ALL
TPB2, NO_SEED_HASH, TPB4, OWN_OFF, OWN_ALL = 0x20, 0x40, 0x80, 0x800000, 0x1000000
MODES = (('default', 0),                        # two launches for all of these sizes (K <= 64), run twice in a row
         ('three_launches', OWN_OFF),
         ('two_tiles', OWN_OFF | TPB2),
         ('four_tiles', OWN_OFF | TPB4),
         ('no_seed_hash', NO_SEED_HASH),
         ('two_launches_forced', OWN_ALL))


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.set_debug(0)
    c.close()


_ref, _resident = {}, {}


def reference(name):
    """computed once per case, from the input alone: the oracle's (pred, ps) and the model's seed sets of the first 8 contigs"""
    if name not in _ref:
        soa = E.case(name)
        rc, pred, ps = c_oracle.ef(soa, 50, 2)
        assert rc == 0
        pred.setflags(write=False)
        ps.setflags(write=False)
        seeds = [np.unique(seed_list(soa, k)).astype(np.uint32) for k in range(min(soa.n_contigs, 8))]
        _ref[name] = (soa, (pred, ps), seeds)
    return _ref[name]


def resident(name):
    """the case's arrays on the device (the last case's only: the cases come one after the other)"""
    if name not in _resident:
        _resident.clear()
        _resident[name] = DeviceProblem(reference(name)[0], 50, 2)
    return _resident[name]


@pytest.mark.parametrize('name,mode', [(n, m) for n in E.NAMES for m, _ in MODES])
def test_case_matches_the_oracle_and_the_model(ctx, name, mode):
    soa, want, seeds = reference(name)
    dbg = dict(MODES)[mode]
    if (dbg & OWN_ALL) and soa.n_contigs > E.SMALL_K:
        pytest.skip('DUET_DBG_EF_OWN_ALL is not defined for more than 64 contigs')
    dp = resident(name)
    ctx.set_debug(dbg)
    try:
        for again in range(2 if dbg == 0 else 1):                          # (the summary pool's counter, the plan reuse)
            dp.out_storage.fill_(0xCD)
            dp.run(ctx)
            ctx.check()
            same((name, mode, 'run %d' % again), dp.results(), want)
            for k, s in enumerate(seeds):
                got = ctx.seed_ps(k)
                assert np.array_equal(got, s), (name, mode, 'seeds of contig %d' % k, len(got), len(s),
                                                np.setxor1d(got, s)[:5])
    finally:
        ctx.set_debug(0)
