# coding=utf-8
"""-m gpu: the sweep of a contig's seed records in ef_finalize_own / ef_finalize_own_wide at the smallest shapes at which it can go
wrong.  The cases were laid out for a flat sweep of the records -- one array of sixteen-byte chunks, lane tid taking chunks tid,
tid + NT, ..., a quad of lanes holding a record's four quarters -- which round 11 built and measured and did not keep
(profiles/history/r11_flat_sweep_REJECTED.txt); they hold the kept sweep, one record per lane, to the same edges, and any later one.
Every case under debug words 0 (the library's own choice of kernel), DUET_DBG_EF_OWN_WIDE (0x1), DUET_DBG_EF_OWN_NARROW (0x2) and
DUET_DBG_EF_OWN_WIDE | DUET_DBG_EF_OWN_SMALLTAB.

  * one contig of 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1,024 and 1,025 tiles: a wavefront's records, the
    records of one load instruction (per lane: 256 narrow, 512 wide; flat: 64 and 128), of the first trip (512 narrow, 1,024 wide) and
    the first record of a later trip;
  * 0, 1, 2, 3, 4, 6, 7, 8, 24 and 25 entries in the first and in the last tile of a contig and in the two tiles on either side of
    tiles 63 | 64 and 127 | 128 of 130: every quarter of a record empty and full, the overflow slots by the lane (up to 24) and by
    the wavefront (beyond);
  * a contig border inside a tile -- one record holds entries of two contigs -- with the second contig's first tile at an odd and at
    an even index; 64 contigs of one tile each; a workgroup over three contigs; a last workgroup of one tile; a contig whose entries
    are all repeats of one seed.

In every contig the LAST entry of the first tile, of the last tile and of the tiles either side of every 64th record occurs nowhere
else, and a two-group candidate (is this PS a seed) and an asker (which seed is nearest) of another tile depend on it: a record, a
quarter or an overflow slot that the sweep misses changes their answers.

Bit for bit: pred and ps of every candidate against oracle.c_oracle.ef, and the seed arrays the ABI hands out against the distinct
values of the CPU model's tile entries, as tests/test_gpu_finalize_own_wide.py does.  The outputs are resident and pre-filled."""
import numpy as np
import pytest

from duet_amd import _lib
from duet_amd.devmem import DeviceProblem
from oracle import c_oracle
from tests import seed_edges as E
from tests.seed_edges import ASK, SKIP, TILE, build, seed, two
from tests.test_gpu_classify_edges import same
from tests.test_gpu_finalize_own_wide import seed_set
from tests.test_seed_edge_cases import tile_entries

pytestmark = pytest.mark.gpu

WIDE, NARROW, SMALLTAB = 0x1, 0x2, 0x2000000      # include/duet_ef.h: DUET_DBG_EF_OWN_WIDE / _OWN_NARROW / _OWN_SMALLTAB
DEBUG_WORDS = (0, WIDE, NARROW, WIDE | SMALLTAB)
TILE_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1024, 1025)
ENTRY_COUNTS = (0, 1, 2, 3, 4, 6, 7, 8, 24, 25)
EDGE_TILES = (0, 63, 64, 127, 128, 129)           # of a contig of 130 tiles


def lone(t, salt=0):
    """the value that only tile t's last entry holds (far from the common values, 10 apart: its asker sits one above it)"""
    return 100000 + 50000 * salt + 10 * t


def marked(t, n_tiles):
    return t == 0 or t == n_tiles - 1 or t % 64 in (63, 0)


def contig(n_tiles, count_of, salt=0, n_cands=None, common=600, near=True):
    """(position, kind) of one contig of n_tiles tiles (the last one cut to n_cands candidates in all): tile t holds count_of(t) seed
    entries at lanes 0, 2, 4, ... -- `common` distinct values shared by all tiles, so that the set stays below kOwnKeys; in a marked
    tile the last entry is lone(t) -- and, at lanes 200 .., the questions that depend on the marked tile (t * 7 + 3) % n_tiles"""
    cands = []
    marks = [t for t in range(n_tiles) if marked(t, n_tiles) and count_of(t) > 0]
    for t in range(n_tiles):
        n = count_of(t)
        assert n <= 100
        vals = [3000 + 50000 * salt + 10 * ((5 * t + j) % common) for j in range(n)]
        if n and marked(t, n_tiles):
            vals[-1] = lone(t, salt)
        tile = [(1000 + 300 * t + l, SKIP) for l in range(TILE)]
        for j, v in enumerate(vals):
            tile[2 * j] = (1000 + 300 * t + 2 * j, seed(v))
        if marks:
            m = marks[t % len(marks)]
            tile[200] = (lone(m, salt) + 1, ASK)
            tile[201] = (lone(m, salt) + 2 if near else 1000 + 300 * t + 201, two(lone(m, salt), 2, 7, 1))
            tile[202] = (lone(m, salt) + 4 if near else 1000 + 300 * t + 202, two(lone(m, salt) + 3, 2, 7, 1))   # (no seed: the nearest one)
        cands += tile
    return cands if n_cands is None else cands[:n_cands]


def usual(t):
    return (2, 3, 1, 2, 7, 2, 3, 4)[t % 8]          # (mostly quarters 0 and 1; a full record and a fourth entry now and then)


def _one_contig(n_tiles):
    return lambda: build([contig(n_tiles, usual)])


def _entries(n):
    return lambda: build([contig(130, lambda t: n if t in EDGE_TILES else 2, near=False)])


def _border_in_tile(first_tiles):
    """contig A ends 100 candidates into tile `first_tiles`, contig B begins there: the record of that tile holds entries of both
    (lanes 0 .. of A, then B's from lane 100 on), and B's first tile has index first_tiles"""
    def make():
        a = contig(first_tiles + 1, lambda t: 5, salt=0, n_cands=first_tiles * TILE + 100)
        b = contig(3, lambda t: 4, salt=1)
        return build([a, b])
    return make


def _contigs_of_one_tile():
    return build([contig(1, lambda t: (k % 7) + 1, salt=k) for k in range(64)])


def _workgroup_over_three_contigs():
    return build([contig(1, lambda t: 5, salt=0, n_cands=150), contig(1, lambda t: 3, salt=1, n_cands=100),
                  contig(2, lambda t: 6, salt=2, n_cands=300)])


def _one_seed_repeated():
    """70 tiles whose single entry is the same seed; every tile asks"""
    cands = []
    for t in range(70):
        tile = [(1000 + 300 * t + l, SKIP) for l in range(TILE)]
        tile[10] = (1000 + 300 * t + 10, seed(4242))
        tile[20] = (50 * t, ASK)
        tile[21] = (1000 + 300 * t + 21, two(4242, 1, 9, 2))
        cands += tile
    return build([cands])


CASES = {}
for _n in TILE_COUNTS:
    CASES['tiles_%d' % _n] = _one_contig(_n)
for _n in ENTRY_COUNTS:
    CASES['entries_%d_at_the_edges' % _n] = _entries(_n)
CASES['border_in_tile_second_contig_odd'] = _border_in_tile(1)
CASES['border_in_tile_second_contig_even'] = _border_in_tile(2)
CASES['contigs_64_of_one_tile'] = _contigs_of_one_tile
CASES['workgroup_over_three_contigs'] = _workgroup_over_three_contigs
CASES['last_workgroup_of_one_tile'] = _one_contig(3)
CASES['one_seed_repeated'] = _one_seed_repeated
NAMES = tuple(CASES)


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.set_debug(0)
    c.close()


_ref, _resident = {}, {}


def reference(name):
    """computed once per case, from the input alone, and shared by its four debug words (the last case's only: they come one after
    the other)"""
    if name not in _ref:
        _ref.clear()
        soa = CASES[name]()
        assert soa.n_contigs <= E.SMALL_K
        rc, pred, ps = c_oracle.ef(soa, 50, 2)
        assert rc == 0
        pred.setflags(write=False)
        ps.setflags(write=False)
        seeds = [seed_set(soa, k) for k in range(min(soa.n_contigs, 8))]
        _ref[name] = (soa, (pred, ps), seeds)
    return _ref[name]


def resident(name):
    if name not in _resident:
        _resident.clear()
        _resident[name] = DeviceProblem(reference(name)[0], 50, 2)
    return _resident[name]


def test_the_cases_have_their_shape():
    """(CPU work only, but it belongs with the cases) the counts the names promise, from the model of the tile records"""
    for n in (1, 65, 513):
        soa = CASES['tiles_%d' % n]()
        assert soa.n_cands == n * TILE and soa.n_contigs == 1
        assert [len(v) for _, v in tile_entries(soa)] == [usual(t) for t in range(n)]
        assert len(seed_set(soa, 0)) < E.OWN_KEYS
    for n in ENTRY_COUNTS:
        soa = CASES['entries_%d_at_the_edges' % n]()
        assert [len(v) for _, v in tile_entries(soa)] == [n if t in EDGE_TILES else 2 for t in range(130)]
    for first, name in ((1, 'odd'), (2, 'even')):
        soa = CASES['border_in_tile_second_contig_%s' % name]()
        at = first * TILE + 100
        assert list(soa.cand_ctg_off) == [0, at, at + 3 * TILE]
        idx, v = tile_entries(soa)[first]
        assert int((idx < at).sum()) == 5 and int((idx >= at).sum()) > 0            # one record, two contigs
    soa = CASES['contigs_64_of_one_tile']()
    assert soa.n_contigs == 64 and list(np.diff(soa.cand_ctg_off)) == [TILE] * 64
    assert list(CASES['workgroup_over_three_contigs']().cand_ctg_off) == [0, 150, 250, 550]
    assert CASES['last_workgroup_of_one_tile']().n_cands == 3 * TILE
    soa = CASES['one_seed_repeated']()
    assert [v.tolist() for _, v in tile_entries(soa)] == [[4242]] * 70 and seed_set(soa, 0).tolist() == [4242]


@pytest.mark.parametrize('name,dbg', [(n, d) for n in NAMES for d in DEBUG_WORDS])
def test_case_matches_the_oracle_and_the_model(ctx, name, dbg):
    soa, want, seeds = reference(name)
    dp = resident(name)
    ctx.set_debug(dbg)
    try:
        dp.out_storage.fill_(0xCD)
        dp.run(ctx)
        ctx.check()
        same((name, hex(dbg)), dp.results(), want)
        for k, s in enumerate(seeds):
            got = ctx.seed_ps(k)
            assert np.array_equal(got, s), (name, hex(dbg), 'seeds of contig %d' % k, len(got), len(s), np.setxor1d(got, s)[:5])
    finally:
        ctx.set_debug(0)
