# coding=utf-8
"""-m gpu: ef_finalize_own_wide -- two tiles of 256 candidates per workgroup of 512 threads -- against ef_finalize_own, on the
two-launch path: every case under DUET_DBG_EF_OWN_WIDE (0x1: the wide kernel whatever the size), DUET_DBG_EF_OWN_NARROW (0x2: one
tile per workgroup whatever the size) and DUET_DBG_EF_OWN_WIDE | DUET_DBG_EF_OWN_SMALLTAB (the wide kernel with a seed set of 8 and
a window of 2: the array-free walk and own_sort_set at 512 threads).

(a) every case of tests/seed_edges.py with at most 64 contigs: the capacity edges the two kernels' common body has (the window, the
    tile records of the first trip, the probe chains, the 3 / 7 / 24 entries of a tile, empty first contigs, a last contig of one
    candidate);
(b) the shapes only two tiles per workgroup can get wrong (built HERE with seed_edges' builder): a last workgroup of one tile, with
    the candidate count one below, at and one above every multiple of 512 and one above every multiple of 256; a contig border
    exactly between a workgroup's two tiles, one candidate before and one behind; a workgroup over three contigs, the middle one
    of one candidate, with an empty contig beside it; a contig without seeds in the second tile only; 65 multi-PS candidates in
    one of the two tiles and none in the other; askers in one tile and the seeds of their answers in the other, and an asking range
    that only the two tiles together span (with 30 seeds inside: the window; with 70: own_sort_set); a contig of 1,024 and of
    1,025 tiles of 5 entries each (the wide kernel's first trip carries 1,024 records).

Bit for bit: pred and ps of every candidate against oracle.c_oracle.ef, and the seed arrays the ABI hands out (ef_seed_sort on
demand) against the distinct values of the CPU model's tile entries.  The outputs are resident and pre-filled with 0xCD."""
import numpy as np
import pytest

from duet_amd import _lib
from duet_amd.devmem import DeviceProblem
from oracle import c_oracle
from tests import seed_edges as E
from tests.seed_edges import ASK, SKIP, TILE, build, pad_tile, seed, spread, three, tile_with, two
from tests.test_gpu_classify_edges import same
from tests.test_seed_edge_cases import tile_entries

pytestmark = pytest.mark.gpu

WIDE, NARROW, SMALLTAB = 0x1, 0x2, 0x2000000      # include/duet_ef.h: DUET_DBG_EF_OWN_WIDE / _OWN_NARROW / _OWN_SMALLTAB
DEBUG_WORDS = (WIDE, NARROW, WIDE | SMALLTAB)


# ---- (b) the cases of two tiles per workgroup -------------------------------------------------------------------------------

def mixed(n, pos0, ps0):
    """n candidates in position order, 10 apart: every 37th a seed whose PS is about its position (the first one too), behind it an
    asker, two-group candidates whose larger group is that seed / is no seed / neither is (the nearest seed), a three-group one;
    the last candidate asks"""
    out = []
    for i in range(n):
        r = i % 37
        near = ps0 + 10 * (i - r)                    # the seed of candidate i - r
        if r == 0:
            kind = seed(ps0 + 10 * i)
        elif r == 5 or i == n - 1:
            kind = ASK
        elif r == 11:
            kind = two(near, 2, near + 3, 1)
        elif r == 19:
            kind = two(near + 3, 3, near, 1)
        elif r == 23:
            kind = two(7, 2, 9, 1)
        elif r == 29:
            kind = three((7, 2), (near, 1), (11, 1))
        else:
            kind = SKIP
        out.append((pos0 + 10 * i, kind))
    return out


def _count(n):
    return lambda: build([mixed(n, 1000, 1000)])


def _border(at, total=1100):
    """contig A ends behind candidate at - 1, contig B (other seeds over the same positions) runs to `total`: five tiles, so the
    last workgroup holds one"""
    return lambda: build([mixed(at, 1000, 1000), mixed(total - at, 1000, 1005)])


def _three_contigs(middle, empty_first):
    def make():
        mid = [[], [(5000, middle)]] if empty_first else [[(5000, middle)], []]
        return build([mixed(300, 1000, 1000)] + mid + [mixed(400, 1000, 1005)])
    return make


def _seedless_second_tile():
    bare = [(1000 + 10 * i, (ASK, two(1000, 2, 1370, 1), SKIP)[i % 3]) for i in range(TILE)]
    return build([mixed(TILE, 1000, 1000), bare, mixed(100, 1000, 1005)])


def _multi_ps(first):
    """65 two-group candidates in one tile of workgroup 0 (64 summaries in the tile's own slots, one in the pool), none in the
    other, which holds the seeds; a third tile (workgroup 1's first) with three more"""
    def make():
        S = [1000 + 80 * j for j in range(32)]
        seeds = [(v, seed(v)) if i % 8 == 0 else (v, SKIP) for i, v in enumerate(range(1000, 1000 + 10 * TILE, 10))]
        kinds = []
        for j in range(65):
            a, b = S[j % 32], S[(j + 5) % 32]
            kinds.append(((a + b) // 2, (two(a, 2, b, 1), two(a + 3, 3, b, 1), two(7, 2, 9, 1), two(a, 2, b, 2), two(b + 3, 1, a, 4))[j % 5]))
        many = tile_with(spread(65), kinds, pos0=1000)
        tail = tile_with([0, 9, 100, 255], [(1500, two(S[3], 1, S[9], 2)), (9000, seed(9000)), (1700, two(5, 1, 6, 1)), (2000, two(S[1], 3, 8, 1))])
        return build([(many + seeds if first else seeds + many) + tail])
    return make


def _askers_and_seeds(askers_first):
    """one tile of askers over [1000, 2000], one tile of seeds: 20 strictly inside that range, one on each end, some outside"""
    def make():
        ask = tile_with(spread(41), [(1000 + 25 * j, ASK) for j in range(41)])
        S = [1100 + 40 * j for j in range(20)] + [1000, 2000, 400, 3000, 2001, 999]
        seeds = tile_with(spread(len(S)), [(10 + j, seed(v)) for j, v in enumerate(S)])
        return build([ask + seeds if askers_first else seeds + ask])
    return make


def _joint_range(inside):
    """askers about 1000 in tile 0 and about 9000 in tile 1; the seeds, in tile 2, lie between: outside either tile's own asking
    range, inside the workgroup's"""
    def make():
        t0 = tile_with(spread(9), [(1000 + 10 * j, ASK) for j in range(9)] )
        t1 = tile_with(spread(9), [(9000 + 10 * j, ASK) for j in range(8)] + [(5001, two(7, 1, 9, 1))])
        S = [2000 + (6000 // inside) * j for j in range(inside)] + [500, 9500]
        t2 = tile_with(spread(len(S)), [(20 + j, seed(v)) for j, v in enumerate(S)])
        return build([t0 + t1 + t2])
    return make


def _long_contig(n_tiles):
    """one contig of n_tiles tiles of 5 seed entries each, 600 distinct values among them; PS 50 occurs only as the LAST entry of the
    LAST tile, and an asker and two two-group candidates of tile 0 depend on it"""
    def make():
        lanes = [10, 60, 110, 160, 210]
        cands = []
        for t in range(n_tiles):
            vals = [3000 + 10 * ((5 * t + j) % 600) for j in range(5)]
            p0 = 1000 + 300 * t
            kl, kk = list(lanes), [seed(v) for v in vals]
            if t == n_tiles - 1:
                kk[4] = seed(50)
                kl, kk = kl + [255], kk + [ASK]
            if t == 0:
                kl, kk = kl + [1, 2, 3], kk + [(1001, ASK), (1002, two(50, 2, 3000, 1)), (1003, two(77, 2, 50, 1))]
            if t % 200 == 7:
                kl, kk = kl + [77, 78], kk + [(3000 + 10 * (t % 600) + 4, ASK), (6000, two(3000 + 10 * (t % 600), 1, 8, 2))]
            cands += tile_with(kl, kk, pos0=p0)
        return build([cands])
    return make


CASES = {}
for _n in (1, 255, 256, 257, 511, 512, 513, 769, 1023, 1024, 1025):
    CASES['candidates_%d' % _n] = _count(_n)
for _n in (255, 256, 257, 767, 768, 769):
    CASES['contig_border_at_%d' % _n] = _border(_n)
CASES['three_contigs_middle_seed'] = _three_contigs(seed(4242), True)
CASES['three_contigs_middle_asks'] = _three_contigs(ASK, False)
CASES['seedless_contig_in_second_tile'] = _seedless_second_tile
CASES['multi_ps_65_in_first_tile'] = _multi_ps(True)
CASES['multi_ps_65_in_second_tile'] = _multi_ps(False)
CASES['askers_first_seeds_second'] = _askers_and_seeds(True)
CASES['seeds_first_askers_second'] = _askers_and_seeds(False)
CASES['joint_range_30_inside'] = _joint_range(30)
CASES['joint_range_70_inside'] = _joint_range(70)
CASES['tiles_1024_of_5_entries'] = _long_contig(1024)
CASES['tiles_1025_of_5_entries'] = _long_contig(1025)

SHARED = tuple(n for n in E.NAMES if n not in ('contigs_65',))          # (a): contigs_65 is the one case of more than 64 contigs
NAMES = SHARED + tuple(CASES)

_made = {}


def case(name):
    if name in CASES:
        if name not in _made:
            _made.clear()
            _made[name] = CASES[name]()
        return _made[name]
    return E.case(name)


def seed_set(soa, k):
    """the distinct seeds of contig k: what its tiles' entries (ef_classify's seeds_tile, modelled in tests/test_seed_edge_cases.py)
    hold of it"""
    c_lo, c_hi = int(soa.cand_ctg_off[k]), int(soa.cand_ctg_off[k + 1])
    vals = [v[(idx >= c_lo) & (idx < c_hi)] for idx, v in tile_entries(soa)[c_lo // TILE:(max(c_hi, 1) - 1) // TILE + 1]]
    return np.unique(np.concatenate(vals + [np.zeros(0, dtype=np.int64)])).astype(np.uint32) if c_lo < c_hi else np.zeros(0, dtype=np.uint32)


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.set_debug(0)
    c.close()


_ref, _resident = {}, {}


def reference(name):
    """computed once per case, from the input alone, and shared by its three debug words (the last case's only: they come one after
    the other)"""
    if name not in _ref:
        _ref.clear()
        soa = case(name)
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


def test_the_new_cases_have_their_shape():
    """(CPU work only, but it belongs with the cases) the counts the names promise"""
    for n in (1, 255, 256, 257, 511, 512, 513, 769, 1023, 1024, 1025):
        assert CASES['candidates_%d' % n]().n_cands == n
    for at in (255, 256, 257, 767, 768, 769):
        soa = CASES['contig_border_at_%d' % at]()
        assert list(soa.cand_ctg_off) == [0, at, 1100]
    soa = CASES['three_contigs_middle_seed']()
    assert list(soa.cand_ctg_off) == [0, 300, 300, 301, 701]
    soa = CASES['seedless_contig_in_second_tile']()
    assert list(soa.cand_ctg_off) == [0, 256, 512, 612] and len(seed_set(soa, 1)) == 0 and len(seed_set(soa, 0)) > 0
    for name, tile in (('multi_ps_65_in_first_tile', 0), ('multi_ps_65_in_second_tile', 1)):
        soa = CASES[name]()
        groups = np.array([len(set(soa.mark_read[soa.cand_off[c]:soa.cand_off[c + 1]].tolist())) for c in range(soa.n_cands)])
        assert [int((groups[t * TILE:(t + 1) * TILE] > 1).sum()) for t in range(3)] == ([65, 0, 3] if tile == 0 else [0, 65, 3])
    soa = CASES['joint_range_70_inside']()
    s = seed_set(soa, 0)
    assert int(((s > 1080) & (s < 9000)).sum()) == 70 > E.OWN_WIN


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
