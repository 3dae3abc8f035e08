# coding=utf-8
"""CPU: every case of tests/seed_edges.py has the structure it is named for -- shown from the input alone by the small models of
ef_classify's seeds_tile, of ef_seed_sort's gather and branches and of ef_finalize_own's set stated HERE (nothing is imported from
the library but the tag layout) -- and the C oracle takes it with a result worth comparing.  The models are the reference for the
shape, the oracle for the result; tests/test_gpu_seed_edges.py then holds the device to both."""
import numpy as np
import pytest

from oracle import c_oracle
from tests import seed_edges as E

TILE = E.TILE


# ---- the models -----------------------------------------------------------------------------------------------------------

def kept_mask(soa):
    return (soa.cand_svlen >= 50) & (soa.cand_svread >= 2) & (soa.cand_gt_ok != 0)


def mark_tags(soa):
    """per mark: tagged, voter, ps"""
    tagged = soa.mark_read != E.ABSENT
    tag = soa.read_tag[np.where(tagged, soa.mark_read, 0)]
    tagged &= tag != np.uint64(0xFFFFFFFFFFFFFFFF)
    ps = (tag & np.uint64(0xFFFFFFFF)).astype(np.int64)
    voter = tagged & (((tag >> np.uint64(32)) & np.uint64(0x3FFFFFFF)) <= 8100)
    return tagged, voter, ps


def cand_seeds(soa):
    """per candidate: the seed it contributes (a kept candidate that sees ONE phase set and has a voter), or -1"""
    tagged, voter, ps = mark_tags(soa)
    off = soa.cand_off.astype(np.int64)[:-1]
    lo = np.minimum.reduceat(np.where(tagged, ps, 1 << 40), off)
    hi = np.maximum.reduceat(np.where(tagged, ps, -1), off)
    votes = np.add.reduceat(voter.astype(np.int64), off)
    return np.where(kept_mask(soa) & (lo == hi) & (votes > 0), lo, -1)


def askers_of(soa):
    """kept candidates without a tagged mark: ps becomes the nearest seed outright"""
    tagged, _, _ = mark_tags(soa)
    n = np.add.reduceat(tagged.astype(np.int64), soa.cand_off.astype(np.int64)[:-1])
    return np.nonzero(kept_mask(soa) & (n == 0))[0]


def may_ask(soa):
    """candidates for whose position ef_finalize_own may want the nearest seed: askers and every multi-PS candidate"""
    tagged, _, ps = mark_tags(soa)
    off = soa.cand_off.astype(np.int64)[:-1]
    lo = np.minimum.reduceat(np.where(tagged, ps, 1 << 40), off)
    hi = np.maximum.reduceat(np.where(tagged, ps, -1), off)
    return kept_mask(soa) & ((hi < 0) | (lo != hi))


def contig_of(soa, c):
    return np.searchsorted(soa.cand_ctg_off.astype(np.int64), c, side='right') - 1


def tile_entries(soa):
    """seeds_tile: per tile of 256 candidates the (candidate, seed) it keeps -- a seed equal to the previous seed-bearing
    candidate's OF THE TILE is dropped unless a contig starts in between"""
    s = cand_seeds(soa)
    idx = np.nonzero(s >= 0)[0]
    v = s[idx]
    k = contig_of(soa, idx)
    drop = np.zeros(len(idx), dtype=bool)
    drop[1:] = (v[1:] == v[:-1]) & (idx[1:] // TILE == idx[:-1] // TILE) & (k[1:] == k[:-1])
    idx, v = idx[~drop], v[~drop]
    n_tiles = -(-soa.n_cands // TILE)
    cut = np.searchsorted(idx // TILE, np.arange(n_tiles + 1))
    return [(idx[cut[t]:cut[t + 1]], v[cut[t]:cut[t + 1]]) for t in range(n_tiles)]


def seed_list(soa, k):
    """ef_seed_sort's gathered list of contig k: its tiles' entries of this contig in candidate order; a tile's first entry that
    repeats the last entry of the tile in front of it (when that one is this contig's too) is dropped -- except in an edge tile of
    more than kLongCnt entries, which the whole workgroup filters without looking at its neighbour"""
    c_lo, c_hi = int(soa.cand_ctg_off[k]), int(soa.cand_ctg_off[k + 1])
    if c_lo == c_hi:
        return np.zeros(0, dtype=np.int64)
    ent = tile_entries(soa)
    b_lo, b_hi = c_lo // TILE, (c_hi - 1) // TILE
    assert b_hi - b_lo + 1 <= 1024                     # (one tile per thread: the rule looks exactly one tile back)
    interior = lambda b: b * TILE >= c_lo and ((b + 1) * TILE <= c_hi or c_hi == soa.n_cands)
    out = []
    for b in range(b_lo, b_hi + 1):
        idx, v = ent[b]
        coop = not interior(b) and len(idx) > E.LONG_CNT and (b == b_lo or b == b_hi)
        mine = v[(idx >= c_lo) & (idx < c_hi)]
        if len(mine) and not coop and b > b_lo and len(ent[b - 1][0]) and ent[b - 1][0][-1] >= c_lo and ent[b - 1][1][-1] == mine[0]:
            mine = mine[1:]
        out.append(mine)
    return np.concatenate(out)


def descents(a):
    return int((a[1:] < a[:-1]).sum())


def oddeven(a, rounds):
    """oddeven_rounds: -> (the list afterwards, whether a round moved nothing)"""
    a = a.copy()
    for _ in range(rounds):
        moved = False
        for par in (0, 1):
            i = np.arange(par, len(a) - 1, 2)
            sw = i[a[i] > a[i + 1]]
            a[sw], a[sw + 1] = a[sw + 1].copy(), a[sw].copy()
            moved = moved or len(sw) > 0
        if not moved:
            return a, True
    return a, False


def probe_lengths(keys, slot_fn, n_slots):
    """linear probing, keys inserted in the order given: -> (table, per key the number of slots it passed)"""
    tab = np.full(n_slots, -1, dtype=np.int64)
    passed = []
    for key in keys:
        h, n = int(slot_fn(key)), 0
        while tab[h] != -1 and tab[h] != key:
            h, n = (h + 1) % n_slots, n + 1
        tab[h] = key
        passed.append(n)
    return tab, np.array(passed)


def hash_takes(lst):
    """ef_seed_sort's hash set takes the list: at most kSeedTab / 2 distinct values and no probe sequence beyond 32 -- the threads
    insert in no fixed order, so the answer has to be the same for the list's order and its reverse"""
    first = lst[np.sort(np.unique(lst, return_index=True)[1])]
    if len(first) > E.SEED_TAB // 2:
        return False
    fwd = probe_lengths(first, E.sort_slot, E.SEED_TAB)[1].max() <= E.SEED_PROBES
    bwd = probe_lengths(first[::-1], E.sort_slot, E.SEED_TAB)[1].max() <= E.SEED_PROBES
    assert fwd == bwd, 'the case leaves the hash set to the order of the threads'
    return bool(fwd)


def sort_branch(lst, no_hash=False):
    """the branch conditions of ef_seed_sort in the order the kernel states them (host-planned launch) -> (branch, descents there)"""
    n = len(lst)
    if n == 0:
        return 'empty', 0
    if n > E.SORT_LDS:
        return ('hbm_network' if descents(lst) else 'hbm_sorted'), descents(lst)
    a, runs = lst, descents(lst)
    if runs == 0:
        return 'sorted', 0
    if runs > E.FEW_RUNS:
        a, done = oddeven(a, 2)
        if done:
            return 'rounds', 0
        runs = descents(a)
    if n >= 256 and runs > E.FEW_RUNS and not no_hash and hash_takes(a):
        return 'hash', runs
    if runs >= E.MAX_RUNS:
        a, done = oddeven(a, 4)
        if done:
            return 'rounds', 0
        runs = descents(a)
    return ('merge' if runs < E.MAX_RUNS else 'network'), runs


def window(soa, tile, k):
    """-> (pmin, pmax, the distinct seeds of contig k strictly inside): the asking range of the tile's candidates of contig k"""
    c_lo, c_hi = int(soa.cand_ctg_off[k]), int(soa.cand_ctg_off[k + 1])
    c = np.arange(max(c_lo, tile * TILE), min(c_hi, (tile + 1) * TILE))
    c = c[may_ask(soa)[c]]
    pos = soa.cand_pos[c].astype(np.int64)
    S = np.unique(seed_list(soa, k))
    return int(pos.min()), int(pos.max()), S[(S > pos.min()) & (S < pos.max())]


def own_path(soa, tile, k):
    """what ef_finalize_own does for the tile's candidates of contig k: 'walk' (more distinct seeds than kOwnKeys), 'sorted' (more
    seeds in the window than kOwnWin), 'window'"""
    u = len(np.unique(seed_list(soa, k)))
    if u > E.OWN_KEYS:
        return 'walk'
    return 'sorted' if len(window(soa, tile, k)[2]) > E.OWN_WIN else 'window'


def tiles_of(soa, k):
    c_lo, c_hi = int(soa.cand_ctg_off[k]), int(soa.cand_ctg_off[k + 1])
    return c_lo // TILE, (c_hi - 1) // TILE


def finalize_view(n_one):
    """ef_finalize (host-planned, K <= kSmallK) for a tile of one contig: the seeds it holds in registers / LDS / leaves in HBM"""
    return 'ahead' if n_one <= 1024 else ('lds' if n_one <= E.ONE_LDS else 'hbm')


def n_distinct(soa, k=0):
    return len(np.unique(seed_list(soa, k)))


def asking_tile(soa):
    t = np.unique(askers_of(soa) // TILE)
    assert len(t) == 1
    return int(t[0])


# ---- every case ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', E.NAMES)
def test_the_oracle_takes_the_case(name):
    soa = E.case(name)
    rc, pred, ps = c_oracle.ef(soa, 50, 2)
    assert rc == 0
    assert int((pred != 0).sum()) > 0, 'nothing is phased: the case would compare zeros'
    ask = askers_of(soa)
    assert len(ask) > 0
    assert len(np.unique(ps[ask])) >= 2, 'every asker gets the same answer: the case would compare constants'
    # the models agree with the oracle on what the seeds are: an asker's ps is the nearest value of the model's seed set
    for c in ask[:: max(1, len(ask) // 8)]:
        k = int(contig_of(soa, c))
        S = np.unique(seed_list(soa, k))
        if len(S) == 0:
            assert ps[c] == 0 and pred[c] == 0
            continue
        d = np.abs(S - int(soa.cand_pos[c]))
        assert ps[c] == S[d == d.min()].max(), (name, c)


def test_the_builder():
    soa = E.build([[(10, E.seed(500)), (20, E.ASK), (30, E.two(500, 2, 600, 1)), (40, E.three((1, 1), (2, 1), (3, 2))), (50, E.SKIP)], [],
                   [(5, E.seed(7))]])
    assert soa.cand_ctg_off.tolist() == [0, 5, 5, 6] and soa.read_off.tolist() == [0, 5, 5, 6]
    assert np.diff(soa.cand_off.astype(np.int64)).tolist() == [2, 1, 3, 4, 1, 2]
    assert cand_seeds(soa).tolist() == [500, -1, -1, -1, -1, 7]
    assert askers_of(soa).tolist() == [1] and may_ask(soa).tolist() == [False, True, True, True, False, False]
    assert soa.cand_svlen.tolist() == [100, 100, 100, 100, 10, 100]
    old = E.seed_list_soa([[5, 5, 9], [3]])
    assert old.cand_pos.tolist() == [1000, 1007, 1014, 1000] and old.n_marks == 8 and old.n_reads == 4
    assert [np.unique(seed_list(old, k)).tolist() for k in range(2)] == [[5, 9], [3]]
    assert seed_list(old, 0).tolist() == [5, 9]


def test_the_hash_classes():
    for slot in (0, 777, E.OWN_TAB - 1):
        m = E.OWN_MEMBERS[slot]
        assert len(m) > 400 and np.all(E.own_slot(m) == slot)
        assert all((int(v) * 2654435761 % (1 << 32)) >> 21 == slot for v in m[:5])
    for slot in (0, 1234, E.SEED_TAB - 1):
        m = E.SORT_MEMBERS[slot]
        assert len(m) > 200 and np.all(E.sort_slot(m) == slot)
        assert all((int(v) * 2654435761 % (1 << 32)) >> 20 == slot for v in m[:5])


@pytest.mark.parametrize('n', (1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097))
def test_distinct(n):
    soa = E.case('distinct_%d' % n)
    assert soa.n_contigs == 2 and n_distinct(soa, 0) == n and len(seed_list(soa, 0)) == n
    pos = soa.cand_pos[:soa.cand_ctg_off[1]].astype(np.int64)
    assert np.all(np.diff(pos) >= 0)                                        # in position order
    assert sort_branch(seed_list(soa, 0))[0] == 'sorted'
    b_lo, b_hi = tiles_of(soa, 0)
    assert b_hi > b_lo and tiles_of(soa, 1)[0] == b_hi                      # the small contig follows in the same last tile
    assert own_path(soa, b_hi, 1) == 'window'
    walk = n > E.OWN_KEYS
    for t in range(b_lo, b_hi + 1):
        assert (own_path(soa, t, 0) == 'walk') == walk
    assert finalize_view(n) == ('ahead' if n <= 1024 else 'lds' if n <= 4096 else 'hbm')
    S = np.unique(seed_list(soa, 0))
    ask = askers_of(soa)
    ask = ask[ask < soa.cand_ctg_off[1]]
    p = soa.cand_pos[ask].astype(np.int64)
    assert (p < S[0]).any() and (p > S[-1]).any() and np.isin(p, S).any()
    assert np.isin(2 * p, S[1:] + S[:-1]).any()                             # exactly halfway between two seeds
    assert len(np.unique(ask // TILE)) >= 3 or n > 4000
    kinds = np.diff(soa.cand_off.astype(np.int64))
    assert (kinds >= 3).sum() >= 4


def test_last_contig_of_one_candidate():
    soa = E.case('last_contig_of_one_candidate')
    K = soa.n_contigs
    assert soa.cand_ctg_off[K] - soa.cand_ctg_off[K - 1] == 1 and n_distinct(soa, K - 1) == 1
    assert n_distinct(soa, K - 2) == 1100 and finalize_view(1100) == 'lds'
    # the prefetch of the last tile's first contig reaches beyond the seed buffer's C + K words
    k0 = int(contig_of(soa, (soa.n_cands - 1) // TILE * TILE))
    base = int(soa.cand_ctg_off[k0]) + k0 + 1
    assert base + 255 + 768 > soa.n_cands + K - 1


@pytest.mark.parametrize('name,w,distinct,path', (('window_63', 63, 69, 'window'), ('window_64', 64, 70, 'window'),
                                                  ('window_65', 65, 71, 'sorted'), ('window_65_of_1023', 65, 1023, 'sorted'),
                                                  ('window_65_of_1024', 65, 1024, 'sorted'), ('window_65_of_1025', 65, 1025, 'walk'),
                                                  ('window_65_of_65', 65, 65, 'sorted'), ('window_65_of_129', 65, 129, 'sorted')))
def test_window(name, w, distinct, path):
    soa = E.case(name)
    t = asking_tile(soa)
    pmin, pmax, inside = window(soa, t, 0)
    S = np.unique(seed_list(soa, 0))
    assert len(inside) == w and len(S) == distinct and own_path(soa, t, 0) == path
    if name != 'window_65_of_65':
        assert pmin in S and pmax in S                                      # a seed ON either end: in neither list nor window
    else:
        assert pmin < S[0] and pmax > S[-1]
    assert len(cand_seeds(soa)[t * TILE:(t + 1) * TILE].nonzero()[0]) == TILE and np.all(cand_seeds(soa)[t * TILE:(t + 1) * TILE] < 0)
    s = cand_seeds(soa)
    s = s[s >= 0]
    assert len(s) > len(np.unique(s))                                       # seeds repeated in several tiles
    p = soa.cand_pos[askers_of(soa)].astype(np.int64)
    assert np.isin(p, S).sum() >= 3 and np.isin(2 * p, S[1:] + S[:-1]).sum() >= 3
    if path == 'sorted':
        assert (len(S) + 63) // 64 == {71: 2, 1023: 16, 1024: 16, 65: 2, 129: 3}[distinct]      # own_sort_set's blocks


@pytest.mark.parametrize('n', (3, 4, 7, 8, 16, 17, 24, 25, 256))
def test_tile_entries(n):
    soa = E.case('tile_entries_%d' % n)
    ent = tile_entries(soa)
    assert len(ent[1][0]) == n and all(len(e[0]) == 0 for e in ent[3:])
    for t in range(3, len(ent)):                                            # the tiles of askers: one on every entry, the window list
        assert own_path(soa, t, 0) == 'window'
    assert np.isin(ent[1][1], soa.cand_pos[askers_of(soa)]).all()
    lone = int(ent[1][1][-1])
    assert (cand_seeds(soa) == lone).sum() == 1
    rc, pred, ps = c_oracle.ef(soa, 50, 2)
    ask = askers_of(soa)
    assert (ps[ask[ask < TILE]] == lone).any()
    assert (ps[:TILE][np.diff(soa.cand_off.astype(np.int64))[:TILE] == 3] == lone).all()       # the two-group candidate of tile 0


def test_tile_repeat_across_tiles():
    one, split = E.case('tile_repeat_across_tiles'), E.case('tile_repeat_across_tiles_contig_start')
    assert np.array_equal(cand_seeds(one), cand_seeds(split))
    assert cand_seeds(one)[[250, 261, 319, 320]].tolist() == [7000, 7000, 8000, 8000]
    assert [e[1].tolist() for e in tile_entries(one)] == [[6000, 7000], [7000, 8000, 9000]]           # lane 64's repeat dropped
    assert seed_list(one, 0).tolist() == [6000, 7000, 8000, 9000]                                   # ... and the one across the tiles
    assert split.cand_ctg_off.tolist() == [0, 256, 320, 512]
    assert [e[1].tolist() for e in tile_entries(split)] == [[6000, 7000], [7000, 8000, 8000, 9000]]
    assert [seed_list(split, k).tolist() for k in range(3)] == [[6000, 7000], [7000, 8000], [8000, 9000]]


@pytest.mark.parametrize('name,total,side', (('edge_tile_17_lo', 17, 'lo'), ('edge_tile_17_hi', 17, 'hi'), ('edge_tile_16_lo', 16, 'lo')))
def test_edge_tile(name, total, side):
    soa = E.case(name)
    idx, v = tile_entries(soa)[1]
    assert len(idx) == total
    k = 1 if side == 'lo' else 0
    c_lo, c_hi = int(soa.cand_ctg_off[k]), int(soa.cand_ctg_off[k + 1])
    b_lo, b_hi = tiles_of(soa, k)
    assert (b_lo if side == 'lo' else b_hi) == 1 and b_hi > b_lo and soa.cand_ctg_off[1] % TILE == TILE // 2
    assert c_hi < soa.n_cands                                               # (a last contig's last tile counts as interior)
    mine = (idx >= c_lo) & (idx < c_hi)
    assert mine.sum() == total - 4 and (~mine).sum() == 4
    lone = int(v[mine][-1])
    assert (cand_seeds(soa) == lone).sum() == 1
    rc, pred, ps = c_oracle.ef(soa, 50, 2)
    ask = askers_of(soa)
    assert (ps[ask[(ask >= c_lo) & (ask < c_hi)]] == lone).any()
    assert len(seed_list(soa, k)) == n_distinct(soa, k) == total - 4 + 1 + (1 if side == 'lo' else 0)


@pytest.mark.parametrize('n', (256, 257))
def test_long_tiles(n):
    soa = E.case('long_tiles_%d' % n)
    ent = tile_entries(soa)
    assert len(ent) == n and all(len(e[0]) == E.LONG_CNT + 1 for e in ent)
    assert sum(1 for e in ent if len(e[0]) > E.LONG_CNT) == n and (n > E.LONG_TILES) == (n == 257)
    lst = seed_list(soa, 0)
    assert len(lst) == 17 * n == n_distinct(soa) and sort_branch(lst)[0] == 'sorted'


def test_first_contigs_empty():
    soa = E.case('first_contigs_empty')
    off = soa.cand_ctg_off.astype(np.int64)
    assert np.all(off[:4] == 0) and off[-1] <= TILE
    assert [n_distinct(soa, k) for k in range(7)] == [0, 0, 0, 0, 2, 0, 5]
    rc, pred, ps = c_oracle.ef(soa, 50, 2)
    for k in (3, 5):
        assert np.all(pred[off[k]:off[k + 1]] == 0) and np.all(ps[off[k]:off[k + 1]] == 0)


@pytest.mark.parametrize('name,n_tiles,entry', (('tiles_512', 512, 5), ('tiles_513_entry_1', 513, 1), ('tiles_513_entry_5', 513, 5),
                                                ('tiles_513_entry_12', 513, 12), ('tiles_513_entry_30', 513, 30),
                                                ('tiles_769', 769, 5)))
def test_tiles(name, n_tiles, entry):
    soa = E.case(name)
    assert soa.n_contigs == 1 and tiles_of(soa, 0) == (0, n_tiles - 1) and soa.n_cands == n_tiles * TILE
    assert np.all(np.diff(soa.cand_pos.astype(np.int64)) >= 0)
    ent = tile_entries(soa)
    where = [(t, j) for t, e in enumerate(ent) for j, v in enumerate(e[1]) if v == 50]
    assert where == [(n_tiles - 1, entry)]                                  # the lone seed: tile and entry index
    assert 25 <= n_distinct(soa) <= 35 and own_path(soa, 0, 0) == 'window'
    rc, pred, ps = c_oracle.ef(soa, 50, 2)
    assert ps[1] == 50 and ps[2] == 50 and ps[3] == 50                      # tile 0: the asker and both two-group candidates
    assert (n_tiles > E.PRE_TILES) == (n_tiles != 512)
    S = np.unique(seed_list(soa, 0))
    assert len(np.setdiff1d(S, ps[askers_of(soa)])) <= 2                    # nearly every seed, the later trips' too, is an asker's answer


@pytest.mark.parametrize('n_desc', (4, 5, 31, 32, 33))
def test_runs(n_desc):
    few, many = E.case('runs_%d_of_300' % n_desc), E.case('runs_%d_of_3000' % n_desc)
    for soa, distinct in ((few, 300), (many, 3000)):
        lst = seed_list(soa, 0)
        assert len(lst) == distinct == n_distinct(soa) and len(lst) >= 256
        if n_desc > E.FEW_RUNS:
            after2, done = oddeven(lst, 2)
            assert descents(lst) > E.FEW_RUNS and not done and descents(after2) == n_desc
            if n_desc >= E.MAX_RUNS:                                        # four more rounds, and still as many: the network
                after6, done = oddeven(lst, 6)
                assert not done and descents(after6) >= E.MAX_RUNS
        else:
            assert descents(lst) == n_desc                                  # five long runs as they come: no rounds
    ladder = 'merge' if n_desc < E.MAX_RUNS else 'network'
    assert sort_branch(seed_list(few, 0))[0] == ('hash' if n_desc > E.FEW_RUNS else 'merge')
    assert sort_branch(seed_list(few, 0), no_hash=True)[0] == ladder
    assert sort_branch(seed_list(many, 0))[0] == ladder
    if ladder == 'merge':
        assert sort_branch(seed_list(many, 0))[1] == n_desc


def test_runs_5_at_256_entries():
    a, b = seed_list(E.case('runs_5_of_255'), 0), seed_list(E.case('runs_5_of_256'), 0)
    assert (len(a), len(b)) == (255, 256)
    assert sort_branch(a) == ('merge', 5) and sort_branch(b) == ('hash', 5)
    assert descents(a) > E.FEW_RUNS and descents(b) > E.FEW_RUNS


@pytest.mark.parametrize('n', (2047, 2048, 2049))
def test_hash_distinct(n):
    lst = seed_list(E.case('hash_distinct_%d' % n), 0)
    assert len(np.unique(lst)) == n == len(np.unique(E.sort_slot(lst)))      # no two values share a slot
    branch, left = sort_branch(lst)
    assert branch == ('hash' if n <= E.SEED_TAB // 2 else 'merge') and E.FEW_RUNS < left < E.MAX_RUNS


def test_hash_probe_chain():
    lst = seed_list(E.case('hash_probe_chain'), 0)
    slots = E.sort_slot(np.unique(lst)).astype(np.int64)
    assert np.bincount(slots).max() == 40 and len(np.unique(lst)) == 340
    branch, left = sort_branch(lst)
    assert branch == 'merge' and E.FEW_RUNS < left < E.MAX_RUNS and not hash_takes(oddeven(lst, 2)[0])
    assert probe_lengths(np.unique(lst), E.sort_slot, E.SEED_TAB)[1].max() > E.SEED_PROBES


@pytest.mark.parametrize('name,n,branch', (('list_15359', 15359, 'sorted'), ('list_15360', 15360, 'sorted'),
                                           ('list_15361', 15361, 'hbm_sorted'),
                                           ('list_15360_unsorted', 15360, 'network'), ('list_15361_unsorted', 15361, 'hbm_network')))
def test_list(name, n, branch):
    lst = seed_list(E.case(name), 0)
    assert len(lst) == n == len(np.unique(lst)) and sort_branch(lst)[0] == branch
    assert finalize_view(n) == 'hbm'


def test_own_chains():
    soa = E.case('own_chain_300')
    S = np.unique(seed_list(soa, 0))
    assert len(S) == 300 and len(np.unique(E.own_slot(S))) == 1
    tab, passed = probe_lengths(S, E.own_slot, E.OWN_TAB)
    assert passed.max() == 299 and (tab == -1).sum() == E.OWN_TAB - 300
    _, _, ps = mark_tags(soa)
    strangers = np.setdiff1d(np.unique(ps), S)
    assert (E.own_slot(strangers) == E.own_slot(S[:1])).sum() >= 5            # keys that walk the whole chain to its empty end
    assert np.isin(S, soa.cand_pos[askers_of(soa)]).all()                     # an asker ON every seed, answered from the window list
    assert all(own_path(soa, int(t), 0) == 'window' for t in np.unique(askers_of(soa) // TILE)[1:])
    soa = E.case('own_chain_wraps')
    S = np.unique(seed_list(soa, 0))
    tab, passed = probe_lengths(S, E.own_slot, E.OWN_TAB)
    assert len(S) == 160 and E.own_slot(S).min() == E.OWN_TAB - 8
    wrapped = tab[:160][tab[:160] >= 0]
    assert len(wrapped) >= 100 and np.all(E.own_slot(wrapped) >= E.OWN_TAB - 8)  # the chain runs over the table's end into slot 0 ...
    _, _, ps = mark_tags(soa)
    strangers = np.setdiff1d(np.unique(ps), S)
    assert (E.own_slot(strangers) == E.OWN_TAB - 1).any()                     # ... and a key of slot 2047 that is no member follows it
    assert np.isin(S, soa.cand_pos[askers_of(soa)]).all()
    assert all(own_path(soa, int(t), 0) == 'window' for t in np.unique(askers_of(soa) // TILE)[1:])


@pytest.mark.parametrize('k', (64, 65))
def test_contigs(k):
    soa = E.case('contigs_%d' % k)
    assert soa.n_contigs == k and (k <= E.SMALL_K) == (k == 64)
    n = [n_distinct(soa, i) for i in range(k)]
    assert max(n) == E.OWN_KEYS + 1 and n.index(max(n)) == k // 2 and min(n) >= 1
