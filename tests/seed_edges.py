# coding=utf-8
"""Named E/F problems at the capacity edges of the three kernels behind ef_classify -- ef_seed_sort, ef_finalize (four launch
variants) and ef_finalize_own -- and the builder they are made with.  Every constant below is one of duet_ef.hip's; each case puts
a contig exactly at, one below and one above the constant it is named for.  tests/test_seed_edge_cases.py shows on the CPU, from
the input alone, that every case has the structure it is named for and that the C oracle takes it;
tests/test_gpu_seed_edges.py runs them on the device.

The builder: a problem is a list of contigs, a contig a list of (position, kind) in the order given (position order is a property
of a case, not of the builder).  Kinds:
  seed(ps)                  kept, two marks of one voting read of phase set ps: it contributes seed ps
  ASK                       kept, no tagged mark: ps becomes the nearest seed to its position, ties to the larger seed
  two(ps_a, n_a, ps_b, n_b) kept, voters in two phase sets: the larger group that is a seed wins, else the nearest seed
  three((ps, n), ...)       three or more voter groups: the vote comes from the marks
  SKIP                      filtered out (svlen below the threshold): it occupies a slot, so seeds land on exact lanes and tiles
Reads belong to one contig; the read of phase set ps has haplotype 1 + ps % 2 and PC 10 + ps % 50 unless a seed says otherwise.

Counting convention of the runs_* cases: N is the number of DESCENTS the gathered list has when ef_seed_sort compares it with
kFewRuns and kMaxRuns -- for more than kFewRuns descents in the input that is after two rounds of odd-even transposition, which
turn the border between two long ascending runs into four descents, leave a single value far right of its place ("straggler") one
descent, and remove a transposition of neighbours.  runs_4 is five long runs as they come (four descents: no rounds are run)."""
import numpy as np

from duet_amd import engine

ABSENT = engine.MARK_ABSENT
TILE = 256               # kCandPerBlock
OWN_KEYS, OWN_TAB, OWN_WIN = 1024, 2048, 64          # kOwnKeys, kOwnTab, kOwnWin
PRE_TILES = 512          # kPre x 256
LONG_CNT, LONG_TILES = 16, 256                       # kLongCnt, kLongTiles
FEW_RUNS, MAX_RUNS = 4, 32                           # kFewRuns, kMaxRuns
SEED_TAB, SEED_PROBES = 4096, 32                     # kSeedTab; a probe sequence longer than this abandons the set
SORT_LDS, ONE_LDS, SMALL_K = 15360, 4096, 64         # kSortLds, kOneLds, kSmallK

SKIP, ASK = ('skip',), ('ask',)


def seed(ps, hap=None, pc=None):
    return ('seed', int(ps), hap, pc)


def two(ps_a, n_a, ps_b, n_b):
    return ('groups', (int(ps_a), n_a), (int(ps_b), n_b))


def three(*groups):
    assert len(groups) >= 3
    return ('groups',) + tuple((int(g), n) for g, n in groups)


def build(contigs):
    """-> engine.EfSoA.  contigs: per contig a list of (position, kind), laid down in the order given."""
    tags, mark_read, cand_off, ctg_off, read_off = [], [], [0], [0], [0]
    pos_col, svlen_col = [], []
    for cands in contigs:
        reads = {}

        def read(ps, hap=None, pc=None):
            key = (1 + ps % 2 if hap is None else hap, 10 + ps % 50 if pc is None else pc, ps)
            if key not in reads:
                reads[key] = len(tags)
                tags.append(key)
            return reads[key]

        for pos, kind in cands:
            svlen = 100
            if kind[0] == 'seed':
                r = read(kind[1], kind[2], kind[3])
                mark_read += [r, r]
            elif kind[0] == 'groups':
                for g, n in kind[1:]:
                    mark_read += [read(g)] * n
            else:
                mark_read.append(ABSENT)
                if kind[0] == 'skip':
                    svlen = 10
                else:
                    assert kind[0] == 'ask', kind
            cand_off.append(len(mark_read))
            pos_col.append(pos)
            svlen_col.append(svlen)
        ctg_off.append(len(pos_col))
        read_off.append(len(tags))
    C = len(pos_col)
    t = np.array(tags, dtype=np.int64).reshape(-1, 3)
    return engine.EfSoA(cand_ctg_off=ctg_off, read_off=read_off, read_tag=engine.pack_tags(t[:, 0], t[:, 1], t[:, 2]),
                        cand_pos=np.array(pos_col, dtype=np.int64), cand_svlen=svlen_col, cand_svread=np.full(C, 5),
                        cand_refread=np.full(C, 5), cand_gt_ok=np.ones(C, dtype=np.uint8), cand_off=cand_off,
                        mark_read=np.array(mark_read, dtype=np.uint64))


def seed_list_soa(seqs):
    """One contig per sequence; candidate i of a contig is a class-1 candidate whose two marks are one read of phase set seq[i]:
    ef_seed_sort's list for the contig is seq with consecutive repeats dropped."""
    return build([[(1000 + 7 * i, seed(ps, 1 + i % 2, 10 + i % 50)) for i, ps in enumerate(seq)] for seq in seqs])


# ---- PS values that collide in a given hash -------------------------------------------------------------------------------

def own_slot(ps):
    """ef_finalize_own's hash: the top 11 bits of the product"""
    return ((np.asarray(ps, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(21)


def sort_slot(ps):
    """ef_seed_sort's hash: the top 12 bits of the product"""
    return ((np.asarray(ps, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(20)


def _by_slot(slot_fn, n_slots):
    ps = np.arange(1, 1 << 20, dtype=np.int64)
    s = slot_fn(ps).astype(np.int64)
    order = np.argsort(s, kind='stable')
    cut = np.searchsorted(s[order], np.arange(n_slots + 1))
    return [ps[order[cut[i]:cut[i + 1]]] for i in range(n_slots)]


OWN_MEMBERS = _by_slot(own_slot, OWN_TAB)            # per slot: the PS values below 2^20 that hash to it, ascending
SORT_MEMBERS = _by_slot(sort_slot, SEED_TAB)


# ---- pieces ----------------------------------------------------------------------------------------------------------------

def askers(S, n_ask, n_two, n_three, strangers=None):
    """(position, kind) that ask the seed set S (ascending, distinct) every kind of question: below the smallest seed, above the
    largest, exactly on a seed, exactly halfway between two seeds (the tie: the larger one), and between; two-group candidates whose
    larger group is a seed, whose larger group is NOT a seed (`strangers`: PS values outside S; default S + 3), with neither a seed
    (the nearest seed), with a tie of sizes; three-group candidates with and without a seed among the groups."""
    S = np.asarray(S, dtype=np.int64)
    n = len(S)
    member = set(S.tolist())
    if strangers is None:
        strangers = [int(v) + 3 for v in S[:: max(1, n // 7)]]
    strangers = [int(v) for v in strangers if int(v) not in member]
    assert len(strangers) >= 3
    at = lambda i, m: int(S[(i * 2654435761 + 12345) % n]) if m else strangers[i % len(strangers)]
    out = [(max(int(S[0]) - 5, 0), ASK), (int(S[-1]) + 7, ASK), (int(S[n // 2]), ASK)]
    mids = [j for j in range(n - 1) if (S[j + 1] - S[j]) % 2 == 0]
    if mids:
        j = mids[len(mids) // 2]
        out.append((int(S[j] + S[j + 1]) // 2, ASK))
    i = 0
    while len(out) < n_ask:
        j = (i * 7919 + 3) % n
        out.append((int(S[j]) + (1, 4, 0, 6)[i % 4], ASK))
        i += 1
    for i in range(n_two):
        p = int(S[(i * 104729 + 11) % n]) + i % 5
        kind = i % 5
        if kind == 0:
            out.append((p, two(at(i, 1), 3, at(i + 1, 1), 2)))
        elif kind == 1:
            out.append((p, two(at(i, 0), 3, at(i, 1), 2)))            # the larger group is no seed: the smaller one wins
        elif kind == 2:
            out.append((p, two(at(i, 0), 2, at(i + 1, 0), 1)))        # neither: the nearest seed
        elif kind == 3:
            out.append((p, two(at(i, 1), 2, at(i + 2, 1), 2)))        # a tie: the first seen
        else:
            out.append((p, two(at(i, 1), 1, at(i, 0), 4)))
    for i in range(n_three):
        p = int(S[(i * 1299709 + 5) % n]) + 2
        if i % 2 == 0:
            out.append((p, three((at(i, 0), 3), (at(i, 1), 2), (at(i + 3, 1), 2))))
        else:
            out.append((p, three((strangers[0], 1), (strangers[1], 2), (strangers[2], 1))))
    return out


def in_position_order(cands):
    return sorted(cands, key=lambda pk: pk[0])


def pad_tile(cands, n=TILE):
    """the candidates, then SKIPs up to a multiple of n"""
    fill = -len(cands) % n
    p = cands[-1][0] if cands else 0
    return list(cands) + [(p, SKIP)] * fill


def tile_with(lanes, kinds, pos0=0):
    """a tile of 256 candidates: kinds[i] at lane lanes[i], SKIP elsewhere; position = pos0 + lane unless the kind carries one"""
    t = [(pos0 + l, SKIP) for l in range(TILE)]
    for l, k in zip(lanes, kinds):
        t[l] = k if isinstance(k[0], (int, np.integer)) else (pos0 + l, k)
    return t


def spread(n):
    """n distinct lanes of a tile, from 0 to 255"""
    return sorted(set(int(x) for x in np.linspace(0, TILE - 1, n).round())) if n > 1 else [100]


def dealt(values, n_desc):
    """the ascending values dealt into n_desc + 1 ascending runs over the whole value range: exactly n_desc descents"""
    v = np.sort(np.asarray(values, dtype=np.int64))
    return np.concatenate([v[r::n_desc + 1] for r in range(n_desc + 1)])


def ask_each(S, per_tile=60):
    """tiles of askers, one ON every value of S (ascending), at most per_tile askers to a tile: fewer than kOwnWin seeds lie inside a
    tile's asking range, so ef_finalize_own answers from its window list -- and every single seed is somebody's answer"""
    S = [int(v) for v in S]
    out = []
    for i in range(0, len(S), per_tile):
        out += pad_tile([(v, ASK) for v in S[i:i + per_tile]])
    return out


def small_contig(base):
    S = [base + 100 * i for i in range(5)]
    return [(v, seed(v)) for v in S] + [(base + 150, ASK), (base + 40, ASK), (base + 320, two(S[1], 1, S[3], 2))]


# ---- the cases -------------------------------------------------------------------------------------------------------------

def _distinct(n, n_ask=30, n_two=30, n_three=10):
    def make():
        S = 1000 + 10 * np.arange(n, dtype=np.int64)
        big = in_position_order([(int(v), seed(v)) for v in S] + askers(S, n_ask, n_two, n_three))
        return build([big, small_contig(50000)])
    return make


def _last_contig_of_one():
    S = 1000 + 10 * np.arange(1100, dtype=np.int64)
    big = in_position_order([(int(v), seed(v)) for v in S] + askers(S, 12, 8, 4))
    front = [small_contig(200), small_contig(7000)]
    big += [(big[-1][0], SKIP)] * (-(len(big) + sum(len(c) for c in front)) % TILE)       # (the last contig opens a tile of its own)
    return build(front + [big, [(77, seed(4242))]])


def _window(w, distinct=None, with_ends=True):
    """tile 1 of the contig asks over [P0, P1]; w distinct seeds lie strictly inside, one ON each end (with_ends); the seeds are
    contributed by the other tiles, some by several of them; `distinct`: seeds of the contig in all (more lie outside the range)"""
    def make():
        P0 = 100000
        inside = [P0 + 100 * (j + 1) for j in range(w)]
        P1 = P0 + 100 * (w + 1)
        S = inside + ([P0, P1] if with_ends else [])
        n_out = (distinct or len(S) + 4) - len(S)
        S += [500 + 6 * j for j in range(n_out // 2)] + [300000 + 6 * j for j in range(n_out - n_out // 2)]
        assert len(set(S)) == len(S) == (distinct or len(S))
        rng = np.random.default_rng(w)
        order = rng.permutation(len(S))
        seeds = [(10 + i, seed(S[j])) for i, j in enumerate(order)]
        front = pad_tile(seeds[:len(seeds) // 2] or seeds)
        back = pad_tile(seeds[len(seeds) // 2:] + seeds[:40])              # (some seeds in several tiles)
        ask = [(P0, ASK), (P1, ASK)]
        for j in range(w):                                                 # (every seed of the window is somebody's answer)
            ask.append((inside[j], ASK))                                   # on a seed
            ask.append((inside[j] - 50, ASK))                              # an exact midpoint
            if j % 8 == 0:
                ask.append((inside[j] + 49, ASK))
        ask.append(((P0 + P1) // 2, two(7, 2, 9, 1)))                      # neither group a seed: the nearest
        ask.append((P0 + 130, two(inside[0], 1, inside[-1], 3)))
        ask.append((P1 - 130, three((7, 2), (9, 1), (11, 1))))
        assert len(ask) <= TILE
        mid = tile_with(spread(len(ask)), ask)
        return build([front + mid + back])
    return make


def _tile_entries(n):
    """tile 1 (interior) holds exactly n seed entries; its last one occurs nowhere else and an asker of tile 0 needs it; tiles of
    askers behind, one on every entry"""
    def make():
        lone = 500000
        t0 = tile_with([3, 70, 200, 201], [seed(1000), seed(2000), (lone - 10, ASK), (lone + 4, two(lone, 2, 777, 1))])
        vals = [10000 + 10 * j for j in range(n - 1)] + [lone]
        t1 = tile_with(spread(n), [seed(v) for v in vals])
        t2 = tile_with([0, 5, 9, 255], [seed(3000), (10020 + 2, ASK), (2500, ASK), seed(1000)])
        return build([t0 + t1 + t2 + ask_each(vals)])
    return make


def _tile_repeat(contig_start):
    """Tile 0's last seed is tile 1's first (7000), and inside tile 1 the last seed of wavefront 0 (lane 63) is the first of
    wavefront 1 (lane 64: 8000).  One contig: seeds_tile drops the repeat at lane 64, ef_seed_sort's gather the one across the
    tiles.  With contig starts at candidate 256 and at lane 64 of tile 1 every one of them stays: 7000 and 8000 are then the only
    seeds of the contig between the starts."""
    def make():
        t0 = tile_with([10, 250], [seed(6000), seed(7000)])
        t1a = [(300 + l, SKIP) for l in range(64)]
        t1a[5] = (305, seed(7000))
        t1a[20] = (7400, ASK)
        t1a[63] = (363, seed(8000))
        t1b = [(400 + l, SKIP) for l in range(TILE - 64)]
        t1b[0] = (400, seed(8000))
        t1b[30] = (7600, ASK)
        t1b[100] = (500, seed(9000))
        t1b[101] = (8400, two(8000, 2, 6000, 1))
        if contig_start:
            return build([t0, t1a, t1b])
        return build([t0 + t1a + t1b])
    return make


def _edge_tile(total, side):
    """Contig A ends and contig B begins in the middle of tile 1, which holds `total` seed entries: total - 4 of the contig under
    test (side 'lo': B, whose FIRST tile it is; 'hi': A, whose LAST tile it is) and 4 of its neighbour.  The last entry of the
    contig under test in that tile occurs nowhere else, and an asker needs it."""
    def make():
        mine = [20000 + 10 * j for j in range(total - 5)] + [90000]
        other = [40000 + 10 * j for j in range(4)]
        half = TILE // 2
        a1 = [(l, SKIP) for l in range(half)]
        b1 = [(l, SKIP) for l in range(half)]
        tgt, oth = (b1, a1) if side == 'lo' else (a1, b1)
        for l, v in zip(spread(len(mine))[:len(mine)], mine):
            tgt[l // 2] = (l // 2, seed(v))
        assert sum(1 for c in tgt if c[1][0] == 'seed') == len(mine)
        for l, v in zip((3, 40, 41, 120), other):
            oth[l] = (l, seed(v))
        rest_a = tile_with([1, 100, 101, 102], [seed(1000), (89990, ASK), (20005, ASK), (90010, two(90000, 2, 1000, 1))])
        rest_b = tile_with([2, 30, 31, 32], [seed(3000), (89000, ASK), (20015, ASK), (60000, two(90000, 1, 3000, 1))]) + \
            [(7, seed(3500)), (8, ASK)]
        return build([rest_a + a1, b1 + rest_b, small_contig(100)])
    return make


def _long_tiles(n_tiles):
    """n_tiles interior tiles of 17 entries each (kLongCnt + 1), ascending and distinct"""
    def make():
        cands = []
        lanes = spread(LONG_CNT + 1)
        for t in range(n_tiles):
            vals = [1000 + 10 * (t * (LONG_CNT + 1) + j) for j in range(LONG_CNT + 1)]
            extra_l, extra_k = [], []
            if t % 64 == 1:
                extra_l, extra_k = [7, 9], [(vals[3] + 5, ASK), (vals[5] + 2, two(vals[16], 1, 13, 2))]
            cands += tile_with(lanes + extra_l, [seed(v) for v in vals] + extra_k, pos0=vals[0])
        return build([cands])
    return make


def _first_contigs_empty():
    seedless_a = [(100, ASK), (200, SKIP), (300, two(5000, 2, 6000, 1))]
    seeded = [(5000, seed(5000)), (5100, ASK), (5600, ASK), (6000, seed(6000)), (5500, two(5000, 1, 6000, 2))]
    seedless_b = [(5000, ASK), (6000, three((5000, 1), (6000, 1), (7, 1)))]
    return build([[], [], [], seedless_a, seeded, seedless_b, small_contig(900)])


def _tiles(n_tiles, entry):
    """One contig of n_tiles tiles in position order, about 30 seeds; PS 50 occurs only as entry `entry` of the LAST tile, and an
    asker and a two-group candidate of tile 0 depend on it"""
    def make():
        cands = []
        has_seed = set(int(x) for x in np.linspace(0, n_tiles - 2, 28).round())
        for t in range(n_tiles - 1):
            p0 = 1000 + 300 * t
            lanes, kinds = [], []
            if t == 0:
                lanes, kinds = [1, 2, 3], [(p0 + 1, ASK), (p0 + 2, two(50, 2, 3000, 1)), (p0 + 3, two(77, 2, 50, 1))]
            if t in has_seed:
                lanes, kinds = lanes + [128], kinds + [seed(3000 + 300 * t)]
            if t == n_tiles // 2:
                lanes, kinds = lanes + [200], kinds + [ASK]
            if t - 7 in has_seed:                                  # (position 3100 + 300 (t - 7): nearest to that tile's seed)
                lanes, kinds = lanes + [0], kinds + [ASK]
            cands += tile_with(lanes, kinds, pos0=p0)
        p0 = 1000 + 300 * (n_tiles - 1)
        before = [3000 + 300 * sorted(has_seed)[i % len(has_seed)] for i in range(entry)]
        cands += tile_with(list(range(10, 10 + 2 * entry + 1, 2)) + [255], [seed(v) for v in before] + [seed(50), ASK], pos0=p0)
        return build([cands])
    return make


def shaped(values, borders, stragglers=0, local=0):
    """the ascending values dealt into borders + 1 long ascending runs; in the first run `stragglers` values moved 8 places to the
    right and `local` pairs of neighbours exchanged"""
    lst = dealt(values, borders).tolist()
    if len(lst) // (borders + 1) < 10 * (stragglers + local) + 6:
        return None
    for j in range(stragglers):
        lst.insert(10 * j + 9, lst.pop(10 * j + 1))
    for j in range(local):
        i = 10 * (stragglers + j) + 2
        lst[i], lst[i + 1] = lst[i + 1], lst[i]
    return np.array(lst, dtype=np.int64)


def _descents(a):
    return int((a[1:] < a[:-1]).sum())


def _two_rounds(a):
    a = a.copy()
    for i0 in (0, 1, 0, 1):
        i = np.arange(i0, len(a) - 1, 2)
        sw = i[a[i] > a[i + 1]]
        a[sw], a[sw + 1] = a[sw + 1].copy(), a[sw].copy()
    return a


def with_descents(values, n_desc):
    """a list of long ascending runs over the values that has n_desc descents where ef_seed_sort looks at their number: as it comes
    for n_desc <= kFewRuns, else after two odd-even rounds (which make four or five descents of a border between two runs, depending
    on where it falls: so the shape is searched for -- the most borders, then a few stragglers, and transpositions of
    neighbours until the input has more than kFewRuns descents)"""
    if n_desc <= FEW_RUNS:
        return dealt(values, n_desc)
    for borders in range(min(n_desc, 12), 0, -1):
        for stragglers in range(8):
            lst = shaped(values, borders, stragglers, max(0, FEW_RUNS + 1 - borders - stragglers))
            if lst is not None and _descents(lst) > FEW_RUNS and _descents(_two_rounds(lst)) == n_desc:
                return lst
    raise ValueError('no shape with %d descents' % n_desc)


def _runs(n_desc, distinct, n_ask=8):
    """a contig whose gathered list has n_desc descents where ef_seed_sort looks at their number, over `distinct` distinct values; a
    tile of askers behind"""
    def make():
        S = 5000 + 14 * np.arange(distinct, dtype=np.int64)
        cands = [(100 + i, seed(v)) for i, v in enumerate(with_descents(S, n_desc))]
        return build([pad_tile(cands) + askers(S, n_ask, 6, 2)])
    return make


def _hash_distinct(distinct):
    """`distinct` values with `distinct` different slots of ef_seed_sort's hash set (no probe sequence at all), in 7 runs"""
    def make():
        S = np.sort(np.array([m[len(m) // 2] for m in SORT_MEMBERS[:distinct]], dtype=np.int64))
        assert len(np.unique(sort_slot(S))) == distinct
        lst = dealt(S, 6)
        cands = [(100 + i, seed(v)) for i, v in enumerate(lst)]
        return build([pad_tile(cands) + askers(S, 6, 4, 2)])
    return make


def _hash_probe_chain():
    chain = SORT_MEMBERS[1234][:40]
    others = 3000 + 37 * np.arange(300, dtype=np.int64)
    S = np.unique(np.concatenate([chain, others]))
    lst = dealt(S, 6)
    cands = [(100 + i, seed(v)) for i, v in enumerate(lst)]
    return build([pad_tile(cands) + askers(S, 8, 6, 2)])


def _list(n, n_desc=0):
    def make():
        S = 2000 + 6 * np.arange(n, dtype=np.int64)
        lst = dealt(S, n_desc)
        cands = [(100 + i, seed(v)) for i, v in enumerate(lst)]
        return build([pad_tile(cands) + askers(S, 6, 4, 2)])
    return make


def _own_chain_300():
    slot = OWN_MEMBERS[777]
    S = np.sort(slot[:300])
    strangers = slot[300:320].tolist()                                     # the chain's slot, not in the set
    cands = [(100 + i, seed(v)) for i, v in enumerate(S)]
    return build([pad_tile(in_position_order(cands)) + pad_tile(askers(S, 12, 15, 4, strangers)) + ask_each(S)])


def _own_chain_wraps():
    S = np.sort(np.concatenate([OWN_MEMBERS[s][:20] for s in range(OWN_TAB - 8, OWN_TAB)]))
    strangers = OWN_MEMBERS[OWN_TAB - 1][20:26].tolist() + OWN_MEMBERS[0][:3].tolist()
    cands = [(100 + i, seed(v)) for i, v in enumerate(S)]
    return build([pad_tile(cands) + pad_tile(askers(S, 12, 15, 4, strangers)) + ask_each(S)])


def _contigs(k):
    def make():
        S = 1000 + 10 * np.arange(OWN_KEYS + 1, dtype=np.int64)
        big = in_position_order([(int(v), seed(v)) for v in S] + askers(S, 10, 10, 4))
        ctgs = [small_contig(100 + 1000 * i) if i % 3 else [(50, seed(900 + i)), (60, ASK)] for i in range(k - 1)]
        ctgs.insert(k // 2, big)
        return build(ctgs)
    return make


CASES = {}
for _n in (1023, 1024, 1025, 2047, 2048, 2049):
    CASES['distinct_%d' % _n] = _distinct(_n)
for _n in (4095, 4096, 4097):
    CASES['distinct_%d' % _n] = _distinct(_n, 6, 4, 2)
CASES['last_contig_of_one_candidate'] = _last_contig_of_one
for _n in (63, 64, 65):
    CASES['window_%d' % _n] = _window(_n)
CASES['window_65_of_1023'] = _window(65, OWN_KEYS - 1)
CASES['window_65_of_1024'] = _window(65, OWN_KEYS)
CASES['window_65_of_1025'] = _window(65, OWN_KEYS + 1)
CASES['window_65_of_65'] = _window(65, 65, with_ends=False)
CASES['window_65_of_129'] = _window(65, 129)
for _n in (3, 4, 7, 8, 16, 17, 24, 25, 256):
    CASES['tile_entries_%d' % _n] = _tile_entries(_n)
CASES['tile_repeat_across_tiles'] = _tile_repeat(False)
CASES['tile_repeat_across_tiles_contig_start'] = _tile_repeat(True)
CASES['edge_tile_17_lo'] = _edge_tile(17, 'lo')
CASES['edge_tile_17_hi'] = _edge_tile(17, 'hi')
CASES['edge_tile_16_lo'] = _edge_tile(16, 'lo')
CASES['long_tiles_256'] = _long_tiles(256)
CASES['long_tiles_257'] = _long_tiles(257)
CASES['first_contigs_empty'] = _first_contigs_empty
CASES['tiles_512'] = _tiles(512, 5)
CASES['tiles_513_entry_1'] = _tiles(513, 1)
CASES['tiles_513_entry_5'] = _tiles(513, 5)
CASES['tiles_513_entry_12'] = _tiles(513, 12)          # (the later trip's overflow slots by the lane, several steps)
CASES['tiles_513_entry_30'] = _tiles(513, 30)          # (... by the wavefront)
CASES['tiles_769'] = _tiles(769, 5)
for _n in (4, 5, 31, 32, 33):
    CASES['runs_%d_of_300' % _n] = _runs(_n, 300)
    CASES['runs_%d_of_3000' % _n] = _runs(_n, 3000)
CASES['runs_5_of_255'] = _runs(5, 255)
CASES['runs_5_of_256'] = _runs(5, 256)
for _n in (2047, 2048, 2049):
    CASES['hash_distinct_%d' % _n] = _hash_distinct(_n)
CASES['hash_probe_chain'] = _hash_probe_chain
for _n in (15359, 15360, 15361):
    CASES['list_%d' % _n] = _list(_n)
CASES['list_15360_unsorted'] = _list(15360, 40)
CASES['list_15361_unsorted'] = _list(15361, 40)
CASES['own_chain_300'] = _own_chain_300
CASES['own_chain_wraps'] = _own_chain_wraps
CASES['contigs_64'] = _contigs(64)
CASES['contigs_65'] = _contigs(65)

NAMES = tuple(CASES)
_made = {}


def case(name):
    if name not in _made:
        _made[name] = CASES[name]()
    return _made[name]
