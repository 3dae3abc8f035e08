# coding=utf-8
"""Named E/F problems at the smallest shapes where ef_classify's addressing can go wrong: its prologue loads every offset, column
and start flag unconditionally at a clamped address, keeps a candidate's two offsets in registers, stages a pass of kChunk marks
with 16-byte index loads that start at m_begin & ~3, and hands out group-summary slots and seed records behind the walk.

The read table and the candidate columns come from tests.soa_fuzz.random_soa (one contig of exactly C candidates); the mark
lists are dealt again by that generator's recipe for the degrees a case asks for -- the generator itself gives every candidate
at least one mark and cannot place a tile's span -- and small arrays are set by hand where a case says so.
tests/test_classify_edge_cases.py checks on the CPU that every case has the shape it is named for and that the C oracle takes
it; tests/test_gpu_classify_edges.py runs them on the device."""
import numpy as np

from duet_amd import engine, synth
from tests import soa_fuzz

ABSENT = engine.MARK_ABSENT
TILE = 256            # kCandPerBlock
CHUNK = 3072          # kChunk
QUOTA = 64            # kC2Quota


class Soa(engine.EfSoA):
    """The arrays of an EfSoA without its constructor's checks: a candidate without marks and an index beyond the read table
    are what some cases are about."""

    def __init__(self, **kw):
        for name, dt in self.FIELDS:
            setattr(self, name, np.ascontiguousarray(kw[name], dtype=dt))
        self.read_off = np.asarray([0, len(self.read_tag)], dtype=np.uint32)


def dealt(seed, deg, ctg_off=None, absent_rate=5):
    """len(deg) candidates of one random_soa contig with deg[c] marks each (random_soa's recipe: reads around a centre, one mark
    in absent_rate without a tag); ctg_off: the contig offsets instead of [0, C]"""
    deg = np.asarray(deg, dtype=np.int64)
    C = len(deg)
    b = soa_fuzz.random_soa(seed, n_contigs=1, cands_per_contig=(C, C), reads_per_contig=(40, 300), deg=(1, 1),
                            empty_contig_rate=0, no_seed_contig_rate=0)
    rng = synth.SplitMix(0xC1A50000 + seed)
    R = b.n_reads
    off = np.concatenate([[0], np.cumsum(deg)])
    M = int(off[-1])
    centre = rng.below(C, R)
    spread = 1 + rng.one(max(2, R // 4))
    mr = (np.repeat(centre, deg) + rng.below(M, spread)) % R if M else np.zeros(0, dtype=np.int64)
    if M and absent_rate:
        mr = np.where(rng.chance(M, 1, absent_rate), ABSENT, mr)
    return Soa(cand_ctg_off=[0, C] if ctg_off is None else ctg_off, read_tag=b.read_tag, cand_pos=b.cand_pos, cand_svlen=b.cand_svlen,
               cand_svread=b.cand_svread, cand_refread=b.cand_refread, cand_gt_ok=b.cand_gt_ok, cand_off=off, mark_read=mr)


def degrees(seed, C, lo=1, hi=20):
    return synth.SplitMix(0xDE600000 + seed).between(C, lo, hi).astype(np.int64)


def kept_columns(C, seed):
    """columns under which every candidate passes the filter (svlen_thres 50, suppread_thres 2) and decides without dividing by zero"""
    rng = synth.SplitMix(0xC0100000 + seed)
    return dict(cand_pos=np.sort(rng.between(C, 1, 40000)), cand_svlen=np.full(C, 100), cand_svread=rng.between(C, 2, 12),
                cand_refread=rng.between(C, 0, 12), cand_gt_ok=np.ones(C, dtype=np.uint8))


def _tile_edge(C):
    def make():
        ctg = [0, C] if C < 3 else [0, C // 3, C // 3, C]                # (an empty contig in between)
        return dealt(10 + C, degrees(C, C), ctg)
    return make


def _mod4(r):
    """cand_off[256] = r and M = r (mod 4): the second tile's first 16-byte load starts r marks in front of its first mark, and the
    array's last 16-byte granule holds r marks"""
    def make():
        d = degrees(40 + r, 300, 2, 20)
        d[255] += (r - int(d[:256].sum())) % 4
        d[299] += (r - int(d.sum())) % 4
        return dealt(40 + r, d)
    return make


def _tile_without_marks():
    d = degrees(50, 3 * TILE)
    d[TILE:2 * TILE] = 0
    return dealt(50, d)


def _only_last_of_tile():
    d = degrees(51, 3 * TILE)
    d[TILE:2 * TILE - 1] = 0
    d[2 * TILE - 1] = 7
    return dealt(51, d)


def _span(first, second):
    """tile 0 spans `first` marks from mark 0, tile 1 `second` marks from its m_begin & ~3"""
    def make():
        d = degrees(60 + first % 7, 2 * TILE + 40, 6, 18)
        d[TILE - 1] += first - int(d[:TILE].sum())
        d[2 * TILE - 1] += (first & ~3) + second - int(d[:2 * TILE].sum())
        assert d.min() >= 1
        return dealt(60 + first % 7, d)
    return make


def _heavy():
    d = degrees(70, 300)
    d[100] = 9000
    return dealt(70, d)


def _no_reads():
    s = dealt(80, degrees(80, 300))
    return Soa(cand_ctg_off=s.cand_ctg_off, read_tag=np.zeros(0, dtype=np.uint64), cand_pos=s.cand_pos, cand_svlen=s.cand_svlen,
               cand_svread=s.cand_svread, cand_refread=s.cand_refread, cand_gt_ok=s.cand_gt_ok, cand_off=s.cand_off,
               mark_read=np.full(s.n_marks, ABSENT))


def _beyond_table():
    """every third candidate: the marks of ONE read, and between them indices at or beyond the table's size that are not all ones
    (n_reads, n_reads + 1, 2^31, 2^32 - 2).  Such a candidate sees at most one phase set, so this case is ef_classify's alone; the
    kernels behind it, which walk the marks of multi-PS candidates again, follow the same rule and have their own cases in
    tests/tag_lookup_edges.py."""
    d = degrees(81, 300, 4, 12)
    s = dealt(81, d)
    R = s.n_reads
    bad = np.array([R, R + 1, 1 << 31, 0xFFFFFFFE], dtype=np.int64)
    mr = s.mark_read.astype(np.int64)
    for c in range(0, 300, 3):
        lo, hi = int(s.cand_off[c]), int(s.cand_off[c + 1])
        mr[lo:hi] = (c * 7) % R
        mr[lo + 1:hi:2] = bad[(np.arange(lo + 1, hi, 2) + c) % 4]
    s.mark_read = mr.astype(np.uint32)
    return s


def as_absent(soa):
    """the problem the C oracle is asked instead: it indexes the table with whatever is not all ones, the library's contract
    (include/duet_ef.h: n_reads) is that an index at or beyond n_reads has no tag"""
    mr = np.where(soa.mark_read >= soa.n_reads, ABSENT, soa.mark_read)
    return Soa(**dict({n: getattr(soa, n) for n, _ in soa.FIELDS}, mark_read=mr))


def _one_read():
    s = dealt(82, degrees(82, 300))
    mr = np.where(s.mark_read == ABSENT, ABSENT, 0)
    return Soa(**dict({n: getattr(s, n) for n, _ in s.FIELDS}, read_tag=engine.pack_tags([1], [500], [7000]), mark_read=mr))


def _two_ps(n_two):
    """Tile 0: 256 kept candidates, the first of every 256 // n_two of which sees two phase sets (reads 0 and 1), the others one:
    n_two group summaries in a tile whose own slots number QUOTA.  Eight more candidates in a second tile see one phase set each
    (reads 0 or 2) and give the contig its two seeds -- a multi-PS candidate's vote counts seeds only."""
    def make():
        C = TILE + 8
        two = np.zeros(C, dtype=bool)
        two[:TILE:TILE // n_two] = True
        d = degrees(90 + n_two, C, 2, 6)
        off = np.concatenate([[0], np.cumsum(d)])
        mr = np.zeros(int(off[-1]), dtype=np.int64)
        for c in np.nonzero(two)[0]:
            mr[off[c] + 1:off[c + 1]:2] = 1
        for c in range(TILE + 1, C, 2):
            mr[off[c]:off[c + 1]] = 2
        tags = engine.pack_tags([1, 2, 1], [100, 8100, 50], [1000, 2000, 2000])
        return Soa(cand_ctg_off=[0, C], read_tag=tags, cand_off=off, mark_read=mr, **kept_columns(C, 90))
    return make


def _starts():
    """tile 1 of two: contigs open at its lanes 0, 63, 64 and 255, and every candidate of the problem has the same seed (one mark of
    one voting read) -- a seed dropped as a repeat ACROSS a start leaves that contig without seeds, and all its candidates drop"""
    C = 2 * TILE
    return Soa(cand_ctg_off=[0, TILE, TILE + 63, TILE + 64, TILE + 255, C], read_tag=engine.pack_tags([1], [100], [5000]),
               cand_off=np.arange(C + 1), mark_read=np.zeros(C, dtype=np.int64), **kept_columns(C, 95))


CASES = dict([('cands_%d' % C, _tile_edge(C)) for C in (1, 255, 256, 257, 513)] +
             [('offsets_mod4_%d' % r, _mod4(r)) for r in (1, 2, 3)])
CASES.update({
    'tile_without_marks': _tile_without_marks,
    'only_last_of_tile_has_marks': _only_last_of_tile,
    'span_3072_then_3073': _span(CHUNK, CHUNK + 1),
    'span_3073_then_3072': _span(CHUNK + 1, CHUNK),
    'candidate_of_9000_marks': _heavy,
    'no_reads': _no_reads,
    'indices_beyond_the_table': _beyond_table,
    'one_read': _one_read,
    'two_ps_256': _two_ps(256),
    'two_ps_64': _two_ps(64),
    'starts_at_lanes_0_63_64_255': _starts,
})
NAMES = tuple(CASES)
_made = {}


def case(name):
    if name not in _made:
        _made[name] = CASES[name]()
    return _made[name]
