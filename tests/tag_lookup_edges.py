# coding=utf-8
"""Named E/F problems for the tag lookup of the kernels behind ef_classify: ef_finalize's vote from the marks (for_each_tag),
the array-free walk of ef_finalize_own / ef_finalize_own_wide (own_each_tag) and their hash-set route (own_vote_from_marks).
A candidate gets there when it is kept, sees several phase sets and has no group summary.  The rule they have to follow
(include/duet_ef.h, duet_ef_problem): a mark has no tag when its index is ABSENT, when its index is at or beyond n_reads, or when
its tag word is all ones -- six spellings here: ABSENT, R, R + 1, 2^31, 2^32 - 2 and a valid index whose word is all ones.

Every case holds the same probes -- every kind of candidate x every degree x every place of the mark without a tag x every
spelling -- on a contig layout of its own.  Kinds (all kept at -s 50 -r 2):
  three_groups      voters of two seeds, two each, and of a phase set that is no seed: a tie that the first seen wins
  group_not_a_seed  voters of three phase sets that are no seeds: the nearest seed
  no_slot           voters of two seeds, in a tile whose candidates ask for more group summaries than its own slots and the
                    whole shared pool hold (the construction of classify_edges._two_ps): some of them are left without one
  all_stripped      several phase sets among the tagged marks, none of them a voter (PC 8101, PC 2^30 - 2, hap 3 with
                    PC 8101): once the mark without a tag is read as one, no voter group is left and the nearest seed decides
Tagged non-voters (the same three) are mixed into every probe that has room for them (degree 8 and up).
Degrees 3, 8, 9, 16, 17: the batch edges of the loops that load eight marks at a time; the mark without a tag is the first
(the address a padded lane is clamped to), the last, and marks 7, 8 and 15 where the candidate has them.  A candidate of 3 marks
has room for two tagged ones, so the two kinds with three voter groups start at degree 8.

What the bug did: an index of R or R + 1 read the bytes behind the table.  The probes are built so that a voter of the contig's
FIRST seed, hap 1, PC 0 in that place (GUARD: what the device tests write there) changes the call: the tie goes to the first
seed, a stranger's group or no group at all becomes the first seed's.  guard_variant() is that misreading as a valid problem;
canonical() is the problem every entry has to compute.  tests/test_tag_lookup_edge_cases.py shows on the CPU that the cases are
what they are named; tests/test_gpu_tag_lookup_edges.py runs them on the device."""
import numpy as np

from duet_amd import engine
from tests.classify_edges import Soa

ABSENT = engine.MARK_ABSENT
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
TILE, QUOTA = 256, 64                    # kCandPerBlock, kC2Quota
OWN_KEYS = 1024                          # kOwnKeys
PC_SAT = (1 << 30) - 2
DEGREES = (3, 8, 9, 16, 17)
KINDS = ('three_groups', 'group_not_a_seed', 'no_slot', 'all_stripped')
SPELLINGS = ('absent', 'R', 'R+1', '2^31', '2^32-2', 'all_ones_word')


def pool_slots(C):
    """c2_slots of duet_ef.hip without the tiles' own: the shared pool"""
    return max(C // 8, 256)


def places(deg):
    """where the mark without a tag sits: first, last, 7, 8, 15"""
    return sorted(set([0, deg - 1] + [p for p in (7, 8, 15) if p < deg]))


def probe_list(kinds):
    """(kind, degree, place, spelling) of every probe of the kinds, in a fixed order"""
    return [(k, d, p, s) for k in kinds for d in DEGREES if d >= 8 or k in ('no_slot', 'all_stripped')
            for p in places(d) for s in range(len(SPELLINGS))]


class Builder(object):
    """one problem: candidates appended contig after contig; reads are made on demand"""

    def __init__(self):
        self.tags, self.by_key = [], {}
        self.marks, self.cand_off, self.ctg_off = [], [0], [0]
        self.pos, self.svlen, self.kind = [], [], []
        self.blank = self.read(0, 0, 0)                                        # (soa(): the all-ones word at a valid index)

    def read(self, hap, pc, ps):
        key = (hap, pc, ps)
        if key not in self.by_key:
            self.by_key[key] = len(self.tags)
            self.tags.append(key)
        return self.by_key[key]

    def voter(self, ps, i=0):
        """a voting read of phase set ps: hap 1 with a small PC, or hap 2 with a large one"""
        return self.read(1, 10 + ps % 50, ps) if i % 2 == 0 else self.read(2, 4000 + ps % 100, ps)

    def cand(self, pos, marks, kind, svlen=100):
        self.marks += marks
        self.cand_off.append(len(self.marks))
        self.pos.append(pos)
        self.svlen.append(svlen)
        self.kind.append(kind)

    def seed(self, ps, pos=None):
        r = self.voter(ps, ps)
        self.cand(ps if pos is None else pos, [r, r], 'seed')

    def ask(self, pos):
        self.cand(pos, [ABSENT], 'ask')

    def skip(self, pos):
        self.cand(pos, [ABSENT], 'skip', svlen=10)

    def probe(self, S, X, pos, kind, deg, place, spelling):
        """S: the contig's seeds, ascending (S[0] is the one the guard words vote for); X: three phase sets that are no seeds"""
        A, B = S[0], S[1]
        nv = [self.read(1, 8101, B), self.read(2, PC_SAT, A), self.read(3, 8101, X[2])]
        room = deg - 1
        if kind == 'three_groups':
            body = [self.voter(B, 0), self.voter(A, 0), self.voter(A, 1), self.voter(B, 1), self.voter(X[0], 0)]
            fill = [self.voter(X[0], 1), self.voter(X[0], 0)]
        elif kind == 'group_not_a_seed':
            body = [self.voter(X[0], 0), self.voter(X[1], 1), self.voter(X[2], 0)]
            fill = [self.voter(X[1], 0), self.voter(X[2], 1)]
        elif kind == 'no_slot':
            body = [self.voter(B, place), self.voter(A, place + 1)]
            fill = [nv[0]]
        else:
            body = [nv[0], nv[1]]
            fill = [nv[2]]
        assert len(body) <= room, (kind, deg)
        if deg >= 8:
            body += nv[:room - len(body)]
        if kind == 'no_slot':                                                  # (pairs keep the tie)
            while len(body) + 2 <= room:
                body += [self.voter(B, len(body)), self.voter(A, len(body))]
        while len(body) < room:
            body.append(fill[len(body) % len(fill)])
        body.insert(place, ('no_tag', spelling))
        self.cand(pos, body, kind)

    def end_contig(self):
        self.ctg_off.append(len(self.pos))

    def soa(self):
        R = len(self.tags)
        spelled = (ABSENT, R, R + 1, 1 << 31, 0xFFFFFFFE, self.blank)
        mr = np.array([spelled[m[1]] if isinstance(m, tuple) else m for m in self.marks], dtype=np.int64)
        t = np.array(self.tags, dtype=np.int64).reshape(-1, 3)
        C = len(self.pos)
        tags = engine.pack_tags(t[:, 0], t[:, 1], t[:, 2])
        tags[self.blank] = ALL_ONES
        s = Soa(cand_ctg_off=self.ctg_off, read_tag=tags, cand_pos=self.pos,
                cand_svlen=self.svlen, cand_svread=np.full(C, 5), cand_refread=np.full(C, 1), cand_gt_ok=np.ones(C, dtype=np.uint8),
                cand_off=self.cand_off, mark_read=mr)
        assert s.read_tag[self.blank] == ALL_ONES
        s.kind = np.array(self.kind)
        for a in (s.read_tag, s.mark_read, s.cand_off, s.cand_pos, s.cand_ctg_off, s.kind):
            a.setflags(write=False)
        return s


def strangers(S):
    member = set(S)
    X = [v for v in range(S[0] + 1, S[0] + 40) if v not in member][:3]
    assert len(X) == 3
    return X


def probe_pos(S, i):
    """a position whose nearest seed is in the upper half of S: never S[0]"""
    up = S[len(S) // 2:]
    return up[i % len(up)] + i % 3


def probes(b, S, kinds, start=0, count=None):
    X = strangers(S)
    todo = probe_list(kinds)
    for i in range(count if count is not None else len(todo)):
        kind, deg, place, sp = todo[(start + i) % len(todo)]
        b.probe(S, X, probe_pos(S, start + i), kind, deg, place, sp)


def flood(b, S, n_tiles):
    """n_tiles full tiles of no_slot and all_stripped probes: each tile asks for 256 group summaries and has 64 slots of its own"""
    assert len(b.pos) % TILE == 0
    probes(b, S, ('no_slot', 'all_stripped'), count=n_tiles * TILE)


def seeded_contig(b, S, flood_tiles):
    """the flood tiles, the probes that need no flood, the contig's seeds and askers on and between them"""
    flood(b, S, flood_tiles)
    probes(b, S, ('three_groups', 'group_not_a_seed'))
    for v in S:
        b.seed(v)
    for i in range(0, len(S), max(1, len(S) // 16)):
        b.ask(S[i] + i % 4)


def _seeds(n):
    def make():
        b = Builder()
        seeded_contig(b, [1000 + 10 * j for j in range(n)], 3)                 # 3 tiles: 576 beyond their own slots, a pool of 256
        b.end_contig()
        return b.soa()
    return make


def _no_seeds():
    """contig 0: the probes and the flood and not one seed (every call 0); contig 1: the probes again, with seeds"""
    b = Builder()
    S = [1000 + 10 * j for j in range(12)]
    flood(b, S, 3)
    probes(b, S, ('three_groups', 'group_not_a_seed'))
    for v in S:
        b.cand(v, [b.read(1, 8101, v)] * 2, 'ask')                             # (a read of one PS that does not vote: no seed)
    b.end_contig()
    for _ in range(-len(b.pos) % TILE):
        b.skip(5)
    seeded_contig(b, S, 3)
    b.end_contig()
    return b.soa()


def _tiles_257():
    """one contig of more than 256 tiles: ef_finalize_own_wide by default.  A pool of C / 8 slots: 48 flood tiles ask for 9216"""
    b = Builder()
    S = [1000 + 50 * j for j in range(40)]
    seeded_contig(b, S, 48)
    n = 257 * TILE + 9 - len(b.pos)
    for i in range(n):
        b.ask(900 + i % 2200) if i % 5 else b.skip(7)
    b.end_contig()
    assert pool_slots(len(b.pos)) < 48 * (TILE - QUOTA)
    return b.soa()


def _contigs_65():
    """the contig with all probes first (its first seed is the one the guard words vote for), then 64 small ones"""
    b = Builder()
    seeded_contig(b, [80000 + 10 * j for j in range(20)], 3)
    b.end_contig()
    for k in range(64):
        S = [100 + 1000 * k, 400 + 1000 * k, 700 + 1000 * k]
        for v in S:
            b.seed(v)
        probes(b, S, ('three_groups', 'group_not_a_seed'), start=7 * k, count=3)
        b.ask(S[1] + 150)
        b.end_contig()
    return b.soa()


CASES = {
    'seeds_8': _seeds(8),                          # the set of 8 of DUET_DBG_EF_OWN_SMALLTAB still holds them
    'seeds_300': _seeds(300),                      # 9 .. 1024: the hash set in LDS
    'seeds_1100': _seeds(OWN_KEYS + 76),           # above kOwnKeys: the array-free walk with the real capacities
    'contig_without_seeds': _no_seeds,
    'tiles_257': _tiles_257,
    'contigs_65': _contigs_65,
}
NAMES = tuple(CASES)
_made = {}


def case(name):
    if name not in _made:
        _made[name] = CASES[name]()
    return _made[name]


def _with(soa, **kw):
    s = Soa(**dict({n: getattr(soa, n) for n, _ in soa.FIELDS}, **kw))
    s.kind = soa.kind
    return s


def canonical(soa):
    """every spelling of "no tag" as ABSENT: an index at or beyond n_reads (classify_edges.as_absent), and the index of an
    all-ones word likewise"""
    mr = soa.mark_read.astype(np.int64)
    inside = mr < soa.n_reads
    blank = np.zeros(len(mr), dtype=bool)
    blank[inside] = soa.read_tag[mr[inside]] == ALL_ONES
    return _with(soa, mark_read=np.where(~inside | blank, ABSENT, mr))


def guard_words(soa):
    """8 voter tags of the first seeded contig's first seed, hap 1, PC 0: what the device tests put behind read_tag"""
    first = soa.cand_pos[np.nonzero(soa.kind == 'seed')[0][0]]
    return engine.pack_tags([1] * 8, [0] * 8, [int(first)] * 8)


def guard_variant(soa):
    """the problem a kernel computes that reads the table at R and R + 1: the guard words appended to the table, so that the two
    near indices are valid; the far ones as in canonical()"""
    c = canonical(soa)
    mr = np.where(np.isin(soa.mark_read, (soa.n_reads, soa.n_reads + 1)), soa.mark_read, c.mark_read)
    return _with(soa, read_tag=np.concatenate([soa.read_tag, guard_words(soa)]), mark_read=mr)


# ---- long candidates: the 500,000-mark rule and PC sums at 2^31 and 2^32 ---------------------------------------------------

SUMMARY_DEG = 500000                     # decide_store: from this many marks on a multi-PS candidate gets no group summary
PC_MAX = 8100
LONG_SUMS = (2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 8100)
LONG_LO_STEP = (0, -1, 1, -1, 0)         # the smaller sum: on the 9.72 threshold, one below it (ratio above), one above it


def lo_on_threshold(hi):
    """the smallest lo with hi / lo <= 9.72 in exact arithmetic (9.72 = 243 / 25)"""
    return -(-25 * hi // 243)


def pcs_adding_to(total, n):
    """n PC values of at most 8100 that add up to total: as equal as they can be"""
    assert 0 < n and total <= PC_MAX * n
    out = np.full(n, total // n, dtype=np.int64)
    out[:total % n] += 1
    return out


def _long_sums():
    """One contig: seeds 1000 (A), 2000 (B), 3000 and a few askers; then, every sum built from PC values of at most 8100 (530,243
    marks are the fewest that reach 2^32):
      two_group    499,999 and 500,000 marks (the first takes the group summary, the second the vote from the marks), and two more whose
                   group A's hap-1 sum is exactly 2^32 - 1 and 530,243 x 8100, just above 2^32.  Group A: hap 1, PC 8100, and ONE hap-2
                   voter of PC 6731 -- with hap1_avgsc 8100 the difference of the averages is 1369 <= 1369.5 and the call 1|1; a sum that
                   lost a bit gives another average and the call 0.  Group B: one voter, at the front, in the middle or at the end.
      class_1      both haplotypes of one phase set; the larger sum at 2^31 - 1, 2^31, 2^32 - 1, 2^32 and 2^32 + 8100, the smaller
                   one on the 9.72 threshold of totsc_ratio, one below and one above it (sv_ratio 0.6: the branch that asks); the
                   smaller sum's count puts |hap2_avgsc - hap1_avgsc| next to 2400
      three_group  500,001 marks, the first spelled n_reads + 1 and the last 2^31; groups B and A of 225,000 voters each, B first
                   seen (it wins the tie; one more vote for A, read from behind the table, and A wins), and a group that is no seed"""
    A, B, X = 1000, 2000, 1500
    tags, by_key = [], {}

    def read(hap, pc, ps):
        key = (hap, int(pc), ps)
        if key not in by_key:
            by_key[key] = len(tags)
            tags.append(key)
        return by_key[key]

    def reads(hap, pcs, ps):
        vals, inv = np.unique(pcs, return_inverse=True)
        return np.array([read(hap, v, ps) for v in vals], dtype=np.int64)[inv]

    marks, kinds, pos, svread, refread = [], [], [], [], []

    def cand(p, m, kind, sv=5, rf=1):
        marks.append(np.asarray(m, dtype=np.int64))
        kinds.append(kind)
        pos.append(p)
        svread.append(sv)
        refread.append(rf)

    for v in (A, B, 3000):
        cand(v, [read(1 + v // 1000 % 2, 20, v)] * 2, 'seed')
    for p in (900, 1499, 1500, 2600, 4000):
        cand(p, [ABSENT], 'ask')
    b_voter, a_hap2 = read(2, 40, B), read(2, 6731, A)
    for i, (n_a, total) in enumerate(((SUMMARY_DEG - 3, None), (SUMMARY_DEG - 2, None), (530243, 2 ** 32 - 1), (530243, 530243 * PC_MAX))):
        a = reads(1, pcs_adding_to(PC_MAX * n_a if total is None else total, n_a), A)
        at = (0, n_a // 2, n_a, 7)[i]                                          # where group B's voter stands
        cand(1200 + i, np.concatenate([a[:at], [b_voter], a[at:], [a_hap2]]), 'two_group')
    for i, (hi, step) in enumerate(zip(LONG_SUMS, LONG_LO_STEP)):
        lo = lo_on_threshold(hi) + step
        n_hi = -(-hi // PC_MAX)
        n_lo = -(-lo // (hi // n_hi - 2400))                                   # (an average of 2400 below the larger sum's, or just less)
        h_hi, h_lo = (1, 2) if i % 2 == 0 else (2, 1)
        m = np.concatenate([reads(h_hi, pcs_adding_to(hi, n_hi), A), reads(h_lo, pcs_adding_to(lo, n_lo), A)])
        cand(1300 + i, np.roll(m, i * 1000), 'class_1', sv=6, rf=4)
    n3 = SUMMARY_DEG + 1
    body = np.concatenate([reads(2, np.full(225000, 4000), B), reads(1, np.full(224999, PC_MAX), A), [a_hap2],
                           reads(1, np.full(n3 - 2 - 450000, 30), X)])
    cand(1400, np.concatenate([[-1], body, [-2]]), 'three_group')
    R = len(tags)
    mr = np.concatenate(marks)
    mr = np.where(mr == -1, R + 1, np.where(mr == -2, 1 << 31, mr))
    t = np.array(tags, dtype=np.int64).reshape(-1, 3)
    C = len(kinds)
    s = Soa(cand_ctg_off=[0, C], read_tag=engine.pack_tags(t[:, 0], t[:, 1], t[:, 2]), cand_pos=pos, cand_svlen=np.full(C, 100),
            cand_svread=svread, cand_refread=refread, cand_gt_ok=np.ones(C, dtype=np.uint8),
            cand_off=np.concatenate([[0], np.cumsum([len(m) for m in marks])]), mark_read=mr)
    s.kind = np.array(kinds)
    for a in (s.read_tag, s.mark_read, s.cand_off, s.cand_pos, s.cand_ctg_off, s.kind):
        a.setflags(write=False)
    return s


LONG = 'long_sums'
_long = {}


def long_case():
    if not _long:
        _long[LONG] = _long_sums()
    return _long[LONG]


# ---- the device-planned instance (duet_svim_phase_device: ef_finalize<DYN>) -------------------------------------------------

_planned = {}


def planned():
    """-> (case, canonical marks): a tests.svim_fuzz input of two contigs whose groups see up to four phase sets; every mark that
    the generator left without a read carries one of the six spellings instead (one read's word is set to all ones for the sixth)"""
    from tests import svim_fuzz
    if not _planned:
        G = 400
        c = svim_fuzz.build('tag_lookup_planned', 7100, np.minimum(np.arange(G) * 2 // G, 1), np.resize([9, 12, 17, 20], G), 2)
        read = c.marks['read'].astype(np.int64)
        R = len(c.read_tag)
        blank = int(read[read != ABSENT][0])
        c.read_tag = c.read_tag.copy()
        c.read_tag[blank] = ALL_ONES
        gone = np.nonzero(read == ABSENT)[0]
        spelled = np.array([ABSENT, R, R + 1, 1 << 31, 0xFFFFFFFE, blank], dtype=np.int64)
        read[gone] = spelled[np.arange(len(gone)) % 6]
        canon = dict(c.marks, read=np.where((read >= R) | (read == blank), ABSENT, read).astype(np.uint32))
        c.marks = dict(c.marks, read=read.astype(np.uint32))
        _planned['case'] = (c, canon)
    return _planned['case']
