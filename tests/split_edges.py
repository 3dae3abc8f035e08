# coding=utf-8
"""Named E/F problems at the smallest shapes where ef_classify_split's split or fold can go wrong: two lanes walk a candidate, the
owner marks [b, mid) and the helper [mid, e) with mid = b + (n + 1) / 2, each from an empty state, and the owner folds the
helper's state into its own behind the last staging pass (duet_ef.hip: fold).  A candidate above heavy_t is walked whole by its
owner's wavefront; a tile's marks are staged kSplitChunk at a time from m_begin & ~3.

Most cases are written mark by mark over a table of eleven reads -- voters (pc <= 8100) of the phase sets X, Y and Z on either
haplotype, tagged reads of X and Y that do not vote (pc > 8100), voters on neither haplotype -- and ABSENT; the cases about
sizes deal random marks by tests/classify_edges.py's recipe.  Every hand-written problem ends with three one-PS candidates that
give the contig the seeds X, Y and Z (a multi-PS candidate's vote counts seeds only).
tests/test_split_edge_cases.py checks on the CPU that every case has the structure it is named for;
tests/test_gpu_split_edges.py runs them on the device."""
import itertools

import numpy as np

from duet_amd import engine
from tests.classify_edges import ABSENT, QUOTA, TILE, Soa, dealt, degrees, kept_columns

SPLIT_CHUNK = 3072      # kSplitChunk
HEAVY_T = 32            # the context's default heavy_t
X, Y, Z = 1000, 2000, 3000
# the read table: (hap, pc, ps); hap 0: neither haplotype
READS = ((1, 100, X), (2, 8100, X), (1, 50, Y), (2, 7000, Y), (1, 10, Z), (2, 900, Z), (1, 8101, X), (2, 9000, Y), (0, 5, X), (0, 77, Y), (0, 33, Z))
X1, X2, Y1, Y2, Z1, Z2, NX, NY, X0, Y0, Z0 = range(11)      # N*: tagged, not a voter
A = int(ABSENT)
SEEDS = [[X1, X2], [Y1, Y2], [Z2, Z1]]


def table():
    h, pc, ps = zip(*READS)
    return engine.pack_tags(h, pc, ps)


def written(cands, ctg_off=None, seed=0, seeds=True):
    """the problem whose candidate i has the marks cands[i] (read numbers or A), all candidates kept"""
    cands = [list(c) for c in cands] + (SEEDS if seeds else [])
    C = len(cands)
    off = np.concatenate([[0], np.cumsum([len(c) for c in cands])])
    mr = np.array([m for c in cands for m in c], dtype=np.int64)
    mr = np.where(mr == A, int(ABSENT), mr)
    return Soa(cand_ctg_off=[0, C] if ctg_off is None else ctg_off, read_tag=table(), cand_off=off, mark_read=mr, **kept_columns(C, 300 + seed))


def halves(marks):
    """(the owner's marks, the helper's)"""
    mid = (len(marks) + 1) // 2
    return list(marks[:mid]), list(marks[mid:])


def rotations(cands, n):
    """n candidates: the given ones over and over, the phase sets of every further round renamed (X -> Y -> Z -> X on voters)"""
    ren = {X1: Y1, X2: Y2, X0: Y0, Y1: Z1, Y2: Z2, Y0: Z0, Z1: X1, Z2: X2, Z0: X0}
    out, cur = [], [list(c) for c in cands]
    while len(out) < n:
        out += [list(c) for c in cur]
        cur = [[ren.get(m, m) for m in c] for c in cur]
    return out[:n]


def _marks_1_2_3():
    """every sequence of 1, 2 and 3 marks over seven kinds of mark: an empty second half, an even split, an odd split"""
    kinds = (A, X1, X2, Y1, Z2, NX, NY)
    return written([s for n in (1, 2, 3) for s in itertools.product(kinds, repeat=n)])


def _first_voter_in_second_half():
    base = [[NX, A, NX, A, X1, X2], [NX, NX, A, Y2, X1], [A, NY, NX, Z1], [NX, A, A, NX, A, X0, X1, X1], [A, NX, X2]]
    return written(rotations(base, 300))


def _opposite_order():
    """group A in the first half; the second half meets B first, then A"""
    base = [[X1, X1, X2, Y1, Y2, X1], [X1, A, Y2, X2], [X2, X1, X1, X0, Y1, Y1, X1, X2], [X1, NX, Y0, X1]]
    return written(rotations(base, 300))


def _b_then_more():
    """A only in the first half, two new groups in the second: B, then a third"""
    base = [[X1, X1, Y2, Z1], [X1, X2, X1, Y1, Y1, Z2], [X2, A, X1, Y1, Z1, Y2], [X0, X1, Y2, Z2]]
    return written(rotations(base, 300))


def _third_ps_across():
    """two phase sets in the first half, a third in the second: only the halves together have three"""
    base = [[X1, Y2, Z1], [X1, Y1, X2, Z2, Z1], [X1, Y1, Y2, X2, Z1, Z1, Z2, A], [Y1, X1, A, Z2, A]]
    return written(rotations(base, 300))


def _r_more_alone():
    """three phase sets among the second half's voters, none in the first"""
    base = [[A, NX, A, X1, Y1, Z1], [NX, NY, A, A, Z1, Y2, X1, X1], [A, A, NY, X2, Z1, Y1]]
    return written(rotations(base, 300))


def _multi_without_voters():
    """two phase sets among tagged marks that do not vote: multi with nv == 0, across the halves and inside one"""
    base = [[NX, NY], [NX, A, NY, A], [NX, NY, A], [A, A, NX, NY], [NX, NX, NX, NY], [NY, A, A, NX, A]]
    return written(rotations(base, 300))


def _absent_at_half_edges():
    """absent marks at the first and last position of each half (8 marks: 4 + 4; 7 marks: 4 + 3; 10: 5 + 5)"""
    base = [[A, X1, X2, A, A, X1, Y1, A], [A, X1, X1, A, A, X2, A], [A, Y1, X1, Y2, A, A, Y1, X2, X1, A], [A, A, A, A], [A, A, A]]
    return written(rotations(base, 300))


def _heavy_edge():
    """candidates of heavy_t and heavy_t + 1 marks side by side: two lanes against the wave-cooperative walk"""
    d = degrees(400, 300, 1, 12)
    d[::3] = HEAVY_T
    d[1::3] = HEAVY_T + 1
    return dealt(400, d)


def _two_passes():
    """Three tiles of more than two passes' marks each (candidates of 600 marks in front).  In every tile a candidate of 30
    marks lies across the first pass boundary and one of 200 marks (two lanes under DUET_DBG_EF_HEAVY_OFF only) across the second;
    their split points fall 5 marks before, on and 5 marks behind the boundary in tiles 0, 1 and 2.  Every tile begins on a multiple
    of 4, so both stagings cut the passes at the same marks."""
    deg = []
    for delta in (-5, 0, 5):
        b30 = SPLIT_CHUNK + delta - 15                      # the 30-mark candidate's first mark, from the tile's first
        d = [600] * ((b30 - 100) // 600)
        fill = b30 - sum(d)
        d += [4] * (fill // 4 - 1) + [4 + fill % 4]
        assert sum(d) == b30
        d += [30]
        b200 = 2 * SPLIT_CHUNK + delta - 100
        fill = b200 - sum(d)
        d += [600] * (fill // 600)
        fill = b200 - sum(d)
        d += [7] * (fill // 7 - 1) + [7 + fill % 7]
        assert sum(d) == b200
        d += [200]
        d += [2] * (TILE - 1 - len(d))
        d += [2 + (-(sum(d) + 2)) % 4]
        assert len(d) == TILE and sum(d) % 4 == 0
        deg += d
    return dealt(401, deg, absent_rate=7)


def _tile_edge(C):
    def make():
        return dealt(410 + C, degrees(410 + C, C, 1, 24))
    return make


def _pool_behind_fold():
    """every candidate of tile 0 has its voters of X in the first half and of Y in the second: 256 multi-PS candidates that only the
    fold reveals, four times the tile's own summary slots"""
    base = [[X1, X2, X1, Y1, Y2, Y1], [X1, X1, Y2, Y2], [X2, A, X1, Y1, A], [X1, X2, Y1]]
    return written(base * (TILE // len(base)))


def _starts():
    """contigs that open on candidate 64 (a wavefront's edge) and on candidate 0 of the second tile.  The seed sets differ per contig
    ({X}, {X, Y}, {Y, Z}), and each contig's first candidate has the seed of the candidate in front of it: dropped as a repeat
    across the start, contig 2 would lose Y"""
    def over(cands, n):
        return (cands * n)[:n]
    cands = over([[X1, X2, X1, X1], [X1, A, X2], [X2, X1, X0, X1, X1]], 64) + [[X1, X1]] + over([[Y1, Y2, Y2, Y1], [Y2, Y1, A]], TILE - 66) + \
        [[Y1]] + [[Y1, Y2]] + over([[Z1, Z2, Z1], [Z2, A, Z1, Z1], [Y1, Z1, Z1, Y2]], 79)
    C = len(cands)
    return written(cands, ctg_off=[0, 64, TILE, C], seeds=False)


CASES = {
    'marks_1_2_3': _marks_1_2_3,
    'first_voter_in_second_half': _first_voter_in_second_half,
    'second_half_meets_b_then_a': _opposite_order,
    'second_half_brings_b_then_more': _b_then_more,
    'third_ps_only_across_the_halves': _third_ps_across,
    'more_in_second_half_alone': _r_more_alone,
    'two_ps_among_non_voters_only': _multi_without_voters,
    'absent_at_the_edges_of_each_half': _absent_at_half_edges,
    'heavy_t_and_one_more': _heavy_edge,
    'two_passes_split_around_the_boundary': _two_passes,
    'pool_behind_the_fold': _pool_behind_fold,
    'contigs_open_on_64_and_on_tile_1': _starts,
}
CASES.update(('cands_%d' % C, _tile_edge(C)) for C in (1, 255, 256, 257))
NAMES = tuple(CASES)
_made = {}


def case(name):
    if name not in _made:
        _made[name] = CASES[name]()
    return _made[name]
