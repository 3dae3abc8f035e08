# coding=utf-8
"""CPU: every case of tests/classify_edges.py has the shape it is named for, and the C oracle takes it (rc 0) with a result
worth comparing -- what tests/test_gpu_classify_edges.py then holds the device to."""
import numpy as np
import pytest

from oracle import c_oracle
from tests import classify_edges as E

TILE, CHUNK = E.TILE, E.CHUNK


def tiles(soa):
    """per tile: (m_begin, m_end)"""
    off = soa.cand_off.astype(np.int64)
    C = soa.n_cands
    return [(int(off[c0]), int(off[min(c0 + TILE, C)])) for c0 in range(0, C, TILE)]


def passes(mb, me):
    return 0 if mb == me else -(-(me - (mb & ~3)) // CHUNK)


@pytest.mark.parametrize('name', E.NAMES)
def test_the_oracle_takes_the_case(name):
    soa = E.case(name)
    C, M = soa.n_cands, soa.n_marks
    assert len(soa.cand_off) == C + 1 and soa.cand_off[0] == 0 and soa.cand_off[-1] == M
    assert np.all(np.diff(soa.cand_off.astype(np.int64)) >= 0)
    assert soa.cand_ctg_off[0] == 0 and soa.cand_ctg_off[-1] == C and np.all(np.diff(soa.cand_ctg_off.astype(np.int64)) >= 0)
    for n in ('cand_pos', 'cand_svlen', 'cand_svread', 'cand_refread', 'cand_gt_ok'):
        assert len(getattr(soa, n)) == C
    ref = E.as_absent(soa)
    live = ref.mark_read[ref.mark_read != E.ABSENT]
    assert live.size == 0 or int(live.max()) < ref.n_reads
    rc, pred, ps = c_oracle.ef(ref, 50, 2)
    assert rc == 0
    if name not in ('no_reads', 'cands_1'):
        assert int((pred != 0).sum()) > 0, 'nothing is phased: the case would compare zeros'


def test_shapes():
    for C in (1, 255, 256, 257, 513):
        assert E.case('cands_%d' % C).n_cands == C
    for r in (1, 2, 3):
        s = E.case('offsets_mod4_%d' % r)
        assert s.cand_off[TILE] % 4 == r and s.n_marks % 4 == r and s.n_cands > TILE
    s = E.case('tile_without_marks')
    t = tiles(s)
    assert len(t) == 3 and t[1][0] == t[1][1] and t[0][0] < t[0][1] and t[2][0] < t[2][1]
    s = E.case('only_last_of_tile_has_marks')
    d = np.diff(s.cand_off.astype(np.int64))
    assert np.all(d[TILE:2 * TILE - 1] == 0) and d[2 * TILE - 1] > 0
    assert [passes(*x) for x in tiles(E.case('span_3072_then_3073'))[:2]] == [1, 2]
    t = tiles(E.case('span_3072_then_3073'))
    assert t[0] == (0, CHUNK) and t[1][1] - (t[1][0] & ~3) == CHUNK + 1
    t = tiles(E.case('span_3073_then_3072'))
    assert t[0] == (0, CHUNK + 1) and t[1][0] % 4 == 1 and t[1][1] - (t[1][0] & ~3) == CHUNK
    assert [passes(*x) for x in t[:2]] == [2, 1]
    s = E.case('candidate_of_9000_marks')
    assert s.cand_off[101] - s.cand_off[100] == 9000 and passes(*tiles(s)[0]) >= 3
    s = E.case('no_reads')
    assert s.n_reads == 0 and np.all(s.mark_read == E.ABSENT)
    s = E.case('indices_beyond_the_table')
    beyond = (s.mark_read >= s.n_reads) & (s.mark_read != E.ABSENT)
    assert beyond.sum() > 100 and len(np.unique(s.mark_read[beyond])) == 4
    owner = np.searchsorted(s.cand_off, np.nonzero(beyond)[0], side='right') - 1
    for c in np.unique(owner):                         # (such a candidate holds one read besides them: one phase set at most)
        m = s.mark_read[s.cand_off[c]:s.cand_off[c + 1]]
        assert len(np.unique(m[m < s.n_reads])) == 1
    assert E.case('one_read').n_reads == 1
    for n_two in (256, 64):
        s = E.case('two_ps_%d' % n_two)
        assert TILE < s.n_cands <= TILE + 8
        two = [len(np.unique(s.mark_read[s.cand_off[c]:s.cand_off[c + 1]])) == 2 for c in range(s.n_cands)]
        assert sum(two[:TILE]) == n_two and sum(two[TILE:]) == 0
        rc, pred, ps = c_oracle.ef(s, 50, 2)
        assert rc == 0 and (pred[:TILE][np.array(two[:TILE])] != 0).sum() > 10          # (multi-PS candidates that end phased)
        assert np.all(s.cand_svlen >= 50) and np.all(s.cand_svread >= 2) and np.all(s.cand_gt_ok == 1)
    s = E.case('starts_at_lanes_0_63_64_255')
    assert sorted(set(int(x) % TILE for x in s.cand_ctg_off[1:-1])) == [0, 63, 64, 255]
    rc, pred, ps = c_oracle.ef(s, 50, 2)
    assert rc == 0 and np.all(ps[pred != 0] == 5000) and (pred != 0).sum() > 100
