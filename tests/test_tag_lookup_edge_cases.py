# coding=utf-8
"""CPU: the cases of tests/tag_lookup_edges.py are what they are named -- shown from the inputs alone, before anything runs on a
device -- and they can tell a kernel that reads the tag table at n_reads and n_reads + 1 from one that does not."""
import numpy as np
import pytest

from oracle import c_oracle, ef_oracle
from tests import tag_lookup_edges as E
from tests.test_gpu_parity import finalize_census

SMALL = tuple(n for n in E.NAMES if n != 'tiles_257')


def unpacked(soa):
    """per mark of the canonical problem: tagged, voter, ps"""
    tagged = soa.mark_read != E.ABSENT
    tag = soa.read_tag[np.where(tagged, soa.mark_read, 0)]
    assert not (tagged & (tag == E.ALL_ONES)).any()
    ps = (tag & np.uint64(0xFFFFFFFF)).astype(np.int64)
    voter = tagged & (((tag >> np.uint64(32)) & np.uint64(0x3FFFFFFF)) <= 8100)
    return tagged, voter, ps


def contig_of(soa):
    return np.searchsorted(soa.cand_ctg_off, np.arange(soa.n_cands), side='right') - 1


def seeds_of(soa):
    """per contig: the set of seeds (the PS of every kept candidate that sees one phase set and has a voter)"""
    tagged, voter, ps = unpacked(soa)
    out = [set() for _ in range(soa.n_contigs)]
    ctg = contig_of(soa)
    for c in np.nonzero(soa.cand_svlen >= 50)[0]:
        m = slice(int(soa.cand_off[c]), int(soa.cand_off[c + 1]))
        if len(set(ps[m][tagged[m]].tolist())) == 1 and voter[m].any():
            out[ctg[c]] |= set(ps[m][voter[m]].tolist())
    return out


def python_oracle(soa):
    """oracle/ef_oracle.py on the arrays: exact (Python integers and floats as upstream)"""
    hap = (soa.read_tag >> np.uint64(62)).astype(np.int64)
    pc = ((soa.read_tag >> np.uint64(32)) & np.uint64(0x3FFFFFFF)).astype(np.int64)
    ps = (soa.read_tag & np.uint64(0xFFFFFFFF)).astype(np.int64)
    table = [(int(h), int(s), int(p)) for h, s, p in zip(hap, ps, pc)]
    chroms = ['c%d' % k for k in range(soa.n_contigs)]
    ctg = contig_of(soa)
    callset = []
    for c in range(soa.n_cands):
        cd = ef_oracle.Candidate()
        cd.contig_index = int(ctg[c])
        cd.chrom, cd.pos, cd.ref, cd.alt, cd.svtype = chroms[ctg[c]], int(soa.cand_pos[c]), 'N', '<DEL>', 'DEL'
        cd.svlen, cd.svread, cd.refread = int(soa.cand_svlen[c]), int(soa.cand_svread[c]), int(soa.cand_refread[c])
        cd.gt = '0/1' if soa.cand_gt_ok[c] else './.'
        cd.marks = [None if r == E.ABSENT else table[r] for r in soa.mark_read[soa.cand_off[c]:soa.cand_off[c + 1]].tolist()]
        callset.append(cd)
    _, trace = ef_oracle.phase_callset(callset, chroms, 50, 2, want_trace=True)
    pred = np.array([t[2] or 0 for t in trace], dtype=np.uint8)
    out_ps = np.array([t[3] or 0 for t in trace], dtype=np.uint32)
    return pred, out_ps


_cen = {}


def census(name):
    """per case: (soa, canonical, per candidate: groups = voter groups of the canonical problem, n_ps, seeds of its contig)"""
    if name not in _cen:
        soa = E.case(name)
        can = E.canonical(soa)
        tagged, voter, ps = unpacked(can)
        seeds = seeds_of(can)
        ctg = contig_of(can)
        rows = {}
        for c in np.nonzero(soa.kind != 'ask')[0]:
            if soa.kind[c] in ('seed', 'skip'):
                continue
            m = slice(int(can.cand_off[c]), int(can.cand_off[c + 1]))
            rows[int(c)] = (set(ps[m][voter[m]].tolist()), len(set(ps[m][tagged[m]].tolist())), seeds[ctg[c]])
        _cen[name] = (soa, can, rows)
    return _cen[name]


@pytest.mark.parametrize('name', E.NAMES)
def test_every_kind_is_there_and_is_what_it_is_named(name):
    soa, can, rows = census(name)
    kept = (soa.cand_svlen >= 50) & (soa.cand_svread >= 2) & (soa.cand_gt_ok != 0)
    count = {k: int((soa.kind == k).sum()) for k in E.KINDS}
    print(name, 'candidates', soa.n_cands, 'marks', soa.n_marks, 'reads', soa.n_reads, count)
    assert min(count.values()) > 0, count
    seeded = {k: 0 for k in E.KINDS}
    for c, (groups, n_ps, seeds) in rows.items():
        kind = soa.kind[c]
        assert kept[c] and n_ps >= 2, (c, kind)
        if kind == 'three_groups':
            assert len(groups) >= 3 and len(groups & seeds) in (0, 2), (c, groups)
        elif kind == 'group_not_a_seed':
            assert len(groups) == 3 and (not seeds or not groups & seeds), (c, groups)
        elif kind == 'no_slot':
            assert len(groups) == 2, (c, groups)
        else:
            assert len(groups) == 0, (c, groups)
        seeded[kind] += 1 if seeds else 0
    assert min(seeded.values()) > 0, seeded                                # each kind on a contig that has seeds
    # no_slot / all_stripped: the candidates that ask for a group summary (several PS, at most two voter groups, deg < 500000) per
    # tile of 256, beyond the tile's own 64 slots, outnumber the shared pool -- whichever of them the pool serves, `short` are left
    asks = np.zeros(soa.n_cands, dtype=np.int64)
    for c, (groups, n_ps, _) in rows.items():
        asks[c] = 1 if len(groups) <= 2 else 0
    per_tile = np.add.reduceat(asks, np.arange(0, soa.n_cands, E.TILE))
    beyond = int(np.maximum(per_tile - E.QUOTA, 0).sum())
    short = beyond - E.pool_slots(soa.n_cands)
    print(name, 'summaries asked for beyond the tiles\' own slots', beyond, 'pool', E.pool_slots(soa.n_cands), 'left without', short)
    assert short >= 100
    full = np.nonzero(per_tile == E.TILE)[0]                               # the flood tiles: both kinds in each of them
    assert len(full) >= 3
    for t in full:
        assert {'no_slot', 'all_stripped'} <= set(soa.kind[t * E.TILE:(t + 1) * E.TILE].tolist())


@pytest.mark.parametrize('name', E.NAMES)
def test_layout(name):
    soa, can, _ = census(name)
    cen = finalize_census(can)
    n_seeds = [n for n, _ in cen]
    print(name, 'contigs', soa.n_contigs, 'seeds per contig', n_seeds[:4], '...' if len(n_seeds) > 4 else '',
          'kinds of the largest', max(cen, key=lambda x: sum(x[1].values()))[1])
    tiles = [(int(soa.cand_ctg_off[k + 1]) - 1) // E.TILE - int(soa.cand_ctg_off[k]) // E.TILE + 1 for k in range(soa.n_contigs)]
    want = dict(seeds_8=lambda: soa.n_contigs == 1 and n_seeds[0] == 8,
                seeds_300=lambda: soa.n_contigs == 1 and n_seeds[0] == 300,
                seeds_1100=lambda: soa.n_contigs == 1 and n_seeds[0] == 1100 > E.OWN_KEYS,
                contig_without_seeds=lambda: n_seeds[0] == 0 and cen[0][1]['marks'] > 0 and n_seeds[1] > 0,
                tiles_257=lambda: soa.n_contigs == 1 and tiles[0] > 256 and n_seeds[0] > 8,
                contigs_65=lambda: soa.n_contigs == 65 and min(n_seeds) > 0)
    assert want[name](), (n_seeds, tiles)
    for n, kinds in cen:
        if n and sum(kinds.values()) > 300:
            assert min(kinds.values()) > 0, kinds                          # nearest, summary and marks on every large seeded contig


@pytest.mark.parametrize('name', E.NAMES)
def test_every_spelling_at_the_first_the_last_and_an_interior_mark(name):
    soa, can, rows = census(name)
    R = soa.n_reads
    blank = int(np.nonzero(soa.read_tag == E.ALL_ONES)[0][0])
    spelled = (E.ABSENT, R, R + 1, 1 << 31, 0xFFFFFFFE, blank)
    seen = set()
    for c, (groups, n_ps, seeds) in rows.items():
        if len(groups) < 3:                                                # `marks` of finalize_census: the vote from the marks for sure
            continue
        lo, hi = int(soa.cand_off[c]), int(soa.cand_off[c + 1])
        mr = soa.mark_read[lo:hi].tolist()
        for i, r in enumerate(mr):
            if r in spelled:
                where = 'first' if i == 0 else ('last' if i == hi - lo - 1 else i)
                seen.add((hi - lo, where, spelled.index(r)))
    for s in range(6):
        for deg in E.DEGREES[1:]:
            for where in ['first', 'last'] + [p for p in (7, 8, 15) if 0 < p < deg - 1]:
                assert (deg, where, s) in seen, (name, deg, where, E.SPELLINGS[s])
    # degree 3: on the two-group kinds
    for s in range(6):
        for place in (0, 2):
            assert any(soa.kind[c] in ('no_slot', 'all_stripped') and soa.cand_off[c + 1] - soa.cand_off[c] == 3 and
                       soa.mark_read[soa.cand_off[c] + place] == spelled[s] for c in list(rows)[:400])


_oracle = {}


def c_reference(name):
    """c_oracle.ef(canonical(soa), 50, 2), computed once and read-only: what tests/test_gpu_tag_lookup_edges.py compares with"""
    if name not in _oracle:
        rc, pred, ps = c_oracle.ef(census(name)[1], 50, 2)
        assert rc == 0
        pred.setflags(write=False)
        ps.setflags(write=False)
        _oracle[name] = (pred, ps)
    return _oracle[name]


@pytest.mark.parametrize('name', E.NAMES)
def test_a_read_of_the_words_behind_the_table_changes_calls_of_every_kind(name):
    soa = census(name)[0]
    pred, ps = c_reference(name)
    rc, bug_pred, bug_ps = c_oracle.ef(E.guard_variant(soa), 50, 2)
    assert rc == 0
    differ = (pred != bug_pred) | (ps != bug_ps)
    by_kind = {k: int(differ[soa.kind == k].sum()) for k in E.KINDS}
    print(name, 'calls that the misreading changes', by_kind, 'phased', int((pred != 0).sum()))
    assert min(by_kind.values()) > 0, by_kind
    assert not differ[np.isin(soa.kind, ('seed', 'ask', 'skip'))].any()
    assert int((pred != 0).sum()) > 100


@pytest.mark.parametrize('name', SMALL)
def test_the_python_oracle_agrees_with_the_c_oracle(name):
    pred, ps = c_reference(name)
    py_pred, py_ps = python_oracle(census(name)[1])
    assert np.array_equal(py_pred, pred) and np.array_equal(py_ps, ps)


def test_canonical_extends_as_absent():
    from tests import classify_edges
    soa = E.case('seeds_8')
    a, c = classify_edges.as_absent(soa), E.canonical(soa)
    blank = int(np.nonzero(soa.read_tag == E.ALL_ONES)[0][0])
    assert np.array_equal(np.where(a.mark_read == blank, E.ABSENT, a.mark_read), c.mark_read)
    assert (a.mark_read == blank).sum() > 0 and (soa.mark_read >= soa.n_reads).sum() > (soa.mark_read == E.ABSENT).sum()


# ---- long candidates ---------------------------------------------------------------------------------------------------------

_long = {}


def long_reference():
    """oracle/ef_oracle.py (Python integers: exact) on the canonical long_sums problem, computed once and read-only"""
    if not _long:
        soa = E.long_case()
        can = E.canonical(soa)
        pred, ps = python_oracle(can)
        pred.setflags(write=False)
        ps.setflags(write=False)
        _long['ref'] = (soa, can, (pred, ps))
    return _long['ref']


def test_long_sums_is_what_it_is_named():
    soa, can, _ = long_reference()
    deg = np.diff(soa.cand_off.astype(np.int64))
    long_ones = np.nonzero(deg > 1000)[0]
    print('long_sums: candidates', soa.n_cands, 'marks', soa.n_marks, 'degrees of the long ones', deg[long_ones].tolist())
    assert len(long_ones) <= 12 and soa.n_marks <= 6000000 and soa.n_contigs == 1
    assert [soa.kind[c] for c in long_ones] == ['two_group'] * 4 + ['class_1'] * 5 + ['three_group']
    tagged, voter, ps = unpacked(can)
    tag = can.read_tag[np.where(tagged, can.mark_read, 0)]
    hap = (tag >> np.uint64(62)).astype(np.int64)
    pc = ((tag >> np.uint64(32)) & np.uint64(0x3FFFFFFF)).astype(np.int64)
    assert voter[tagged].all()
    sums = []
    for c in long_ones:
        m = slice(int(can.cand_off[c]), int(can.cand_off[c + 1]))
        a = tagged[m] & (ps[m] == 1000)
        sums.append((int(pc[m][a & (hap[m] == 1)].sum()), int(pc[m][a & (hap[m] == 2)].sum()), len(set(ps[m][tagged[m]].tolist()))))
    two, one, three = sums[:4], sums[4:9], sums[9]
    assert deg[long_ones[:2]].tolist() == [E.SUMMARY_DEG - 1, E.SUMMARY_DEG] and deg[long_ones[-1]] == E.SUMMARY_DEG + 1
    assert [s[0] for s in two] == [8100 * 499997, 8100 * 499998, 2 ** 32 - 1, 2 ** 32 + 1004] and all(s[1:] == (6731, 2) for s in two)
    for (s1, s2, n_ps), hi, step in zip(one, E.LONG_SUMS, E.LONG_LO_STEP):
        lo = min(s1, s2)
        assert n_ps == 1 and max(s1, s2) == hi and lo == E.lo_on_threshold(hi) + step
        assert (25 * hi <= 243 * lo) == (step >= 0) and 25 * hi > 243 * (E.lo_on_threshold(hi) - 1)
    assert three[2] == 3
    first, last = int(soa.cand_off[long_ones[-1]]), int(soa.cand_off[long_ones[-1] + 1]) - 1
    assert soa.mark_read[first] == soa.n_reads + 1 and soa.mark_read[last] == 1 << 31


def test_long_sums_the_c_oracle_equals_the_python_oracle_and_sees_a_misreading():
    soa, can, (pred, ps) = long_reference()
    rc, c_pred, c_ps = c_oracle.ef(can, 50, 2)
    assert rc == 0 and np.array_equal(c_pred, pred) and np.array_equal(c_ps, ps)
    long_ones = np.isin(soa.kind, ('two_group', 'class_1', 'three_group'))
    print('long_sums: calls', pred[long_ones].tolist(), 'ps', ps[long_ones].tolist())
    assert pred[long_ones].tolist() == [3, 3, 3, 3, 3, 2, 3, 2, 3, 3]            # (1|1 on and below the thresholds, 0|1 above 9.72)
    rc, bug_pred, bug_ps = c_oracle.ef(E.guard_variant(soa), 50, 2)
    assert rc == 0 and bug_ps[-1] == 1000 != ps[-1]


def test_planned_input_carries_every_spelling_on_candidates_that_vote_from_their_marks():
    from tests import svim_ref
    c, canon = E.planned()
    w = svim_ref.fused(canon, c.read_tag, c.depth, c.depth_off, c.depth_bin, c.svlen_thres, c.suppread_thres, **c.kw)
    assert w['rc'] == 0
    soa = svim_ref.adapt(w, canon, c.read_tag, c.depth, c.depth_off, c.depth_bin)[0]
    cen = finalize_census(soa, c.svlen_thres, c.suppread_thres)
    print('tag_lookup_planned: candidates', soa.n_cands, 'census', cen)
    assert all(n > 0 and kinds['marks'] >= 10 for n, kinds in cen)
    raw = c.marks['read'][w['order']]
    R = len(c.read_tag)
    blank = int(np.nonzero(c.read_tag == E.ALL_ONES)[0][0])
    tagged, voter, ps = unpacked(soa)
    kept = (soa.cand_svlen >= c.svlen_thres) & (soa.cand_svread >= c.suppread_thres)
    seen = set()
    for cand in np.nonzero(kept)[0]:
        m = slice(int(soa.cand_off[cand]), int(soa.cand_off[cand + 1]))
        if len(set(ps[m][voter[m]].tolist())) >= 3:
            seen |= set(raw[m].tolist()) & {E.ABSENT, R, R + 1, 1 << 31, 0xFFFFFFFE, blank}
    assert len(seen) == 6, seen
