# coding=utf-8
"""CPU: the fold of ef_classify_split (duet_ef.hip: fold) and the structure of the cases in tests/split_edges.py.

The serial walk's state (CandState as consume_range leaves it) and the fold are restated here, once on numpy arrays -- one
element per sequence of marks -- and once on plain integers.

* fold(walk(a), walk(b)) == walk(a + b) for EVERY sequence of at most six marks over an alphabet of 21 marks -- absent; tagged
  but not a voter, phase set x / y; a voter of x / y / z on haplotype 0 / 1 / 2 with one of two PC values -- and every split point,
  the empty halves included: 21^6 = 85,766,121 sequences of six marks alone, seven split points each (about a minute).  Compared: first_ps, multi, nv,
  the two groups' phase sets, n_a, `more` always; n_b, the hap counts and the PC sums where `more` is false (where it is true no
  kernel reads them).  The states of all sequences of a length are built from those one mark shorter, a split point is a
  broadcast of prefix states against suffix states.
* what E/F makes of a folded state -- class, seed, vote, decision -- equals oracle.ef_oracle on the same marks: every sequence of
  at most three marks at every split point, and every candidate of the hand-written cases at its own split point, under several
  seed sets.  (Multi-PS candidates with a voter on neither haplotype are outside the oracle's domain -- upstream raises there --
  and are left to the C oracle on the device.)
* every named case has the structure it is named for."""
from unittest import mock

import numpy as np
import pytest

from oracle import c_oracle, ef_oracle
from tests import split_edges as S

DT = np.uint16                  # every count and sum of six marks fits (6 * 8100)
E = 65535                       # "empty" in the restatement (the device: all ones); phase sets are 1, 2, 3 here
PCS = (40, 8100)
# the alphabet: (tagged, ps, voter, hap, pc)
ALPHABET = [(False, 0, False, 0, 0)] + [(True, ps, False, 1, 9000) for ps in (1, 2)] + \
    [(True, ps, True, hap, pc) for ps in (1, 2, 3) for hap in (0, 1, 2) for pc in PCS]
NSYM = len(ALPHABET)
MAXLEN = 6
COUNTS = ('n_b', 'a1', 'a2', 'b1', 'b2', 'TA1', 'TA2', 'tb1', 'tb2')
ALWAYS = ('first_ps', 'multi', 'nv', 'ps_a', 'ps_b', 'more', 'n_a')


def empty(n=1):
    st = {k: np.zeros(n, dtype=DT) for k in ('nv', 'n_a') + COUNTS}
    st.update({k: np.full(n, E, dtype=DT) for k in ('first_ps', 'ps_a', 'ps_b')})
    st.update(multi=np.zeros(n, dtype=bool), more=np.zeros(n, dtype=bool))
    return st


def restate_n_a(st):
    st['n_a'] = np.where(st['more'], (st['ps_a'] != E).astype(DT), st['nv'] - st['n_b'])


def step(st, sym):
    """the state one mark later (consume_range's rule, mark by mark)"""
    tagged, ps, voter, hap, pc = sym
    st = dict(st)
    if tagged:
        st['multi'] = st['multi'] | ((st['first_ps'] != E) & (st['first_ps'] != ps))
        st['first_ps'] = np.minimum(st['first_ps'], DT(ps))
    if voter:
        st['nv'] = st['nv'] + DT(1)
        st['ps_a'] = np.where(st['ps_a'] == E, DT(ps), st['ps_a'])
        in_a = st['ps_a'] == ps
        st['ps_b'] = np.where(~in_a & (st['ps_b'] == E), DT(ps), st['ps_b'])
        in_b = ~in_a & (st['ps_b'] == ps)
        st['more'] = st['more'] | (~in_a & ~in_b)
        st['n_b'] = st['n_b'] + in_b.astype(DT)
        if hap in (1, 2):
            st['a%d' % hap] = st['a%d' % hap] + in_a.astype(DT)
            st['b%d' % hap] = st['b%d' % hap] + in_b.astype(DT)
            st['TA%d' % hap] = st['TA%d' % hap] + DT(pc) * in_a.astype(DT)
            st['tb%d' % hap] = st['tb%d' % hap] + DT(pc) * in_b.astype(DT)
    restate_n_a(st)
    return st


def fold(l, r):
    """duet_ef.hip: fold -- L = the state of [lo, mid), R = the state of [mid, hi), each from empty (arrays broadcast)"""
    o = {}
    o['multi'] = l['multi'] | r['multi'] | ((l['first_ps'] != E) & (r['first_ps'] != E) & (l['first_ps'] != r['first_ps']))
    o['first_ps'] = np.minimum(l['first_ps'], r['first_ps'])
    o['nv'] = l['nv'] + r['nv']
    z = np.zeros(np.broadcast(l['nv'], r['nv']).shape, dtype=DT)
    for k in ('ps_a', 'ps_b', 'n_b', 'a1', 'a2', 'b1', 'b2', 'TA1', 'TA2', 'tb1', 'tb2'):
        o[k] = l[k] + z
    more = l['more'] | (z != 0)
    for ps, n, h1, h2, t1, t2 in ((r['ps_a'], r['nv'] - r['n_b'], r['a1'], r['a2'], r['TA1'], r['TA2']),
                                  (r['ps_b'], r['n_b'], r['b1'], r['b2'], r['tb1'], r['tb2'])):
        there = ps != E
        to_a = there & ((o['ps_a'] == E) | (o['ps_a'] == ps))
        to_b = there & ~to_a & ((o['ps_b'] == E) | (o['ps_b'] == ps))
        o['ps_a'] = np.where(to_a, ps, o['ps_a'])
        o['ps_b'] = np.where(to_b, ps, o['ps_b'])
        o['n_b'] = o['n_b'] + to_b.astype(DT) * n
        for dst, src, to in (('a1', h1, to_a), ('a2', h2, to_a), ('TA1', t1, to_a), ('TA2', t2, to_a),
                             ('b1', h1, to_b), ('b2', h2, to_b), ('tb1', t1, to_b), ('tb2', t2, to_b)):
            o[dst] = o[dst] + to.astype(DT) * src
        more = more | (there & ~to_a & ~to_b)
    o['more'] = more | r['more']
    restate_n_a(o)
    return o


def walk(seq):
    st = empty()
    for sym in seq:
        st = step(st, sym)
    return st


STORED = 5                      # the states of all sequences of up to this many marks are kept; those of six are made block by block


@pytest.fixture(scope='module')
def states():
    """states[k]: the state of every sequence of k marks, the first mark the most significant digit of the index (k <= STORED)"""
    out = [empty()]
    for _ in range(STORED):
        out.append(one_more(out[-1]))
    return out


def one_more(st):
    """the states of the sequences one mark longer: index * NSYM + the last mark"""
    nxt = [step(st, sym) for sym in ALPHABET]
    return {k: np.stack([s[k] for s in nxt], axis=1).reshape(-1) for k in nxt[0]}


def whole_range(states, length, g0, g1):
    """the states of the sequences number g0 .. g1 - 1 of `length` marks (multiples of NSYM where length > STORED)"""
    if length <= STORED:
        return {k: v[g0:g1] for k, v in states[length].items()}
    assert length == STORED + 1 and g0 % NSYM == 0 and g1 % NSYM == 0
    return one_more({k: v[g0 // NSYM:g1 // NSYM] for k, v in states[STORED].items()})


def blocks(n, size):
    return [(i, min(i + size, n)) for i in range(0, n, size)]


@pytest.mark.parametrize('length', range(MAXLEN + 1))
def test_fold_of_the_halves_is_the_walk_of_the_whole(states, length):
    for i in range(length + 1):                                 # the first half: i marks
        nl, nr = NSYM ** i, NSYM ** (length - i)
        cb = min(nr, NSYM ** 4)
        rb = max(1, NSYM ** 4 // cb)
        for r0, r1 in blocks(nl, rb):
            l = whole_range(states, i, r0, r1)
            l = {k: v[:, None] for k, v in l.items()}
            for c0, c1 in blocks(nr, cb):
                got = fold(l, {k: v[None, :] for k, v in whole_range(states, length - i, c0, c1).items()})
                if cb == nr:
                    want = {k: v.reshape(r1 - r0, nr) for k, v in whole_range(states, length, r0 * nr, r1 * nr).items()}
                else:                                           # (one first half, a block of second halves)
                    want = {k: v.reshape(1, c1 - c0) for k, v in whole_range(states, length, r0 * nr + c0, r0 * nr + c1).items()}
                for k in ALWAYS:
                    assert np.array_equal(got[k], want[k]), (length, i, k)
                ok = ~want['more']
                for k in COUNTS:
                    assert np.array_equal(got[k][ok], want[k][ok]), (length, i, k)


# ---- what E/F makes of a state, against oracle.ef_oracle -----------------------------------------------------------------------

class Forced(ef_oracle.Candidate):
    """a candidate whose vote is given: the oracle's decision is then taken on what a state says"""
    __slots__ = ('forced',)


@pytest.fixture(scope='module', autouse=True)
def votes_may_be_forced():
    real = ef_oracle.vote
    with mock.patch.object(ef_oracle, 'vote', side_effect=lambda cd, cls, seeds: cd.forced if isinstance(cd, Forced) else real(cd, cls, seeds)):
        yield


def scalars(st):
    """arrays of states -> one dict of plain integers per element"""
    flat = {k: v.reshape(-1).tolist() for k, v in st.items()}
    return [dict(zip(flat, vals)) for vals in zip(*flat.values())]


def outputs_from_state(st, cd, seeds):
    """(class, seed, (pred, ps)) as ef_classify and ef_finalize* derive them from a state; None for the decision of a candidate with
    three voter groups (no summary: the kernels gather its vote from the marks again)"""
    cls = 0 if st['first_ps'] == E else (2 if st['multi'] else 1)
    seed = None if st['ps_a'] == E else st['ps_a']
    if cls == 2 and st['more']:
        return cls, seed, None
    h1 = h2 = h0 = allhap = t1 = t2 = ps = 0
    if cls == 1:
        h1, h2, t1, t2, ps = st['a1'], st['a2'], st['TA1'], st['TA2'], (0 if seed is None else seed)
        allhap = h1 + h2
    elif cls == 2:
        allhap, best = st['nv'], 0
        for g in (('ps_a', 'n_a', 'a1', 'a2', 'TA1', 'TA2'), ('ps_b', 'n_b', 'b1', 'b2', 'tb1', 'tb2')):
            gps, n = st[g[0]], st[g[1]]
            if n > best and gps in seeds:
                best = n
                h1, h2, t1, t2, ps = st[g[2]], st[g[3]], st[g[4]], st[g[5]], gps
                h0 = allhap - h1 - h2
    if cls == 0 or (h1 == 0 and h2 == 0):
        ps = ef_oracle.nearest_ps(sorted(seeds), cd.pos)
    f = Forced()
    f.marks, f.svread, f.refread, f.pos, f.forced = cd.marks, cd.svread, cd.refread, cd.pos, (h1, h2, h0, allhap, t1, t2, ps)
    return cls, seed, ef_oracle.decide(f, cls, seeds)


def candidate(marks, svread, refread, pos):
    cd = ef_oracle.Candidate()
    cd.marks, cd.svread, cd.refread, cd.pos = marks, svread, refread, pos
    return cd


def check_outputs(st, syms, tag):
    """st: a folded state of the marks syms, (tagged, ps, voter, hap, pc) each, as plain integers; against the oracle on the list"""
    marks = [(s[3], s[1], s[4]) if s[0] else None for s in syms]
    for seeds in ({1, 2, 3}, {1}, {2, 3}):
        for svread, refread, pos in ((5, 1, 0), (3, 4, 2)):
            cd = candidate(marks, svread, refread, pos)
            cls, seed, dec = outputs_from_state(st, cd, seeds)
            assert cls == ef_oracle.ps_class(cd), tag
            assert seed == ef_oracle.seed_ps(cd), tag
            if dec is not None:
                assert dec == ef_oracle.decide(cd, cls, seeds), (tag, seeds, svread, refread)


def in_domain(syms):
    """(upstream raises on a multi-PS candidate with a voter on neither haplotype)"""
    return len(set(s[1] for s in syms if s[0])) < 2 or not any(s[2] and s[3] == 0 for s in syms)


def test_outputs_of_a_folded_state_are_the_oracles(states):
    import itertools
    n = 0
    for length in (1, 2, 3):
        seqs = list(itertools.product(ALPHABET, repeat=length))                # (in the order of the states' index)
        for mid in range(length + 1):
            folded = scalars(fold({k: v[:, None] for k, v in states[mid].items()}, {k: v[None, :] for k, v in states[length - mid].items()}))
            assert len(folded) == len(seqs)
            for st, syms in zip(folded, seqs):
                if in_domain(syms):
                    check_outputs(st, syms, (syms, mid))
                    n += 1
    assert n > 2 * NSYM + 3 * NSYM ** 2 // 2 + 4 * NSYM ** 3 // 4           # (most sequences are inside the oracle's domain)


def symbols_of(soa, c):
    """candidate c's marks as alphabet-style tuples, phase sets as they are in the table"""
    out = []
    for r in soa.mark_read[soa.cand_off[c]:soa.cand_off[c + 1]]:
        if r == S.ABSENT:
            out.append((False, 0, False, 0, 0))
        else:
            hap, pc, ps = S.READS[int(r)]
            out.append((True, ps, pc <= 8100, hap, pc))
    return out


HAND_WRITTEN = [n for n in S.NAMES if not (n.startswith('cands_') or n in ('heavy_t_and_one_more', 'two_passes_split_around_the_boundary'))]


@pytest.mark.parametrize('name', HAND_WRITTEN)
def test_outputs_of_the_named_cases_candidates(name):
    soa = S.case(name)
    seen = set()
    for c in range(soa.n_cands):
        syms = symbols_of(soa, c)
        if tuple(syms) in seen or not in_domain(syms):
            continue
        seen.add(tuple(syms))
        mid = (len(syms) + 1) // 2
        check_outputs(scalars(fold(walk(syms[:mid]), walk(syms[mid:])))[0], syms, (name, c))


# ---- the structure of the named cases ------------------------------------------------------------------------------------------

def marks(soa, c):
    return [int(m) if m != S.ABSENT else S.A for m in soa.mark_read[soa.cand_off[c]:soa.cand_off[c + 1]]]


def voter_ps(ms):
    """the voters' phase sets in first-seen order"""
    out = []
    for m in ms:
        if m != S.A and S.READS[m][1] <= 8100 and S.READS[m][2] not in out:
            out.append(S.READS[m][2])
    return out


def tagged_ps(ms):
    return set(S.READS[m][2] for m in ms if m != S.A)


def own(soa):
    """the candidates a case is about (without the three that only give the contig its seeds)"""
    return range(soa.n_cands - len(S.SEEDS))


def passes(soa, tile):
    off = soa.cand_off.astype(np.int64)
    mb, me = int(off[tile * S.TILE]), int(off[min((tile + 1) * S.TILE, soa.n_cands)])
    return 0 if mb == me else -(-(me - (mb & ~3)) // S.SPLIT_CHUNK)


@pytest.mark.parametrize('name', S.NAMES)
def test_the_oracle_takes_the_case(name):
    soa = S.case(name)
    assert soa.cand_off[0] == 0 and soa.cand_off[-1] == soa.n_marks and np.all(np.diff(soa.cand_off.astype(np.int64)) >= 1)
    rc, pred, ps = c_oracle.ef(soa, 50, 2)
    assert rc == 0
    if name != 'cands_1':
        assert int((pred != 0).sum()) > 10, 'hardly anything is phased: the case would compare zeros'
    if name in HAND_WRITTEN:
        assert all(passes(soa, t) <= 1 for t in range((soa.n_cands + S.TILE - 1) // S.TILE))


def test_structure():
    s = S.case('marks_1_2_3')
    d = np.diff(s.cand_off.astype(np.int64))[:len(own(s))]
    assert sorted(set(d)) == [1, 2, 3] and [int((d == n).sum()) for n in (1, 2, 3)] == [7, 49, 343]
    assert [len(h) for h in S.halves([0])] == [1, 0] and [len(h) for h in S.halves([0, 0, 0])] == [2, 1]

    s = S.case('first_voter_in_second_half')
    for c in own(s):
        l, r = S.halves(marks(s, c))
        assert voter_ps(l) == [] and voter_ps(r) != []
        assert any(m == S.A for m in l) and any(m != S.A and S.READS[m][1] > 8100 for m in l)

    s = S.case('second_half_meets_b_then_a')
    for c in own(s):
        l, r = S.halves(marks(s, c))
        a = voter_ps(l)
        assert len(a) == 1 and len(voter_ps(r)) == 2 and voter_ps(r)[1] == a[0]

    s = S.case('second_half_brings_b_then_more')
    for c in own(s):
        l, r = S.halves(marks(s, c))
        assert len(voter_ps(l)) == 1 and len(voter_ps(r)) == 2 and voter_ps(l)[0] not in voter_ps(r)

    s = S.case('third_ps_only_across_the_halves')
    for c in own(s):
        l, r = S.halves(marks(s, c))
        assert len(voter_ps(l)) == 2 and len(voter_ps(r)) == 1 and len(voter_ps(l + r)) == 3

    s = S.case('more_in_second_half_alone')
    for c in own(s):
        l, r = S.halves(marks(s, c))
        assert voter_ps(l) == [] and len(voter_ps(r)) == 3

    s = S.case('two_ps_among_non_voters_only')
    across = 0
    for c in own(s):
        l, r = S.halves(marks(s, c))
        assert voter_ps(l + r) == [] and len(tagged_ps(l + r)) == 2
        across += len(tagged_ps(l)) == 1 and len(tagged_ps(r)) == 1
    assert 50 < across < len(own(s)) - 50

    s = S.case('absent_at_the_edges_of_each_half')
    sizes = set()
    for c in own(s):
        l, r = S.halves(marks(s, c))
        assert l[0] == S.A and l[-1] == S.A and r[0] == S.A and r[-1] == S.A
        sizes.add((len(l), len(r)))
    assert {(4, 4), (4, 3), (5, 5)} <= sizes

    s = S.case('heavy_t_and_one_more')
    d = np.diff(s.cand_off.astype(np.int64))
    assert (d == S.HEAVY_T).sum() == 100 and (d == S.HEAVY_T + 1).sum() == 100 and d.max() == S.HEAVY_T + 1

    s = S.case('two_passes_split_around_the_boundary')
    off = s.cand_off.astype(np.int64)
    d = np.diff(off)
    assert s.n_cands == 3 * S.TILE
    for t, delta in enumerate((-5, 0, 5)):
        mb = int(off[t * S.TILE])
        assert mb % 4 == 0 and passes(s, t) == 3
        tile = range(t * S.TILE, (t + 1) * S.TILE)
        for n, boundary in ((30, S.SPLIT_CHUNK), (200, 2 * S.SPLIT_CHUNK)):
            c, = [c for c in tile if d[c] == n]
            assert off[c] - mb < boundary < off[c + 1] - mb
            assert int(off[c]) + (n + 1) // 2 - mb == boundary + delta

    for C in (1, 255, 256, 257):
        assert S.case('cands_%d' % C).n_cands == C

    s = S.case('pool_behind_the_fold')
    for c in range(S.TILE):
        l, r = S.halves(marks(s, c))
        assert len(tagged_ps(l)) == 1 and len(tagged_ps(r)) == 1 and tagged_ps(l) != tagged_ps(r)
    assert S.TILE > S.QUOTA

    s = S.case('contigs_open_on_64_and_on_tile_1')
    assert list(s.cand_ctg_off[1:-1]) == [64, S.TILE]
    rc, pred, ps = c_oracle.ef(s, 50, 2)
    assert rc == 0 and len(set(ps[pred != 0][:30])) >= 1
    seeds = [set(v for c in range(int(a), int(b)) for v in voter_ps(marks(s, c))[:1] if len(tagged_ps(marks(s, c))) == 1)
             for a, b in zip(s.cand_ctg_off[:-1], s.cand_ctg_off[1:])]
    assert seeds[0] != seeds[1] and seeds[1] != seeds[2]
