# coding=utf-8
"""Cases of the evaluator's per-record outcome (duet_amd/evaluation.py: details; include/duet_ef.h: duet_eval_details_host),
shared by tests/test_eval_details_host.py (the Python path) and tests/test_gpu_eval_details.py (the device against it).

CASES: parsed records written by hand with both tables spelled out, every column; a row is written with blanks for its tabs.
random_problem: seeded flat arrays with positions from a small range (ties everywhere), ids that repeat and a list that has
truth records and no call.  brute: the records once more, the slow obvious way (tests/eval_ref.py's nearest and accepts, a
minimum over every call of the key for the reverse search) -- it shares no code with details_host."""
import numpy as np

from duet_amd import _lib as L
from tests import eval_ref


def rec(name, pos, ln, hp, chrom='chr1', typ='INS', ps=None):
    """A record as evaluation.parse_vcf leaves it: the id is ID + CHROM + POS."""
    return {'chr': chrom, 'pos': pos, 'id': name + chrom + str(pos), 'hp': hp, 'ps': ps or chrom + '_:1', 'len': ln, 'type': typ}


def rows(text):
    return [ln.split() for ln in text.strip().splitlines()]


# name -> (truth, calls, refdist, ratio, the rows of the calls table, the rows of the truth table)
CASES = {}

# A call half-way between two records takes the right one; a call before the first record and one beyond the last.  The group
# has one "same" pair (2 ids) and one "flip" pair (2 ids): the tie goes to flip.
CASES['halfway_and_both_ends'] = (
    [rec('tA', 1000, 100, '1|0'), rec('tB', 1200, 100, '0|1')],
    [rec('c1', 1100, 100, '1|0'), rec('c2', 5, 100, '1|0'), rec('c3', 9000, 100, '1|0')], 1000, 0.0,
    rows('''chr1 1100 c1chr11100 INS 100 1|0 chr1_:1 1200 tBchr11200 100 0|1 100 1 1 flip flip 1
            chr1 5 c2chr15 INS 100 1|0 chr1_:1 1000 tAchr11000 100 1|0 995 1 1 same flip 0
            chr1 9000 c3chr19000 INS 100 1|0 chr1_:1 1200 tBchr11200 100 0|1 7800 0 0 . flip 0'''),
    rows('''chr1 1000 tAchr11000 INS 100 1|0 1 1 0 1100 c1chr11100 100 .
            chr1 1200 tBchr11200 INS 100 0|1 1 1 1 1100 c1chr11100 100 .'''))

# dist == refdist is accepted, one more is not; a '1|1' pair is "both", and alone in its group it ties: flip
CASES['refdist_and_one_more'] = (
    [rec('t', 50000, 100, '1|1')],
    [rec('c1', 49700, 100, '1|1'), rec('c2', 50301, 100, '1|1')], 300, 0.0,
    rows('''chr1 49700 c1chr149700 INS 100 1|1 chr1_:1 50000 tchr150000 100 1|1 300 1 1 both flip 1
            chr1 50301 c2chr150301 INS 100 1|1 chr1_:1 50000 tchr150000 100 1|1 301 0 0 . flip 0'''),
    rows('''chr1 50000 tchr150000 INS 100 1|1 1 1 1 49700 c1chr149700 300 .'''))

# 700 / 1000 == 0.7 in binary64: accepted at -p 0.7; 699 / 1000 is not.  "same" 2 ids against "flip" 0: same
CASES['ratio_exactly_at_p'] = (
    [rec('t1', 1000, 1000, '1|0'), rec('t2', 5000, 1000, '1|0')],
    [rec('c1', 1000, 700, '1|0'), rec('c2', 5000, 699, '1|0')], 10, 0.7,
    rows('''chr1 1000 c1chr11000 INS 700 1|0 chr1_:1 1000 t1chr11000 1000 1|0 0 1 1 same same 1
            chr1 5000 c2chr15000 INS 699 1|0 chr1_:1 5000 t2chr15000 1000 1|0 0 0 0 . same 0'''),
    rows('''chr1 1000 t1chr11000 INS 1000 1|0 1 1 1 1000 c1chr11000 0 .
            chr1 5000 t2chr15000 INS 1000 1|0 0 0 0 5000 c2chr15000 0 size'''))

# 300 / 1000 == 0.3 < 0.1 + 0.2: refused; a group without a single pair has 0 against 0 ids: flip
CASES['ratio_just_below_p'] = (
    [rec('t', 1000, 1000, '1|0')], [rec('c', 1000, 300, '1|0')], 10, 0.1 + 0.2,
    rows('''chr1 1000 cchr11000 INS 300 1|0 chr1_:1 1000 tchr11000 1000 1|0 0 0 0 . flip 0'''),
    rows('''chr1 1000 tchr11000 INS 1000 1|0 0 0 0 1000 cchr11000 0 size'''))

# call ids tie 2 : 2, truth ids 2 : 1 -- "same" wins through the truth side alone
CASES['same_wins_by_a_truth_id'] = (
    [rec('t1', 1000, 100, '1|0'), rec('t2', 2000, 100, '1|0'), rec('t3', 4000, 100, '0|1')],
    [rec('c1', 1000, 100, '1|0'), rec('c2', 2000, 100, '1|0'), rec('c3', 4000, 100, '1|0'), rec('c4', 4001, 100, '1|0')], 10, 0.0,
    rows('''chr1 1000 c1chr11000 INS 100 1|0 chr1_:1 1000 t1chr11000 100 1|0 0 1 1 same same 1
            chr1 2000 c2chr12000 INS 100 1|0 chr1_:1 2000 t2chr12000 100 1|0 0 1 1 same same 1
            chr1 4000 c3chr14000 INS 100 1|0 chr1_:1 4000 t3chr14000 100 0|1 0 1 1 flip same 0
            chr1 4001 c4chr14001 INS 100 1|0 chr1_:1 4000 t3chr14000 100 0|1 1 1 1 flip same 0'''),
    rows('''chr1 1000 t1chr11000 INS 100 1|0 1 1 1 1000 c1chr11000 0 .
            chr1 2000 t2chr12000 INS 100 1|0 1 1 1 2000 c2chr12000 0 .
            chr1 4000 t3chr14000 INS 100 0|1 2 2 0 4000 c3chr14000 0 .'''))

# ... and without the second "same" pair it is 2 ids against 3: flip
CASES['flip_wins'] = (
    [rec('t1', 1000, 100, '1|0'), rec('t3', 4000, 100, '0|1')],
    [rec('c1', 1000, 100, '1|0'), rec('c3', 4000, 100, '1|0'), rec('c4', 4001, 100, '1|0')], 10, 0.0,
    rows('''chr1 1000 c1chr11000 INS 100 1|0 chr1_:1 1000 t1chr11000 100 1|0 0 1 1 same flip 0
            chr1 4000 c3chr14000 INS 100 1|0 chr1_:1 4000 t3chr14000 100 0|1 0 1 1 flip flip 1
            chr1 4001 c4chr14001 INS 100 1|0 chr1_:1 4000 t3chr14000 100 0|1 1 1 1 flip flip 1'''),
    rows('''chr1 1000 t1chr11000 INS 100 1|0 1 1 0 1000 c1chr11000 0 .
            chr1 4000 t3chr14000 INS 100 0|1 2 2 2 4000 c3chr14000 0 .'''))

# two rows with one id string, one accepted and one refused by its length; the truth record is hit by three calls, the nearest
# of them is the one on its position.  A genotype pair that is no "gt": '1|0' against '1|1'
CASES['one_id_twice_and_three_hits'] = (
    [rec('t', 1000, 1000, '1|1')],
    [rec('dup', 990, 1000, '1|1'), rec('dup', 990, 100, '1|1'), rec('c3', 1000, 1000, '1|0'), rec('c4', 1010, 1000, '1|1')], 100, 0.5,
    rows('''chr1 990 dupchr1990 INS 1000 1|1 chr1_:1 1000 tchr11000 1000 1|1 10 1 1 both flip 1
            chr1 990 dupchr1990 INS 100 1|1 chr1_:1 1000 tchr11000 1000 1|1 10 0 0 . flip 0
            chr1 1000 c3chr11000 INS 1000 1|0 chr1_:1 1000 tchr11000 1000 1|1 0 1 0 . flip 0
            chr1 1010 c4chr11010 INS 1000 1|1 chr1_:1 1000 tchr11000 1000 1|1 10 1 1 both flip 1'''),
    rows('''chr1 1000 tchr11000 INS 1000 1|1 3 2 2 1000 c3chr11000 0 .'''))

# the four reasons: too far; the length; the nearest call went to the record next door; a list without a call
CASES['four_reasons'] = (
    [rec('tfar', 1000, 1000, '1|1'), rec('tsize', 5000, 1000, '1|1'), rec('telse', 9000, 1000, '1|1'), rec('thit', 9010, 1000, '1|1'),
     rec('tnone', 500, 1000, '1|1', chrom='chr2')],
    [rec('cA', 2000, 1000, '1|1'), rec('cB', 5000, 100, '1|1'), rec('cC', 9008, 1000, '1|1')], 100, 0.5,
    rows('''chr1 2000 cAchr12000 INS 1000 1|1 chr1_:1 1000 tfarchr11000 1000 1|1 1000 0 0 . flip 0
            chr1 5000 cBchr15000 INS 100 1|1 chr1_:1 5000 tsizechr15000 1000 1|1 0 0 0 . flip 0
            chr1 9008 cCchr19008 INS 1000 1|1 chr1_:1 9010 thitchr19010 1000 1|1 2 1 1 both flip 1'''),
    rows('''chr1 1000 tfarchr11000 INS 1000 1|1 0 0 0 2000 cAchr12000 1000 far
            chr1 5000 tsizechr15000 INS 1000 1|1 0 0 0 5000 cBchr15000 0 size
            chr1 9000 telsechr19000 INS 1000 1|1 0 0 0 9008 cCchr19008 8 elsewhere
            chr1 9010 thitchr19010 INS 1000 1|1 1 1 1 9008 cCchr19008 2 .
            chr2 500 tnonechr2500 INS 1000 1|1 0 0 0 . . . no_call'''))

# the reverse search's ties: calls at equal distance on either side -- the lower position; two calls on that position -- the one
# that comes first in the callset.  The DEL list: the same with the callset order turned round, and another phase set
CASES['reverse_ties'] = (
    [rec('t', 1000, 100, '1|0'), rec('d', 1000, 100, '0|1', typ='DEL')],
    [rec('c1', 1100, 100, '1|0'), rec('c2', 900, 100, '1|0'), rec('c3', 900, 100, '1|0'),
     rec('e3', 900, 100, '1|0', typ='DEL', ps='chr1_:7'), rec('e2', 900, 100, '1|0', typ='DEL', ps='chr1_:7'),
     rec('e1', 1100, 100, '1|0', typ='DEL', ps='chr1_:7')], 1000, 0.0,
    rows('''chr1 1100 c1chr11100 INS 100 1|0 chr1_:1 1000 tchr11000 100 1|0 100 1 1 same same 1
            chr1 900 c2chr1900 INS 100 1|0 chr1_:1 1000 tchr11000 100 1|0 100 1 1 same same 1
            chr1 900 c3chr1900 INS 100 1|0 chr1_:1 1000 tchr11000 100 1|0 100 1 1 same same 1
            chr1 900 e3chr1900 DEL 100 1|0 chr1_:7 1000 dchr11000 100 0|1 100 1 1 flip flip 1
            chr1 900 e2chr1900 DEL 100 1|0 chr1_:7 1000 dchr11000 100 0|1 100 1 1 flip flip 1
            chr1 1100 e1chr11100 DEL 100 1|0 chr1_:7 1000 dchr11000 100 0|1 100 1 1 flip flip 1'''),
    rows('''chr1 1000 tchr11000 INS 100 1|0 3 3 3 900 c2chr1900 100 .
            chr1 1000 dchr11000 DEL 100 0|1 3 3 3 900 e3chr1900 100 .'''))


LENS = (300, 700, 1000, 4900, 7000, 1000)
RATIOS = (0.0, 0.3, 0.7, 0.1 + 0.2, 1.0)
REFDISTS = (0, 3, 10, 1000)


def random_problem(seed, n_calls, n_base, n_keys, call_pos=None, base_pos=None, unlisted=0):
    """Flat arrays as evaluation.flatten makes them, with 'refdist' and 'ratio'.  The truth records are dealt to the keys at random
    (with 48 keys and a few records most lists are empty); when more than one list has records the last of them gets no call.
    call_pos / base_pos: every call / truth record of the FIRST list that has records sits there.  unlisted: one call in that
    many has no list key (all-ones: flatten never makes one, the C interface takes it), the first and the last call among them."""
    rng = np.random.default_rng(seed)
    bkey = np.sort(rng.integers(0, n_keys, n_base))
    off = np.searchsorted(bkey, np.arange(n_keys + 1)).astype(np.uint32)
    span = int(rng.integers(24, 24 + (n_base + n_calls) // 4 + 1))
    bpos = rng.integers(0, span, n_base)
    used = np.unique(bkey)
    if base_pos is not None:
        bpos[bkey == used[0]] = base_pos
    bpos = bpos[np.lexsort((bpos, bkey))]
    with_calls = used[:-1] if len(used) > 1 else used
    ckey = with_calls[rng.integers(0, len(with_calls), n_calls)]
    cpos = rng.integers(0, span, n_calls)
    if call_pos is not None:
        cpos[ckey == used[0]] = call_pos

    ckey = ckey.astype(np.uint32)
    if unlisted:
        ckey[rng.integers(0, unlisted, n_calls) == 0] = L.EVAL_NONE
        ckey[[0, -1]] = L.EVAL_NONE

    def ids(n):                                  # one in 16 repeats an earlier record's id
        own = np.arange(n)
        return np.where(rng.integers(0, 16, n) == 0, rng.integers(0, np.maximum(own, 1)), own).astype(np.uint32)

    n_groups = n_calls // 5 + 1
    return dict(base_off=off, base_pos=bpos.astype(np.uint32), base_len=np.array(LENS, dtype=np.uint32)[rng.integers(0, len(LENS), n_base)],
                base_uid=ids(n_base), base_hp=rng.integers(0, 5, n_base).astype(np.uint8),
                call_key=ckey.astype(np.uint32), call_pos=cpos.astype(np.uint32),
                call_len=np.array(LENS, dtype=np.uint32)[rng.integers(0, len(LENS), n_calls)], call_uid=ids(n_calls),
                call_group=rng.integers(0, n_groups, n_calls).astype(np.uint32), call_hp=rng.integers(0, 5, n_calls).astype(np.uint8),
                n_groups=n_groups, n_base_uid=n_base, n_call_uid=n_calls,
                refdist=int(REFDISTS[int(rng.integers(0, len(REFDISTS)))]), ratio=float(RATIOS[int(rng.integers(0, len(RATIOS)))]))


def brute(a):
    """-> (the six counts, calls, base) of the problem `a`, one record at a time."""
    refdist, ratio = a['refdist'], a['ratio']
    off, bpos, blen, buid, bhp = ([int(x) for x in a[k]] for k in ('base_off', 'base_pos', 'base_len', 'base_uid', 'base_hp'))
    ckey, cpos, clen, cuid, cgrp, chp = ([int(x) for x in a[k]] for k in ('call_key', 'call_pos', 'call_len', 'call_uid', 'call_group', 'call_hp'))
    nb, nc = len(bpos), len(cpos)
    calls = np.zeros(nc, dtype=L.EVAL_CALL_DTYPE)
    base = np.zeros(nb, dtype=L.EVAL_BASE_DTYPE)
    groups = {}
    pair = [None] * nc
    for c in range(nc):
        k = ckey[c]
        if k == L.EVAL_NONE:                     # compared with nothing: it only carries its group's labelling
            pair[c] = (L.EVAL_NONE, L.EVAL_NONE, 0)
            continue
        b = off[k] + eval_ref.nearest(bpos[off[k]:off[k + 1]], cpos[c])
        dist = abs(cpos[c] - bpos[b])
        near = dist <= refdist
        size = eval_ref.accepts(cpos[c], cpos[c], clen[c], blen[b], 0, ratio)
        bits = near * L.EVAL_NEAR | size * L.EVAL_SIZE
        if near and size:
            ch, bh = chp[c], bhp[b]
            gt = (ch in (0, 1) and bh in (0, 1)) or ch == bh == 2
            same = ch == bh
            flip = ch == bh == 2 or (ch, bh) in ((0, 1), (1, 0))
            bits |= L.EVAL_MATCHED | gt * L.EVAL_GT | same * L.EVAL_SAME | flip * L.EVAL_FLIP
            s = groups.setdefault(cgrp[c], [set(), set()])
            if same:
                s[0] |= {('c', cuid[c]), ('b', buid[b])}
            if flip:
                s[1] |= {('c', cuid[c]), ('b', buid[b])}
        pair[c] = (b, dist, bits)
    sets = [set() for _ in range(6)]
    for c in range(nc):
        b, dist, bits = pair[c]
        s = groups.get(cgrp[c], [set(), set()])
        flipped = not len(s[0]) > len(s[1])
        if flipped:
            bits |= L.EVAL_LABEL
        if bits & L.EVAL_MATCHED and bits & (L.EVAL_FLIP if flipped else L.EVAL_SAME):
            bits |= L.EVAL_HP
        calls[c] = (b, dist, bits)
        for at, bit, field in ((0, L.EVAL_MATCHED, 'n_calls'), (2, L.EVAL_GT, 'n_gt'), (4, L.EVAL_HP, 'n_hp')):
            if bits & bit:
                base[b][field] += 1
                sets[at].add(cuid[c])
                sets[at + 1].add(buid[b])
    for k in range(len(off) - 1):
        mine = [c for c in range(nc) if ckey[c] == k]
        for j in range(off[k], off[k + 1]):
            if not mine:
                base[j]['nearest'] = base[j]['nearest_dist'] = L.EVAL_NONE
                base[j]['reason'] = 0
                continue
            dist, _, c = min((abs(cpos[c] - bpos[j]), cpos[c], c) for c in mine)
            base[j]['nearest'], base[j]['nearest_dist'] = c, dist
            if base[j]['n_calls']:
                base[j]['reason'] = L.EVAL_HIT
            elif dist > refdist:
                base[j]['reason'] = 1
            elif not eval_ref.accepts(0, 0, clen[c], blen[j], 0, ratio):
                base[j]['reason'] = 2
            else:
                assert pair[c][0] != j
                base[j]['reason'] = 3
    return tuple(len(s) for s in sets), calls, base
