# coding=utf-8
"""Test-side restatement of the evaluator's six counts (duet_eval_counts, include/duet_ef.h) over the flat arrays of
evaluation.flatten -- the slow obvious way: a loop per call, bisect, Python ints and sets.  It shares no code with
duet_amd/evaluation.py (nothing of it is imported): a second, independent reading of src/scripts/evaluation.py:99-159."""
import bisect

NAMES = ('call_tp', 'base_tp', 'call_gt', 'base_gt', 'call_hp', 'base_hp')
NO_KEY = 0xFFFFFFFF


def nearest(bp, pos):
    """Index into the ascending list bp (len >= 1) of the record a call at pos is compared with (:117-125)."""
    i = bisect.bisect_left(bp, pos)              # the insertion point: in front of the first of equal positions
    if i == len(bp):
        return i - 1                             # behind the last record: the last record
    if i == 0:
        return 0                                 # below the first record: the first record
    if abs(pos - bp[i]) > abs(pos - bp[i - 1]):
        return i - 1                             # the left neighbour only when it is strictly nearer: a tie goes right
    return i


def accepts(pos, bpos, clen, blen, refdist, ratio):
    """:126-127.  The quotient is Python's true division of two ints (binary64, correctly rounded, as numpy's is for integers
    below 2^53); 0 / 0 is numpy's nan, and nan >= ratio is False for every ratio."""
    if abs(pos - bpos) > refdist:
        return False
    lo, hi = min(clen, blen), max(clen, blen)
    if hi == 0:
        return False
    return lo / hi >= ratio


def counts(arrays, refdist, ratio):
    """-> (call_tp, base_tp, call_gt, base_gt, call_hp, base_hp)"""
    off = [int(x) for x in arrays['base_off']]
    bpos = [int(x) for x in arrays['base_pos']]
    blen = [int(x) for x in arrays['base_len']]
    buid = [int(x) for x in arrays['base_uid']]
    bhp = [int(x) for x in arrays['base_hp']]
    refdist, ratio = int(refdist), float(ratio)
    call_tp, base_tp, call_gt, base_gt, call_hp, base_hp = set(), set(), set(), set(), set(), set()
    groups = {}                                  # group -> [same_c, same_b, flip_c, flip_b]
    lists = {}                                   # list key -> its positions
    for c in range(len(arrays['call_pos'])):
        key = int(arrays['call_key'][c])
        if key == NO_KEY:
            continue
        if key not in lists:
            lists[key] = bpos[off[key]:off[key + 1]]
        lst = lists[key]
        pos, ln, cu, ch = int(arrays['call_pos'][c]), int(arrays['call_len'][c]), int(arrays['call_uid'][c]), int(arrays['call_hp'][c])
        b = off[key] + nearest(lst, pos)
        if not accepts(pos, bpos[b], ln, blen[b], refdist, ratio):
            continue
        bu, bh = buid[b], bhp[b]
        call_tp.add(cu)
        base_tp.add(bu)
        if (ch in (0, 1) and bh in (0, 1)) or (ch == 2 and bh == 2):                    # :130-133
            call_gt.add(cu)
            base_gt.add(bu)
        sets = groups.setdefault(int(arrays['call_group'][c]), [set(), set(), set(), set()])
        if ch == bh:                                                                    # :134-136
            sets[0].add(cu)
            sets[1].add(bu)
        if (ch == 2 and bh == 2) or (ch, bh) in ((1, 0), (0, 1)):                       # :137-141
            sets[2].add(cu)
            sets[3].add(bu)
    for same_c, same_b, flip_c, flip_b in groups.values():                              # :143-148
        if len(same_c) + len(same_b) > len(flip_c) + len(flip_b):
            call_hp |= same_c
            base_hp |= same_b
        else:                                                                           # a tie goes to the mirrored labelling
            call_hp |= flip_c
            base_hp |= flip_b
    return len(call_tp), len(base_tp), len(call_gt), len(base_gt), len(call_hp), len(base_hp)
