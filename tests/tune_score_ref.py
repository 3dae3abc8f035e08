# coding=utf-8
"""Test-side restatement of the sweep's scoring (tune_decide with a truth set, tune_groups, tune_popcount of
duet_amd/csrc/duet_tune.hip): one COUNTS_DTYPE record per vector from the features, the vectors and the truth arrays, with Python
sets over the arrays exactly as the comment above duet_tune_truth in include/duet_ef.h defines them.  The predictions are
tune_ref.preds_from_features'."""
import numpy as np

from duet_amd import _lib
from tests import tune_ref

IN, RAISES, MATCHED = _lib.TUNE_IN_CALLS, _lib.TUNE_RAISES, _lib.TUNE_MATCHED


def counts_of_preds(feat, preds, truth):
    """One vector: dict of the COUNTS_DTYPE fields."""
    out = dict.fromkeys(_lib.COUNTS_NAMES, 0)
    if truth is None:
        out['n_calls'] = sum(1 for p in preds if p)                 # every emitted candidate
        return out
    flags, group, uid, pair = truth['cand_flags'], truth['cand_group'], truth['cand_uid'], truth['cand_pair']
    off, pair_uid = truth['group_pair_off'], truth['pair_uid']
    groups = {}                                                     # group -> [same calls, same pairs, flip calls, flip pairs]
    base_tp, base_gt, base_hp = set(), set(), set()
    for c, p in enumerate(preds):
        fl = int(flags[c])
        if not feat['eligible'][c] or p == 0 or not fl & IN:        # not emitted, or not in the evaluator's call list
            continue
        out['n_calls'] += 1
        g = int(group[c])
        sets = groups.setdefault(g, [set(), set(), set(), set()])
        if fl & RAISES:
            out['n_raise'] += 1
        if not fl & MATCHED:
            continue
        u, pr = int(uid[c]), int(pair[c])
        assert int(off[g]) <= pr < int(off[g + 1]) and int(pair_uid[pr]) == u, 'truth arrays are not valid at candidate %d' % c
        gt, same, flip = ((fl >> (3 * (p - 1)) + k) & 1 for k in range(3))
        out['call_tp'] += 1                                         # a candidate is one call id
        base_tp.add(u)
        if gt:
            out['call_gt'] += 1
            base_gt.add(u)
        if same:
            sets[0].add(c)
            sets[1].add(pr)
        if flip:
            sets[2].add(c)
            sets[3].add(pr)
    out['n_groups'] = len(groups)
    for same_c, same_p, flip_c, flip_p in groups.values():          # :143-148, ties to "flip"
        take_c, take_p = (same_c, same_p) if len(same_c) + len(same_p) > len(flip_c) + len(flip_p) else (flip_c, flip_p)
        out['call_hp'] += len(take_c)
        base_hp |= set(int(pair_uid[pr]) for pr in take_p)
    out['base_tp'], out['base_gt'], out['base_hp'] = len(base_tp), len(base_gt), len(base_hp)
    return out


def preds_and_counts(feat, vectors, truth=None):
    """-> (pred u8[K, C], COUNTS_DTYPE[K])"""
    vectors = np.asarray(vectors, dtype=np.float64).reshape(-1, len(_lib.TUNE_NAMES))
    pred = np.zeros((len(vectors), len(feat)), dtype=np.uint8)
    out = np.zeros(len(vectors), dtype=_lib.COUNTS_DTYPE)
    for k, v in enumerate(vectors):
        pred[k] = tune_ref.preds_from_features(feat, v)
        rec = counts_of_preds(feat, pred[k].tolist(), truth)
        for name in _lib.COUNTS_NAMES:
            out[name][k] = rec[name]
    return pred, out


def counts(feat, vectors, truth=None):
    """-> COUNTS_DTYPE[K]"""
    return preds_and_counts(feat, vectors, truth)[1]
