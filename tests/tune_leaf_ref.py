# coding=utf-8
"""Test-side restatement of the leaf census (duet_amd/csrc/duet_tune_leaf.hip; include/duet_ef.h, "Leaf census"): the 18 exits of
predict_hp's tree on top of tune_ref.decide_vec's arithmetic, and one LEAF_COUNTS_DTYPE record per (vector, stratum, leaf) with
the group labelling of tune_score_ref.counts_of_preds (call ids plus pair ids, ties to "flip")."""
import numpy as np

from duet_amd import _lib

IN, RAISES, MATCHED = _lib.TUNE_IN_CALLS, _lib.TUNE_RAISES, _lib.TUNE_MATCHED


def leaf_of(cls, svread, refread, deg, hap1, hap2, hap0, allhap, t1, t2, v):
    """-> (leaf, pred): the table of include/duet_ef.h, in Python's own arithmetic and comparisons (a comparison with nan is
    false and takes the else branch)."""
    (c0_min_sv_num, c2_min_sv_ratio, c2_max_avgsc_diff, c2_min_sv_num, c2_min_hap0, lo_r, hi_r, hr_t, c1_diff, r1, r2, max_ref,
     r3, max_tot) = v if type(v) is tuple else [float(x) for x in v]
    hapread_ratio = allhap / deg
    a1 = t1 / hap1 if hap1 > 0 else 0
    a2 = t2 / hap2 if hap2 > 0 else 0
    sv_ratio = svread / (svread + refread)
    lo, hi = min(t1, t2), max(t1, t2)
    totsc_ratio = hi / lo if lo > 0 else 0
    onehap = lo == 0 and hi != 0
    avgsc_diff = abs(a2 - a1)
    if cls == 0:
        return (0, 3) if sv_ratio == 1 and svread >= c0_min_sv_num else (1, 0)
    if cls == 2:
        if not sv_ratio >= c2_min_sv_ratio:
            return 2, 0
        if avgsc_diff <= c2_max_avgsc_diff:
            return (3, 3) if svread >= c2_min_sv_num else (4, 0)
        return (5, 3) if hap0 >= c2_min_hap0 else (6, 0)
    gate = hapread_ratio <= hr_t and avgsc_diff <= c1_diff or hapread_ratio > hr_t
    if onehap:
        if sv_ratio <= lo_r:
            return 7, 0
        if sv_ratio <= hi_r:
            return (8, 1 if a1 > 0 else 2) if gate else (9, 0)
        return (10, 3) if gate else (11, 0)
    if sv_ratio <= r1:
        return 12, 0
    if sv_ratio <= r2:
        return (13, 0) if refread > max_ref else (14, 1 if t1 > t2 else 2)
    if sv_ratio <= r3:
        return (15, 3) if totsc_ratio <= max_tot else (16, 1 if t1 > t2 else 2)
    return 17, 3


ARGS = ('cls', 'svread', 'refread', 'deg', 'hap1', 'hap2', 'hap0', 'allhap', 't1', 't2')


def feature_rows(feat):
    """Per candidate the arguments of leaf_of as Python integers, or None where it is not eligible."""
    cols = [feat[n].tolist() for n in ARGS]
    return [row if e else None for e, row in zip(feat['eligible'].tolist(), zip(*cols))]


def leaves_from_features(feat, v, rows=None):
    """-> (leaf int[C], pred int[C]); -1 / 0 for a candidate that is not eligible."""
    rows = rows if rows is not None else feature_rows(feat)
    v = tuple(float(x) for x in v)
    got = [leaf_of(*(row + (v,))) if row is not None else (-1, 0) for row in rows]
    return (np.array([g[0] for g in got], dtype=np.int64).reshape(len(feat)), np.array([g[1] for g in got], dtype=np.int64).reshape(len(feat)))


def group_labels(feat, pred, truth):
    """group -> True where the group takes "same" under these preds: counts_of_preds' rule over all leaves together."""
    flags, group, pair = truth['cand_flags'], truth['cand_group'], truth['cand_pair']
    sets = {}
    for c, p in enumerate(pred):
        fl = int(flags[c])
        if not feat['eligible'][c] or p == 0 or not fl & IN:
            continue
        s = sets.setdefault(int(group[c]), [set(), set(), set(), set()])
        if not fl & MATCHED:
            continue
        same, flip = ((fl >> (3 * (int(p) - 1)) + k) & 1 for k in (1, 2))
        if same:
            s[0].add(c)
            s[1].add(int(pair[c]))
        if flip:
            s[2].add(c)
            s[3].add(int(pair[c]))
    return {g: len(s[0]) + len(s[1]) > len(s[2]) + len(s[3]) for g, s in sets.items()}


def census(feat, vectors, truth=None, cand_stratum=None, n_strata=1):
    """-> LEAF_COUNTS_DTYPE[K, S, 18]"""
    vectors = np.asarray(vectors, dtype=np.float64).reshape(-1, len(_lib.TUNE_NAMES))
    out = np.zeros((len(vectors), n_strata, _lib.N_LEAVES), dtype=_lib.LEAF_COUNTS_DTYPE)
    rows = feature_rows(feat)
    st = np.asarray(cand_stratum, dtype=np.int64) if cand_stratum is not None else np.zeros(len(feat), dtype=np.int64)
    if truth is not None:
        flags, group = np.asarray(truth['cand_flags'], dtype=np.int64), np.asarray(truth['cand_group'], dtype=np.int64)
        listed, matched = (flags & IN) != 0, (flags & (IN | MATCHED)) == (IN | MATCHED)
    for k, v in enumerate(vectors):
        leaf, pred = leaves_from_features(feat, v, rows)
        elig = leaf >= 0
        key = st * _lib.N_LEAVES + np.maximum(leaf, 0)
        rec = {n: np.zeros(n_strata * _lib.N_LEAVES, dtype=np.int64) for n in _lib.LEAF_COUNTS_NAMES}

        def add(name, mask):
            np.add.at(rec[name], key[elig & mask], 1)

        add('n_cands', elig)
        if truth is None:
            add('n_calls', pred != 0)
        else:
            labels = group_labels(feat, pred, truth)
            takes_same = np.zeros(max(int(truth['n_groups']), 1), dtype=bool)
            for g, same in labels.items():
                takes_same[g] = same
            call = listed & (pred != 0)
            bits = (flags >> (3 * np.maximum(pred - 1, 0))) & 7                  # gt, same, flip for the pred the candidate gets
            hit = call & matched
            add('n_listed', listed)
            add('n_matched', matched)
            add('n_calls', call)
            add('n_raise', call & ((flags & RAISES) != 0))
            add('call_tp', hit)
            add('call_gt', hit & ((bits & 1) != 0))
            add('call_hp', hit & (np.where(takes_same[np.where(listed, group, 0)], bits & 2, bits & 4) != 0))
        for n in _lib.LEAF_COUNTS_NAMES:
            out[n][k] = rec[n].reshape(n_strata, _lib.N_LEAVES)
    return out


def summed(census_, axis):
    """The records summed over the leaves (axis 2) or the strata (axis 1), field by field."""
    out = np.zeros(tuple(n for i, n in enumerate(census_.shape) if i != axis), dtype=_lib.LEAF_COUNTS_DTYPE)
    for n in _lib.LEAF_COUNTS_NAMES:
        out[n] = census_[n].sum(axis=axis)
    return out
