# coding=utf-8
"""Test-side restatement of the line of one axis (duet_amd/csrc/duet_tune_line.hip, include/duet_ef.h: duet_tune_line_device) and of
the coordinate descent built on it (duet_amd/tune.py: fit), in plain Python.

    compared(f, axis)      does the record take part in the axis, and the feature the axis is compared with -- Python's own float
                           arithmetic on the record's integers, the expressions of tune_ref.decide_vec
    line(feat, axis, base, max_values)   the vectors of the line and the number of distinct values
    fit(...)               the descent, its counts from tests/tune_score_ref.py (tests/tune_strata_ref.py with a holdout) over
                           tune_ref.preds_from_features, its scores from the unchanged tune.scores

(Python divides two ints exactly and rounds once; the device converts each to binary64 first.  The two agree whenever both ints
are binary64 values, which every count and score sum of a real work directory is; the tests keep their large t1 / t2 that way.)"""
import math

import numpy as np

from duet_amd import _lib, tune
from tests import tune_score_ref, tune_strata_ref

NAMES = _lib.TUNE_NAMES
GE_AXES = (0, 1, 3, 4)                  # compared by >=: the line ends with +inf; every other axis (<=, >) starts with -inf


def compared(f, axis):
    """-> (takes part, value or None).  Raises ZeroDivisionError where the feature of a participant has no value."""
    if not f['eligible']:
        return False, None
    cls = int(f['cls'])
    svread, refread, deg = int(f['svread']), int(f['refread']), int(f['deg'])
    hap1, hap2, hap0, allhap, t1, t2 = (int(f[n]) for n in ('hap1', 'hap2', 'hap0', 'allhap', 't1', 't2'))
    lo, hi = min(t1, t2), max(t1, t2)
    onehap_totsc = hi if lo == 0 else 0

    def avgsc_diff():
        a1 = t1 / hap1 if hap1 > 0 else 0
        a2 = t2 / hap2 if hap2 > 0 else 0
        return abs(a2 - a1)

    if axis == 0:
        return cls == 0, float(svread)
    if axis in (1, 2, 3, 4):
        if cls != 2:
            return False, None
        return True, (svread / (svread + refread), avgsc_diff(), float(svread), float(hap0))[axis - 1]
    if cls != 1:
        return False, None
    if axis in (5, 6, 7, 8):
        if onehap_totsc == 0:
            return False, None
        return True, svread / (svread + refread) if axis in (5, 6) else (allhap / deg if axis == 7 else avgsc_diff())
    if onehap_totsc != 0:
        return False, None
    if axis in (9, 10, 12):
        return True, svread / (svread + refread)
    if axis == 11:
        return True, float(refread)
    return True, (hi / lo if lo > 0 else 0.0)


def values(feat, axis):
    """The distinct feature values of the axis's participants, ascending."""
    out = set()
    for f in feat:
        part, x = compared(f, axis)
        if part:
            x = float(x)
            assert math.isfinite(x) and (x > 0 or math.copysign(1.0, x) == 1.0)
            out.add(x)
    return sorted(out)


def line_values(feat, axis):
    """The D + 1 values of the whole line."""
    xs = values(feat, axis)
    return xs + [math.inf] if axis in GE_AXES else [-math.inf] + xs


def sample_indices(D, N):
    """The entries of the D + 1 kept with max_values = N."""
    if N >= 2 and D + 1 > N:
        return [i * D // (N - 1) for i in range(N)]
    return list(range(D + 1))


def line(feat, axis, base, max_values=0):
    """-> (float64[n_vec, 14], D)"""
    vals = line_values(feat, axis)
    D = len(vals) - 1
    keep = sample_indices(D, max_values)
    out = np.tile(np.asarray(base, dtype=np.float64), (len(keep), 1))
    out[:, axis] = [vals[i] for i in keep]
    return out, D


def better(x, best):
    return not math.isnan(x) and (math.isnan(best) or x > best)


def fit(feat, truth, n_base, objective, start, axes=None, rounds=8, max_values=0, hold=None):
    """The descent of tune.fit on host arrays -> (vector, trace rows as tune.fit's, without the setting columns).
    truth: the plain truth arrays; hold: dict(truth = the truth arrays numbered for the holdout strata, cand_stratum u8[C],
    n_base = [train, test])."""
    score_of = tune.SCORES.index(objective)
    axes = list(range(14)) if axes is None else [NAMES.index(a) if isinstance(a, str) else int(a) for a in axes]
    cur = np.array(start, dtype=np.float64)
    trace = []
    for rnd in range(1, rounds + 1):
        moved = False
        for ax in axes:
            vecs, D = line(feat, ax, cur, max_values)
            n_vec = len(vecs)
            batch = np.concatenate([vecs, cur[None, :]])
            if hold is not None:
                sc = tune_strata_ref.counts(feat, batch, hold['truth'], hold['cand_stratum'], 2)
                objs = [tune.scores(sc[k, 0], hold['n_base'][0])[score_of] for k in range(len(batch))]
            else:
                pc = tune_score_ref.counts(feat, batch, truth)
                objs = [tune.scores(pc[k], n_base)[score_of] for k in range(len(batch))]
            before, best, pick = objs[n_vec], objs[n_vec], n_vec
            for i in range(n_vec):
                if better(objs[i], best):
                    best, pick = objs[i], i
            old = float(cur[ax])
            if pick != n_vec:
                cur[ax] = vecs[pick, ax]
                moved = True
            row = dict(round=rnd, axis=NAMES[ax], n_distinct=D, n_vec=n_vec, exact=int(n_vec == D + 1), old=old, new=float(cur[ax]),
                       objective_before=before, objective_after=objs[pick])
            plain = tune_score_ref.counts(feat, batch[pick:pick + 1], truth)[0] if hold is not None else pc[pick]
            row.update(zip(tune.SCORES, tune.scores(plain, n_base)))
            if hold is not None:
                for s, part in enumerate(('train', 'test')):
                    row.update(('%s_%s' % (part, n), x) for n, x in zip(tune.SCORES, tune.scores(sc[pick, s], hold['n_base'][s])))
            trace.append(row)
        if not moved:
            break
    return cur, trace


def bits(a):
    """float64 array -> its 64-bit patterns."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
