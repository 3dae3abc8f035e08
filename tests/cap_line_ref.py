# coding=utf-8
"""Test-side restatement of the line of the PC cap (duet_amd/csrc/duet_tune_capline.hip, include/duet_ef.h:
duet_tune_cap_line_device, duet_svim_cap_line_device) and of the descent with a cap axis (duet_amd/tune.py: fit), in plain Python.

    participants(soa, s, r)      the pc of every mark of a kept candidate whose read is tagged with pc <= 2^30 - 3
    raw_participants(mark_read, read_tag)   the same over raw marks, without a kept test (the svim form)
    line(values)                 the distinct values ascending, 0 in front unless it is one of them -> (line, D)
    pick(line, max_values)       the entries an entry writes
    fit(world, ...)              the descent: the 14 axes as tests/tune_line_ref.py walks them, the cap axis over the line, the
                                 features of a cap from tests/pc_cap_ref.py, the counts from tests/tune_score_ref.py
"""
import math

import numpy as np

from duet_amd import _lib, tune
from tests import tune_line_ref as L
from tests import tune_score_ref, tune_strata_ref

CAP_MAX = (1 << 30) - 3
ABSENT = 0xFFFFFFFF
UNTAGGED = (1 << 64) - 1
CAP_AXIS = 'pc_cap'


def mark_pc(mark_read, read_tag, m):
    """The pc of mark m when it can vote under some cap, else None (mark_tag's test in duet_tune_feat.hip.h)."""
    r = int(mark_read[m])
    if r == ABSENT or r >= len(read_tag):
        return None
    t = int(read_tag[r])
    if t == UNTAGGED:
        return None
    pc = (t >> 32) & 0x3FFFFFFF
    return pc if pc <= CAP_MAX else None


def participants(soa, svlen_thres, suppread_thres):
    out = []
    for c in range(soa.n_cands):
        if not (int(soa.cand_svlen[c]) >= svlen_thres and int(soa.cand_svread[c]) >= suppread_thres and int(soa.cand_gt_ok[c]) != 0):
            continue
        for m in range(int(soa.cand_off[c]), int(soa.cand_off[c + 1])):
            pc = mark_pc(soa.mark_read, soa.read_tag, m)
            if pc is not None:
                out.append(pc)
    return out


def raw_participants(mark_read, read_tag):
    return [pc for pc in (mark_pc(mark_read, read_tag, m) for m in range(len(mark_read))) if pc is not None]


def line(values):
    """-> (the line, D)"""
    xs = sorted(set(int(v) for v in values))
    return (xs if xs and xs[0] == 0 else [0] + xs), len(xs)


def pick(full, max_values=0):
    n, N = len(full), int(max_values)
    if N >= 2 and n > N:
        return [full[i * (n - 1) // (N - 1)] for i in range(N)]
    return list(full)


def soa_line(soa, svlen_thres, suppread_thres, max_values=0):
    """-> (values written, D, L) of the candidate form"""
    full, D = line(participants(soa, svlen_thres, suppread_thres))
    return pick(full, max_values), D, len(full)


def raw_line(mark_read, read_tag, max_values=0):
    full, D = line(raw_participants(mark_read, read_tag))
    return pick(full, max_values), D, len(full)


def records(dicts):
    """tune_ref.oracle_features' dicts -> FEATURE_DTYPE array."""
    out = np.zeros(len(dicts), dtype=_lib.FEATURE_DTYPE)
    for name in ('kept', 'eligible', 'cls', 'hap1', 'hap2', 'hap0', 'allhap', 't1', 't2', 'ps', 'deg', 'svread', 'refread'):
        out[name] = [d[name] for d in dicts]
    return out


def div_zero(feat):
    return bool(np.any((feat['eligible'] != 0) & (feat['svread'].astype(np.int64) + feat['refread'].astype(np.int64) == 0)))


def fit(world, objective, start, cap, axes, rounds=8, max_values=0, hold=False):
    """The descent of tune.fit with a cap axis -> (vector, final cap, trace rows as tune.fit's, without the setting columns).
    world: features(cap) -> FEATURE_DTYPE[C]; truth(feat) -> the plain truth arrays (with n_base); hold(feat) -> dict(truth,
    cand_stratum, n_base = [train, test]) (hold = True); line() -> (the whole cap line, D).  axes: field names and 'pc_cap'."""
    score_of = tune.SCORES.index(objective)
    cur = np.array(start, dtype=np.float64)
    cap = int(cap)
    NAMES = _lib.TUNE_NAMES

    def scored(feat, vecs):
        """-> (objective per vector, plain counts, strata counts or None, n_base, hold or None)"""
        truth = world.truth(feat)
        pc = tune_score_ref.counts(feat, vecs, truth)
        if hold:
            h = world.hold(feat)
            sc = tune_strata_ref.counts(feat, vecs, h['truth'], h['cand_stratum'], 2)
            return [tune.scores(sc[k, 0], h['n_base'][0])[score_of] for k in range(len(vecs))], pc, sc, truth['n_base'], h
        return [tune.scores(pc[k], truth['n_base'])[score_of] for k in range(len(vecs))], pc, None, truth['n_base'], None

    def finish(row, pc_rec, sc_rec, n_base, h):
        row.update(zip(tune.SCORES, tune.scores(pc_rec, n_base)))
        if h is not None:
            for s, part in enumerate(('train', 'test')):
                row.update(('%s_%s' % (part, n), x) for n, x in zip(tune.SCORES, tune.scores(sc_rec[s], h['n_base'][s])))
        return row

    feat = world.features(cap)
    if div_zero(feat):
        raise ZeroDivisionError
    trace = []
    for rnd in range(1, rounds + 1):
        moved = False
        for ax in axes:
            if ax == CAP_AXIS:
                full, D = world.line()
                vals = pick(full, max_values)
                res = []
                for c in vals + [cap]:
                    f = world.features(c)
                    res.append(None if div_zero(f) else scored(f, cur[None, :]))
                objs = [math.nan if r is None else r[0][0] for r in res]
                n_vec = len(vals)
                before, best, at = objs[n_vec], objs[n_vec], n_vec
                for i in range(n_vec):
                    if L.better(objs[i], best):
                        best, at = objs[i], i
                old = cap
                if at != n_vec:
                    cap = vals[at]
                    moved = True
                    feat = world.features(cap)
                _, pc, sc, n_base, h = res[at]
                row = dict(round=rnd, axis=CAP_AXIS, n_distinct=D, n_vec=n_vec, exact=int(n_vec == len(full)), old=old, new=cap,
                           objective_before=before, objective_after=objs[at])
                trace.append(finish(row, pc[0], sc[0] if sc is not None else None, n_base, h))
                continue
            ax = NAMES.index(ax) if isinstance(ax, str) else int(ax)
            vecs, D = L.line(feat, ax, cur, max_values)
            n_vec = len(vecs)
            batch = np.concatenate([vecs, cur[None, :]])
            objs, pc, sc, n_base, h = scored(feat, batch)
            before, best, at = objs[n_vec], objs[n_vec], n_vec
            for i in range(n_vec):
                if L.better(objs[i], best):
                    best, at = objs[i], i
            old = float(cur[ax])
            if at != n_vec:
                cur[ax] = vecs[at, ax]
                moved = True
            row = dict(round=rnd, axis=NAMES[ax], n_distinct=D, n_vec=n_vec, exact=int(n_vec == D + 1), old=old, new=float(cur[ax]),
                       objective_before=before, objective_after=objs[at])
            trace.append(finish(row, pc[at], sc[at] if sc is not None else None, n_base, h))
        if not moved:
            break
    return cur, cap, trace
