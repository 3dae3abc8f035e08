# coding=utf-8
"""No GPU: the exactness claim behind the fit (duet_amd/tune.py: fit; include/duet_ef.h: duet_tune_line_device), on the test-side
restatements alone.  With the other 13 constants fixed, the count record of a sweep is a piecewise-constant function of one
constant that can change only at a feature value some participant has -- so the line of tests/tune_line_ref.py (one vector per
distinct value and one sentinel) holds every behaviour of the axis: any probe value scores exactly like the line vector of its
interval, and no probe beats the best of the line."""
import bisect
import math

import numpy as np
import pytest

from duet_amd import _lib, tune
from tests import tune_line_ref as L
from tests import tune_score_ref
from tests.test_gpu_tune_score_edges import random_features, random_truth

IN, RAISES = _lib.TUNE_IN_CALLS, _lib.TUNE_RAISES


def base_vector(seed):
    """Near the defaults, every field a number."""
    rng = np.random.default_rng(seed)
    return tune.vector() * rng.uniform(0.5, 1.5, 14)


def truth_without_raises(seed, C, n_groups=9, n_uid=40):
    """random_truth with RAISES cleared: the objective then has a number wherever a call is emitted."""
    t = random_truth(seed, C, n_groups, n_uid)
    t['cand_flags'] = (t['cand_flags'] & np.uint16(~RAISES & 0xFFFF)).astype(np.uint16)
    return t


def interval_index(axis, xs, p):
    """The index in the line of the vector that behaves like constant p: for x <= T and x > T what matters is how many values are
    <= p (the line is -inf, x_1 .. x_D); for x >= T how many are < p (the line is x_1 .. x_D, +inf)."""
    return bisect.bisect_left(xs, p) if axis in L.GE_AXES else bisect.bisect_right(xs, p)


def best_of(objs):
    out = math.nan
    for x in objs:
        if L.better(x, out):
            out = x
    return out


@pytest.mark.parametrize('seed,C', [(1, 300), (2, 120), (3, 33)])
def test_every_probe_scores_like_the_line_vector_of_its_interval(seed, C):
    feat = random_features(seed, C)
    truth = truth_without_raises(seed, C)
    n_base = 50
    base = base_vector(seed)
    numbers = 0
    for axis in range(14):
        vecs, D = L.line(feat, axis, base)
        xs = L.values(feat, axis)
        assert len(vecs) == D + 1 == len(xs) + 1
        on_line = tune_score_ref.counts(feat, vecs, truth)
        probes = {-math.inf, math.inf, float(base[axis])}
        for v in vecs[:, axis]:
            probes.update((float(v), float(np.nextafter(v, -np.inf)), float(np.nextafter(v, np.inf))))
        probes = sorted(probes)
        pv = np.tile(base, (len(probes), 1))
        pv[:, axis] = probes
        got = tune_score_ref.counts(feat, pv, truth)
        for p, rec in zip(probes, got):
            want = on_line[interval_index(axis, xs, p)]
            assert rec == want, (tune.NAMES[axis], p, rec, want)
        for name in ('hp_f1', 'call_f1', 'gt_precision'):
            i = tune.SCORES.index(name)
            a = best_of(tune.scores(r, n_base)[i] for r in got)
            b = best_of(tune.scores(r, n_base)[i] for r in on_line)
            assert (math.isnan(a) and math.isnan(b)) or a == b, (tune.NAMES[axis], name, a, b)
            numbers += not math.isnan(b)
    assert numbers > 20                                     # (the objectives compared were mostly numbers, not nan)


def test_the_line_of_every_axis_has_its_shape():
    feat = random_features(4, 200)
    base = tune.vector()
    for axis in range(14):
        vecs, D = L.line(feat, axis, base)
        col = vecs[:, axis]
        assert D >= 2 and len(col) == D + 1
        assert np.all(np.diff(col) > 0)                     # ascending and distinct, the sentinel included
        assert (col[-1] == math.inf and col[0] >= 0) if axis in L.GE_AXES else (col[0] == -math.inf and col[-1] < math.inf)
        others = np.delete(vecs, axis, axis=1)
        assert np.array_equal(L.bits(others), L.bits(np.tile(np.delete(base, axis), (D + 1, 1))))


def test_without_a_participant_the_line_is_its_sentinel():
    feat = random_features(5, 64)
    feat['eligible'] = 0
    for axis in range(14):
        vecs, D = L.line(feat, axis, tune.vector())
        assert D == 0 and len(vecs) == 1
        assert vecs[0, axis] == (math.inf if axis in L.GE_AXES else -math.inf)
    vecs, D = L.line(feat[:0], 7, tune.vector(), max_values=5)
    assert D == 0 and len(vecs) == 1 and vecs[0, 7] == -math.inf


def test_a_feature_without_a_value_raises():
    feat = random_features(6, 40)
    feat['cls'], feat['eligible'], feat['hap2'], feat['t2'] = 1, 1, 0, 0
    feat['hap1'], feat['t1'] = np.maximum(feat['hap1'], 1), np.maximum(feat['t1'], 1)         # one voting haplotype: axes 5 - 8
    L.line(feat, 7, tune.vector())
    feat['deg'][17] = 0
    with pytest.raises(ZeroDivisionError):
        L.line(feat, 7, tune.vector())
    L.line(feat, 8, tune.vector())                          # (only the compared feature matters)
    feat['svread'][3], feat['refread'][3] = 0, 0
    with pytest.raises(ZeroDivisionError):
        L.line(feat, 5, tune.vector())


def test_subsampling_indices():
    for D in list(range(0, 45)) + [255, 256, 4095, 100001, 2 ** 32 - 2]:
        small = D < 5000                                    # (a large line is only ever sampled here, never listed whole)
        for N in ([0] if small else []) + list(range(2, 50)) + ([D - 1, D, D + 1, D + 2] if small else []) + [4096]:
            if N < 0 or N == 1:
                continue
            idx = L.sample_indices(D, N)
            if N >= 2 and D + 1 > N:
                assert len(idx) == N and idx[0] == 0 and idx[-1] == D
                assert all(b > a for a, b in zip(idx, idx[1:]))         # never a repeat while N <= D + 1
            else:
                assert idx == list(range(D + 1))
    feat = random_features(7, 250)
    whole, D = L.line(feat, 9, tune.vector())
    for N in (2, 3, D, D + 1, D + 2):
        vecs, d = L.line(feat, 9, tune.vector(), max_values=N)
        assert d == D and len(vecs) == min(N, D + 1)
        assert np.array_equal(L.bits(vecs), L.bits(whole[L.sample_indices(D, N)]))


def test_the_descent_never_loses_and_ends_at_a_fixed_point():
    feat = random_features(8, 90)
    truth = truth_without_raises(8, 90)
    n_base = 45
    start = base_vector(8)
    vec, trace = L.fit(feat, truth, n_base, 'hp_f1', start, rounds=4)
    assert any(r['old'] != r['new'] for r in trace)
    objs = [trace[0]['objective_before']] + [r['objective_after'] for r in trace]
    assert not math.isnan(objs[-1])
    for a, b in zip(objs, objs[1:]):
        assert math.isnan(a) or b >= a
    for r in trace:
        assert (r['old'] == r['new']) == (not L.better(r['objective_after'], r['objective_before']))
        assert r['exact'] == 1 and r['n_vec'] == r['n_distinct'] + 1
    again, t2 = L.fit(feat, truth, n_base, 'hp_f1', vec, rounds=4)
    assert np.array_equal(L.bits(again), L.bits(vec)) and len(t2) == 14 and all(r['old'] == r['new'] for r in t2)
    # one spoiled axis, fitted alone, gets back at least what the unspoiled vector scores
    spoiled = vec.copy()
    spoiled[9] = 0.999
    one, t3 = L.fit(feat, truth, n_base, 'hp_f1', spoiled, axes=['c1_twohap_sv_ratio_1'], rounds=2)
    assert t3[-1]['objective_after'] >= objs[-1]
