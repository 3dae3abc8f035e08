# coding=utf-8
"""-m gpu: the line of one axis (duet_tune_line_host / _device, duet_amd/csrc/duet_tune_line.hip) against tests/tune_line_ref.py
by the 64-bit patterns of all 14 fields of every vector, for every axis, at its edge shapes; then the fit built on it
(duet_amd/tune.py: fit, --fit) against the reference's descent, trace row for trace row."""
import ctypes
import json
import math

import numpy as np
import pytest

from duet_amd import _lib, tune
from tests import tune_line_ref as L
from tests import tune_ref
from tests.test_gpu_tune import scoring_workdir, write_truth
from tests.test_gpu_tune_score_edges import random_features

pytestmark = pytest.mark.gpu

NAMES = _lib.TUNE_NAMES


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def base_vector(seed=0):
    """Every field its own recognisable number (a copy that lands in the wrong field shows), two of them 0.1 + 0.2."""
    v = tune.vector() * np.random.default_rng(seed).uniform(0.5, 1.5, 14)
    v[9] = v[10] = 0.1 + 0.2
    return v


def device_line(ctx, feat, base, axis, max_values=0):
    import torch
    C = len(feat)
    dev = torch.device('cuda', ctx.device_id)
    d_feat = torch.zeros(C * _lib.FEATURE_DTYPE.itemsize + 64, dtype=torch.uint8, device=dev)
    if C:
        d_feat[:C * _lib.FEATURE_DTYPE.itemsize] = torch.from_numpy(np.ascontiguousarray(feat).view(np.uint8).copy()).to(dev)
    out = torch.full(((C + 1) * 14,), -7.0, dtype=torch.float64, device=dev)
    n_vec, D = ctx.line_device(d_feat.data_ptr(), C, base, axis, max_values, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(C + 1, 14)
    assert np.all(got[n_vec:] == -7.0)                      # nothing written behind the vectors
    return got[:n_vec], D


def check(ctx, feat, base=None, axes=range(14), max_values=0, forms=('host', 'device')):
    base = base_vector() if base is None else base
    out = {}
    for axis in axes:
        want, D = L.line(feat, axis, base, max_values)
        for form in forms:
            got, d = ctx.line_host(feat, base, axis, max_values) if form == 'host' else device_line(ctx, feat, base, axis, max_values)
            assert d == D and got.shape == want.shape, (form, NAMES[axis], d, D, got.shape, want.shape)
            bad = np.nonzero(L.bits(got) != L.bits(want))
            assert bad[0].size == 0, (form, NAMES[axis], bad[0][:4], bad[1][:4], got[bad][:4], want[bad][:4])
        out[axis] = D
    return out


@pytest.mark.parametrize('C', [0, 1, 63, 64, 65, 256, 257, 513, 2049])
def test_shapes(ctx, C):
    D = check(ctx, random_features(100 + C, C, eligible=0.9))
    assert C < 63 or min(D.values()) >= 2


def twohap(n):
    """n eligible class-1 records in which both haplotypes voted: the participants of axes 9 - 13."""
    f = np.zeros(n, dtype=_lib.FEATURE_DTYPE)
    f['cls'], f['eligible'], f['kept'] = 1, 1, 1
    f['deg'], f['allhap'], f['hap1'], f['hap2'] = 4, 2, 1, 1
    f['t1'], f['t2'] = 300, 200
    f['svread'], f['refread'] = 1, 1
    return f


def onehap(n):
    """... in which one haplotype voted: axes 5 - 8."""
    f = twohap(n)
    f['hap2'], f['t2'], f['allhap'] = 0, 0, 1
    return f


def test_no_participant(ctx):
    f = random_features(1, 300)
    f['eligible'] = 0
    assert set(check(ctx, f).values()) == {0}
    assert check(ctx, onehap(70), axes=(0, 1, 2, 3, 4, 9, 10, 11, 12, 13)) == dict.fromkeys((0, 1, 2, 3, 4, 9, 10, 11, 12, 13), 0)
    check(ctx, onehap(70), max_values=2, axes=(0, 9))       # (one vector, whatever max_values says)


def test_every_participant_has_one_value(ctx):
    f = twohap(700)
    assert check(ctx, f, axes=(9, 10, 11, 12, 13)) == dict.fromkeys((9, 10, 11, 12, 13), 1)
    g = onehap(700)
    assert check(ctx, g, axes=(5, 6, 7, 8)) == dict.fromkeys((5, 6, 7, 8), 1)


def test_all_values_distinct(ctx):
    f = twohap(1000)
    f['refread'] = np.random.default_rng(2).permutation(1000)
    f['t1'] = 1000 + 7 * np.arange(1000)
    D = check(ctx, f, axes=(9, 11, 13))
    assert D == {9: 1000, 11: 1000, 13: 1000}


def test_runs_of_equal_values_across_positions_63_64_and_255_256(ctx):
    """All participants: value 1 at sorted positions 0 - 59, 2 at 60 - 67, 3 at 68 - 252, 4 at 253 - 260, 5 behind."""
    vals = np.repeat([1, 2, 3, 4, 5], [60, 8, 185, 8, 20])
    f = twohap(len(vals))
    f['refread'] = np.random.default_rng(3).permutation(vals)
    assert check(ctx, f, axes=(9, 11)) == {9: 5, 11: 5}
    f['cls'] = 2                                            # the same runs in svread (>=) for class 2
    f['svread'], f['refread'] = f['refread'], 7
    assert check(ctx, f, axes=(1, 3)) == {1: 5, 3: 5}


def test_equal_quotients_and_last_bit_neighbours(ctx):
    f = twohap(8)
    f['svread'] = [7, 49, 1, 2, 3, 0, 2 ** 32 - 1, 1]
    f['refread'] = [3, 21, 2, 4, 7, 5, 2 ** 32 - 1, 2 ** 32 - 1]
    xs = L.values(f, 9)
    assert xs == [0.0, 1 / (1 + (2 ** 32 - 1)), 0.3, 1 / 3, 0.5, 0.7]      # 7/10 = 49/70, 1/3 = 2/6; 0.0; (2^32 - 1) / (2^33 - 2)
    base = base_vector()
    assert base[9] == 0.1 + 0.2 != 0.3 and abs(base[9] - 0.3) < 1e-16       # the base differs from the feature 3/10 in the last bit
    assert check(ctx, f, base, axes=(9, 10, 12)) == {9: 6, 10: 6, 12: 6}
    assert check(ctx, f, base, axes=(11,)) == {11: 7}                       # refread 2^32 - 1 twice
    g = f.copy()
    g['cls'] = 0
    assert check(ctx, g, base, axes=(0,)) == {0: 7}                         # svread 0 .. 2^32 - 1, +inf behind


def test_sums_near_2_to_the_62(ctx):
    """t1, t2 near 2^62 and 2^61 in steps of 2^10 (binary64 values, see tests/tune_line_ref.py): totsc_ratio, and the average
    scores' difference of a one-haplotype vote."""
    f = twohap(40)
    k = np.arange(40, dtype=np.uint64)
    f['t1'] = (np.uint64(1) << np.uint64(62)) + (k << np.uint64(10))
    f['t2'] = (np.uint64(1) << np.uint64(61)) + ((k % np.uint64(7)) << np.uint64(10))
    f['t2'][5] = 0
    f['t1'][6] = f['t2'][6] = 0                             # lo == 0 and hi == 0: not a one-haplotype vote, totsc_ratio 0.0
    D = check(ctx, f, axes=(13,))
    assert D[13] >= 30
    g = onehap(40)
    g['t1'], g['hap1'] = f['t1'], 3
    assert check(ctx, g, axes=(8,))[8] >= 14


@pytest.mark.parametrize('axis', [3, 9])
def test_max_values(ctx, axis):
    f = random_features(9, 400)
    D = check(ctx, f, axes=(axis,))[axis]
    assert D >= 8
    for N in (2, 3, D, D + 1, D + 2, 0):
        check(ctx, f, axes=(axis,), max_values=N)


def test_refusals(ctx):
    f = random_features(10, 50)
    base = tune.vector()
    for bad in (lambda: ctx.line_host(f, base, 14), lambda: ctx.line_host(f, base, 2 ** 32 - 1), lambda: ctx.line_host(f, base, 3, 1),
                lambda: ctx.line_host(f[:0], base, 3, 1)):
        with pytest.raises(_lib.DuetLibraryError):
            bad()
    out = np.zeros((51, 14))
    n, d = ctypes.c_uint32(0), ctypes.c_uint32(0)
    full = [ctx.handle, f.ctypes.data, 50, base.ctypes.data, 3, 0, out.ctypes.data, ctypes.byref(n), ctypes.byref(d)]
    assert ctx.lib.duet_tune_line_host(*full) == 0 and n.value == d.value + 1
    for hole in (1, 3, 6, 7, 8):
        args = list(full)
        args[hole] = None
        assert ctx.lib.duet_tune_line_host(*args) == _lib.DUET_ERR_INVALID, hole
        assert ctx.lib.duet_tune_line_device(*(args + [None])) == _lib.DUET_ERR_INVALID, hole
    args = list(full)
    args[1], args[2] = None, 0                              # no candidates: the feature array may be null
    assert ctx.lib.duet_tune_line_host(*args) == 0 and (n.value, d.value) == (1, 0)


def test_deg_zero_sets_the_status(ctx):
    f = onehap(300)
    f['svread'] = np.arange(300) % 9 + 1
    check(ctx, f, axes=(7,))
    f['deg'][211] = 0
    for form in (lambda: ctx.line_host(f, tune.vector(), 7), lambda: device_line(ctx, f, tune.vector(), 7)):
        with pytest.raises(ZeroDivisionError):
            form()
    check(ctx, f, axes=(5, 6, 8, 9))                        # only the compared feature matters; and the context goes on working
    f['deg'][211] = 4
    f['svread'][7], f['refread'][7] = 0, 0
    with pytest.raises(ZeroDivisionError):
        ctx.line_host(f, tune.vector(), 5)
    check(ctx, f, axes=(7, 8))
    f['eligible'][7] = 0
    check(ctx, f, axes=(5,))


def test_workspace_is_reused_by_a_smaller_and_a_larger_call():
    c = _lib.Context(0)
    try:
        for C in (513, 65, 9000, 513):
            check(c, random_features(C, C), axes=(1, 7, 11))
    finally:
        c.close()


# ---- the fit --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def case(ctx, tmp_path_factory):
    """The small scoring work directory of tests/test_gpu_tune.py, its truth set, and the reference's inputs from the host."""
    d = tmp_path_factory.mktemp('fit')
    home, truth = str(d / 'w'), str(d / 'truth.vcf')
    scoring_workdir(home, 3)
    cands = tune.features(home, 50, 2, ctx=ctx)
    write_truth(home, cands, truth, 3)
    arrays = tune.prepare_truth(cands, truth)
    texts = list(dict.fromkeys(cands['chrom']))
    held = texts[:1]
    strata = tune.strata_holdout(held)
    hold = dict(truth=arrays, cand_stratum=np.array([tune.stratum_of(strata, t) for t in cands['chrom']], dtype=np.uint8),
                n_base=tune.truth_side(truth, strata=strata)['n_base_strata'])
    return dict(home=home, truth=truth, cands=cands, arrays=arrays, held=held, hold=hold, dir=d)


def same_trace(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        for k in ('round', 'axis', 'n_distinct', 'n_vec', 'exact'):
            assert g[k] == w[k], (k, g, w)
        assert L.bits([g['old'], g['new']]).tolist() == L.bits([w['old'], w['new']]).tolist(), (g, w)
        names = [k for k in w if k not in ('round', 'axis', 'n_distinct', 'n_vec', 'exact', 'old', 'new')]
        assert len(names) in (12, 32)
        assert tune_ref.same_floats([g[k] for k in names], [w[k] for k in names]), (g, w)


def objectives(trace):
    return [trace[0]['objective_before']] + [r['objective_after'] for r in trace]


def test_fit_reproduces_the_reference_trace(ctx, case):
    got = tune.fit(case['home'], case['truth'], 'hp_f1', rounds=3, ctx=ctx)
    vec, want = L.fit(case['cands']['feat'], case['arrays'], case['arrays']['n_base'], 'hp_f1', tune.vector(), rounds=3)
    assert len(got['fits']) == 1 and got['best'] is got['fits'][0] and got['trace'] == got['fits'][0]['trace']
    same_trace(got['trace'], want)
    assert any(r['old'] != r['new'] for r in want)
    assert all(r['svlen_thres'] == 50 and r['suppread_thres'] == 2 for r in got['trace'])
    assert np.array_equal(L.bits(got['best']['vector']), L.bits(vec))
    objs = objectives(got['trace'])
    assert not math.isnan(objs[-1]) and got['best']['objective'] == objs[-1]
    for a, b in zip(objs, objs[1:]):
        assert math.isnan(a) or b >= a                      # the objective never decreases
    # started from its own result, the fit moves nothing: one round, 14 rows
    again = tune.fit(case['home'], case['truth'], 'hp_f1', start=vec, rounds=3, ctx=ctx)
    assert len(again['trace']) == 14 and all(r['old'] == r['new'] for r in again['trace'])
    assert np.array_equal(L.bits(again['best']['vector']), L.bits(vec))
    # one spoiled axis, fitted alone, scores at least what the unspoiled vector scores
    spoiled = vec.copy()
    spoiled[9] = 0.999
    one = tune.fit(case['home'], case['truth'], 'hp_f1', start=spoiled, axes=['c1_twohap_sv_ratio_1'], rounds=2, ctx=ctx)
    assert one['best']['objective'] >= objs[-1]
    assert np.array_equal(L.bits(np.delete(one['best']['vector'], 9)), L.bits(np.delete(vec, 9)))


def test_fit_with_holdout_and_two_axes(ctx, case):
    axes = ['c1_twohap_sv_ratio_2', 'c0_min_sv_num']
    got = tune.fit(case['home'], case['truth'], 'gt_f1', axes=axes, rounds=3, max_values=5, ctx=ctx, holdout=case['held'])
    _, want = L.fit(case['cands']['feat'], case['arrays'], case['arrays']['n_base'], 'gt_f1', tune.vector(), axes=axes, rounds=3,
                    max_values=5, hold=case['hold'])
    same_trace(got['trace'], want)
    assert [r['axis'] for r in want[:2]] == axes and any(r['exact'] == 0 for r in want)
    assert all(r['objective_after'] == r['train_gt_f1'] or math.isnan(r['objective_after']) for r in got['trace'])
    whole = tune.fit(case['home'], case['truth'], 'hp_f1', rounds=2, ctx=ctx, holdout=case['held'])
    _, want = L.fit(case['cands']['feat'], case['arrays'], case['arrays']['n_base'], 'hp_f1', tune.vector(), rounds=2, hold=case['hold'])
    same_trace(whole['trace'], want)
    assert any(not math.isnan(r['test_hp_f1']) for r in want) and any(not math.isnan(r['train_hp_f1']) for r in want)


def test_command_line_writes_a_vector_that_load_vector_accepts(ctx, case, capsys):
    best, trace = str(case['dir'] / 'best.json'), str(case['dir'] / 'fit.tsv')
    tune.main([case['home'], case['truth'], '--fit', 'hp_f1', '--rounds', '2', '--axes', 'c1_max_ref_num,c2_min_sv_ratio', '-s', '50,30',
               '--out_vector', best, '--trace', trace])
    line = capsys.readouterr().out.strip().splitlines()
    assert len(line) == 1 and line[0].startswith('fit hp_f1=') and 'svlen_thres=' in line[0]
    with open(best) as f:
        obj = json.load(f)
    assert list(obj) == list(NAMES)
    vec = tune.load_vector(best)
    both = tune.fit(case['home'], case['truth'], 'hp_f1', axes=['c1_max_ref_num', 'c2_min_sv_ratio'], rounds=2, svlen_thres=(50, 30), ctx=ctx)
    assert [f['setting']['svlen_thres'] for f in both['fits']] == [50, 30]
    assert np.array_equal(L.bits(vec), L.bits(both['best']['vector']))
    top = max(f['objective'] for f in both['fits'])
    assert both['best'] is [f for f in both['fits'] if f['objective'] == top][0]        # ties: the earlier setting
    with open(trace) as f:
        rows = [l.split('\t') for l in f.read().splitlines()]
    assert rows[0] == ['svlen_thres', 'suppread_thres'] + list(tune.TRACE) + list(tune.SCORES)
    assert len(rows) == 1 + len(both['trace'])
    with pytest.raises(SystemExit):
        tune.parse_args([case['home'], case['truth'], '--fit', 'hp_f1', '--grid', 'g.json'])
    with pytest.raises(SystemExit):
        tune.parse_args([case['home'], case['truth']])
