# coding=utf-8
"""The leaf census's reference (tests/tune_leaf_ref.py) tied to what is already pinned, on the CPU: its leaves give the pred the
unmodified predict_hp recorded (tests/golden/kat_random.npz) and the pred of tune_ref.decide_vec for any vector; its records sum
to tune_score_ref's counts over the leaves and to the S = 1 records over the strata.  And the rows of --by_leaf."""
import math
import os

import numpy as np
import pytest

from duet_amd import _lib, tune
from oracle import ef_oracle as O
from tests import tune_leaf_ref, tune_ref, tune_score_ref
from tests.test_gpu_tune_score_edges import random_features, random_truth, random_vectors

SUMMED = ('n_calls', 'call_tp', 'call_gt', 'call_hp', 'n_raise')       # the fields the sweep's record shares with the leaf record


def test_table_and_binding_agree():
    assert _lib.N_LEAVES == 18 == len(_lib.LEAF_NAMES) == len(set(_lib.LEAF_NAMES)) == len(_lib.LEAF_PRED)
    assert _lib.LEAF_COUNTS_DTYPE.itemsize == 32
    assert set(_lib.LEAF_PRED) == {0, 1, 3} and set(tune.LEAF_PRED_TEXT) == {0, 1, 3}
    for name, pred in zip(_lib.LEAF_NAMES, _lib.LEAF_PRED):           # a name says what the leaf emits
        assert (pred == 3) == name.endswith(('_call', '_hom')) and (pred == 1) == name.endswith('_het')


def test_header_names_the_same_leaves():
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'duet_ef.h')) as f:
        text = f.read()
    body = re.search(r'#define DUET_TUNE_LEAF_NAMES(.*?)\}', text, flags=re.S).group(1)
    assert tuple(re.findall(r'"([a-z0-9_]+)"', body)) == _lib.LEAF_NAMES
    preds = re.search(r'#define DUET_TUNE_LEAF_PRED \{(.*?)\}', text).group(1)
    assert tuple(int(x) for x in preds.split(',')) == _lib.LEAF_PRED
    assert re.search(r'#define DUET_TUNE_N_LEAVES (\d+)', text).group(1) == '18'


def test_leaves_give_the_recorded_pred_and_all_are_reached(golden_dir):
    with np.load(os.path.join(golden_dir, 'kat_random.npz')) as zf:
        z = {k: zf[k] for k in zf.files}
    off = z['off']
    sets = [set(int(x) for x in z['oneps_val'][z['oneps_off'][s]:z['oneps_off'][s + 1]]) for s in range(len(z['oneps_off']) - 1)]
    v = tune.vector()
    reached, bad = np.zeros(18, dtype=np.int64), 0
    for i in range(len(z['cls'])):
        cd = O.Candidate()
        cd.pos, cd.svread, cd.refread = int(z['pos'][i]), int(z['svread'][i]), int(z['refread'][i])
        a, b = off[i], off[i + 1]
        cd.marks = [(int(h), int(p), int(c)) if t else None
                    for t, h, p, c in zip(z['m_tagged'][a:b], z['m_hap'][a:b], z['m_ps'][a:b], z['m_pc'][a:b])]
        cls = int(z['cls'][i])
        hap1, hap2, hap0, allhap, t1, t2, _ = O.vote(cd, cls, sets[int(z['oneps_set'][i])])
        leaf, pred = tune_leaf_ref.leaf_of(cls, cd.svread, cd.refread, len(cd.marks), hap1, hap2, hap0, allhap, t1, t2, v)
        bad += pred != int(z['pred'][i])
        assert pred == _lib.LEAF_PRED[leaf] or (_lib.LEAF_PRED[leaf] == 1 and pred == 2)
        reached[leaf] += 1
    assert bad == 0
    assert reached.min() > 0, 'leaves never reached: %s' % [_lib.LEAF_NAMES[i] for i in np.nonzero(reached == 0)[0]]


def test_leaf_pred_is_decide_vec_for_any_vector():
    feat = random_features(7, 1500, eligible=1.0)
    vecs = random_vectors(8, 40)
    vecs[0, :], vecs[1, :], vecs[2, :] = np.nan, np.inf, -np.inf
    assert np.isnan(vecs).any() and np.isposinf(vecs).any() and np.isneginf(vecs).any()
    seen = set()
    for v in vecs:
        for f in feat:
            args = (int(f['cls']), int(f['svread']), int(f['refread']), int(f['deg']), int(f['hap1']), int(f['hap2']), int(f['hap0']),
                    int(f['allhap']), int(f['t1']), int(f['t2']), v)
            leaf, pred = tune_leaf_ref.leaf_of(*args)
            assert pred == tune_ref.decide_vec(*args)
            assert pred == _lib.LEAF_PRED[leaf] or (_lib.LEAF_PRED[leaf] == 1 and pred == 2)
            seen.add(leaf)
    assert seen == set(range(18))


@pytest.mark.parametrize('seed,C,S', [(1, 300, 1), (2, 700, 2), (3, 500, 5)])
def test_sums_over_leaves_and_over_strata(seed, C, S):
    feat = random_features(seed, C)
    truth = random_truth(seed + 10, C, n_groups=max(1, C // 9), n_uid=C // 2)
    vecs = random_vectors(seed + 20, 6)
    # a group lies inside one stratum: the stratum of a candidate is a function of its group (those outside the list: anything)
    st = (truth['cand_group'] % S).astype(np.uint8)
    st[(truth['cand_flags'] & _lib.TUNE_IN_CALLS) == 0] = np.random.default_rng(seed).integers(0, S, C)[(truth['cand_flags'] & _lib.TUNE_IN_CALLS) == 0]
    one = tune_leaf_ref.census(feat, vecs, truth)
    want = tune_score_ref.counts(feat, vecs, truth)
    over_leaves = tune_leaf_ref.summed(one, 2)
    for n in SUMMED:
        assert np.array_equal(over_leaves[n][:, 0], want[n]), n
    assert int(want['call_hp'].max()) > 5 and int(one['n_cands'].sum()) == len(vecs) * int(feat['eligible'].sum())
    assert np.array_equal(over_leaves['n_listed'][:, 0], np.full(len(vecs), int(((truth['cand_flags'] & _lib.TUNE_IN_CALLS) != 0)[feat['eligible'] != 0].sum())))
    per = tune_leaf_ref.census(feat, vecs, truth, st, S)
    assert per.shape == (len(vecs), S, 18)
    assert np.array_equal(tune_leaf_ref.summed(per, 1), one[:, 0])
    # without a truth set: the candidates and the emitted ones, nothing else
    bare = tune_leaf_ref.census(feat, vecs)
    assert np.array_equal(bare['n_cands'], one['n_cands'])
    assert np.array_equal(tune_leaf_ref.summed(bare, 2)['n_calls'][:, 0], tune_score_ref.counts(feat, vecs)['n_calls'])
    assert not any(bare[n].any() for n in _lib.LEAF_COUNTS_NAMES if n not in ('n_cands', 'n_calls'))


def test_rows_of_by_leaf(tmp_path):
    census = np.zeros((2, 2, 18), dtype=_lib.LEAF_COUNTS_DTYPE)
    census[1, 1, 14] = (9, 8, 7, 6, 3, 2, 1, 0)
    census[0, 0, 1] = (5, 4, 3, 0, 0, 0, 0, 0)
    rows = tune.leaf_rows(dict(pc_cap=4000), range(2), census, ('train', 'test'))
    assert len(rows) == 2 * 2 * 18
    assert [r['vector'] for r in rows[::36]] == [0, 1] and [r['stratum'] for r in rows[::18]] == ['train', 'test'] * 2
    assert tuple(r['leaf'] for r in rows[:18]) == _lib.LEAF_NAMES
    assert [r['pred'] for r in rows[:18]] == ['1|1', '0', '0', '1|1', '0', '1|1', '0', '0', '1|0,0|1', '0', '1|1', '0', '0', '0', '1|0,0|1',
                                              '1|1', '1|0,0|1', '1|1']
    r = rows[36 + 18 + 14]
    assert (r['pc_cap'], r['vector'], r['stratum'], r['leaf']) == (4000, 1, 'test', 'c1_two_het')
    assert [r[n] for n in tune.LEAF_COUNTS] == [9, 8, 7, 6, 3, 2, 1, 0]
    assert [r[n] for n in tune.LEAF_RATES] == [3 / 6, 2 / 6, 1 / 6]
    r = rows[1]                                                        # a leaf without a call: the quotients are nan
    assert [r[n] for n in tune.LEAF_COUNTS] == [5, 4, 3, 0, 0, 0, 0, 0] and all(math.isnan(r[n]) for n in tune.LEAF_RATES)
    nan = tune.leaf_rows({}, ('start',), None)
    assert len(nan) == 18 and all(math.isnan(r[n]) for r in nan for n in tune.LEAF_COUNTS + tune.LEAF_RATES)
    assert tuple(r['leaf'] for r in nan) == _lib.LEAF_NAMES and all(r['stratum'] == 'all' and r['vector'] == 'start' for r in nan)
    path = str(tmp_path / 'leaf.tsv')
    cols = ('pc_cap',) + tune.LEAF_COLS
    tune._write_tsv(path, cols, ([r[n] for n in cols] for r in rows))
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0].split('\t') == ['pc_cap', 'vector', 'stratum', 'leaf', 'pred', 'n_cands', 'n_listed', 'n_matched', 'n_calls', 'call_tp',
                                    'call_gt', 'call_hp', 'n_raise', 'call_precision', 'gt_precision', 'hp_precision']
    assert lines[1 + 36 + 18 + 14] == '4000\t1\ttest\tc1_two_het\t1|0,0|1\t9\t8\t7\t6\t3\t2\t1\t0\t0.5\t%r\t%r' % (2 / 6, 1 / 6)
    assert lines[2] == '4000\t0\ttrain\tc0_drop\t0\t5\t4\t3\t0\t0\t0\t0\t0\tnan\tnan\tnan'


def test_by_leaf_is_an_option_of_the_grid_and_of_the_fit():
    a = tune.parse_args(['w', 't.vcf', '--grid', 'g.json', '--by_leaf', 'leaf.tsv'])
    assert a.by_leaf == 'leaf.tsv'
    a = tune.parse_args(['w', 't.vcf', '--fit', 'hp_f1', '--by_leaf', 'leaf.tsv'])
    assert a.by_leaf == 'leaf.tsv' and a.fit == 'hp_f1'
    assert tune.parse_args(['w', 't.vcf', '--grid', 'g.json']).by_leaf == ''
