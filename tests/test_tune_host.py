# coding=utf-8
"""Threshold sweep, host side (no GPU): the vector's names and defaults, grid parsing, and the restated tree of
tests/tune_ref.py against oracle/ef_oracle.decide at the defaults."""
import json
import math
import os

import numpy as np
import pytest

from duet_amd import tune
from oracle import ef_oracle as O
from tests import helpers as H
from tests import tune_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

TABLE = [('c0_min_sv_num', 4), ('c2_min_sv_ratio', 0.72), ('c2_max_avgsc_diff', 1369.5), ('c2_min_sv_num', 3), ('c2_min_hap0', 6),
         ('c1_onehap_sv_ratio_lo', 0.24), ('c1_onehap_sv_ratio_hi', 0.9), ('c1_hapread_ratio', 0.75), ('c1_max_avgsc_diff', 2400),
         ('c1_twohap_sv_ratio_1', 0.3), ('c1_twohap_sv_ratio_2', 0.45), ('c1_max_ref_num', 10), ('c1_twohap_sv_ratio_3', 0.75),
         ('c1_max_totsc_ratio', 9.72)]


def test_names_and_defaults_follow_the_table():
    assert list(tune.NAMES) == [n for n, _ in TABLE]
    assert [tune.DEFAULTS[n] for n in tune.NAMES] == [float(v) for _, v in TABLE]
    assert list(tune.vector()) == [float(v) for _, v in TABLE]


def test_header_struct_has_the_same_fields():
    with open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'duet_ef.h')) as f:
        text = f.read()
    body = text[text.index('typedef struct duet_tune_thresholds {'):text.index('} duet_tune_thresholds;')]
    assert [l.split()[1].rstrip(';') for l in body.splitlines()[1:] if l.strip().startswith('double')] == list(tune.NAMES)


def test_grid_list_and_product():
    g = tune.expand_grid([{}, {'c1_max_ref_num': 5}, {'c2_min_sv_ratio': 'nan', 'c1_max_totsc_ratio': '-inf'}])
    assert g.shape == (3, 14)
    assert list(g[0]) == list(tune.vector())
    assert g[1][tune.NAMES.index('c1_max_ref_num')] == 5.0
    assert math.isnan(g[2][1]) and g[2][13] == -math.inf
    p = tune.expand_grid({'c2_min_sv_ratio': [0.7, 0.72, 0.8], 'c1_max_ref_num': [5, 'inf']})
    assert p.shape == (6, 14)
    assert [(r[1], r[11]) for r in p] == [(a, b) for a in (0.7, 0.72, 0.8) for b in (5.0, math.inf)]
    assert tune.expand_grid({'c0_min_sv_num': 2}).shape == (1, 14)


@pytest.mark.parametrize('bad', [{'no_such_name': [1]}, [{'c2_min_sv_ratio': 0.7, 'typo': 1}], [], {'c0_min_sv_num': ['x']}, 3])
def test_grid_errors(bad):
    with pytest.raises(ValueError):
        tune.expand_grid(bad)


def test_grid_file_and_vector_file(tmp_path):
    p = tmp_path / 'g.json'
    p.write_text(json.dumps({'c1_hapread_ratio': [0.5, 0.75]}))
    assert tune.load_grid(str(p)).shape == (2, 14)
    q = tmp_path / 'v.json'
    q.write_text(json.dumps({'c1_max_ref_num': 7}))
    assert tune.load_vector(str(q))[11] == 7.0
    q.write_text(json.dumps([{}]))
    with pytest.raises(ValueError):
        tune.load_vector(str(q))


def test_scores_are_the_evaluators_quotients():
    c = dict(n_calls=10, n_groups=4, call_tp=6, base_tp=5, call_gt=4, base_gt=4, call_hp=3, base_hp=2, n_raise=0)
    got = tune.scores(c, 20)
    p, r = 6 / 10, 5 / 20
    assert got[:4] == (10 / 4, p, r, 2 * p * r / (p + r))
    assert all(math.isnan(x) for x in tune.scores(dict(c, n_calls=0, n_groups=0), 20))
    assert all(math.isnan(x) for x in tune.scores(dict(c, call_hp=0, base_hp=0), 20))
    assert all(math.isnan(x) for x in tune.scores(dict(c, n_raise=1), 20))


def test_restated_tree_equals_oracle_on_known_answers():
    with open(os.path.join(GOLDEN, 'kat_predict_hp.json')) as f:
        kat = json.load(f)
    from tests.test_oracle_golden import _kat_candidate
    seeds = set(kat['oneps'])
    v = tune.vector()
    for r in kat['rows']:
        cd = _kat_candidate(r['marks'], r['pos'], r['svread'], r['refread'])
        assert tune_ref.decide_cd(cd, r['cls'], seeds, v) == O.decide(cd, r['cls'], seeds) == (r['pred'], r['ps'])


@pytest.mark.parametrize('name,src,params', H.full_cases(), ids=[c[0] for c in H.full_cases()])
def test_restated_tree_equals_oracle_on_golden_cases(name, src, params):
    v = tune.vector()
    want = O.sv_phasing_text(src, params['svlen_thres'], params['suppread_thres'])
    assert tune_ref.phased_text(src, params['svlen_thres'], params['suppread_thres'], v) == want
    with open(os.path.join(src, 'phased_sv.vcf')) as f:
        assert f.read() == want
