# coding=utf-8
"""-m gpu: the PC cap as an axis of the fit (duet_amd/tune.py: fit(axes=[.., 'pc_cap', ..]), fit(fit_cap=True), --fit_cap) against
the descent of tests/cap_line_ref.py, trace row for trace row, on small work directories whose PC tags come from a pool of seven
values (and one read with a value of its own) -- so the cap line has at most nine values and the reference (the oracle's features per cap, the host truth match, the
restated counts) stays quick.  The truth sets are written from the reference's own predictions under a chosen cap, which makes that
cap (or one that predicts the same) the best and any cap that predicts otherwise strictly worse."""
import json
import math
import os
import shutil
import sys

import numpy as np
import pytest

from duet_amd import _lib, svim_mode, synth, tune
from tests import cap_line_ref as R
from tests import helpers as H
from tests import pc_cap_ref, tune_ref
from tests import tune_line_ref as L

pytestmark = pytest.mark.gpu

POOL = np.array([0, 300, 972, 2400, 8100, 9000, 15000], dtype=np.int64)
HEAD = ['##fileformat=VCFv4.2\n', '#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n']


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


class World(object):
    """What tests/cap_line_ref.py's descent asks of a problem: the reference's features per cap, the host truth match of a
    feature array, the holdout's arrays, the cap line."""

    def __init__(self, soa, txt, s, r, line=None):
        self.soa, self.s, self.r = soa, s, r
        self.cands = dict(pos=soa.cand_pos, svlen=soa.cand_svlen, **txt)
        self.truth_vcf, self.held = None, None
        self.memo, self.tmemo = {}, {}
        self.full = line or R.line(R.participants(soa, s, r))

    def features(self, cap):
        if cap not in self.memo:
            self.memo[cap] = R.records(pc_cap_ref.features(self.soa, self.s, self.r, cap))
        return self.memo[cap]

    def truth(self, feat):
        key = (self.truth_vcf, feat.tobytes())
        if key not in self.tmemo:
            self.tmemo[key] = tune.prepare_truth(dict(self.cands, feat=feat), self.truth_vcf)
        return self.tmemo[key]

    def hold(self, feat):
        strata = tune.strata_holdout(self.held)
        return dict(truth=self.truth(feat), n_base=tune.truth_side(self.truth_vcf, strata=strata)['n_base_strata'],
                    cand_stratum=np.array([tune.stratum_of(strata, t) for t in self.cands['chrom']], dtype=np.uint8))

    def line(self):
        return self.full

    def write_truth(self, path, cap, vec=None):
        """The truth set that agrees with the reference's predictions under `cap`: one record per emitted call."""
        feat = self.features(cap)
        preds = tune_ref.preds_from_features(feat, tune.vector() if vec is None else vec)
        rows = list(HEAD)
        for c, p in enumerate(preds):
            if p:
                t, ln = self.cands['svtype'][c], int(self.cands['svlen'][c])
                rows.append('%s\t%d\ttruth%d\tN\t<%s>\t.\tPASS\tSVTYPE=%s;SVLEN=%d\tGT:PS\t%s:%d\n' % (
                    self.cands['chrom'][c], int(self.cands['pos'][c]), c, t, t, ln if t in ('INS', 'DUP') else -ln, tune.HP_TEXT[p],
                    int(feat['ps'][c])))
        with open(path, 'w') as f:
            f.writelines(rows)
        return path


def pooled_workdir(home, seed, div_zero=False, lone=None):
    """tests/test_gpu_tune.py's scoring work directory with every PC tag taken from POOL.  div_zero: the last contig's reads all
    carry 15000 -- it has a seed only from that cap on -- and one of its candidates has svread = refread = 0.  lone = (contig,
    read): that one read carries 1000, a line value of its own between 972 and 2400."""
    contigs = synth.fuzz_case(seed, n_contigs=3)
    for c in contigs:
        c.spelled, c.has_bam = 'chr' + c.label, True
        c.line_pc = POOL[np.asarray(c.line_pc, dtype=np.int64) % len(POOL)]
    if lone is not None:
        c = contigs[lone[0]]
        c.line_pc[np.asarray(c.line_name_id) == lone[1]] = 1000
    if div_zero:
        c = contigs[-1]
        c.line_pc = np.full(len(c.line_pc), 15000, dtype=np.int64)
        c.cand_svread, c.cand_refread = np.array(c.cand_svread), np.array(c.cand_refread)
        c.cand_svread[0] = c.cand_refread[0] = 0
        c.cand_gt[0], c.cand_svtype[0], c.cand_svlen[0] = '0/1', 'INS', 300
    synth.write_workdir(home, contigs, dialect='cutesv', seed=seed)
    return home


def world_of(home, s=50, r=2):
    soa, txt = tune._candidates(home, s, r, False, 4)
    return World(soa, txt, s, r)


@pytest.fixture(scope='module')
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp('fit_cap')
    home = pooled_workdir(str(d / 'w'), 3, lone=(0, 2))       # (with that read at 1000, caps 972 and 1000 tie for the best of t972)
    w = world_of(home)
    w.held = list(dict.fromkeys(w.cands['chrom']))[:1]
    return dict(home=home, world=w, dir=d, at_972=w.write_truth(str(d / 't972.vcf'), 972), at_8100=w.write_truth(str(d / 't8100.vcf'), 8100))


def same_trace(got, want):
    assert len(got) == len(want), (len(got), len(want), [r['axis'] for r in got], [r['axis'] for r in want])
    for g, w in zip(got, want):
        for k in ('round', 'axis', 'n_distinct', 'n_vec', 'exact'):
            assert g[k] == w[k], (k, g, w)
        if w['axis'] == 'pc_cap':
            assert (g['old'], g['new']) == (w['old'], w['new']) and isinstance(g['old'], int) and isinstance(g['new'], int), (g, w)
        else:
            assert L.bits([g['old'], g['new']]).tolist() == L.bits([w['old'], w['new']]).tolist(), (g, w)
        names = [k for k in w if k not in ('round', 'axis', 'n_distinct', 'n_vec', 'exact', 'old', 'new')]
        assert len(names) in (12, 32)
        assert tune_ref.same_floats([g[k] for k in names], [w[k] for k in names]), (g, w)


def run(ctx, world, home, truth, objective='hp_f1', start_cap=8100, holdout=None, want_moved=None, **kw):
    """tune.fit against the reference's descent; the objective never decreases; the final objective is the score of a fresh sweep
    of the fitted vector under the fitted cap.  -> (the fit's result, the reference's trace)"""
    world.truth_vcf = truth
    from_bams = kw.pop('from_bams', False)
    s_r = dict(svlen_thres=(world.s,), suppread_thres=(world.r,))
    got = tune.fit(home, truth, objective, ctx=ctx, holdout=holdout, from_bams=from_bams, **dict(s_r, **kw))
    axes = tune._axes(kw.get('axes'), kw.get('fit_cap', False))
    names = [a if a == 'pc_cap' else tune.NAMES[a] for a in axes]
    start = kw.get('start')
    vec0 = tune.vector({k: v for k, v in (start or {}).items() if k != 'pc_cap'})
    vec, cap, want = R.fit(world, objective, vec0, start_cap, names, kw.get('rounds', 8), kw.get('max_values', 0), hold=holdout is not None)
    assert len(got['fits']) == 1
    fit = got['fits'][0]
    same_trace([{k: v for k, v in r.items() if k not in tune.LEAD} for r in fit['trace']], want)
    assert fit['pc_cap'] == cap and np.array_equal(L.bits(fit['vector']), L.bits(vec))
    objs = [want[0]['objective_before']] + [r['objective_after'] for r in fit['trace']]
    assert not math.isnan(objs[-1]) and fit['objective'] == objs[-1]
    for a, b in zip(objs, objs[1:]):
        assert math.isnan(a) or b >= a, objs
    if want_moved is not None:
        assert any(r['axis'] == 'pc_cap' and r['old'] != r['new'] for r in want) == want_moved, [(r['axis'], r['old'], r['new']) for r in want]
    rows = tune.sweep_settings(home, truth, fit['vector'][None, :], ctx=ctx, holdout=holdout, from_bams=from_bams, pc_cap=[cap], **s_r)
    final = rows[0][objective if holdout is None else 'train_' + objective]
    assert final == fit['objective'], (final, fit['objective'])
    return got, want


def test_the_cap_moves_and_the_lowest_of_two_best_values_wins(ctx, case):
    w = case['world']
    got, want = run(ctx, w, case['home'], case['at_972'], axes=['pc_cap'], rounds=3, want_moved=True)
    first = want[0]
    assert first['exact'] == 1 and first['n_vec'] == len(w.full[0]) and first['old'] == 8100 and first['new'] != 8100
    assert first['objective_after'] > first['objective_before']
    # the best of the line is attained by more than one value, and the fit took the lowest of them
    w.truth_vcf = case['at_972']
    objs = {}
    for cap in w.full[0]:
        f = w.features(cap)
        t = w.truth(f)
        from tests import tune_score_ref
        objs[cap] = tune.scores(tune_score_ref.counts(f, tune.vector()[None, :], t)[0], t['n_base'])[tune.SCORES.index('hp_f1')]
    best = max(v for v in objs.values() if not math.isnan(v))
    winners = [cap for cap in w.full[0] if objs[cap] == best]
    assert len(winners) >= 2 and first['new'] == winners[0] and got['best']['pc_cap'] == winners[0]
    assert 'pc_cap' not in got['best']['setting']


def test_the_cap_does_not_move_from_the_best(ctx, case):
    got, want = run(ctx, case['world'], case['home'], case['at_8100'], axes=['pc_cap'], rounds=3, want_moved=False)
    assert len(want) == 1 and got['best']['pc_cap'] == 8100


def test_holdout(ctx, case):
    w = case['world']
    got, want = run(ctx, w, case['home'], case['at_972'], axes=['pc_cap', 'c1_max_ref_num'], rounds=2, holdout=w.held, want_moved=True)
    assert all(r['objective_after'] == r['train_hp_f1'] or math.isnan(r['objective_after']) for r in got['trace'])
    assert any(not math.isnan(r['test_hp_f1']) for r in want)


def test_the_cap_first_then_a_threshold_on_the_features_of_the_new_cap(ctx, case):
    got, want = run(ctx, case['world'], case['home'], case['at_972'], axes=['pc_cap', 'c1_hapread_ratio'], rounds=2, want_moved=True)
    assert [r['axis'] for r in want[:2]] == ['pc_cap', 'c1_hapread_ratio']
    # the threshold's line is that of the moved cap's features, not of 8100's
    w = case['world']
    assert want[1]['n_distinct'] == L.line(w.features(want[0]['new']), tune.NAMES.index('c1_hapread_ratio'), tune.vector())[1]


def test_fit_cap_appends_the_axis_and_a_listed_cap_is_the_start(ctx, case):
    w = case['world']
    # each listed cap alone, through every check of run(): the trace, the objective's course, the fresh sweep of the result
    for start in (15000, 300):
        got, want = run(ctx, w, case['home'], case['at_972'], start_cap=start, axes=['c1_max_ref_num'], fit_cap=True, rounds=2,
                        pc_cap=(start,), want_moved=True)
        assert [r['axis'] for r in want[:2]] == ['c1_max_ref_num', 'pc_cap']
        assert got['fits'][0]['setting']['pc_cap'] == start and all(r['pc_cap'] == start for r in got['trace'])   # the setting keeps the start
    # both in one call: a fit per start, in the order given
    both = tune.fit(case['home'], case['at_972'], 'hp_f1', axes=['c1_max_ref_num'], fit_cap=True, rounds=2, ctx=ctx, pc_cap=(15000, 300))
    assert [f['setting']['pc_cap'] for f in both['fits']] == [15000, 300]
    for f in both['fits']:
        vec, cap, want = R.fit(w, 'hp_f1', tune.vector(), f['setting']['pc_cap'], ['c1_max_ref_num', 'pc_cap'], 2)
        same_trace([{k: v for k, v in r.items() if k not in tune.LEAD} for r in f['trace']], want)
        assert f['pc_cap'] == cap
    assert both['fits'][0]['pc_cap'] != 15000


def test_max_values_3(ctx, case):
    got, want = run(ctx, case['world'], case['home'], case['at_972'], axes=['pc_cap'], rounds=2, max_values=3)
    assert want[0]['exact'] == 0 and want[0]['n_vec'] == 3
    # as many values as the line has, 0 being one of them (L = D = max_values): the whole line, and the trace says so
    D = case['world'].full[1]
    assert D == len(case['world'].full[0])
    got, want = run(ctx, case['world'], case['home'], case['at_972'], axes=['pc_cap'], rounds=1, max_values=D)
    assert want[0]['exact'] == 1 and want[0]['n_vec'] == D


def test_a_start_from_the_start_dict(ctx, case):
    got, want = run(ctx, case['world'], case['home'], case['at_972'], start={'c1_max_ref_num': 3, 'pc_cap': 15000}, start_cap=15000,
                    axes=['pc_cap'], rounds=2)
    assert want[0]['old'] == 15000


def test_a_line_value_that_divides_by_zero_scores_nan_and_the_fit_goes_on(ctx, tmp_path):
    home = pooled_workdir(str(tmp_path / 'w'), 3, div_zero=True)
    w = world_of(home, 50, 0)
    assert not R.div_zero(w.features(9000)) and R.div_zero(w.features(15000)) and w.full[0][-1] == 15000
    truth = w.write_truth(str(tmp_path / 't.vcf'), 972)
    got, want = run(ctx, w, home, truth, axes=['pc_cap', 'c1_max_ref_num'], rounds=2)
    assert want[0]['exact'] == 1 and want[0]['n_vec'] == len(w.full[0]) and got['best']['pc_cap'] < 15000
    # started there, the setting has no fit
    none = tune.fit(home, truth, 'hp_f1', axes=['pc_cap'], rounds=1, ctx=ctx, suppread_thres=(0,), pc_cap=[15000])
    assert none['best'] is None and none['fits'][0]['vector'] is None and math.isnan(none['trace'][0]['objective_after'])


def test_from_bams(ctx, tmp_path):
    home, copy = str(tmp_path / 'w'), str(tmp_path / 'copy')
    synth.write_svim_workdir(home, H.case_contigs('genome_small', 5), 5)
    shutil.copytree(home, copy)
    svim_mode.sv_phasing_from_bams(copy, 50, 2, 4, False, 0.9, 0, write_sv_calls=True)
    from duet_amd.native import NativeIngest
    from duet_amd.read_file import init_chrom_list
    ing, marks = NativeIngest.extract(home + '/snp_phasing/', init_chrom_list(False, home), 4, 50, 20, 1000)
    assert ing is not None, marks
    ing.close()
    soa, txt = tune._candidates(copy, 50, 2, False, 4)
    w = World(soa, txt, 50, 2, line=R.line(R.raw_participants(marks['read'], marks['read_tag'])))     # the raw marks' line
    assert len(w.full[0]) > 50
    target = R.pick(w.full[0], 4)[1]
    truth = w.write_truth(str(tmp_path / 't.vcf'), target)
    got, want = run(ctx, w, home, truth, axes=['pc_cap', 'c1_max_ref_num'], rounds=2, max_values=4, from_bams=True, want_moved=True)
    assert want[0]['exact'] == 0 and want[0]['n_vec'] == 4 and 'cluster_max_distance' in got['best']['setting']


def test_command_line_and_the_product_run(ctx, case, tmp_path, capsys, monkeypatch):
    best, trace = str(tmp_path / 'best.json'), str(tmp_path / 'fit.tsv')
    tune.main([case['home'], case['at_972'], '--fit', 'hp_f1', '--rounds', '2', '--axes', 'c1_max_ref_num', '--fit_cap',
               '--out_vector', best, '--trace', trace])
    line = capsys.readouterr().out.strip().splitlines()
    assert len(line) == 1 and line[0].startswith('fit hp_f1=') and 'fitted pc_cap=' in line[0]
    with open(best) as f:
        obj = json.load(f)
    assert list(obj) == list(tune.NAMES) + ['pc_cap'] and obj['pc_cap'] != 8100
    with open(trace) as f:
        cells = [ln.split('\t') for ln in f.read().splitlines()]
    assert cells[0] == ['svlen_thres', 'suppread_thres'] + list(tune.TRACE) + list(tune.SCORES)
    moved = [r for r in cells[1:] if r[3] == 'pc_cap'][0]
    assert moved[cells[0].index('old')] == '8100' and moved[cells[0].index('new')] == str(obj['pc_cap'])
    # duet --thresholds FILE applies the fitted cap: the rows of duet --pc_cap P --thresholds with the 14 keys
    from duet_amd import cli, stages
    home = str(tmp_path / 'run')
    shutil.copytree(case['home'], home)
    for name in ('snp_calling', 'sv_calling', 'snp_phasing'):
        monkeypatch.setattr(stages, name, lambda *a: None)
    monkeypatch.setattr(cli, 'check_envs', lambda *a: None)
    monkeypatch.setattr(cli, 'set_logging', lambda *a: None)
    only14 = str(tmp_path / 'v14.json')
    with open(only14, 'w') as f:
        json.dump({k: v for k, v in obj.items() if k != 'pc_cap'}, f)
    texts = []
    for extra in (['--thresholds', best], ['--pc_cap', str(obj['pc_cap']), '--thresholds', only14]):
        monkeypatch.setattr(sys, 'argv', ['duet', 'in.bam', 'ref.fa', home] + extra)
        cli.main(None)
        with open(home + '/phased_sv.vcf', 'rb') as f:
            texts.append(f.read())
    assert texts[0] == texts[1] and texts[0].count(b'\n') > 10
    assert texts[0].decode() == pc_cap_ref.phased_text(home, 50, 2, tune.load_vector(best), obj['pc_cap'])


def test_without_the_axis_the_fit_is_what_it_was(ctx, case):
    w = case['world']
    w.truth_vcf = case['at_972']
    got = tune.fit(case['home'], case['at_972'], 'hp_f1', rounds=2, ctx=ctx)
    feat = tune.features(case['home'], 50, 2, ctx=ctx)['feat']
    arrays = w.truth(feat)
    vec, want = L.fit(feat, arrays, arrays['n_base'], 'hp_f1', tune.vector(), rounds=2)
    from tests.test_gpu_tune_line import same_trace as plain_trace
    plain_trace(got['trace'], want)
    assert np.array_equal(L.bits(got['best']['vector']), L.bits(vec))
    assert 'pc_cap' not in got['best'] and 'pc_cap' not in got['best']['setting'] and all(r['axis'] != 'pc_cap' for r in got['trace'])
    assert all(list(r)[:2] == ['svlen_thres', 'suppread_thres'] and list(r)[2:2 + len(tune.TRACE)] == list(tune.TRACE) for r in got['trace'])
