# coding=utf-8
"""-m gpu: `tune --join_ps` (duet_amd/tune.py: sweep_settings(join_min_sv=..), fit(join_min_sv=..)) against the reference: the
ingested SoA remapped by tests/ps_links_ref.py -> duet_amd/ps_links.py: blocks -> tests/ps_join_ref.py, then the reference's
features, the host truth match and the restated counts on that SoA, as the tests of the sweep and of the cap axis do.  The work
directories are the golden callset case of tests/test_gpu_ps_join.py and the pooled one of tests/test_gpu_fit_cap.py (its cap line
has at most nine values)."""
import json
import os
import shutil
import sys

import numpy as np
import pytest

from duet_amd import _lib, ps_join, ps_links, tune
from tests import cap_line_ref as R
from tests import helpers as H
from tests import pc_cap_ref, tune_leaf_ref, tune_ref, tune_score_ref, tune_strata_ref
from tests import ps_join_ref as J
from tests import ps_links_ref as L
from tests.test_gpu_fit_cap import World, pooled_workdir, same_trace

pytestmark = pytest.mark.gpu

GRID = [{}, {'c1_max_ref_num': 3, 'c0_min_sv_num': 2}, {'c1_hapread_ratio': 0.4}]


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


class JoinedWorld(World):
    """World whose features under a cap are those of the SoA remapped over the blocks of the links under that cap."""

    def __init__(self, soa, txt, s, r, min_sv):
        World.__init__(self, soa, txt, s, r)
        self.min_sv = min_sv

    def remapped(self, cap):
        if not self.min_sv:
            return self.soa
        rows, _ = ps_links.blocks(L.links(self.soa, self.s, self.r, cap), self.min_sv)
        return J.remapped_soa(self.soa, rows)

    def features(self, cap):
        if cap not in self.memo:
            self.memo[cap] = R.records(pc_cap_ref.features(self.remapped(cap), self.s, self.r, cap))
        return self.memo[cap]


def worlds(home, truth=None, held=None):
    soa, txt = tune._candidates(home, 50, 2, False, 4)
    out = {}
    for n in (0, 1, 2):
        out[n] = w = JoinedWorld(soa, txt, 50, 2, n)
        w.truth_vcf, w.held = truth, held
    return out


def write_truth(w, path, cap=8100):
    return w.write_truth(path, cap)


@pytest.fixture(scope='module')
def golden(tmp_path_factory):
    from tests.test_c_oracle import materialise_bams
    d = tmp_path_factory.mktemp('tune_join_golden')
    home = str(d / 'w')
    shutil.copytree(os.path.join(H.GOLDEN, 'cases', 'fuzz_cutesv_s2'), home)
    materialise_bams(home)
    ws = worlds(home)
    # the truth set agrees with the joined run: a wrong or missing join costs calls and phasing
    truth = write_truth(ws[2], str(d / 'truth.vcf'))
    held = list(dict.fromkeys(ws[0].cands['chrom']))[:1]
    for w in ws.values():
        w.truth_vcf, w.held = truth, held
    return dict(home=home, dir=d, truth=truth, worlds=ws, held=held)


@pytest.fixture(scope='module')
def pooled(tmp_path_factory):
    d = tmp_path_factory.mktemp('tune_join_pooled')
    home = pooled_workdir(str(d / 'w'), 3, lone=(0, 2))
    ws = worlds(home)
    truth = write_truth(ws[2], str(d / 'truth.vcf'), 972)
    held = list(dict.fromkeys(ws[0].cands['chrom']))[:1]
    for w in ws.values():
        w.truth_vcf, w.held = truth, held
    return dict(home=home, dir=d, truth=truth, worlds=ws, held=held)


def want_scores(w, cap, vecs, holdout=False):
    """Per vector: the ten scores (and train_ / test_ ones) of the reference under `cap`."""
    feat = w.features(cap)
    if R.div_zero(feat):
        return None
    t = w.truth(feat)
    pc = tune_score_ref.counts(feat, vecs, t)
    out = [dict(zip(tune.SCORES, tune.scores(pc[k], t['n_base']))) for k in range(len(vecs))]
    if holdout:
        h = w.hold(feat)
        sc = tune_strata_ref.counts(feat, vecs, h['truth'], h['cand_stratum'], 2)
        for k in range(len(vecs)):
            for s_i, part in enumerate(('train', 'test')):
                out[k].update(('%s_%s' % (part, n), x) for n, x in zip(tune.SCORES, tune.scores(sc[k, s_i], h['n_base'][s_i])))
    return out


def check_rows(rows, case, vecs, caps, joins, holdout=False):
    """rows of sweep_settings: caps outer, join_min_sv inner, vectors innermost, each against the reference."""
    at = 0
    for cap in caps:
        for n in joins:
            want = want_scores(case['worlds'][n], 8100 if cap is None else cap, vecs, holdout)
            for k in range(len(vecs)):
                row = rows[at]
                at += 1
                assert row['join_min_sv'] == n and row.get('pc_cap') == cap
                names = sorted(want[k])
                assert tune_ref.same_floats([row[x] for x in names], [want[k][x] for x in names]), (cap, n, k, row, want[k])
    assert at == len(rows)


@pytest.mark.parametrize('which', ['golden', 'pooled'])
def test_the_condition_holds_by_the_reference_alone(which, request):
    """A candidate's feature record differs between join_min_sv 0 and 2, and so does a count: the tests below can tell a joined run
    from a plain one."""
    case = request.getfixturevalue(which)
    vecs = tune.expand_grid(GRID)
    f0, f2 = case['worlds'][0].features(8100), case['worlds'][2].features(8100)
    assert f0.tobytes() != f2.tobytes() and len(f0) == len(f2)
    t0, t2 = case['worlds'][0].truth(f0), case['worlds'][2].truth(f2)
    assert tune_score_ref.counts(f0, vecs, t0).tobytes() != tune_score_ref.counts(f2, vecs, t2).tobytes()


@pytest.mark.parametrize('which', ['golden', 'pooled'])
def test_sweep_rows(ctx, which, request):
    case = request.getfixturevalue(which)
    vecs = tune.expand_grid(GRID)
    plain = tune.sweep_settings(case['home'], case['truth'], vecs, ctx=ctx)
    rows = tune.sweep_settings(case['home'], case['truth'], vecs, ctx=ctx, join_min_sv=[0, 1, 2])
    assert len(rows) == 3 * len(plain) and list(rows[0])[:3] == ['svlen_thres', 'suppread_thres', 'join_min_sv']
    # 0: the rows of a run without the argument
    for a, b in zip(rows[:len(plain)], plain):
        assert {k: v for k, v in a.items() if k != 'join_min_sv'}.keys() == b.keys()
        assert tune_ref.same_floats([a[k] for k in b], [b[k] for k in b])
    check_rows(rows, case, vecs, [None], [0, 1, 2])
    assert not tune_ref.same_floats([r['hp_f1'] for r in rows[:len(plain)]], [r['hp_f1'] for r in rows[2 * len(plain):]])


def test_sweep_rows_under_caps_with_holdout_and_leaves(ctx, pooled):
    case, vecs = pooled, tune.expand_grid(GRID)
    leaf, leaf_plain = [], []
    rows = tune.sweep_settings(case['home'], case['truth'], vecs, ctx=ctx, pc_cap=[2400, 8100], holdout=case['held'], by_leaf=leaf,
                               join_min_sv=[0, 2, 1])
    check_rows(rows, case, vecs, [2400, 8100], [0, 2, 1], holdout=True)
    plain = tune.sweep_settings(case['home'], case['truth'], vecs, ctx=ctx, pc_cap=[2400, 8100], holdout=case['held'], by_leaf=leaf_plain)
    # the leaf rows: per setting `all`, then train / test, against the reference's census of the remapped SoA
    from tests.test_gpu_tune_leaf import want_rows as leaf_text
    want = []
    for cap in (2400, 8100):
        for n in (0, 2, 1):
            w = case['worlds'][n]
            feat = w.features(cap)
            want += leaf_text(tune._lead(None, 50, 2, cap, n), range(len(vecs)), feat, vecs, w.truth(feat), w.cands, case['held'])
    cols = tuple(tune._lead(None, 50, 2, 8100, 0)) + tune.LEAF_COLS
    assert [[repr(r[c]) if isinstance(r[c], float) else str(r[c]) for c in cols] for r in leaf] == want
    zero = [r for r in leaf if r['join_min_sv'] == 0]
    assert len(zero) == len(leaf_plain)
    for a, b in zip(zero, leaf_plain):
        assert [repr(a[k]) for k in b] == [repr(b[k]) for k in b]
    for a, b in zip([r for r in rows if r['join_min_sv'] == 0], plain):
        assert tune_ref.same_floats([a[k] for k in b], [b[k] for k in b])


def test_features_of_the_joined_setting(ctx, golden):
    """on_features hands over the joined run's records: the PS column holds block names."""
    got = {}
    tune.sweep_settings(golden['home'], golden['truth'], tune.expand_grid(GRID), ctx=ctx, join_min_sv=[0, 2],
                        on_features=lambda lead, cands: got.__setitem__(lead['join_min_sv'], cands['feat'].copy()))
    for n in (0, 2):
        want = golden['worlds'][n].features(8100)
        for name in ('eligible', 'cls', 'hap1', 'hap2', 'hap0', 'allhap', 't1', 't2'):
            assert np.array_equal(got[n][name], want[name]), (n, name)
        el = want['eligible'] != 0
        assert np.array_equal(got[n]['ps'][el], want['ps'][el])


def test_the_cap_line_is_the_same_with_and_without_a_join(pooled):
    """The remap keeps pc bit for bit and leaves untagged words alone: the participants' pc values do not move."""
    w0, w2 = pooled['worlds'][0], pooled['worlds'][2]
    assert R.line(R.participants(w2.remapped(8100), 50, 2)) == w0.full
    assert R.line(R.participants(w2.remapped(972), 50, 2)) == w0.full


def test_fit_with_the_cap_axis(ctx, pooled, monkeypatch):
    """--fit hp_f1 --fit_cap --max_values 8 --join_ps --join_min_sv 1,2: per setting the trace equals the reference's descent, whose
    every cap value remaps under that value; the vector file carries join_min_sv, and duet --thresholds --join_ps joins with it."""
    case = pooled
    d = case['dir']
    got = tune.fit(case['home'], case['truth'], 'hp_f1', axes=['c1_max_ref_num'], fit_cap=True, rounds=2, max_values=8, ctx=ctx,
                   join_min_sv=[1, 2])
    assert [f['setting']['join_min_sv'] for f in got['fits']] == [1, 2]
    tables = lambda m, cap: ps_links.blocks(L.links(case['worlds'][0].soa, 50, 2, cap), m)[0]
    for f in got['fits']:
        w = case['worlds'][f['setting']['join_min_sv']]
        # the condition, by the reference alone: the blocks differ between values of the cap line, so a build that remapped under
        # one fixed cap would not give this trace
        assert len(set(tuple(tables(w.min_sv, int(cap))) for cap in R.pick(w.full[0], 8))) >= 3
        vec, cap, want = R.fit(w, 'hp_f1', tune.vector(), 8100, ['c1_max_ref_num', 'pc_cap'], 2, 8)
        same_trace([{k: v for k, v in r.items() if k not in tune.LEAD} for r in f['trace']], want)
        assert f['pc_cap'] == cap and any(r['axis'] == 'pc_cap' for r in want)
    best = got['fits'][0]
    for f in got['fits'][1:]:
        if f['objective'] > best['objective']:
            best = f
    assert got['best'] is best
    # the command: the same fit, the file, and the product run that reads it
    out_vec, trace = str(d / 'best.json'), str(d / 'fit.tsv')
    tune.main([case['home'], case['truth'], '--fit', 'hp_f1', '--axes', 'c1_max_ref_num', '--fit_cap', '--rounds', '2', '--max_values', '8',
               '--join_ps', '--join_min_sv', '1,2', '--out_vector', out_vec, '--trace', trace])
    with open(out_vec) as f:
        obj = json.load(f)
    n = best['setting']['join_min_sv']
    assert obj['join_min_sv'] == n and obj['pc_cap'] == best['pc_cap']
    with open(trace) as f:
        head = f.readline().rstrip('\n').split('\t')
    assert 'join_min_sv' in head
    assert tune.load_vector(out_vec, with_cap=True, with_join=True)[1:] == (best['pc_cap'], n)
    from duet_amd import cli
    from tests.test_gpu_ps_join import read, stub_stages
    stub_stages(monkeypatch)
    files = {}
    for name, extra in (('file', []), ('flag', ['--join_min_sv', str(n)]), ('other', ['--join_min_sv', str(3 - n)])):
        monkeypatch.setattr(sys, 'argv', ['duet', 'in.bam', 'ref.fa', case['home'], '--thresholds', out_vec, '--join_ps'] + extra)
        cli.main(None)
        files[name] = read(ps_join.path_vcf(case['home'])), read(ps_join.path_blocks(case['home']))
    assert files['file'] == files['flag']
    # the blocks of the other N differ on this input (by the reference): the file's value was the one used
    assert tables(n, best['pc_cap']) != tables(3 - n, best['pc_cap']) and files['file'][1] != files['other'][1]


def test_without_the_flag_the_files_are_what_they_were(ctx, golden):
    d = golden['dir']
    grid = str(d / 'grid.json')
    with open(grid, 'w') as f:
        json.dump(GRID, f)
    out = lambda n: str(d / n)
    tune.main([golden['home'], golden['truth'], '--grid', grid, '--out', out('plain.tsv')])
    tune.main([golden['home'], golden['truth'], '--grid', grid, '--out', out('join.tsv'), '--join_ps', '--join_min_sv', '0,2',
               '--features', out('feat.tsv')])
    with open(out('plain.tsv')) as f:
        plain = [l.rstrip('\n').split('\t') for l in f]
    with open(out('join.tsv')) as f:
        join = [l.rstrip('\n').split('\t') for l in f]
    assert join[0] == ['join_min_sv'] + plain[0]
    assert [r[1:] for r in join[1:len(plain)]] == plain[1:] and all(r[0] == '0' for r in join[1:len(plain)])
    assert all(r[0] == '2' for r in join[len(plain):]) and len(join) == 2 * len(plain) - 1
    assert os.path.exists(out('feat.s50.r2.j0.tsv')) and os.path.exists(out('feat.s50.r2.j2.tsv'))



def test_from_bams(ctx, tmp_path_factory):
    """The synthetic svim-gpu directory, --from_bams, under --pc_cap 2400,8100 with --holdout and --by_leaf: the rows and leaf rows
    of join_min_sv 0, 1, 2 against the reference on the SoA its clustered candidates adapt to (read back from a copy's
    sv_calling/variants.vcf, as tests/test_gpu_fit_cap.py does), remapped under N and the cap; the rows of 0 are those of a run
    without the argument; on_features hands over the joined run's records."""
    from tests.test_gpu_ps_join import SvimCase
    from tests.test_gpu_tune_leaf import want_rows as leaf_text
    c = SvimCase(tmp_path_factory.mktemp('tune_join_svim'))
    vecs = tune.expand_grid(GRID[:1])                       # (one vector: the reference walks every candidate per vector and setting)
    txt = tune._candidates(str(c.root / 'copy'), 50, 2, False, 4)[1]
    ws = {n: JoinedWorld(c.soa, txt, 50, 2, n) for n in (0, 1, 2)}
    truth = ws[2].write_truth(str(c.root / 'truth.vcf'), 8100)
    held = list(dict.fromkeys(ws[0].cands['chrom']))[:1]
    for w in ws.values():
        w.truth_vcf, w.held = truth, held
    case = dict(worlds=ws)
    # the condition, by the reference alone
    f0, f2 = ws[0].features(8100), ws[2].features(8100)
    assert f0.tobytes() != f2.tobytes()
    assert tune_score_ref.counts(f0, vecs, ws[0].truth(f0)).tobytes() != tune_score_ref.counts(f2, vecs, ws[2].truth(f2)).tobytes()
    feats, leaf, leaf_plain = {}, [], []
    kw = dict(from_bams=True, ctx=ctx, pc_cap=[2400, 8100], holdout=held)
    rows = tune.sweep_settings(c.home, truth, vecs, join_min_sv=[0, 1, 2], by_leaf=leaf,
                               on_features=lambda lead, got: feats.__setitem__((lead['pc_cap'], lead['join_min_sv']), got['feat'].copy()), **kw)
    assert all(r['cluster_max_distance'] == 0.9 for r in rows)
    check_rows(rows, case, vecs, [2400, 8100], [0, 1, 2], holdout=True)
    want = []
    for cap in (2400, 8100):
        for n in (0, 1, 2):
            feat = ws[n].features(cap)
            want += leaf_text(tune._lead(0.9, 50, 2, cap, n), range(len(vecs)), feat, vecs, ws[n].truth(feat), ws[n].cands, held)
    cols = tuple(tune._lead(0.9, 50, 2, 8100, 0)) + tune.LEAF_COLS
    assert [[repr(r[x]) if isinstance(r[x], float) else str(r[x]) for x in cols] for r in leaf] == want
    plain = tune.sweep_settings(c.home, truth, vecs, by_leaf=leaf_plain, **kw)
    for a, b in zip([r for r in rows if r['join_min_sv'] == 0], plain):
        assert tune_ref.same_floats([a[k] for k in b], [b[k] for k in b])
    zero = [r for r in leaf if r['join_min_sv'] == 0]
    assert len(zero) == len(leaf_plain) and all([repr(a[k]) for k in b] == [repr(b[k]) for k in b] for a, b in zip(zero, leaf_plain))
    for (cap, n), got in feats.items():
        ref = ws[n].features(cap)
        assert len(got) == len(ref)
        for name in ('eligible', 'cls', 'hap1', 'hap2', 'hap0', 'allhap', 't1', 't2'):
            assert np.array_equal(got[name], ref[name]), (cap, n, name)
        el = ref['eligible'] != 0
        assert np.array_equal(got['ps'][el], ref['ps'][el])
    j0, j2 = [r['hp_f1'] for r in rows if r['join_min_sv'] == 0], [r['hp_f1'] for r in rows if r['join_min_sv'] == 2]
    assert not tune_ref.same_floats(j0, j2)
