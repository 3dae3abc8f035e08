# coding=utf-8
"""-m gpu: `tune --vote_sv_tags` (duet_amd/tune.py: sweep_settings(vote_sv_tags=True, sv_tag_min=.., sv_tag_pc=..)) against the
references (tests/tune_sv_tags_ref.py): per vector its own two-pass run, then the host truth match and the restated counts on the
second run's records.  The work directories are the golden callset case and the pooled one of tests/test_gpu_tune_join.py; the truth
set agrees with the default vector's second run.  tests/test_sv_tags_plan_host.py shows by the references alone that these rows
tell per-vector tags from reused ones."""
import json
import math
import os
import shutil

import numpy as np
import pytest

from duet_amd import _lib, tune
from tests import helpers as H
from tests import tune_ref, tune_strata_ref
from tests import tune_sv_tags_ref as T
from tests.test_gpu_fit_cap import pooled_workdir

pytestmark = pytest.mark.gpu

MINS = [0, 1, 2]


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def golden(tmp_path_factory):
    from tests.test_c_oracle import materialise_bams
    d = tmp_path_factory.mktemp('tune_sv_tags_golden')
    home = str(d / 'w')
    shutil.copytree(os.path.join(H.GOLDEN, 'cases', 'fuzz_cutesv_s2'), home)
    materialise_bams(home)
    w = T.world_of(home)
    w.held = list(dict.fromkeys(w.cands['chrom']))[:1]
    return dict(home=home, dir=d, world=w, truth=w.write_truth2(str(d / 'truth.vcf')))


@pytest.fixture(scope='module')
def pooled(tmp_path_factory):
    d = tmp_path_factory.mktemp('tune_sv_tags_pooled')
    home = pooled_workdir(str(d / 'w'), 3, lone=(0, 2))
    w = T.world_of(home)
    w.held = list(dict.fromkeys(w.cands['chrom']))[:1]
    return dict(home=home, dir=d, world=w, truth=w.write_truth2(str(d / 'truth.vcf')))


def want_row(w, cap, vec, m, q, holdout=False):
    """The ten scores (and train_ / test_ ones) and the marks of vector `vec` by the reference; None: its second run divides by
    zero."""
    feat, marks = w.second(cap, vec, m, q)
    rec = w.counts(feat, vec)
    if rec is None:
        return None
    t = w.truth(feat)
    out = dict(zip(tune.SCORES, tune.scores(rec, t['n_base'])))
    out.update(zip(tune.MARKS, marks))
    if holdout:
        h = w.hold(feat)
        sc = tune_strata_ref.counts(feat, vec.reshape(1, -1), h['truth'], h['cand_stratum'], 2)
        for s_i, part in enumerate(('train', 'test')):
            out.update(('%s_%s' % (part, n), x) for n, x in zip(tune.SCORES, tune.scores(sc[0, s_i], h['n_base'][s_i])))
    return out


def check_rows(rows, w, vecs, caps, mins, pcs, holdout=False):
    """rows of sweep_settings: caps outer, sv_tag_min, sv_tag_pc, the vectors innermost, each against the reference."""
    at = 0
    for cap in caps:
        for m in mins:
            for q in pcs:
                for k, v in enumerate(vecs):
                    row = rows[at]
                    at += 1
                    assert (row['sv_tag_min'], row['sv_tag_pc'], row.get('pc_cap')) == (m, q, cap)
                    want = want_row(w, 8100 if cap is None else cap, v, m, q, holdout)
                    names = sorted(n for n in want if n not in tune.MARKS)
                    assert tune_ref.same_floats([row[x] for x in names], [want[x] for x in names]), (cap, m, q, k, row, want)
                    assert tuple(row[x] for x in tune.MARKS) == tuple(want[x] for x in tune.MARKS), (cap, m, q, k)
    assert at == len(rows)


@pytest.mark.parametrize('which', ['golden', 'pooled'])
def test_sweep_rows(ctx, which, request):
    case = request.getfixturevalue(which)
    vecs = tune.expand_grid(T.GRID)
    plain = tune.sweep_settings(case['home'], case['truth'], vecs, ctx=ctx)
    rows = tune.sweep_settings(case['home'], case['truth'], vecs, ctx=ctx, vote_sv_tags=True, sv_tag_min=MINS)
    assert len(rows) == 3 * len(plain)
    assert list(rows[0])[:7] == ['svlen_thres', 'suppread_thres', 'sv_tag_min', 'sv_tag_pc'] + list(tune.MARKS)
    # 0: the rows of a run without the argument, in every shared column
    for a, b in zip(rows[:len(plain)], plain):
        assert set(a) - set(b) == set(tune.SV_TAG + tune.MARKS) and tune_ref.same_floats([a[k] for k in b], [b[k] for k in b])
        assert [a[k] for k in tune.MARKS] == [0, 0, 0]
    check_rows(rows, case['world'], vecs, [None], MINS, [0])
    # a voted run is another run, for every vector
    for k in range(len(vecs)):
        assert not tune_ref.same_floats([rows[k][n] for n in tune.SCORES], [rows[len(plain) + k][n] for n in tune.SCORES])
    # the default lists are the product's defaults
    dflt = tune.sweep_settings(case['home'], case['truth'], vecs[:2], ctx=ctx, vote_sv_tags=True)
    for a, b in zip(dflt, rows[len(plain):len(plain) + 2]):
        assert list(a) == list(b) and tune_ref.same_floats([a[k] for k in a], [b[k] for k in a])


def test_sweep_rows_under_caps_with_holdout_contigs_and_leaves(ctx, pooled):
    from tests.test_gpu_tune_leaf import want_rows as leaf_text
    case, w, vecs = pooled, pooled['world'], tune.expand_grid(T.GRID)
    caps = [972, 8100]
    leaf, contig, leaf_plain, contig_plain = [], [], [], []
    rows = tune.sweep_settings(case['home'], case['truth'], vecs, ctx=ctx, pc_cap=caps, holdout=w.held, by_leaf=leaf, by_contig=contig,
                               vote_sv_tags=True, sv_tag_min=MINS)
    check_rows(rows, w, vecs, caps, MINS, [0], holdout=True)
    plain = tune.sweep_settings(case['home'], case['truth'], vecs, ctx=ctx, pc_cap=caps, holdout=w.held, by_leaf=leaf_plain,
                                by_contig=contig_plain)
    zero = [r for r in rows if r['sv_tag_min'] == 0]
    assert len(zero) == len(plain)
    for a, b in zip(zero, plain):
        assert tune_ref.same_floats([a[k] for k in b], [b[k] for k in b])
    # the leaf rows: per setting `all` for every vector, then train / test, by the reference's census of each vector's own records
    want = []
    for cap in caps:
        for m in MINS:
            lead = tune._lead(None, 50, 2, cap, None, m, 0)
            per = []
            for k, v in enumerate(vecs):
                feat = w.second(cap, v, m)[0]
                per.append(leaf_text(lead, [k], feat, v.reshape(1, -1), w.truth(feat), w.cands, w.held))
            half = len(per[0]) // 3                              # (all: 18 rows; train / test: 36)
            want += [r for p in per for r in p[:half]] + [r for p in per for r in p[half:]]
    cols = tuple(tune._lead(None, 50, 2, 8100, None, 1, 0)) + tune.LEAF_COLS
    assert [[repr(r[c]) if isinstance(r[c], float) else str(r[c]) for c in cols] for r in leaf] == want
    zero = [r for r in leaf if r['sv_tag_min'] == 0]
    assert len(zero) == len(leaf_plain)
    for a, b in zip(zero, leaf_plain):
        assert [repr(a[k]) for k in b] == [repr(b[k]) for k in b]
    # the contig rows gain the two setting columns only; those of 0 are the plain ones; every row against the reference's strata
    # counts of the vector's own second-run records, at both caps
    assert set(contig[0]) - set(contig_plain[0]) == set(tune.SV_TAG)
    zero = [r for r in contig if r['sv_tag_min'] == 0]
    assert len(zero) == len(contig_plain)
    for a, b in zip(zero, contig_plain):
        assert [repr(a[k]) for k in b] == [repr(b[k]) for k in b]
    want = [r for cap in caps for m in MINS for k, v in enumerate(vecs) for r in want_contig_rows(w, cap, v, m, 0, k)]
    assert len(contig) == len(want) and len(set(r['contig'] for r in want)) >= 3
    for got, ref in zip(contig, want):
        assert list(got) == list(ref)
        for name in ref:
            if isinstance(ref[name], float):
                assert tune_ref.same_floats([got[name]], [ref[name]]), (name, got, ref)
            else:
                assert got[name] == ref[name] and type(got[name]) is type(ref[name]), (name, got, ref)
    # the reference's contig rows do tell the vectors and the settings apart
    sig = lambda m, k: [tuple(r[n] for n in ('contig',) + tune.COUNTS) for r in want if (r['pc_cap'], r['sv_tag_min'], r['vector']) == (8100, m, k)]
    assert sig(1, 0) != sig(0, 0) and sig(1, 0) != sig(1, 2)


def want_contig_rows(w, cap, vec, m, q, k):
    """The --by_contig rows of vector `vec` (label k) by the reference: the strata counts of its own second-run records."""
    feat = w.second(cap, vec, m, q)[0]
    st = tune.strata_by_contig()
    cs = np.array([tune.stratum_of(st, t) for t in w.cands['chrom']], dtype=np.uint8)
    counts = tune_strata_ref.counts(feat, vec.reshape(1, -1), w.truth(feat), cs, len(st['names']))[0]
    n_base = tune.truth_side(w.truth_vcf, strata=st)['n_base_strata']
    lead = tune._lead(None, w.s, w.r, cap, None, m, q)
    out = []
    for s_i, name in enumerate(st['names']):
        if int(counts[s_i]['n_calls']) or n_base[s_i]:
            row = dict(lead, vector=k, contig=name, n_base=n_base[s_i])
            row.update((n, int(counts[s_i][n])) for n in tune.COUNTS)
            row.update(zip(tune.SCORES, tune.scores(counts[s_i], n_base[s_i])))
            out.append(row)
    return out


def test_a_vector_the_plan_cannot_serve_has_nan_rows_alone(ctx, golden, monkeypatch):
    """The per-vector nan path: the apply of vector 1 at sv_tag_min 1 is handed calls of 4 (above 3), so its fourth counter is not
    0 -- that vector's rows, contig rows and leaf rows are nan at that setting, every other row is what it is without the fault."""
    import torch
    case, vecs = golden, tune.expand_grid(T.GRID[:3])
    kw = dict(ctx=ctx, vote_sv_tags=True, sv_tag_min=[1, 2], holdout=case['world'].held)
    leaf0, contig0 = [], []
    good = tune.sweep_settings(case['home'], case['truth'], vecs, by_leaf=leaf0, by_contig=contig0, **kw)
    C = len(case['world'].cands['pos'])
    fours = torch.full((C,), 4, dtype=torch.uint8, device='cuda:0')
    real, calls = ctx.sv_tags_apply_device, []

    def apply(pred_ptr, out_ptr, counts_ptr, **settings):
        calls.append(settings['min_votes'])
        return real(fours.data_ptr() if len(calls) == 2 else pred_ptr, out_ptr, counts_ptr, **settings)
    monkeypatch.setattr(ctx, 'sv_tags_apply_device', apply)
    leaf1, contig1 = [], []
    rows = tune.sweep_settings(case['home'], case['truth'], vecs, by_leaf=leaf1, by_contig=contig1, **kw)
    assert calls == [1, 1, 1, 2, 2, 2]
    hit = lambda r: (r['sv_tag_min'], r.get('vector', None)) == (1, 1)
    for k, (a, b) in enumerate(zip(rows, good)):
        if k == 1:
            assert all(math.isnan(a[n]) for n in tune.SCORES + tune.MARKS) and all(math.isnan(a['test_' + n]) for n in tune.SCORES)
            assert not math.isnan(b['call_precision']) and a['sv_tag_min'] == 1
        else:
            assert list(a) == list(b) and tune_ref.same_floats([a[n] for n in a], [b[n] for n in a]), k
    assert len(leaf1) == len(leaf0)
    for a, b in zip(leaf1, leaf0):
        if hit(a):
            assert all(math.isnan(a[n]) for n in tune.LEAF_COUNTS + tune.LEAF_RATES)
        else:
            assert [repr(a[n]) for n in a] == [repr(b[n]) for n in a]
    assert any(hit(r) for r in leaf1) and any(hit(r) for r in contig1)
    for r in contig1:
        if hit(r):
            assert all(math.isnan(r[n]) for n in tune.SCORES) and r['n_calls'] == 0
    rest = lambda rs: [[repr(r[n]) for n in r] for r in rs if not hit(r)]
    assert rest(contig1) == rest(contig0)


def test_a_derived_tag_above_the_cap_does_not_vote(ctx, pooled):
    case, w, vecs = pooled, pooled['world'], tune.expand_grid(T.GRID)
    rows = tune.sweep_settings(case['home'], case['truth'], vecs, ctx=ctx, pc_cap=[8100], vote_sv_tags=True, sv_tag_min=[1],
                               sv_tag_pc=[0, 9000])
    check_rows(rows, w, vecs, [8100], [1], [0, 9000])
    K = len(vecs)
    for k, v in enumerate(vecs):
        a, b = want_row(w, 8100, v, 1, 0), want_row(w, 8100, v, 1, 9000)
        assert not tune_ref.same_floats([a[n] for n in tune.SCORES], [b[n] for n in tune.SCORES])     # by the reference
        assert [rows[K + k][n] for n in tune.MARKS] == [rows[k][n] for n in tune.MARKS]               # the marks are given all the same


def test_a_first_run_that_divides_by_zero_gives_nan_rows_for_the_setting(ctx, tmp_path):
    """No input gives a second run that divides by zero for one vector only (a contig gains a seed in the
    second run only through het calls it already had, and `kept` does not read the tags): the whole-setting case instead -- under
    cap 15000, with -r 0, the last contig has a seed and a kept candidate without reads."""
    home = pooled_workdir(str(tmp_path / 'w'), 3, div_zero=True)
    w = T.world_of(home, 50, 0)
    truth = w.write_truth2(str(tmp_path / 'truth.vcf'))
    assert T.R.div_zero(w.features(15000)) and not T.R.div_zero(w.features(8100))
    vecs = tune.expand_grid(T.GRID[:2])
    for v in vecs:
        assert not T.R.div_zero(w.second(8100, v, 1)[0])
    rows = tune.sweep_settings(home, truth, vecs, ctx=ctx, suppread_thres=(0,), pc_cap=[8100, 15000], vote_sv_tags=True, sv_tag_min=[0, 1])
    check_rows(rows[:4], w, vecs, [8100], [0, 1], [0])
    for r in rows[4:]:
        assert r['pc_cap'] == 15000 and all(math.isnan(r[n]) for n in tune.SCORES + tune.MARKS)


def test_the_command_and_its_files(ctx, golden):
    d = golden['dir']
    grid, one = str(d / 'grid.json'), str(d / 'one.json')
    with open(grid, 'w') as f:
        json.dump(T.GRID[:2], f)
    with open(one, 'w') as f:
        json.dump(T.GRID[2:3], f)
    out = lambda n: str(d / n)
    tune.main([golden['home'], golden['truth'], '--grid', grid, '--out', out('plain.tsv')])
    tune.main([golden['home'], golden['truth'], '--grid', grid, '--out', out('voted.tsv'), '--vote_sv_tags', '--sv_tag_min', '0,1'])
    read = lambda n: [l.rstrip('\n').split('\t') for l in open(out(n))]
    plain, voted = read('plain.tsv'), read('voted.tsv')
    assert voted[0] == list(tune.SV_TAG + tune.MARKS) + plain[0]
    assert [r[5:] for r in voted[1:len(plain)]] == plain[1:] and all(r[:5] == ['0', '0', '0', '0', '0'] for r in voted[1:len(plain)])
    assert all(r[:2] == ['1', '0'] for r in voted[len(plain):]) and len(voted) == 2 * len(plain) - 1
    assert voted[len(plain)][2:5] == ['747', '86', '30']
    # --features with one vector: the second run's records of that vector
    tune.main([golden['home'], golden['truth'], '--grid', one, '--out', out('one.tsv'), '--vote_sv_tags', '--features', out('feat.tsv')])
    rows = read('feat.s50.r2.v1.q0.tsv')
    w, v = golden['world'], tune.expand_grid(T.GRID[2:3])[0]
    want = w.second(8100, v, 1)[0]
    col = {n: i for i, n in enumerate(rows[0])}
    for name in ('eligible', 'cls', 'hap1', 'hap2', 'hap0', 'allhap', 't1', 't2'):
        assert [int(r[col[name]]) for r in rows[1:]] == [int(x) for x in want[name]], name
    assert [int(r[col['hap1']]) for r in rows[1:]] != [int(x) for x in w.features(8100)['hap1']]


def test_from_bams(ctx, tmp_path_factory):
    """The synthetic svim-gpu directory, --from_bams: the second-run feature records of two vectors against the reference on the
    problem its clustered candidates adapt to, names and all (read back from a copy's sv_calling/variants.vcf by the native ingest:
    the independent route of DESIGN.md section 25); the rows of both against the reference; the rows of sv_tag_min 0 are those of a
    run without the flag."""
    from tests.test_gpu_ps_join import SvimCase
    c = SvimCase(tmp_path_factory.mktemp('tune_sv_tags_svim'))
    w = T.world_of(str(c.root / 'copy'))
    truth = w.write_truth2(str(c.root / 'truth.vcf'))
    vecs = tune.expand_grid(T.GRID[:3:2])                   # (the default vector and VEC_A)
    t0, t1 = (w.tags(8100, v)[0] for v in vecs)
    assert t0 != t1                                         # the condition: the two vectors' tags differ
    kw = dict(from_bams=True, ctx=ctx, pc_cap=[8100])
    for k, v in enumerate(vecs):
        feats = {}
        rows = tune.sweep_settings(c.home, truth, vecs[k:k + 1], vote_sv_tags=True, sv_tag_min=[0, 1],
                                   on_features=lambda lead, got: feats.__setitem__(lead['sv_tag_min'], got['feat'].copy()), **kw)
        assert all(r['cluster_max_distance'] == 0.9 for r in rows)
        check_rows(rows, w, vecs[k:k + 1], [8100], [0, 1], [0])
        for m in (0, 1):
            ref = w.second(8100, v, m)[0]
            assert len(feats[m]) == len(ref)
            for name in ('eligible', 'cls', 'hap1', 'hap2', 'hap0', 'allhap', 't1', 't2'):
                assert np.array_equal(feats[m][name], ref[name]), (k, m, name)
            el = ref['eligible'] != 0
            assert np.array_equal(feats[m]['ps'][el], ref['ps'][el])
        assert feats[0].tobytes() != feats[1].tobytes()
    both = tune.sweep_settings(c.home, truth, vecs, vote_sv_tags=True, sv_tag_min=[0, 1], **kw)
    plain = tune.sweep_settings(c.home, truth, vecs, **kw)
    check_rows(both, w, vecs, [8100], [0, 1], [0])
    for a, b in zip(both[:len(plain)], plain):
        assert tune_ref.same_floats([a[n] for n in b], [b[n] for n in b])
