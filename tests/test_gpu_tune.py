# coding=utf-8
"""-m gpu: the threshold sweep (duet_amd/tune.py, duet_amd/csrc/duet_tune.hip) against the oracle, the E/F kernels and the
evaluator: features bit-exact, the default vector reproducing production, random vectors against the restated tree, the ten
numbers against evaluation.evaluation, and `duet --thresholds`."""
import json
import math
import os
import shutil

import numpy as np
import pytest

from duet_amd import _lib, engine, evaluation, synth, tune
from duet_amd.sv_phasing import sv_phasing
from tests import helpers as H
from tests import soa_fuzz
from tests import tune_ref
from tests.test_c_oracle import materialise_bams

pytestmark = pytest.mark.gpu

FIELDS = ('kept', 'eligible', 'cls', 'hap1', 'hap2', 'hap0', 'allhap', 't1', 't2', 'ps', 'deg', 'svread', 'refread')


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def check_features(ctx, soa, s=50, r=2):
    feat = ctx.features_host(soa, s, r)
    want = tune_ref.oracle_features(soa, s, r)
    for name in FIELDS:
        got = feat[name].astype(np.int64)
        exp = np.array([w[name] for w in want], dtype=np.int64)
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, '%s differs at %s: %s vs %s' % (name, bad[:5], got[bad[:5]], exp[bad[:5]])
    return feat


def check_defaults_equal_production(ctx, soa, feat, s=50, r=2):
    pred, ps = ctx.run_host(soa, s, r)
    _, tp, tps = ctx.sweep_host(feat, tune.vector()[None, :], want_pred=True, want_ps=True)
    assert np.array_equal(tp[0], pred) and np.array_equal(tps, ps)


EDGE_SOAS = [
    ('fuzz%d' % s, dict(seed=s, n_contigs=1 + s % 5, sorted_pos=bool(s % 3))) for s in range(6)] + [
    ('many_ps', dict(seed=41, n_contigs=2, n_ps=(3, 130), cands_per_contig=(300, 600))),
    ('deg9000', dict(seed=42, n_contigs=2, big_deg=9000, cands_per_contig=(60, 120), n_ps=(2, 9))),
    ('k65', dict(seed=43, n_contigs=65, cands_per_contig=(0, 40))),
    ('k64', dict(seed=44, n_contigs=64, cands_per_contig=(0, 40))),
    ('k3000', dict(seed=45, n_contigs=3000, cands_per_contig=(0, 6), reads_per_contig=(5, 30))),
    ('seedless', dict(seed=46, n_contigs=6, empty_contig_rate=2, no_seed_contig_rate=2)),
]


@pytest.mark.parametrize('name,kw', EDGE_SOAS, ids=[e[0] for e in EDGE_SOAS])
def test_features_and_defaults_on_soas(ctx, name, kw):
    soa = soa_fuzz.random_soa(kw.pop('seed'), **kw)
    for s, r in ((50, 2), (0, 0)):
        feat = check_features(ctx, soa, s, r)
        check_defaults_equal_production(ctx, soa, feat, s, r)


def test_undivisible_candidate_reports_div_zero(ctx):
    soa = soa_fuzz.random_soa(47, n_contigs=2, allow_divzero=True)
    with pytest.raises(ZeroDivisionError):
        ctx.run_host(soa, 0, 0)
    with pytest.raises(ZeroDivisionError):
        ctx.features_host(soa, 0, 0)


@pytest.mark.parametrize('name,src,params', H.full_cases(), ids=[c[0] for c in H.full_cases()])
def test_features_on_golden_work_directories(ctx, name, src, params, tmp_path):
    from oracle import ef_oracle as O
    home = str(tmp_path / name)
    shutil.copytree(src, home)
    materialise_bams(home)
    s, r = params['svlen_thres'], params['suppread_thres']
    cands = tune.features(home, s, r, ctx=ctx)
    _, trace, _ = O.sv_phasing_text(home, s, r, want_trace=True)
    feat = cands['feat']
    assert len(feat) == len(trace)
    for f, (kept, cls, pred, ps) in zip(feat, trace):
        assert bool(f['kept']) == bool(kept)
        if kept:
            assert int(f['cls']) == cls
        assert bool(f['eligible']) == (pred is not None)
        if pred is not None:
            assert int(f['ps']) == ps
    check_defaults_equal_production(ctx, cands['soa'], feat, s, r)
    assert tune_ref.phased_text(home, s, r, tune.vector()) == O.sv_phasing_text(home, s, r)


def test_defaults_equal_production_on_a_million_marks(ctx):
    soa = engine.soa_from_synth(synth.bench_genome(1000000, 2))
    feat = ctx.features_host(soa, 50, 2)
    check_defaults_equal_production(ctx, soa, feat)


def random_vectors(feat, n, seed):
    """Vectors near the defaults, with nan / +-inf and thresholds set exactly to candidates' own sv_ratio, a1 - a2 and
    totsc_ratio values."""
    rng = np.random.default_rng(seed)
    e = feat[feat['eligible'] != 0]
    sv = e['svread'] / (e['svread'].astype(np.float64) + e['refread'])
    a1 = np.where(e['hap1'] > 0, e['t1'] / np.maximum(e['hap1'], 1), 0.0)
    a2 = np.where(e['hap2'] > 0, e['t2'] / np.maximum(e['hap2'], 1), 0.0)
    lo, hi = np.minimum(e['t1'], e['t2']), np.maximum(e['t1'], e['t2'])
    tot = np.where(lo > 0, hi / np.maximum(lo, 1), 0.0)
    hr = e['allhap'] / e['deg'].astype(np.float64)
    pools = {1: sv, 5: sv, 6: sv, 9: sv, 10: sv, 12: sv, 2: np.abs(a2 - a1), 8: np.abs(a2 - a1), 13: tot, 7: hr}
    base = tune.vector()
    out = []
    for i in range(n):
        v = base.copy()
        for j in range(14):
            u = rng.random()
            if u < 0.05:
                v[j] = (math.nan, math.inf, -math.inf)[rng.integers(3)]
            elif u < 0.45 and j in pools and len(pools[j]):
                v[j] = float(pools[j][rng.integers(len(pools[j]))])
            elif u < 0.7:
                v[j] = base[j] * float(rng.uniform(0.5, 1.5))
            elif u < 0.8 and j in (0, 3, 4, 11):
                v[j] = float(rng.integers(0, 12))
        out.append(v)
    return np.stack(out)


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_random_vectors_against_the_restated_tree(ctx, seed):
    soa = soa_fuzz.random_soa(60 + seed, n_contigs=3, n_ps=(1, 8))
    feat = ctx.features_host(soa, 50, 2)
    vecs = random_vectors(feat, 48, seed)
    counts, pred, ps = ctx.sweep_host(feat, vecs, want_pred=True, want_ps=True)
    for k, v in enumerate(vecs):
        want = np.array(tune_ref.preds_from_features(feat, v), dtype=np.uint8)
        bad = np.nonzero(pred[k] != want)[0]
        assert bad.size == 0, (k, v, bad[:5], pred[k][bad[:5]], want[bad[:5]])
        assert int(counts['n_calls'][k]) == int((want != 0).sum())


# ---- scoring against the evaluator ---------------------------------------------------------------------------------------

def scoring_workdir(home, seed):
    contigs = synth.fuzz_case(seed, n_contigs=3)
    for c in contigs:
        c.spelled = 'chr' + c.label
    synth.write_workdir(home, contigs, dialect='cutesv', seed=seed)
    return contigs


def write_truth(home, cands, path, seed):
    """A truth VCF from the candidates: jittered positions and lengths, HP flips, misses, some extra records."""
    rng = np.random.default_rng(seed)
    lines = ['##fileformat=VCFv4.2\n', '#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n']
    n = 0
    for c in range(len(cands['pos'])):
        if rng.random() < 0.25:
            continue
        ch = cands['chrom'][c]
        pos = int(cands['pos'][c]) + int(rng.integers(-600, 600))
        ln = max(1, int(cands['svlen'][c] * rng.uniform(0.6, 1.4)))
        t = cands['svtype'][c]
        signed = ln if t in ('INS', 'DUP') else -ln
        hp = ('1|0', '0|1', '1|1', '0/1', '1/1')[int(rng.integers(5))]
        ps = int(rng.integers(1, 6))
        n += 1
        lines.append('%s\t%d\ttruth%d\tN\t<%s>\t.\tPASS\tSVTYPE=%s;SVLEN=%d\tGT:PS\t%s:%d\n' % (ch, max(pos, 1), n % 900, t, t, signed,
                                                                                           hp, ps))
    with open(path, 'w') as f:
        f.writelines(lines)


def evaluate(truth, called, refdist, pctsim, bed, skip):
    try:
        return evaluation.evaluation(evaluation.parse_vcf(truth, skip, bed), evaluation.parse_vcf(called, skip, bed), refdist, pctsim)
    except (ZeroDivisionError, IndexError):
        return (math.nan,) * 10


@pytest.mark.parametrize('seed,refdist,pctsim,skip,with_bed', [(3, 1000, 0.0, False, False), (4, 1000, 0.0, True, False),
                                                               (5, 1000, 0.0, False, True), (6, 300, 0.7, False, False)])
def test_sweep_rows_equal_the_evaluator(ctx, tmp_path, seed, refdist, pctsim, skip, with_bed):
    home = str(tmp_path / 'w')
    scoring_workdir(home, seed)
    cands = tune.features(home, 50, 2, ctx=ctx)
    assert int(cands['feat']['eligible'].sum()) > 20
    truth = str(tmp_path / 'truth.vcf')
    write_truth(home, cands, truth, seed)
    bed = ''
    if with_bed:
        bed = str(tmp_path / 'r.bed')
        with open(bed, 'w') as f:
            for ch in sorted(set(cands['chrom'])):
                f.write('%s\t0\t2500000\n' % ch)
    vecs = random_vectors(cands['feat'], 7, seed)
    vecs = np.concatenate([tune.vector()[None, :], vecs])
    rows = tune.sweep(home, truth, vecs, refdist, pctsim, bed, skip, ctx=ctx, cands=cands)
    for v, row in zip(vecs, rows):
        called = str(tmp_path / 'called.vcf')
        with open(called, 'w') as f:
            f.write(tune_ref.phased_text(home, 50, 2, v))
        want = evaluate(truth, called, refdist, pctsim, bed, skip)
        got = tuple(row[n] for n in tune.SCORES)
        assert tune_ref.same_floats(got, want), (v, got, want)


def test_sweep_of_4096_vectors_agrees_with_single_rows(ctx, tmp_path):
    home = str(tmp_path / 'w')
    scoring_workdir(home, 7)
    cands = tune.features(home, 50, 2, ctx=ctx)
    truth = str(tmp_path / 'truth.vcf')
    write_truth(home, cands, truth, 7)
    grid = {'c2_min_sv_ratio': list(np.linspace(0.5, 0.9, 8)), 'c1_hapread_ratio': list(np.linspace(0.4, 0.9, 8)),
            'c1_max_totsc_ratio': list(np.linspace(2, 20, 8)),
            'c1_max_ref_num': [5, 10, 'inf', 'nan'], 'c0_min_sv_num': [2, 4]}
    vecs = tune.expand_grid(grid)
    assert len(vecs) == 4096
    rows = tune.sweep(home, truth, vecs, ctx=ctx, cands=cands)
    for k in (0, 1, 777, 2048, 4095):
        one = tune.sweep(home, truth, vecs[k:k + 1], ctx=ctx, cands=cands)[0]
        assert tune_ref.same_floats([rows[k][n] for n in tune.SCORES], [one[n] for n in tune.SCORES])
        called = str(tmp_path / 'called.vcf')
        with open(called, 'w') as f:
            f.write(tune_ref.phased_text(home, 50, 2, vecs[k]))
        assert tune_ref.same_floats([rows[k][n] for n in tune.SCORES], evaluate(truth, called, 1000, 0.0, '', False))


def test_cli_writes_the_sweep(ctx, tmp_path):
    home = str(tmp_path / 'w')
    scoring_workdir(home, 8)
    cands = tune.features(home, 50, 2, ctx=ctx)
    truth = str(tmp_path / 'truth.vcf')
    write_truth(home, cands, truth, 8)
    grid = str(tmp_path / 'g.json')
    with open(grid, 'w') as f:
        json.dump([{}, {'c1_max_ref_num': 3}], f)
    out, fo = str(tmp_path / 'sweep.tsv'), str(tmp_path / 'features.tsv')
    tune.main([home, truth, '--grid', grid, '--out', out, '--features', fo])
    with open(out) as f:
        lines = f.read().splitlines()
    assert len(lines) == 3 and lines[0].split('\t') == list(tune.NAMES + tune.SCORES)
    with open(fo) as f:
        assert len(f.read().splitlines()) == len(cands['feat']) + 1


# ---- apply path ------------------------------------------------------------------------------------------------------------

def test_sv_phasing_with_thresholds(tmp_path):
    from oracle import ef_oracle as O
    home = str(tmp_path / 'w')
    H.build_case(home, 'fuzz', 5, 'cutesv')
    sv_phasing(home, 50, 2, 4, False)
    with open(os.path.join(home, 'phased_sv.vcf'), 'rb') as f:
        plain = f.read()
    sv_phasing(home, 50, 2, 4, False, thresholds=tune.vector())
    with open(os.path.join(home, 'phased_sv.vcf'), 'rb') as f:
        assert f.read() == plain
    v = tune.vector({'c1_twohap_sv_ratio_1': 0.2, 'c1_max_ref_num': 3, 'c2_min_sv_ratio': 0.6, 'c0_min_sv_num': 2})
    sv_phasing(home, 50, 2, 4, False, thresholds=v)
    with open(os.path.join(home, 'phased_sv.vcf')) as f:
        got = f.read()
    assert got == tune_ref.phased_text(home, 50, 2, v)
    assert got != plain.decode()
    with pytest.raises(ValueError):
        sv_phasing(home, 50, 2, 4, False, gpus=2, thresholds=v)
