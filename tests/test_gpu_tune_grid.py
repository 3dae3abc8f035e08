# coding=utf-8
"""-m gpu: the sweep over -s, -r and -c (duet_amd/tune.py: sweep_settings; duet_tune_truth_build_device,
duet_svim_features_device): every row against evaluation.evaluation on the callset the oracle -- or, in the svim-gpu mode, the
product run itself -- writes for that setting, the fused pipeline's features against the E/F problem read back from the callset
it wrote, and the command line."""
import json
import math
import os
import shutil

import numpy as np
import pytest

from duet_amd import _lib, evaluation, svim_mode, synth, tune
from duet_amd.native import NativeIngest
from duet_amd.read_file import init_chrom_list
from tests import helpers as H
from tests import tune_ref
from tests.test_gpu_tune import FIELDS, random_vectors

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


# ---- the construction of tests/test_gpu_tune.py, restated ----------------------------------------------------------------

def scoring_workdir(home, seed):
    contigs = synth.fuzz_case(seed, n_contigs=3)
    for c in contigs:
        c.spelled = 'chr' + c.label
    synth.write_workdir(home, contigs, dialect='cutesv', seed=seed)
    return contigs


def write_truth(cands, path, seed):
    """A truth VCF from the candidates: jittered positions and lengths, HP flips, misses, ids that repeat."""
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


def rows_of(rows, **setting):
    return [r for r in rows if all(r[k] == v for k, v in setting.items())]


# ---- candidates of sv_calling/variants.vcf -------------------------------------------------------------------------------------

SS, RS = (30, 50, 80), (2, 3)


@pytest.mark.parametrize('seed,refdist,pctsim,skip,with_bed', [(3, 1000, 0.0, False, False), (6, 300, 0.7, False, False),
                                                               (3, 1000, 0.0, False, True), (6, 1000, 0.0, True, False)])
def test_vcf_mode_rows_equal_the_evaluator(ctx, tmp_path, seed, refdist, pctsim, skip, with_bed):
    home = str(tmp_path / 'w')
    scoring_workdir(home, seed)
    cands = tune.features(home, 50, 2, ctx=ctx)
    # the settings are different problems, and the strictest still has something to score
    elig = {(s, r): int(tune.features(home, s, r, ctx=ctx)['feat']['eligible'].sum()) for s in SS for r in RS}
    assert len(set(elig.values())) == len(elig) and elig[(80, 3)] >= 20, elig
    truth = str(tmp_path / 'truth.vcf')
    write_truth(cands, truth, seed)
    bed = ''
    if with_bed:
        bed = str(tmp_path / 'r.bed')
        with open(bed, 'w') as f:
            for ch in sorted(set(cands['chrom'])):
                f.write('%s\t0\t2500000\n' % ch)
                f.write('%s\t2000000\t2600000\n' % ch)      # (overlapping ranges)
    vecs = np.concatenate([tune.vector()[None, :], random_vectors(cands['feat'], 3, seed)])
    rows = tune.sweep_settings(home, truth, vecs, SS, RS, refdist=refdist, pctsim=pctsim, bed=bed, skip_phasing=skip, ctx=ctx)
    assert [(r['svlen_thres'], r['suppread_thres']) for r in rows] == [(s, r) for s in SS for r in RS for _ in vecs]
    assert 'cluster_max_distance' not in rows[0]
    called = str(tmp_path / 'called.vcf')
    scored = 0
    for i, row in enumerate(rows):
        v = vecs[i % len(vecs)]
        assert [row[n] for n in tune.NAMES] == [float(x) for x in v] or any(math.isnan(x) for x in v)
        with open(called, 'w') as f:
            f.write(tune_ref.phased_text(home, row['svlen_thres'], row['suppread_thres'], v))
        want = evaluate(truth, called, refdist, pctsim, bed, skip)
        got = tuple(row[n] for n in tune.SCORES)
        assert tune_ref.same_floats(got, want), (row['svlen_thres'], row['suppread_thres'], v, got, want)
        scored += not math.isnan(want[0])
    assert scored >= len(rows) // 2
    # the one-setting sweep of the function that was there before: the same rows
    one = tune.sweep(home, truth, vecs, refdist, pctsim, bed, skip, ctx=ctx, cands=cands)
    for a, b in zip(one, rows_of(rows, svlen_thres=50, suppread_thres=2)):
        assert tune_ref.same_floats([a[n] for n in tune.SCORES], [b[n] for n in tune.SCORES])


def test_a_setting_with_a_division_by_zero_gives_nan_rows_and_the_sweep_goes_on(ctx, tmp_path):
    """tests/golden/make_golden_r2.py's case -- with -r 0 a candidate without a single read reaches the decision, where upstream
    raises -- and two more candidates, so that -r 2 has calls to score: only the settings with -r 0 are nan."""
    from tests.test_gpu_r2 import _divzero_home
    home = _divzero_home(tmp_path)
    rec = 'chr1\t%d\tid%d\tN\t<DEL>\t.\tPASS\tPRECISE;SVTYPE=DEL;SVLEN=-80;END=180;RE=%d;RNAMES=%s;STRAND=+-\tGT:DR:DV:PL:GQ\t0/1:%d:5:1,2,3:9\n'
    with open(home + '/sv_calling/variants.vcf', 'a') as f:
        f.write(rec % (300, 3, 6, 'a,a,a,b,a,a', 0) + rec % (700, 4, 5, 'b,b,b,b,b', 1))
    truth = str(tmp_path / 'truth.vcf')
    with open(truth, 'w') as f:
        f.write('#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n')
        for pos, hp in ((310, '1|1'), (650, '0|1'), (90000, '1|0')):
            f.write('chr1\t%d\tt%d\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;SVLEN=-70\tGT:PS\t%s:1\n' % (pos, pos, hp))
    with pytest.raises(ZeroDivisionError):
        tune.features(home, 50, 0, ctx=ctx)
    vecs = tune.vector()[None, :]
    rows = tune.sweep_settings(home, truth, vecs, (50, 60), (0, 2), ctx=ctx)
    assert [(r['svlen_thres'], r['suppread_thres']) for r in rows] == [(50, 0), (50, 2), (60, 0), (60, 2)]
    called = str(tmp_path / 'called.vcf')
    with open(called, 'w') as f:
        f.write(tune_ref.phased_text(home, 50, 2, vecs[0]))
    want = evaluate(truth, called, 1000, 0.0, '', False)
    assert not any(math.isnan(x) for x in want) and want[1] > 0
    for row in rows:
        got = tuple(row[n] for n in tune.SCORES)
        assert tune_ref.same_floats(got, want if row['suppread_thres'] == 2 else (math.nan,) * 10), (row, want)


# ---- candidates of the fused pipeline (--from_bams) ---------------------------------------------------------------------------

CS, BS, BR = (0.5, 0.9), (40, 50), (2, 3)


@pytest.fixture(scope='module')
def bams(ctx, tmp_path_factory):
    """The work directory (BAMs only), a copy for the product runs, the truth set written from the candidates of the c = 0.9 run,
    the vectors, and the sweep's rows over the whole grid."""
    root = tmp_path_factory.mktemp('bams')
    home, copy = str(root / 'w'), str(root / 'copy')
    synth.write_svim_workdir(home, H.case_contigs('genome_small', 5), 5)
    shutil.copytree(home, copy)
    svim_mode.sv_phasing_from_bams(copy, 50, 2, 4, False, 0.9, 0, write_sv_calls=True)
    cands = tune.features(copy, 50, 2, ctx=ctx)
    truth = str(root / 'truth.vcf')
    write_truth(cands, truth, 5)
    vecs = np.concatenate([tune.vector()[None, :], random_vectors(cands['feat'], 2, 5)])
    rows = tune.sweep_settings(home, truth, vecs, BS, BR, CS, from_bams=True, ctx=ctx)
    assert not os.path.exists(home + '/sv_calling') and not os.path.exists(home + '/phased_sv.vcf')
    return dict(home=home, copy=copy, truth=truth, vecs=vecs, rows=rows, cands=cands, counts={})


def test_from_bams_row_order(bams):
    got = [(r['cluster_max_distance'], r['svlen_thres'], r['suppread_thres']) for r in bams['rows']]
    assert got == [(c, s, r) for c in CS for s in BS for r in BR for _ in bams['vecs']]


@pytest.mark.parametrize('c', CS)
@pytest.mark.parametrize('s', BS)
def test_from_bams_rows_equal_the_evaluator_on_the_product_run(bams, tmp_path, c, s):
    copy, truth, vecs = bams['copy'], bams['truth'], bams['vecs']
    for r in BR:
        svim_mode.sv_phasing_from_bams(copy, s, r, 4, False, c, 0, write_sv_calls=True)
        with open(svim_mode.callset_path(copy)) as f:
            bams['counts'][(c, s, r)] = sum(1 for ln in f if not ln.startswith('#'))
        rows = rows_of(bams['rows'], cluster_max_distance=c, svlen_thres=s, suppread_thres=r)
        assert len(rows) == len(vecs)
        # the default vector: the product run's own phased_sv.vcf
        want = evaluate(truth, copy + '/phased_sv.vcf', 1000, 0.0, '', False)
        assert not math.isnan(want[0])
        assert tune_ref.same_floats(tuple(rows[0][n] for n in tune.SCORES), want), (c, s, r, rows[0], want)
        # the other vectors: the oracle's E/F over the callset that run wrote
        called = str(tmp_path / 'called.vcf')
        for v, row in zip(vecs[1:], rows[1:]):
            with open(called, 'w') as f:
                f.write(tune_ref.phased_text(copy, s, r, v))
            want = evaluate(truth, called, 1000, 0.0, '', False)
            assert tune_ref.same_floats(tuple(row[n] for n in tune.SCORES), want), (c, s, r, v, row, want)
    if len(bams['counts']) == len(CS) * len(BS) * len(BR):
        # the two cluster distances are different callsets
        assert all(bams['counts'][(CS[0], s_, r_)] != bams['counts'][(CS[1], s_, r_)] for s_ in BS for r_ in BR), bams['counts']


def test_from_bams_with_a_bed_file(ctx, bams, tmp_path):
    """The BED ranges reach the device as merged per-contig tables; the row equals the evaluator's with the same file."""
    cands, copy = bams['cands'], bams['copy']
    bed = str(tmp_path / 'r.bed')
    pos = np.sort(np.asarray(cands['pos'], dtype=np.int64))
    mid = int(pos[len(pos) // 2])
    with open(bed, 'w') as f:
        for ch in sorted(set(cands['chrom'])):
            f.write('%s\t0\t%d\n%s\t%d\t%d\n' % (ch, mid, ch, mid // 2, mid))
    rows = tune.sweep_settings(bams['home'], bams['truth'], tune.vector()[None, :], (50,), (2,), (0.9,), from_bams=True, bed=bed, ctx=ctx)
    svim_mode.sv_phasing_from_bams(copy, 50, 2, 4, False, 0.9, 0, write_sv_calls=True)
    want = evaluate(bams['truth'], copy + '/phased_sv.vcf', 1000, 0.0, bed, False)
    plain = evaluate(bams['truth'], copy + '/phased_sv.vcf', 1000, 0.0, '', False)
    assert not math.isnan(want[0]) and not tune_ref.same_floats(want, plain)
    assert tune_ref.same_floats(tuple(rows[0][n] for n in tune.SCORES), want), (rows[0], want)


def test_svim_features_equal_the_features_of_the_written_callset(ctx, bams):
    from duet_amd.devmem import DeviceSvim
    copy = bams['copy']
    svim_mode.sv_phasing_from_bams(copy, 50, 2, 4, False, 0.9, 0, write_sv_calls=True)
    want = tune.features(copy, 50, 2, ctx=ctx)['feat']                  # duet_ef_features_host on the callset read back
    assert int(want['eligible'].sum()) > 100
    chroms = init_chrom_list(False, copy)
    ing, got = NativeIngest.extract(copy + '/snp_phasing/', chroms, 4, 50, 20, 1000)
    assert ing is not None, got
    ing.close()
    host = ctx.svim_features_host(got, got['read_tag'], got['depth'], got['depth_off'], 1000, 50, 2, max_dist=0.9)
    import torch
    ds = DeviceSvim(got, got['read_tag'], got['depth'], got['depth_off'], 1000, 50, 2, max_dist=0.9, device='cuda:0')
    buf = torch.zeros(len(got['pos']) * _lib.FEATURE_DTYPE.itemsize + 64, dtype=torch.uint8, device='cuda:0')
    n = ds.run_features(ctx, buf.data_ptr())
    dev = buf[:n * _lib.FEATURE_DTYPE.itemsize].cpu().numpy().view(_lib.FEATURE_DTYPE)
    assert n == len(want) == len(host['feat'])
    for name in FIELDS:
        assert np.array_equal(host['feat'][name], want[name]), name
        assert np.array_equal(dev[name], want[name]), name
    # the cluster result stays in the caller's arrays
    res = ds.fetch()
    for k in ('cand_contig', 'cand_type', 'cand_pos', 'cand_span'):
        assert np.array_equal(res[k], host[k]), k


# ---- command line ------------------------------------------------------------------------------------------------------------

def test_cli(ctx, tmp_path, capsys):
    home = str(tmp_path / 'w')
    scoring_workdir(home, 8)
    cands = tune.features(home, 50, 2, ctx=ctx)
    truth = str(tmp_path / 'truth.vcf')
    write_truth(cands, truth, 8)
    grid = str(tmp_path / 'g.json')
    with open(grid, 'w') as f:
        json.dump([{}, {'c1_max_ref_num': 3}], f)
    out = lambda name: str(tmp_path / name)
    # single values, given or not: byte for byte the file without the new flags, whose columns are the 14 + 10
    tune.main([home, truth, '--grid', grid, '--out', out('a.tsv'), '--features', out('fa.tsv')])
    tune.main([home, truth, '--grid', grid, '--out', out('b.tsv'), '-s', '50', '-r', '2'])
    with open(out('a.tsv'), 'rb') as fa, open(out('b.tsv'), 'rb') as fb:
        a = fa.read()
        assert a == fb.read()
    lines = a.decode().splitlines()
    assert len(lines) == 3 and lines[0].split('\t') == list(tune.NAMES + tune.SCORES)
    want = tune.sweep(home, truth, tune.load_grid(grid), ctx=ctx, cands=cands)
    assert lines[1].split('\t') == [repr(want[0][n]) for n in tune.NAMES + tune.SCORES]
    with open(out('fa.tsv')) as f:
        assert len(f.read().splitlines()) == len(cands['feat']) + 1
    # a 2 x 2 grid: leading columns, settings outermost in the order s, r; one feature file per setting
    tune.main([home, truth, '--grid', grid, '--out', out('c.tsv'), '-s', '30,50', '-r', '3,2', '--features', out('f.tsv')])
    with open(out('c.tsv')) as f:
        rows = [ln.split('\t') for ln in f.read().splitlines()]
    assert rows[0] == ['svlen_thres', 'suppread_thres'] + list(tune.NAMES + tune.SCORES) and len(rows) == 9
    assert [tuple(r[:2]) for r in rows[1:]] == [(s, r) for s in ('30', '50') for r in ('3', '2') for _ in range(2)]
    assert rows[7][2:] == lines[1].split('\t') and rows[8][2:] == lines[2].split('\t')          # (50, 2) is the plain run
    assert rows[1][2:] != rows[7][2:]
    for s, r in ((30, 3), (30, 2), (50, 3), (50, 2)):
        with open(out('f.s%d.r%d.tsv' % (s, r))) as f:
            assert len(f.read().splitlines()) == len(cands['feat']) + 1
    assert not os.path.exists(out('f.tsv'))
    # -c only acts on candidates clustered from the BAMs
    with pytest.raises(SystemExit):
        tune.main([home, truth, '--grid', grid, '--out', out('d.tsv'), '-c', '0.5'])
    assert not os.path.exists(out('d.tsv'))
    capsys.readouterr()
