# coding=utf-8
"""-m gpu: `duet -b svim-gpu --thresholds FILE` on one GPU (svim_mode.sv_phasing_from_bams(..., thresholds=v)): the default vector
reproduces the run without the flag byte for byte, phased_sv.vcf and (--write_sv_calls) sv_calling/variants.vcf alike; another
vector gives the rows of the restated tree (tests/tune_ref.py) over the features the sweep's --from_bams path hands out; several
GPUs stay refused."""
import sys

import numpy as np
import pytest

from duet_amd import _lib, cli, svim_mode, synth, tune
from tests import helpers as H
from tests import tune_ref

pytestmark = pytest.mark.gpu

HEAD = '##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n'


@pytest.fixture(scope='module')
def home(tmp_path_factory):
    h = str(tmp_path_factory.mktemp('svim_thr') / 'w')
    synth.write_svim_workdir(h, H.case_contigs('genome_small', 5), 5)
    return h


def read(path):
    with open(path, 'rb') as f:
        return f.read()


def test_default_vector_is_the_run_without_the_flag(home):
    for calls in (False, True):
        svim_mode.sv_phasing_from_bams(home, 50, 2, 4, False, 0.9, 0, write_sv_calls=calls)
        plain = read(home + '/phased_sv.vcf')
        plain_calls = read(svim_mode.callset_path(home)) if calls else None
        assert plain.count(b'Duet.') > 100
        svim_mode.sv_phasing_from_bams(home, 50, 2, 4, False, 0.9, 0, write_sv_calls=calls, thresholds=tune.vector())
        assert read(home + '/phased_sv.vcf') == plain
        if calls:
            assert read(svim_mode.callset_path(home)) == plain_calls


def test_another_vector_gives_the_rows_of_the_restated_tree(home, tmp_path):
    ctx = _lib.Context(0)
    try:
        truth = str(tmp_path / 'truth.vcf')
        with open(truth, 'w') as f:
            f.write(HEAD + 'chr1\t1000\tt1\tN\t<INS>\t.\tPASS\tSVTYPE=INS;SVLEN=100\tGT:PS\t1|0:1\n')
        v = tune.vector({'c1_twohap_sv_ratio_1': 0.2, 'c1_max_ref_num': 3, 'c2_min_sv_ratio': 0.6, 'c0_min_sv_num': 2,
                         'c1_onehap_sv_ratio_hi': 0.7, 'c1_twohap_sv_ratio_3': 0.5, 'c1_max_totsc_ratio': 2.0})
        seen = []
        tune.sweep_settings(home, truth, v[None, :], (50,), (2,), (0.9,), from_bams=True, ctx=ctx, on_features=lambda s, c: seen.append(c))
    finally:
        ctx.close()
    assert len(seen) == 1
    cands = seen[0]
    feat = cands['feat']
    chroms = svim_mode.init_chrom_list(False, home)
    texts = svim_mode.spelled_contigs(home, chroms)
    res = dict(chroms=chroms, cand_contig=np.array([texts.index(t) for t in cands['chrom']], dtype=np.uint16),
               cand_type=np.array([svim_mode.SV_TYPE_NAMES.index(t) for t in cands['svtype']], dtype=np.uint8),
               cand_pos=cands['pos'], cand_span=cands['svlen'], ps=np.where(feat['eligible'] != 0, feat['ps'], 0))
    want = svim_mode.rows_text(home, dict(res, pred=np.array(tune_ref.preds_from_features(feat, v), dtype=np.uint8)))
    plain = svim_mode.rows_text(home, dict(res, pred=np.array(tune_ref.preds_from_features(feat, tune.vector()), dtype=np.uint8)))
    assert want != plain and want.count('\n') > 100          # the vector changes at least one row
    svim_mode.sv_phasing_from_bams(home, 50, 2, 4, False, 0.9, 0, thresholds=v)
    got = read(home + '/phased_sv.vcf').decode()
    assert got == svim_mode.header_text(home, chroms) + want
    svim_mode.sv_phasing_from_bams(home, 50, 2, 4, False, 0.9, 0)
    assert read(home + '/phased_sv.vcf').decode() == svim_mode.header_text(home, chroms) + plain


def test_several_gpus_stay_refused(home, tmp_path, monkeypatch):
    vec = str(tmp_path / 'v.json')
    with open(vec, 'w') as f:
        f.write('{"c1_max_ref_num": 3}')
    svim_mode.sv_phasing_from_bams(home, 50, 2, 4, False, 0.9, 0)
    before = read(home + '/phased_sv.vcf')
    monkeypatch.setattr(sys, 'argv', ['duet', 'in.bam', 'ref.fa', home, '-b', 'svim-gpu', '--gpus', '2', '--thresholds', vec])
    with pytest.raises(SystemExit, match='--thresholds works on the single-GPU path'):
        cli.main(None)
    monkeypatch.setattr(sys, 'argv', ['duet', 'in.bam', 'ref.fa', home, '-b', 'svim-gpu', '--thresholds', vec])
    monkeypatch.setenv('DUET_FORCE_RANKS', '1')
    with pytest.raises(SystemExit, match='--thresholds works on the single-GPU path'):
        cli.main(None)
    monkeypatch.delenv('DUET_FORCE_RANKS')
    with pytest.raises(ValueError):
        svim_mode.sv_phasing_from_bams(home, 50, 2, 4, False, 0.9, 0, gpus=2, thresholds=tune.vector())
    assert read(home + '/phased_sv.vcf') == before
