# coding=utf-8
"""The host side of the sweep over -s, -r and -c (duet_amd/tune.py), without a GPU: the command line and its refusals, what the
evaluator's parser makes of a candidate's row (candidate_keys, contig_tables) against evaluation.parse_vcf on written rows, the
BED ranges as per-contig tables, and the resources of the truth build's kernels."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from duet_amd import _lib, evaluation, svim_mode, tune
from tests import helpers as H
from tests.test_c_oracle import materialise_bams

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
NONE, SKIP = _lib.TUNE_KEY_NONE, _lib.TUNE_KEY_SKIP


def test_the_new_symbols_are_bound():
    for sym in ('duet_svim_features_device', 'duet_svim_features_host', 'duet_tune_truth_build_device', 'duet_tune_truth_build_host'):
        assert sym in _lib.EXPORTS
    assert (NONE, SKIP) == (0xFFFFFFFE, 0xFFFFFFFF)


def test_arguments():
    base = ['w', 't.vcf', '--grid', 'g.json']
    a = tune.parse_args(base)
    assert (a.sv_min_size, a.min_support_read, a.cluster_max_distance, a.from_bams) == ([50], [2], None, False)
    a = tune.parse_args(base + ['-s', '30,50,80', '-r', '2,3'])
    assert (a.sv_min_size, a.min_support_read) == ([30, 50, 80], [2, 3])
    a = tune.parse_args(base + ['--from_bams', '-c', '0.5,0.9', '-s', '40'])
    assert (a.cluster_max_distance, a.sv_min_size, a.from_bams) == ([0.5, 0.9], [40], True)
    assert tune.parse_args(base + ['--from_bams']).cluster_max_distance is None        # (sweep_settings: 0.9)
    for bad in (['-c', '0.5'], ['-s', '30,'], ['-s', 'x'], ['-r', '-1'], ['-s', ''], ['--from_bams', '-c', '0.5,y']):
        with pytest.raises(SystemExit):
            tune.parse_args(base + bad)


def test_sweep_settings_refusals():
    v = tune.vector()[None, :]
    with pytest.raises(ValueError, match='from_bams'):
        tune.sweep_settings('w', 't.vcf', v, cluster_max_distance=(0.5,))
    for kw in (dict(svlen_thres=()), dict(suppread_thres=(2, -1)), dict(svlen_thres=(50.5,))):
        with pytest.raises(ValueError):
            tune.sweep_settings('w', 't.vcf', v, **kw)
    with pytest.raises(ValueError, match='unknown'):
        tune.sweep_settings('w', 't.vcf', {'no_such_threshold': [1]})


def test_features_path():
    assert tune.features_path('d/f.tsv', dict(svlen_thres=30, suppread_thres=2)) == 'd/f.s30.r2.tsv'
    assert tune.features_path('f', dict(cluster_max_distance=0.5, svlen_thres=30, suppread_thres=2)) == 'f.c0.5.s30.r2'


def expected_keys(rows, bed=''):
    """rows: (chrom, pos, ref, alt, svtype, svlen >= 50), written as phased_sv.vcf holds them and read by the evaluator's parser."""
    import tempfile
    fd, path = tempfile.mkstemp(suffix='.vcf')
    try:
        with os.fdopen(fd, 'w') as f:
            for i, (chrom, pos, ref, alt, svtype, svlen) in enumerate(rows):
                f.write(tune.row_text(chrom, pos, 7, ref, alt, svlen, svtype, '0|1', 1000 + i))
        recs = evaluation.parse_vcf(path, False, bed)
    finally:
        os.remove(path)
    out = [SKIP] * len(rows)
    for r in recs:
        i = int(r['ps'][r['ps'].rfind(':') + 1:]) - 1000
        if r['chr'] in evaluation.CHROMS and r['type'] in ('INS', 'DEL'):
            out[i] = 2 * evaluation.CHROMS.index(r['chr']) + ('INS', 'DEL').index(r['type'])
        else:
            out[i] = NONE
    return out


@pytest.mark.parametrize('name', ['fuzz_cutesv_s1', 'fuzz_sniffles_s5', 'fuzz_svim_s7'])
def test_candidate_keys_on_the_three_caller_dialects(tmp_path, name):
    home = str(tmp_path / name)
    shutil.copytree(os.path.join(H.GOLDEN, 'cases', name), home)
    materialise_bams(home)
    soa, txt = tune._candidates(home, 50, 2, False, 2)
    cands = dict(pos=soa.cand_pos, svlen=soa.cand_svlen, **txt)
    C = soa.n_cands
    assert C > 50
    key, chrom, n_chrom = tune.candidate_keys(cands)
    assert len(key) == len(chrom) == C and n_chrom == len(set(cands['chrom'])) > 1
    assert all((chrom[a] == chrom[b]) == (cands['chrom'][a] == cands['chrom'][b]) for a in range(0, C, 7) for b in range(0, C, 5))
    # the length is the device's test, not the key's: every row is written with a length the parser keeps
    rows = [(cands['chrom'][c], int(cands['pos'][c]), cands['ref'][c], cands['alt'][c], cands['svtype'][c], max(int(cands['svlen'][c]), 50))
            for c in range(C)]
    want = expected_keys(rows)
    assert key.tolist() == want
    assert sum(1 for k in want if k < NONE) > 20
    # with a BED file a candidate outside the ranges is dropped
    bed = str(tmp_path / 'r.bed')
    mid = int(np.median(soa.cand_pos))
    with open(bed, 'w') as f:
        for ch in sorted(set(cands['chrom'])):
            f.write('%s\t%d\t%d\n' % (ch, 0, mid))
    key_bed = tune.candidate_keys(cands, bed)[0]
    assert key_bed.tolist() == expected_keys(rows, bed)
    inside = soa.cand_pos <= mid
    assert (key_bed[~inside] == SKIP).all() and np.array_equal(key_bed[inside], key[inside]) and (key[~inside] != SKIP).any()


def test_parser_quirks_carry_over():
    cands = dict(chrom=['chr1', 'chr1', 'chr2', 'abc7', 'chrUn', '1', 'chrX', 'chr1', 'chr1'], pos=[10] * 9, svlen=[100] * 9,
                 ref=['N', 'N', 'N', 'N', 'N', 'N', 'N', 'ACGT', 'N'], alt=['<INS>', 'ACGTACGT', '<DUP>', '<INS>', '<INS>', '<INS>', '<DEL>', 'A', '<INV>'],
                 svtype=['INS', 'INS', 'DUP', 'INS', 'INS', 'INS', 'DEL', 'DEL', 'INV'])
    key, chrom, n_chrom = tune.candidate_keys(cands)
    #                      INS  SVTYPE=<INS> beside a sequence ALT: type '<INS>', no list
    assert key.tolist() == [0, NONE, 2, NONE, SKIP, SKIP, 2 * 22 + 1, NONE, SKIP]
    assert chrom.tolist() == [0, 0, 1, 2, 3, 4, 5, 0, 0] and n_chrom == 6
    rows = [(cands['chrom'][c], 10, cands['ref'][c], cands['alt'][c], cands['svtype'][c], 100) for c in range(9)]
    assert key.tolist() == expected_keys(rows)


def test_contig_tables_on_the_four_types_and_odd_spellings(tmp_path):
    texts = ['chr1', '1', 'chr22', 'chrX', 'chrY', 'abc7', 'chrUn', 'CHR3', 'chr1']
    table, chrom_id, n_chrom = tune.contig_tables(texts)
    assert table.shape == (4 * len(texts),) and chrom_id.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 0] and n_chrom == 8
    # the rows svim_mode.rows_text writes for one phased candidate per (contig, type), read by the evaluator's parser
    want = []
    for k, text in enumerate(texts):
        home = str(tmp_path / ('h%d' % k))
        os.makedirs(home + '/snp_phasing')
        label = text[3:] if text.startswith('chr') else text
        if text.startswith('chr'):
            open(home + '/snp_phasing/' + text + '.bam', 'wb').close()
        assert svim_mode.spelled_contigs(home, [label]) == [text]
        res = dict(chroms=[label], pred=np.ones(4, dtype=np.uint8), cand_contig=np.zeros(4, dtype=np.uint16),
                   cand_type=np.arange(4, dtype=np.uint8), cand_pos=np.array([5, 6, 7, 8]), cand_span=np.full(4, 60), ps=np.arange(4) + 1000)
        path = home + '/rows.vcf'
        with open(path, 'w') as f:
            f.write(svim_mode.rows_text(home, res))
        got = [SKIP] * 4
        for r in evaluation.parse_vcf(path, False, ''):
            t = r['pos'] - 5
            got[t] = 2 * evaluation.CHROMS.index(r['chr']) + ('INS', 'DEL').index(r['type']) if r['chr'] in evaluation.CHROMS else NONE
        want.extend(got)
    assert table.tolist() == want
    # DEL, INS, INV, DUP on chr1; a bare label has no 'chr...'[3:] label; 'abc7' passes the label test and is never matched
    assert table[:4].tolist() == [1, 0, SKIP, 0] and table[4:8].tolist() == [SKIP] * 4 and table[20:24].tolist() == [NONE, NONE, SKIP, NONE]
    assert table[12:16].tolist() == [45, 44, SKIP, 44] and table[28:32].tolist() == [NONE, NONE, SKIP, NONE]


def test_merge_ranges():
    assert tune.merge_ranges([]) == []
    assert tune.merge_ranges([(5, 10), (1, 3), (10, 12), (20, 19), (14, 15), (-5, 0), (2 ** 32 - 1, 2 ** 40), (2 ** 33, 2 ** 34)]) == \
        [(0, 3), (5, 12), (14, 15), (2 ** 32 - 1, 2 ** 32 - 1)]
    rng = np.random.default_rng(4)
    for _ in range(50):
        ranges = [(int(a), int(a + d)) for a, d in zip(rng.integers(0, 200, 12), rng.integers(-3, 30, 12))]
        merged = tune.merge_ranges(ranges)
        assert all(a <= b for a, b in merged) and all(merged[i][1] < merged[i + 1][0] for i in range(len(merged) - 1))
        for p in range(-2, 240):
            assert any(a <= p <= b for a, b in ranges) == any(a <= p <= b for a, b in merged)


def test_bed_tables(tmp_path):
    bed = str(tmp_path / 'r.bed')
    with open(bed, 'w') as f:
        f.write('chr1\t100\t200\nchr1\t150\t300\nchr2\t5\t5\nchrX\t7\t9\nchr1\t1000\t1100\n1\t0\t99999\nchrUn\t1\t2\n')
    texts = ['chr1', 'chr2', 'chr3', 'abc1', '1', 'chrX']
    off, lo, hi = tune.bed_tables(bed, texts)
    assert off.tolist() == [0, 2, 3, 3, 5, 5, 6]                 # 'abc1' is tested against chr1's ranges: the label is CHROM[3:]
    assert list(zip(lo.tolist(), hi.tolist())) == [(100, 300), (1000, 1100), (5, 5), (100, 300), (1000, 1100), (7, 9)]
    spans = evaluation.parse_bed(bed)
    for k, text in enumerate(texts):
        if text[3:] not in evaluation.LABELS:
            continue
        for p in (0, 99, 100, 200, 201, 300, 301, 999, 1000, 1100, 1101, 5, 6, 7, 9, 10):
            assert any(a <= p <= b for a, b in spans[text[3:]]) == any(lo[j] <= p <= hi[j] for j in range(off[k], off[k + 1]))


def test_truth_build_kernels_use_no_scratch_and_make_no_call(tmp_path):
    csrc = os.path.join(REPO, 'duet_amd', 'csrc')
    asm = str(tmp_path / 'duet_tune_truth.s')
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fvisibility=hidden',
           '-Wno-unused-function', '-I' + os.path.join(REPO, 'include'), '--cuda-device-only', '-S',
           '-Rpass-analysis=kernel-resource-usage', os.path.join(csrc, 'duet_tune_truth.hip'), '-o', asm]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    found = re.findall(r'Function Name: (\S+) \[.*?\n(?:.*\n){0,8}?.*ScratchSize \[bytes/lane\]: (\d+)', r.stderr)
    # its own (tt_*) and the scans it instantiates from duet_prims.hip.h with its head-flag functors
    kernels = {n: int(v) for n, v in found if 'tt_' in n or 'GroupHead' in n or 'PairHead' in n}
    assert len(kernels) == 3 + 2 * 3, found
    assert all(v == 0 for v in kernels.values()), kernels
    with open(asm) as f:
        assert 's_swappc' not in f.read()
