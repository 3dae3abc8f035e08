# coding=utf-8
"""--write_sv_calls over several ranks (duet_amd/svim_mode.py: rank_body) on CPU, over the torch-free TCP star: every rank
writes its contigs' callset rows before the count exchange, rank 0 assembles sv_calling/variants.vcf in contig-list order and
writes phased_sv.vcf whole; a read name that READS= cannot hold on any rank fails every rank and leaves no file.  The rows come
from tests/callset_ref.py on the composed C oracles' candidates (the device kernels are checked against the same formatter in
tests/test_gpu_callset.py)."""
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

from duet_amd import bamio, launch, svim_mode, synth
from oracle import c_oracle
from tests import callset_ref
from tests import helpers as H
from tests.test_svim_multi import oracle_compute


def calls_compute(texts):
    def compute(got, svlen_thres, suppread_thres, max_dist, depth_bin):
        out = oracle_compute(got, svlen_thres, suppread_thres, max_dist, depth_bin)
        cl = c_oracle.cluster(got['contig'], got['type'], got['pos'], got['span'], max_dist=max_dist)
        out['calls'] = callset_ref.rows(cl, callset_ref.names_of(got), got['depth'], got['depth_off'], depth_bin, texts).encode()
        return out
    return compute


def _worker(rank, world, port, home, out_dir):
    from duet_amd import comm
    star = comm.TcpStar(rank, world, '127.0.0.1', port, timeout=60)
    try:
        texts = svim_mode.spelled_contigs(home, svim_mode.init_chrom_list(False, home))
        rc = svim_mode.rank_body(home, 50, 2, 4, False, 0.9, rank, world, calls_compute(texts), star=star,
                                 gather=comm.HostGather(star), write_sv_calls=True)
        with open(os.path.join(out_dir, 'rc%d' % rank), 'w') as f:
            f.write(str(rc))
    finally:
        star.close()


@pytest.mark.parametrize('world', [2, 8])
def test_sharded_callset_equals_the_single_process_file(world, tmp_path):
    home = str(tmp_path / 'w')
    synth.write_svim_workdir(home, H.case_contigs('genome_small', 5), 5)
    chroms = svim_mode.init_chrom_list(False, home)
    one = svim_mode.phase_from_bams(home, 50, 2, 2, min_sv_size=50, names=True,
                                    compute=calls_compute(svim_mode.spelled_contigs(home, chroms)))
    want_calls = svim_mode.callset_header_text(home, chroms).encode() + one['calls']
    want_phased = svim_mode.header_text(home, chroms) + svim_mode.rows_text(home, one)
    assert one['calls'].count(b'\n') == len(one['pred']) > 1000
    mp.spawn(_worker, args=(world, launch.free_port(), home, str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        assert open(os.path.join(str(tmp_path), 'rc%d' % r)).read() == '0'
    assert open(svim_mode.callset_path(home), 'rb').read() == want_calls
    assert open(home + '/phased_sv.vcf').read() == want_phased
    assert os.listdir(os.path.join(home, 'sv_calling')) == ['variants.vcf']


def test_sharded_bad_read_name_fails_every_rank_and_leaves_no_file(tmp_path):
    home = str(tmp_path / 'w')
    d = os.path.join(home, 'snp_phasing')
    os.makedirs(d)
    line = '%s\t0\t%s\t%d\t60\t100M60I100M\t*\t0\t0\t*\t*\tHP:i:1\tPC:i:10\tPS:i:7'
    bamio.write_bam_from_sam_lines(os.path.join(d, 'chr1.bam'), [('chr1', 249250621)],
                                   [line % ('a%d' % i, 'chr1', 1000 + 10 * i) for i in range(4)])
    bamio.write_bam_from_sam_lines(os.path.join(d, 'chr2.bam'), [('chr2', 243199373)],
                                   [line % ('b;%d' % i, 'chr2', 1000 + 10 * i) for i in range(4)])
    mp.spawn(_worker, args=(2, launch.free_port(), home, str(tmp_path)), nprocs=2, join=True)
    assert [open(os.path.join(str(tmp_path), 'rc%d' % r)).read() for r in range(2)] == ['6', '6']
    assert not os.path.exists(home + '/phased_sv.vcf')
    calls_dir = os.path.join(home, 'sv_calling')                 # (the good rank's part, if it got that far, is removed)
    assert not os.path.exists(calls_dir) or os.listdir(calls_dir) == []
