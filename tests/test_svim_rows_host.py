# coding=utf-8
"""The rows of phased_sv.vcf in the svim-gpu mode, CPU side: the plain-Python restatement the GPU tests
compare against equals svim_mode.rows_text, rank 0 writes what an injected format_rows returns, and the gfx950 resource usage of
duet_svim_rows.hip's kernels."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from duet_amd import launch, svim_mode, synth
from duet_amd.read_file import init_chrom_list
from tests import helpers as H
from tests import svim_rows_ref
from tests.test_svim_multi import oracle_compute

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_equals_rows_text_on_a_work_directory(tmp_path):
    """24 contigs spelled both ways (chr<c>.bam for the odd ones of the list, <c>.bam for the others), four types, ties on
    (CHROM, POS) within a type and across types, pred 0-3."""
    home = str(tmp_path)
    os.makedirs(os.path.join(home, 'snp_phasing'))
    chroms = init_chrom_list(False, home)
    assert len(chroms) == 24
    for k, c in enumerate(chroms):
        open(os.path.join(home, 'snp_phasing', ('chr' + c if k % 2 else c) + '.bam'), 'wb').close()
    texts = svim_mode.spelled_contigs(home, chroms)
    assert texts == [('chr' + c if k % 2 else c) for k, c in enumerate(chroms)]
    rng = np.random.default_rng(16)
    N = 6000
    res = dict(chroms=chroms, cand_contig=rng.integers(0, 24, N).astype(np.uint16), cand_type=rng.integers(0, 4, N).astype(np.uint8),
               cand_pos=rng.integers(0, 400, N).astype(np.uint32),                   # 6000 candidates on 9600 (contig, POS): ties
               cand_span=rng.choice(np.array([0, 1, 9, 10, 50, 999, 1000, 4294967295], dtype=np.uint32), N),
               pred=rng.integers(0, 4, N).astype(np.uint8), ps=rng.integers(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32))
    keys = list(zip(res['cand_contig'][res['pred'] != 0].tolist(), res['cand_pos'][res['pred'] != 0].tolist()))
    assert len(set(keys)) < len(keys)
    want = svim_mode.rows_text(home, res)
    assert svim_rows_ref.rows_of(texts, res) == want.encode()
    assert want.count('\n') == int(np.count_nonzero(res['pred'])) and 'SVLEN=0;' in want and 'SVLEN=-0' not in want
    assert all('<%s>' % t in want for t in svim_rows_ref.TYPES)


def _refuse(*a, **k):
    raise AssertionError('rows_text was called although a format_rows was given')


def _worker(rank, world, port, home, out_dir):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    svim_mode.rows_text = _refuse

    def format_rows(merged, texts):
        with open(os.path.join(out_dir, 'called%d' % rank), 'a') as f:
            f.write('%d %d %s\n' % (len(merged['pred']), int(np.count_nonzero(merged['pred'])), ','.join(texts)))
        return b'rows of %d candidates from the hook\n\xc3\xa9\n' % len(merged['pred'])

    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        rc = svim_mode.rank_body(home, 50, 2, 4, False, 0.9, rank, world, oracle_compute, format_rows=format_rows)
        with open(os.path.join(out_dir, 'rc%d' % rank), 'w') as f:
            f.write(str(rc))
    finally:
        dist.destroy_process_group()


def test_rank_0_writes_what_format_rows_returns(tmp_path):
    home = str(tmp_path / 'w')
    synth.write_svim_workdir(home, H.case_contigs('genome_small', 5), 5)
    chroms = init_chrom_list(False, home)
    one = svim_mode.phase_from_bams(home, 50, 2, 2, min_sv_size=50, compute=oracle_compute)       # (rank_body's min_sv_size)
    head = svim_mode.header_text(home, chroms)
    with open(home + '/phased_sv.vcf', 'w') as f:
        f.write(head)
    mp.spawn(_worker, args=(2, launch.free_port(), home, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        assert open(os.path.join(str(tmp_path), 'rc%d' % r)).read() == '0'
    # called once, on rank 0, with the merged records and the CHROM texts
    assert not os.path.exists(os.path.join(str(tmp_path), 'called1'))
    assert open(os.path.join(str(tmp_path), 'called0')).read() == '%d %d %s\n' % (
        len(one['pred']), int(np.count_nonzero(one['pred'])), ','.join(svim_mode.spelled_contigs(home, chroms)))
    assert open(home + '/phased_sv.vcf', 'rb').read() == \
        head.encode() + b'rows of %d candidates from the hook\n\xc3\xa9\n' % len(one['pred'])


HIPCC = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)


@pytest.mark.skipif(HIPCC is None, reason='hipcc not found')
def test_svim_rows_kernels_use_no_scratch_and_make_no_call(tmp_path):
    csrc = os.path.join(REPO, 'duet_amd', 'csrc')
    asm = str(tmp_path / 'duet_svim_rows.s')
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fvisibility=hidden',
           '-Wno-unused-function', '-I' + os.path.join(REPO, 'include'), '--cuda-device-only', '-S',
           '-Rpass-analysis=kernel-resource-usage', os.path.join(csrc, 'duet_svim_rows.hip'), '-o', asm]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    found = re.findall(r'Function Name: (\S+) \[.*?\n(?:.*\n){0,8}?.*ScratchSize \[bytes/lane\]: (\d+)', r.stderr)
    # every kernel of the unit: its own (sr_*), the 64-bit spine scan it takes from duet_text.hip.h and the scan / radix
    # instances it takes from duet_prims.hip.h
    own = {n: int(v) for n, v in found if 'sr_' in n or 'scan_spine_u64' in n}
    assert len(own) == 5, found
    assert len(found) >= 5 + 5 and all(int(v) == 0 for _, v in found), found
    with open(asm) as f:
        assert 's_swappc' not in f.read()
