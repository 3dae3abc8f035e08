# coding=utf-8
"""sv_calling/variants.vcf of the svim-gpu mode (--write_sv_calls), CPU side: the marks' read names of the
native extraction, the dialect read back through the repository's VCF readers, the flag's refusals and the name check, and the
gfx950 resource usage of duet_callset.hip's kernels."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from duet_amd import bamio, evaluation, native, read_file, svim_mode, synth
from duet_amd.native import NativeIngest
from duet_amd.read_file import init_chrom_list
from oracle import c_oracle, svim_oracle
from tests import callset_ref
from tests import helpers as H

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def workdir(tmp_path, kind, seed):
    home = str(tmp_path / kind)
    synth.write_svim_workdir(home, H.case_contigs(kind, seed), seed)
    return home, init_chrom_list(False, home)


@pytest.mark.parametrize('kind,seed', [('chr21', 3), ('genome_small', 5)])
def test_mark_names_match_the_rule(tmp_path, kind, seed):
    home, chroms = workdir(tmp_path, kind, seed)
    want = svim_oracle.extract_workdir(home, chroms)
    ing, got = NativeIngest.extract(home + '/snp_phasing/', chroms, thread=2, names=True)
    assert ing is not None, got
    assert np.array_equal(got['pos'], want['pos']) and len(got['pos']) > 100
    assert callset_ref.names_of(got) == want['name']
    if kind == 'genome_small':                      # split-read marks (INV / DUP) carry their read's name too
        assert set(np.unique(got['type']).tolist()) == {0, 1, 2, 3}
    # interned per contig: one pool entry per distinct (contig, read)
    assert len(got['name_off']) - 1 == len(set(zip(got['contig'].tolist(), want['name'])))
    ing.close()
    ing, plain = NativeIngest.extract(home + '/snp_phasing/', chroms, thread=2)
    assert 'mark_name' not in plain and 'name_pool' not in plain
    m = native.IngestMarkNames()
    assert ing.lib.duet_ingest_get_mark_names(ing.handle, ctypes.byref(m)) != native.OK      # no names were kept
    ing.close()


def cpu_callset(home, chroms, depth_bin=1000):
    """The CPU pipeline's candidates (native extraction = the oracle's marks, cluster oracle) and their callset text."""
    ing, got = NativeIngest.extract(home + '/snp_phasing/', chroms, thread=2, min_sv_size=50, names=True)
    ing.close()
    res = c_oracle.cluster(got['contig'], got['type'], got['pos'], got['span'])
    names = callset_ref.names_of(got)
    texts = svim_mode.spelled_contigs(home, chroms)
    text = callset_ref.rows(res, names, got['depth'], got['depth_off'], depth_bin, texts)
    return got, res, names, text


@pytest.mark.parametrize('kind,seed', [('chr21', 3), ('genome_small', 5)])
def test_rows_read_back_through_both_vcf_readers(tmp_path, kind, seed):
    home, chroms = workdir(tmp_path, kind, seed)
    got, res, names, text = cpu_callset(home, chroms)
    svim_mode.write_callset(home, chroms, text.encode())
    vcf = svim_mode.callset_path(home)
    N = len(res['cand_pos'])
    n = np.diff(res['cand_off'].astype(np.int64))
    members = [[names[int(m)] for m in res['order'][res['cand_off'][c]:res['cand_off'][c + 1]]] for c in range(N)]
    texts = svim_mode.spelled_contigs(home, chroms)
    d = np.array([got['depth'][got['depth_off'][k] + min(p // 1000, got['depth_off'][k + 1] - got['depth_off'][k] - 1)]
                  if got['depth_off'][k + 1] > got['depth_off'][k] else 0
                  for k, p in zip(res['cand_contig'].astype(np.int64), res['cand_pos'].astype(np.int64))], dtype=np.int64)
    ref = np.maximum(d - n, 0)
    gt = [callset_ref.genotype(int(a), int(a + b)) for a, b in zip(n, ref)]
    assert {'0/1', '1/1'} <= set(gt)
    tab = read_file.parse_vcf(vcf, False)
    assert len(tab) == N
    assert tab.chrom == [texts[int(k)] for k in res['cand_contig']]
    assert np.array_equal(tab.pos, res['cand_pos'].astype(np.int64))
    assert np.array_equal(tab.svlen_abs, res['cand_span'].astype(np.int64))
    assert tab.svtype == [callset_ref.TYPES[int(t)] for t in res['cand_type']]
    assert np.array_equal(tab.svread, n) and np.array_equal(tab.refread, ref)
    assert tab.names == members and tab.gt == gt
    ing = NativeIngest.load(vcf, home + '/snp_phasing/', chroms, thread=2)
    assert ing is not None and ing.soa is not None, getattr(ing, 'why', None)
    soa = ing.soa
    assert soa.n_cands == N and soa.n_marks == int(n.sum())
    assert np.array_equal(soa.cand_svlen, res['cand_span']) and np.array_equal(soa.cand_svread, n)
    assert np.array_equal(soa.cand_refread, ref) and soa.cand_gt_ok.all()
    assert np.array_equal(np.diff(soa.cand_off.astype(np.int64)), n)
    # READS= joins like the fused pipeline's mark_read: the members' reads in cluster order
    want_read = got['read'][res['order'][:int(n.sum())]] if N else np.zeros(0, np.uint32)
    tagged = want_read != 0xFFFFFFFF
    assert np.array_equal(soa.mark_read != 0xFFFFFFFF, tagged)
    assert np.array_equal(soa.read_tag[soa.mark_read[tagged]], got['read_tag'][want_read[tagged]])
    ing.close()
    # IDs unique (the evaluator counts sets of ids), numbered per contig
    ids = [l.split('\t')[2] for l in text.splitlines()]
    assert len(set(ids)) == N
    assert all(i.startswith('svim_gpu.' + texts[int(k)] + '.') for i, k in zip(ids, res['cand_contig']))


def test_evaluation_keeps_the_called_ins_del_dup_rows(tmp_path):
    home, chroms = workdir(tmp_path, 'genome_small', 5)
    got, res, names, text = cpu_callset(home, chroms)
    assert not any(s in n for n in names for s in ('INS', 'DEL', 'DUP'))
    svim_mode.write_callset(home, chroms, text.encode())
    rows = [l.split('\t') for l in text.splitlines()]
    want = [r for r in rows if r[0].startswith('chr') and r[7].split(';')[0][7:] in ('INS', 'DEL', 'DUP')
            and int(r[7].split(';')[2][6:].lstrip('-')) >= 50 and not r[9].startswith('0/0')]
    assert len(want) > 100 and len(want) < len(rows)
    calls = evaluation.parse_vcf(svim_mode.callset_path(home), True)
    assert [(c['chr'], c['pos']) for c in calls] == [(r[0], int(r[1])) for r in want]
    assert [c['type'] for c in calls] == [{'DUP': 'INS'}.get(r[4][1:-1], r[4][1:-1]) for r in want]


@pytest.mark.parametrize('caller', ['cutesv', 'svim', 'sniffles'])
def test_flag_refused_with_an_external_caller(tmp_path, caller):
    bam, ref = tmp_path / 'x.bam', tmp_path / 'x.fa'
    for f in (bam, ref):
        f.write_bytes(b'')
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bin', 'duet'), str(bam), str(ref), str(tmp_path / 'out'), '-b', caller,
                        '--write_sv_calls'], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, PYTHONPATH=REPO))
    assert r.returncode != 0
    assert '--write_sv_calls works with -b svim-gpu only' in r.stderr
    assert not (tmp_path / 'out').exists()


def test_read_name_with_comma_or_semicolon_fails_before_any_file(tmp_path):
    d = tmp_path / 'snp_phasing'
    d.mkdir()
    lines = ['good\t0\tchr1\t1000\t60\t100M60I100M\t*\t0\t0\t*\t*\tHP:i:1\tPC:i:10\tPS:i:7',
             'bad,name\t0\tchr1\t1010\t60\t100M60I100M\t*\t0\t0\t*\t*\tHP:i:1\tPC:i:10\tPS:i:7']
    bamio.write_bam_from_sam_lines(str(d / 'chr1.bam'), [('chr1', 249250621)], lines)
    with pytest.raises(ValueError, match='bad,name'):
        svim_mode.sv_phasing_from_bams(str(tmp_path), 50, 2, 2, False, 0.9, 0, write_sv_calls=True)
    assert sorted(os.listdir(str(tmp_path))) == ['snp_phasing']


HIPCC = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)


@pytest.mark.skipif(HIPCC is None, reason='hipcc not found')
def test_callset_kernels_use_no_scratch_and_make_no_call(tmp_path):
    csrc = os.path.join(REPO, 'duet_amd', 'csrc')
    asm = str(tmp_path / 'duet_callset.s')
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fvisibility=hidden',
           '-Wno-unused-function', '-I' + os.path.join(REPO, 'include'), '--cuda-device-only', '-S',
           '-Rpass-analysis=kernel-resource-usage', os.path.join(csrc, 'duet_callset.hip'), '-o', asm]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    found = re.findall(r'Function Name: (\S+) \[.*?\n(?:.*\n){0,8}?.*ScratchSize \[bytes/lane\]: (\d+)', r.stderr)
    # its own (cs_*) and the 64-bit spine scan it takes from duet_text.hip.h
    kernels = {n: int(v) for n, v in found if 'cs_' in n or 'scan_spine_u64' in n}
    assert len(kernels) == 6, found
    assert all(v == 0 for v in kernels.values()), kernels
    with open(asm) as f:
        assert 's_swappc' not in f.read()
