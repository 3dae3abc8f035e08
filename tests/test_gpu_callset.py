# coding=utf-8
"""-m gpu: sv_calling/variants.vcf of the svim-gpu mode (--write_sv_calls) -- the rows kernels
(duet_svim_vcf_rows_device / _host) against tests/callset_ref.py byte for byte, the out_cap contract, the round trip through the
VCF path, and the sharded run."""
import ctypes
import os
import shutil

import numpy as np
import pytest

from duet_amd import _lib, engine, svim_mode, synth
from duet_amd.native import NativeIngest
from duet_amd.read_file import init_chrom_list
from oracle import c_oracle
from tests import callset_ref
from tests import helpers as H
from tests.test_gpu_r2 import fresh_interpreter

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    return engine.default_context(0)


def device_rows(ctx, res, n_marks, names, depth, depth_off, depth_bin, texts, cap=None):
    """duet_svim_vcf_rows_device on torch-resident copies of the given host arrays -> (rc, out_len, text bytes or None)."""
    import torch
    dev = torch.device('cuda:0')
    keep = []

    def up(a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        t = torch.zeros(a.nbytes + 64, dtype=torch.uint8, device=dev)
        if a.nbytes:
            t[:a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1)).to(dev)
        keep.append(t)
        return t.data_ptr()

    r = _lib.ClusterResult()
    for k, dt in (('order', np.uint32), ('cand_off', np.uint32), ('cand_contig', np.uint16), ('cand_type', np.uint8),
                  ('cand_pos', np.uint32), ('cand_span', np.uint32)):
        setattr(r, k, up(res[k], dt))
    depth_off = np.ascontiguousarray(depth_off, dtype=np.uint32)
    p = _lib.SvimProblem()
    p.marks.n_marks = n_marks
    p.n_contigs = len(depth_off) - 1
    p.depth, p.depth_off, p.depth_bin = up(depth, np.uint32), depth_off.ctypes.data, depth_bin
    hold = []
    nm = _lib.callset_names(up(names['mark_name'], np.uint32), up(names['name_off'], np.uint64), up(names['name_pool'], np.uint8),
                            texts, hold)
    nm.n_names = len(names['name_off']) - 1
    N = len(res['cand_pos'])
    bound = _lib.callset_bound(N, n_marks, names['name_off'], texts)
    cap = bound if cap is None else cap
    out = torch.full((max(cap, 1) + 64,), 0xAB, dtype=torch.uint8, device=dev)
    n = ctypes.c_uint64(0)
    rc = ctx.lib.duet_svim_vcf_rows_device(ctx.handle, ctypes.byref(p), ctypes.byref(r), N, ctypes.byref(nm), ctypes.c_void_p(out.data_ptr()),
                                           ctypes.c_uint64(cap), ctypes.byref(n), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    return rc, n.value, out.cpu().numpy()


def extracted(home, chroms):
    ing, got = NativeIngest.extract(home + '/snp_phasing/', chroms, thread=2, min_sv_size=50, names=True)
    assert ing is not None, got
    ing.close()
    return got


def check_both(ctx, res, got, texts, depth_bin=1000):
    want = callset_ref.rows(res, callset_ref.names_of(got), got['depth'], got['depth_off'], depth_bin, texts).encode()
    M = len(got['mark_name'])
    host = ctx.svim_vcf_rows_host(res, M, got['mark_name'], got['name_off'], got['name_pool'], got['depth'], got['depth_off'],
                                  depth_bin, texts)
    assert host == want
    rc, n, out = device_rows(ctx, res, M, got, got['depth'], got['depth_off'], depth_bin, texts)
    assert rc == 0 and n == len(want)
    assert out[:n].tobytes() == want and (out[n:] == 0xAB).all()
    return want


@pytest.mark.parametrize('kind,seed', [('chr21', 3), ('genome_small', 5)])
def test_rows_equal_the_reference_on_the_cpu_pipelines_candidates(ctx, tmp_path, kind, seed):
    home = str(tmp_path / kind)
    synth.write_svim_workdir(home, H.case_contigs(kind, seed), seed)
    chroms = init_chrom_list(False, home)
    got = extracted(home, chroms)
    res = c_oracle.cluster(got['contig'], got['type'], got['pos'], got['span'])
    if kind == 'genome_small':
        assert set(np.unique(res['cand_type']).tolist()) == {0, 1, 2, 3}
    want = check_both(ctx, res, got, svim_mode.spelled_contigs(home, chroms))
    # out_cap one byte short: nothing written, DUET_ERR_INVALID, the exact size reported
    M = len(got['mark_name'])
    rc, n, out = device_rows(ctx, res, M, got, got['depth'], got['depth_off'], 1000, svim_mode.spelled_contigs(home, chroms),
                             cap=len(want) - 1)
    assert rc == _lib.DUET_ERR_INVALID and n == len(want) and (out == 0xAB).all()


def synthetic(n_marks, contigs_with_marks, K, seed, bins_on=None):
    """Raw marks on a few of K contigs with synthetic names; depth bins only on the contigs in bins_on."""
    rng = np.random.default_rng(seed)
    k = np.sort(rng.choice(np.array(contigs_with_marks), n_marks)).astype(np.uint16)
    t = rng.integers(0, 4, n_marks).astype(np.uint8)
    pos = rng.integers(1, 5_000_000, n_marks).astype(np.uint32)
    span = rng.integers(50, 3000, n_marks).astype(np.uint32)
    n_reads = max(n_marks // 5, 1)
    pool = b''.join(b'rd%d_%x' % (i, i * 2654435761 % 1000003) for i in range(n_reads))
    lens = np.array([len(b'rd%d_%x' % (i, i * 2654435761 % 1000003)) for i in range(n_reads)], dtype=np.uint64)
    name_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    mark_name = rng.integers(0, n_reads, n_marks).astype(np.uint32)
    bins_on = set(contigs_with_marks if bins_on is None else bins_on)
    counts = [5000 if kk in bins_on else 0 for kk in range(K)]
    depth_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    depth = rng.integers(0, 60, int(depth_off[-1])).astype(np.uint32)
    return dict(contig=k, type=t, pos=pos, span=span, read=np.full(n_marks, 0xFFFFFFFF, np.uint32), mark_name=mark_name,
                name_off=name_off, name_pool=np.frombuffer(pool, dtype=np.uint8).copy(), depth=depth, depth_off=depth_off,
                read_tag=np.zeros(0, np.uint64))


def test_rows_on_contigs_without_marks_or_bins(ctx):
    K = 24
    got = synthetic(3000, [2, 19], K, 7, bins_on=[2])
    res = c_oracle.cluster(got['contig'], got['type'], got['pos'], got['span'])
    texts = ['chr%d' % (k + 1) for k in range(K)]
    want = check_both(ctx, res, got, texts)
    assert ':0,' in want.decode()                     # contig 20 has no bins: ref 0


def test_two_million_marks_against_the_device_cluster_result(ctx):
    """>= 2e6 raw marks: the length scan takes more than one level; the text against the reference on the device's own clusters."""
    from duet_amd.devmem import DeviceSvim
    K = 24
    got = synthetic(2_100_000, list(range(K)), K, 11)
    texts = ['chr%d' % (k + 1) for k in range(K)]
    ds = DeviceSvim(got, got['read_tag'], got['depth'], got['depth_off'], 1000, 50, 2, device='cuda:0')
    ds.run_fused(ctx)
    text = ds.vcf_rows(ctx, got, texts).tobytes()
    res = ds.fetch()
    assert len(res['cand_pos']) > 2048 * 2
    want = callset_ref.rows(res, callset_ref.names_of(got), got['depth'], got['depth_off'], 1000, texts).encode()
    assert text == want


def data_rows(path, drop_id=False):
    rows = [l for l in open(path).read().split('\n') if l and not l.startswith('#')]
    if drop_id:
        rows = [l.split('\t', 3)[0:2] + l.split('\t', 3)[3:] for l in rows]
    return rows


def test_round_trip_through_the_vcf_path_and_sharded_run(ctx, tmp_path):
    from duet_amd import tune
    from duet_amd.sv_phasing import sv_phasing
    home = str(tmp_path / 'w')
    synth.write_svim_workdir(home, H.case_contigs('genome_small', 5), 5)
    # without the flag: no sv_calling/ directory
    svim_mode.sv_phasing_from_bams(home, 50, 2, 4, False, 0.9, 0)
    assert not os.path.exists(os.path.join(home, 'sv_calling'))
    plain = open(home + '/phased_sv.vcf', 'rb').read()
    svim_mode.sv_phasing_from_bams(home, 50, 2, 4, False, 0.9, 0, write_sv_calls=True)
    assert open(home + '/phased_sv.vcf', 'rb').read() == plain             # byte-for-byte what it is without the flag
    calls = open(svim_mode.callset_path(home), 'rb').read()
    # the fused run's (pred, ps) per candidate, in the callset's order
    chroms = init_chrom_list(False, home)
    got = extracted(home, chroms)
    from duet_amd.devmem import DeviceSvim
    ds = DeviceSvim(got, got['read_tag'], got['depth'], got['depth_off'], 1000, 50, 2, device='cuda:0')
    ds.run_fused(ctx)
    fused = ds.fetch()
    assert calls.count(b'\n') - calls.count(b'\n#') - 1 == len(fused['pred'])
    # VCF path on a copy of the work directory
    home2 = str(tmp_path / 'w2')
    shutil.copytree(home, home2)
    os.remove(home2 + '/phased_sv.vcf')
    cands = tune.features(home2)
    pred, ps = tune.apply(cands, tune.vector())
    assert np.array_equal(pred, fused['pred']) and np.array_equal(ps, fused['ps'])
    sv_phasing(home2, 50, 2, 4, False)
    a, b = open(home + '/phased_sv.vcf').read(), open(home2 + '/phased_sv.vcf').read()
    head = lambda t: [l for l in t.split('\n') if l.startswith('#')]
    assert head(a) == head(b)
    assert sorted(data_rows(home + '/phased_sv.vcf', True)) == sorted(data_rows(home2 + '/phased_sv.vcf', True))
    keys = [tuple(r.split('\t')[:2]) for r in data_rows(home + '/phased_sv.vcf')]
    if len(set(keys)) == len(keys):
        assert a == b
    # the same through two ranks (plumbing mode: both on device 0): byte-identical callset, no part files left
    os.remove(svim_mode.callset_path(home))
    r = fresh_interpreter('from duet_amd import svim_mode\nsvim_mode.sv_phasing_from_bams(%r, 50, 2, 4, False, 0.9, 0, gpus=2, '
                          'write_sv_calls=True)\n' % home, {'DUET_ONE_GPU': '1'})
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert open(svim_mode.callset_path(home), 'rb').read() == calls
    assert open(home + '/phased_sv.vcf', 'rb').read() == plain
    assert sorted(os.listdir(os.path.join(home, 'sv_calling'))) == ['variants.vcf']
