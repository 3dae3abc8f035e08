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


def host_rows(ctx, res, n_marks, names, depth, depth_off, depth_bin, texts, cap=None):
    """duet_svim_vcf_rows_host on the given host arrays, the output pre-filled -> (rc, out_len, the whole buffer)."""
    arr = {k: np.ascontiguousarray(res[k], dtype=dt) for k, dt in (
        ('order', np.uint32), ('cand_off', np.uint32), ('cand_contig', np.uint16), ('cand_type', np.uint8),
        ('cand_pos', np.uint32), ('cand_span', np.uint32))}
    r = _lib.ClusterResult()
    for k in arr:
        setattr(r, k, arr[k].ctypes.data)
    depth = np.ascontiguousarray(depth, dtype=np.uint32)
    depth_off = np.ascontiguousarray(depth_off, dtype=np.uint32)
    p = _lib.SvimProblem()
    p.marks.n_marks = int(n_marks)
    p.n_contigs = len(depth_off) - 1
    p.depth = depth.ctypes.data if depth.size else None
    p.depth_off, p.depth_bin = depth_off.ctypes.data, int(depth_bin)
    hold = []
    name_off = np.ascontiguousarray(names['name_off'], dtype=np.uint64)
    nm = _lib.callset_names(np.ascontiguousarray(names['mark_name'], dtype=np.uint32), name_off,
                            np.ascontiguousarray(names['name_pool'], dtype=np.uint8), texts, hold)
    nm.n_names = len(name_off) - 1
    N = len(arr['cand_pos'])
    cap = _lib.callset_bound(N, n_marks, name_off, texts) if cap is None else cap
    out = np.full(max(cap, 1) + 64, 0xAB, dtype=np.uint8)
    n = ctypes.c_uint64(0)
    rc = ctx.lib.duet_svim_vcf_rows_host(ctx.handle, ctypes.byref(p), ctypes.byref(r), N, ctypes.byref(nm), out.ctypes.data,
                                         ctypes.c_uint64(cap), ctypes.byref(n))
    return rc, n.value, out


def check_both(ctx, res, got, texts, depth_bin=1000):
    want = callset_ref.rows(res, callset_ref.names_of(got), got['depth'], got['depth_off'], depth_bin, texts).encode()
    M = len(got['mark_name'])
    # the bound a caller allocates (include/duet_ef.h) holds the text
    assert len(want) <= _lib.callset_bound(len(res['cand_pos']), M, got['name_off'], texts)
    host = ctx.svim_vcf_rows_host(res, M, got['mark_name'], got['name_off'], got['name_pool'], got['depth'], got['depth_off'],
                                  depth_bin, texts)
    assert host == want
    rc, n, out = host_rows(ctx, res, M, got, got['depth'], got['depth_off'], depth_bin, texts)
    assert rc == 0 and n == len(want)
    assert out[:n].tobytes() == want and (out[n:] == 0xAB).all()
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


# ---------------------------------------------------------------------------------------------------------------------------
# The rows at their extremes: hand-made cluster results (duet_svim_vcf_rows_* take any), no clustering.  Sizes covered: members
# per row around cs_write's rounds of 64 names, name lengths around its 64-lane copy steps, numbers at digit boundaries, row
# counts around kCsTile and the 32768-row step of the 8192-workgroup grid-stride loop.  NOT covered: a text of 4 GiB or more
# (the 64-bit scan's high word, flag bit 1) -- it costs too much memory and time for this suite.
# ---------------------------------------------------------------------------------------------------------------------------

def handmade(members, names, name_of=None, contig=None, types=None, pos=None, span=None, depth=None, depth_off=None, K=1, seed=1):
    """Rows of members[i] marks each -> (res, got).  names: the read-name table (bytes); name_of(i, j) -> the name index of row
    i's j-th member (default: round robin); order is a shuffle of the raw marks, so that the rows depend on it."""
    rng = np.random.default_rng(seed)
    members = np.asarray(members, dtype=np.int64)
    N, M = len(members), int(members.sum())
    off = np.concatenate([[0], np.cumsum(members)])
    order = rng.permutation(M).astype(np.uint32)
    by_slot = np.arange(M) % max(len(names), 1) if name_of is None else \
        np.array([name_of(i, j) for i in range(N) for j in range(int(members[i]))], dtype=np.int64)
    mark_name = np.zeros(M, dtype=np.uint32)
    mark_name[order] = by_slot                                  # slot s of the cluster order holds raw mark order[s]
    lens = np.array([len(x) for x in names], dtype=np.uint64)
    got = dict(mark_name=mark_name, name_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64),
               name_pool=np.frombuffer(b''.join(names) + b'\0', dtype=np.uint8).copy()[:-1] if sum(map(len, names)) else np.zeros(0, np.uint8),
               depth=np.asarray([30] * 8 if depth is None else depth, dtype=np.uint32),
               depth_off=np.asarray([0] + [8] * K if depth_off is None else depth_off, dtype=np.uint32))
    res = dict(order=order, cand_off=off.astype(np.uint32),
               cand_contig=np.asarray(np.zeros(N) if contig is None else contig, dtype=np.uint16),
               cand_type=np.asarray(np.arange(N) % 4 if types is None else types, dtype=np.uint8),
               cand_pos=np.asarray(1000 + 10 * np.arange(N) if pos is None else pos, dtype=np.uint32),
               cand_span=np.asarray(50 + np.arange(N) % 700 if span is None else span, dtype=np.uint32))
    return res, got


NAMES = [b'rd%d_%x' % (i, i * 2654435761 % 1000003) for i in range(300)]           # 5-14 bytes


@pytest.mark.parametrize('n', [1, 63, 64, 65, 127, 128, 129, 200, 1000])
def test_extreme_members_per_row(ctx, n):
    """the header does not limit a row to part_max members: cs_write places the names 64 at a time"""
    res, got = handmade([3, n, 2, n, 1], NAMES, seed=n)
    want = check_both(ctx, res, got, ['chr1'])
    assert want.count(b'\n') == 5 and want.split(b'\n')[1].count(b',') == n      # (n - 1 between the names, one in AD)
    if n == 1000:
        # out_cap one byte short on the largest row: nothing written, DUET_ERR_INVALID, the exact size reported -- by both entries
        M = len(got['mark_name'])
        for fn in (host_rows, device_rows):
            rc, size, out = fn(ctx, res, M, got, got['depth'], got['depth_off'], 1000, ['chr1'], cap=len(want) - 1)
            assert rc == _lib.DUET_ERR_INVALID and size == len(want) and (out == 0xAB).all(), fn.__name__


@pytest.mark.parametrize('L', [0, 1, 63, 64, 65, 300])
def test_extreme_name_lengths(ctx, L):
    """names of L bytes between ordinary ones: the copy loops stride 64 lanes"""
    names = NAMES[:7] + [bytes(97 + (i + k) % 26 for i in range(L)) for k in range(3)]
    res, got = handmade([1, 2, 5, 70, 3], names, name_of=lambda i, j: (7 + j % 3) if (i + j) % 2 == 0 else j % 7, seed=L)
    check_both(ctx, res, got, ['chr1'])


def test_extreme_rows_of_empty_and_repeated_names(ctx):
    names = [b'', b'ab', b'', b'read_twice']
    pick = {0: lambda j: 0, 1: lambda j: 2 * (j % 2), 2: lambda j: 3, 3: lambda j: (0, 3, 3, 1, 0)[j % 5], 4: lambda j: 0}
    res, got = handmade([1, 66, 2, 130, 5], names, name_of=lambda i, j: pick[i](j))
    want = check_both(ctx, res, got, ['chr1']).split(b'\n')
    assert b';READS=\t' in want[0] and b';READS=' + b',' * 65 + b'\t' in want[1] and b';READS=,,,,\t' in want[4]
    assert b';READS=read_twice,read_twice\t' in want[2]


def test_extreme_numbers_at_digit_boundaries(ctx):
    big = 0xFFFFFFFF
    pos = [0, 9, 10, 999999999, 1000000000, big, big, 5, 5]
    span = [50, 50, 50, 50, 50, big, big, 0, 0]
    types = [0, 1, 2, 3, 0, 0, 1, 0, 1]
    res, got = handmade([2] * 9, NAMES, pos=pos, span=span, types=types)
    want = check_both(ctx, res, got, ['chr1']).split(b'\n')
    assert want[5].startswith(b'chr1\t4294967295\t') and b';END=8589934590;SVLEN=-4294967295;' in want[5]
    assert b';END=4294967295;SVLEN=4294967295;' in want[6]
    assert b'<DEL>' in want[7] and b';SVLEN=0;' in want[7] and b';SVLEN=0;' in want[8]
    assert want[0].startswith(b'chr1\t0\t') and b';END=50;SVLEN=-50;' in want[0]


def test_extreme_row_numbers_cross_their_digit_counts(ctx):
    """9 -> 10, 99 -> 100, 99999 -> 100000 within one contig; the numbering restarts on the next occupied contig behind empty ones"""
    N0 = 100003
    contig = [0] * N0 + [3] * 12 + [4]
    res, got = handmade([1] * len(contig), NAMES[:5], contig=contig, K=6)
    want = check_both(ctx, res, got, ['c%d' % k for k in range(6)]).split(b'\n')
    for i in (9, 10, 99, 100, 99999, 100000, N0):
        assert b'\tsvim_gpu.c0.%d\t' % i in want[i - 1]
    assert b'\tsvim_gpu.c3.1\t' in want[N0] and b'\tsvim_gpu.c3.10\t' in want[N0 + 9] and b'\tsvim_gpu.c4.1\t' in want[N0 + 12]


def test_extreme_genotype_boundaries(ctx):
    """(n, depth): 5n against 4 DP and against DP, one below / on / one above; depth below n, equal to n, 2^32 - 1"""
    pairs = [(3, 4, b'0/1'), (4, 5, b'1/1'), (5, 6, b'1/1'),                   # 5n = 4 DP - 1, 4 DP, 4 DP + 1
             (1, 6, b'0/0'), (1, 5, b'0/1'), (1, 4, b'0/1'),                   # 5n = DP - 1, DP, DP + 1
             (7, 9, b'0/1'), (8, 10, b'1/1'), (9, 11, b'1/1'), (2, 11, b'0/0'), (2, 10, b'0/1'), (2, 9, b'0/1'),
             (5, 2, b'1/1'), (5, 5, b'1/1'), (5, 0, b'1/1'), (3, 0xFFFFFFFF, b'0/0'), (64, 80, b'1/1'), (63, 79, b'0/1')]
    for n, d, gt in pairs:                                                     # (the table itself, by the rule of the header)
        dp = n + max(d - n, 0)
        assert gt == (b'1/1' if 5 * n >= 4 * dp else (b'0/1' if 5 * n >= dp else b'0/0'))
    res, got = handmade([n for n, _, _ in pairs], NAMES, pos=[7 * i + 3 for i in range(len(pairs))],
                        depth=[d for _, d, _ in pairs], depth_off=[0, len(pairs)])
    want = check_both(ctx, res, got, ['chr1'], depth_bin=7).split(b'\n')
    for i, (n, d, gt) in enumerate(pairs):
        dp = max(n, d)
        assert want[i].endswith(b'\tGT:DP:AD\t%s:%d:%d,%d' % (gt, dp, dp - n, n)), (i, want[i][-40:])


@pytest.mark.parametrize('depth_bin', [1, 7, 0xFFFFFFFF])
def test_extreme_depth_bins(ctx, depth_bin):
    """bins of 1 bp, 7 bp and 2^32 - 1 bp; POS / depth_bin beyond the contig's bins (the last bin counts); a contig without bins"""
    nb = [5, 0, 3, 1]
    depth = [11, 12, 13, 14, 99, 21, 22, 77, 55]
    contig = [0] * 6 + [1] * 2 + [2] * 4 + [3] * 2
    pos = [0, depth_bin - 1, depth_bin, 4 * min(depth_bin, 1 << 29), 5 * min(depth_bin, 1 << 29), 0xFFFFFFFF, 0, 0xFFFFFFFF,
           0, 2 * min(depth_bin, 1 << 30), 3 * min(depth_bin, 1 << 30), 0xFFFFFFFF, 0, 0xFFFFFFFF]
    res, got = handmade([2] * len(contig), NAMES, contig=contig, pos=pos, depth=depth, depth_off=np.concatenate([[0], np.cumsum(nb)]),
                        K=4)
    want = check_both(ctx, res, got, ['a', 'b', 'c', 'd'], depth_bin=depth_bin).split(b'\n')
    wide = depth_bin == 0xFFFFFFFF                                               # (POS 2^32 - 1 is then in bin 1)
    assert want[5].endswith(b':12:10,2' if wide else b':99:97,2')                # beyond contig a's five bins: its last one
    assert want[6].endswith(b'1/1:2:0,2') and want[7].endswith(b'1/1:2:0,2')     # contig b has no bins
    assert want[11].endswith(b':22:20,2' if wide else b':77:75,2') and want[13].endswith(b':55:53,2')


def test_extreme_chrom_texts(ctx):
    texts = ['', 'x', 'c' * 64, 'd' * 65, 'e' * 200, 'unused']
    contig = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    res, got = handmade([1, 2, 3, 64, 65, 1, 2, 3, 4, 5], NAMES, contig=contig, K=6)
    want = check_both(ctx, res, got, texts).split(b'\n')
    assert want[0].startswith(b'\t1000\tsvim_gpu..1\t') and want[9].startswith(b'e' * 200 + b'\t1090\tsvim_gpu.' + b'e' * 200 + b'.2\t')


@pytest.mark.parametrize('N', [1, 2047, 2048, 2049, 32768, 32769, 40000])
def test_extreme_row_counts(ctx, N):
    """short rows across kCsTile (2048 rows per scan tile) and the 32768 rows one sweep of cs_write's 8192 workgroups takes"""
    rng = np.random.default_rng(N)
    contig = np.sort(rng.integers(0, 3, N))
    res, got = handmade(1 + (np.arange(N) % 3 == 0), NAMES[:50], contig=contig, K=3, seed=N)
    want = check_both(ctx, res, got, ['chr1', 'chr2', 'chrX'])
    assert want.count(b'\n') == N


def test_extreme_type_code_4_is_refused_by_both_entries(ctx):
    for at in (0, 2500):
        types = np.arange(3000) % 4
        res, got = handmade([1] * 3000, NAMES[:9], types=types)
        res['cand_type'][at] = 4
        with pytest.raises(ValueError):
            callset_ref.rows(res, callset_ref.names_of(got), got['depth'], got['depth_off'], 1000, ['chr1'])
        M = len(got['mark_name'])
        for fn in (host_rows, device_rows):
            rc, n, out = fn(ctx, res, M, got, got['depth'], got['depth_off'], 1000, ['chr1'])
            assert rc == _lib.DUET_ERR_INVALID and (out == 0xAB).all(), (fn.__name__, at)
