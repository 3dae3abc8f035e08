# coding=utf-8
"""-m gpu: the rows of phased_sv.vcf in the svim-gpu mode, sorted and formatted on the device --
duet_svim_phased_rows_device / _host against tests/svim_rows_ref.py byte for byte on hand-made cluster results (no clustering),
the out_cap contract, the refusals, and one real case through the product path.
NOT covered: a text of 4 GiB or more (the 64-bit tile offsets' high word), and the sort beyond 1,024 radix tiles (more than
4,194,304 rows; radix_sort_pairs takes that path unchanged for the VCF mode's 2e7-mark cases)."""
import ctypes
import os

import numpy as np
import pytest

from duet_amd import _lib, engine, svim_mode, synth
from duet_amd.native import NativeIngest
from duet_amd.read_file import init_chrom_list
from tests import helpers as H
from tests import svim_rows_ref
from tests.test_gpu_r2 import fresh_interpreter

pytestmark = pytest.mark.gpu

FIELDS = (('cand_contig', np.uint16), ('cand_type', np.uint8), ('cand_pos', np.uint32), ('cand_span', np.uint32),
          ('pred', np.uint8), ('ps', np.uint32))
CANARY = 0xAB
BIG = 0xFFFFFFFF


@pytest.fixture(scope='module')
def ctx():
    return engine.default_context(0)


def cands(N, seed=1, K=3, **over):
    """N hand-made candidates (random unless given) -> dict of the six arrays."""
    rng = np.random.default_rng(seed)
    a = dict(cand_contig=rng.integers(0, K, N), cand_type=rng.integers(0, 4, N), cand_pos=rng.integers(0, 3_000_000, N),
             cand_span=rng.integers(0, 20000, N), pred=rng.integers(0, 4, N), ps=rng.integers(0, 3_000_000, N))
    a.update(over)
    return {k: np.ascontiguousarray(np.broadcast_to(np.asarray(a[k], dtype=np.int64), (N,)).astype(dt)) for k, dt in FIELDS}


def chrom_array(texts):
    """-> (ctypes array of the texts, n_contigs); a text of None stays a NULL pointer."""
    return (ctypes.c_char_p * max(len(texts), 1))(*[None if t is None else (t if isinstance(t, bytes) else t.encode()) for t in texts])


def bound(a, texts):
    return _lib.phased_rows_bound(int(np.count_nonzero(a['pred'])), [t for t in texts if t is not None])


def host_rows(ctx, texts, a, cap=None, null=None):
    """duet_svim_phased_rows_host, the output pre-filled -> (rc, out_len, n_rows, the whole buffer)."""
    N = len(a['pred'])
    r = _lib.ClusterResult()
    for k in ('cand_contig', 'cand_type', 'cand_pos', 'cand_span'):
        setattr(r, k, None if k == null else a[k].ctypes.data)
    cap = bound(a, texts) if cap is None else cap
    out = np.full(cap + 64, CANARY, dtype=np.uint8)
    n, rows = ctypes.c_uint64(77), ctypes.c_uint32(77)
    rc = ctx.lib.duet_svim_phased_rows_host(ctx.handle, ctypes.byref(r), N, None if null == 'pred' else a['pred'].ctypes.data,
                                            None if null == 'ps' else a['ps'].ctypes.data, len(texts), chrom_array(texts),
                                            out.ctypes.data, ctypes.c_uint64(cap), ctypes.byref(n), ctypes.byref(rows))
    return rc, n.value, rows.value, out


def device_rows(ctx, texts, a, cap=None, null=None, odd=0):
    """duet_svim_phased_rows_device on torch-resident copies; out_text starts `odd` bytes behind 64 canary bytes
    -> (rc, out_len, n_rows, the buffer from out_text on, the 64 + odd bytes in front of it)."""
    import torch
    dev = torch.device('cuda:0')
    keep = {}
    for k, _ in FIELDS:
        t = torch.zeros(a[k].nbytes + 64, dtype=torch.uint8, device=dev)
        if a[k].nbytes:
            t[:a[k].nbytes] = torch.from_numpy(a[k].view(np.uint8).reshape(-1)).to(dev)
        keep[k] = t
    r = _lib.ClusterResult()
    for k in ('cand_contig', 'cand_type', 'cand_pos', 'cand_span'):
        setattr(r, k, None if k == null else keep[k].data_ptr())
    cap = bound(a, texts) if cap is None else cap
    front = 64 + odd
    out = torch.full((front + cap + 64,), CANARY, dtype=torch.uint8, device=dev)
    n, rows = ctypes.c_uint64(77), ctypes.c_uint32(77)
    rc = ctx.lib.duet_svim_phased_rows_device(ctx.handle, ctypes.byref(r), len(a['pred']),
                                              None if null == 'pred' else ctypes.c_void_p(keep['pred'].data_ptr()),
                                              None if null == 'ps' else ctypes.c_void_p(keep['ps'].data_ptr()), len(texts),
                                              chrom_array(texts), ctypes.c_void_p(out.data_ptr() + front), ctypes.c_uint64(cap),
                                              ctypes.byref(n), ctypes.byref(rows),
                                              ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    got = out.cpu().numpy()
    return rc, n.value, rows.value, got[front:], got[:front]


def check_both(ctx, texts, a, odd=0):
    """Both entries against the restatement: the text, out_len, n_rows, and nothing written outside the text."""
    want = svim_rows_ref.rows_of(texts, a)
    n_rows = int(np.count_nonzero(a['pred']))
    assert len(want) <= bound(a, texts)
    rc, n, rows, out = host_rows(ctx, texts, a)
    assert (rc, n, rows) == (0, len(want), n_rows)
    assert out[:n].tobytes() == want and (out[n:] == CANARY).all()
    rc, n, rows, out, front = device_rows(ctx, texts, a, odd=odd)
    assert (rc, n, rows) == (0, len(want), n_rows)
    assert out[:n].tobytes() == want and (out[n:] == CANARY).all() and (front == CANARY).all()
    assert ctx.svim_phased_rows_host(a, texts) == (want, n_rows)
    return want


# around a wavefront (a tile of sr_write), the 2,048-element scan tile, the 4,096-key radix tile, the spine-less scan's 16 tiles
# (32,768), six digits of Duet.<n>
@pytest.mark.parametrize('N', [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 32768, 32769, 100001])
def test_row_counts(ctx, N):
    texts = ['chr1', 'chr2', 'chrX']
    a = cands(N, seed=N, pred=0)
    assert check_both(ctx, texts, a) == b''                                           # nothing kept: zero rows, zero bytes
    want = check_both(ctx, texts, cands(N, seed=N, pred=np.random.default_rng(N).integers(1, 4, N)))      # all kept
    assert want.count(b'\n') == N
    mixed = cands(N, seed=N + 1)
    want = check_both(ctx, texts, mixed, odd=N % 4)
    assert want.count(b'\n') == int(np.count_nonzero(mixed['pred']))


EDGES = sorted(set([0, BIG] + [10 ** k - 1 for k in range(1, 10)] + [10 ** k for k in range(1, 10)]))


def test_digit_boundaries_of_pos_span_and_ps(ctx):
    """every 10^k - 1 / 10^k, 0 and 2^32 - 1 in each number while the others vary; span 0 on every type; the longest row"""
    E = len(EDGES)
    idx = np.arange(3 * E)
    v = np.array(EDGES, dtype=np.int64)
    other = v[(idx * 7 + 3) % E]
    a = cands(3 * E, cand_contig=0, cand_type=idx % 4, pred=1 + idx % 3,
              cand_pos=np.where(idx // E == 0, v[idx % E], other), cand_span=np.where(idx // E == 1, v[idx % E], v[(idx * 5 + 1) % E]),
              ps=np.where(idx // E == 2, v[idx % E], v[(idx * 11 + 2) % E]))
    want = check_both(ctx, ['chr1'], a).decode()
    for e in EDGES:
        assert 'chr1\t%d\t' % e in want and ':%d\n' % e in want and ('SVLEN=%d;' % e in want or 'SVLEN=-%d;' % e in want)
    zero = cands(8, cand_contig=0, cand_type=[0, 1, 2, 3, 0, 1, 2, 3], cand_span=0, pred=[1, 2, 3, 1, 2, 3, 1, 2],
                 cand_pos=[5, 5, 5, 5, 0, 0, 0, 0], ps=0)
    want = check_both(ctx, ['c'], zero).decode()
    assert want.count('SVLEN=0;') == 8 and '-0' not in want
    # the longest row: every number at ten digits, the sign present -- 95 bytes behind CHROM; 1,000,000,000 kept rows are out of
    # reach, so the row number stays short here and has its own test
    long_ = cands(3, cand_contig=0, cand_type=[0, 2, 1], cand_pos=BIG, cand_span=BIG, ps=BIG, pred=3)
    want = check_both(ctx, ['chr1'], long_)
    assert want.startswith(b'chr1\t4294967295\tDuet.1\tN\t<DEL>\t.\tPASS\tSVLEN=-4294967295;SVTYPE=<DEL>\tHP:PS\t1|1:4294967295\n')
    assert len(want.split(b'\n')[0]) + 1 == 4 + 95 - 9


def test_row_numbers_cross_their_digit_counts(ctx):
    """10,001 kept rows (among dropped ones): Duet.9 -> Duet.10, ... Duet.9999 -> Duet.10000"""
    N = 12000
    pred = np.ones(N, dtype=np.int64)
    pred[np.random.default_rng(5).choice(N, N - 10001, replace=False)] = 0
    a = cands(N, seed=3, K=2, pred=pred)
    want = check_both(ctx, ['chr2', 'chr1'], a, odd=1).split(b'\n')
    assert len(want) == 10002
    for n in (1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 10001):
        assert b'\tDuet.%d\t' % n in want[n - 1]


@pytest.mark.parametrize('texts', [['1', '10', '2'], ['chr10', 'chr2', 'chrX'], ['chr11', 'chr1'], ['chr1', '1', 'chr1'],
                                   ['b' * 300, 'a', 'b' * 299], ['chr\xe9', 'chr\xff', 'chrz', 'ch', '中']],
                         ids=['1-10-2', 'chr10-chr2-chrX', 'chr11-chr1', 'equal-texts', '300-bytes', 'high-bytes'])
def test_order_of_the_chrom_texts(ctx, texts):
    """text order against list order; two contigs with one text share a rank (their rows interleave by POS, ties in candidate
    order); a 300-byte CHROM; bytes >= 0x80 (UTF-8 of the str: the same order)"""
    a = cands(700, seed=len(texts[0]), K=len(texts), cand_pos=np.random.default_rng(2).integers(0, 60, 700),
              pred=np.random.default_rng(3).integers(0, 4, 700))
    want = check_both(ctx, texts, a, odd=3)
    first = [l.split(b'\t')[0] for l in want.split(b'\n')[:-1]]
    assert first == sorted(first) and len(set(first)) == len(set(texts))


def test_order_on_3000_contigs(ctx):
    texts = ['ctg%d' % (k * 7919 % 3000) for k in range(3000)]                         # a permutation: text order != list order
    a = cands(20000, seed=9, K=3000, pred=np.random.default_rng(4).integers(0, 4, 20000), cand_pos=np.random.default_rng(5).integers(0, 50, 20000))
    check_both(ctx, texts, a)


def test_ties_stay_in_candidate_order_and_positions_may_descend(ctx):
    # equal (CHROM, POS) across the four types and within one type: told apart by ps only
    N = 600
    a = cands(N, cand_contig=np.arange(N) % 2, cand_pos=np.where(np.arange(N) < 400, 1000, 7), cand_type=np.where(np.arange(N) < 200, np.arange(N) % 4, 1),
              pred=1 + np.arange(N) % 3, ps=np.arange(N), cand_span=50)
    want = check_both(ctx, ['chrB', 'chrA'], a).split(b'\n')[:-1]
    ps = [int(l.rsplit(b':', 1)[1]) for l in want]
    assert ps == [i for c in (1, 0) for p in (7, 1000) for i in range(N) if i % 2 == c and (1000 if i < 400 else 7) == p]
    # positions descending within a contig, contigs descending
    N = 5000
    a = cands(N, cand_contig=(N - 1 - np.arange(N)) // 1700, cand_pos=4_000_000_000 - 3 * np.arange(N), pred=2, ps=np.arange(N))
    want = check_both(ctx, ['x', 'y', 'z'], a).split(b'\n')[:-1]
    assert [int(l.rsplit(b':', 1)[1]) for l in want][:3] == [N - 1, N - 2, N - 3]


def test_out_cap_contract_and_odd_addresses(ctx):
    texts = ['chr1', 'chr2', 'chrX']
    a = cands(3000, seed=8)
    want = svim_rows_ref.rows_of(texts, a)
    n_rows = int(np.count_nonzero(a['pred']))
    rc, n, rows, out = host_rows(ctx, texts, a, cap=len(want))                          # out_cap == out_len works
    assert (rc, n, rows) == (0, len(want), n_rows) and out[:n].tobytes() == want and (out[n:] == CANARY).all()
    rc, n, rows, out = host_rows(ctx, texts, a, cap=len(want) - 1)                      # one byte short: nothing written
    assert rc == _lib.DUET_ERR_INVALID and n == len(want) and (out == CANARY).all()
    assert 'too small' in ctx.last_error()
    for odd in (0, 1, 2, 3):
        rc, n, rows, out, front = device_rows(ctx, texts, a, cap=len(want), odd=odd)
        assert (rc, n, rows) == (0, len(want), n_rows)
        assert out[:n].tobytes() == want and (out[n:] == CANARY).all() and (front == CANARY).all()
        rc, n, rows, out, front = device_rows(ctx, texts, a, cap=len(want) - 1, odd=odd)
        assert rc == _lib.DUET_ERR_INVALID and n == len(want) and (out == CANARY).all() and (front == CANARY).all()


@pytest.mark.parametrize('entry', ['host', 'device'])
def test_refusals(ctx, entry):
    fn = (lambda *args, **kw: host_rows(*args, **kw)[:4]) if entry == 'host' else (lambda *args, **kw: device_rows(*args, **kw)[:4])
    texts = ['chr1', 'chr2']

    def refused(texts_, a, says, **kw):
        rc, n, rows, out = fn(ctx, texts_, a, **kw)
        assert rc == _lib.DUET_ERR_INVALID and (out == CANARY).all(), says
        assert says in ctx.last_error(), ctx.last_error()

    for at in (0, 4999):
        a = cands(5000, seed=2, K=2, pred=1)
        a['pred'][at] = 4
        with pytest.raises(ValueError):
            svim_rows_ref.rows_of(texts, a)
        refused(texts, a, 'pred', cap=600000)
        a = cands(5000, seed=2, K=2, pred=1)
        a['cand_contig'][at] = 2                                                         # == n_contigs
        refused(texts, a, 'contig', cap=600000)
    # a dropped candidate may hold anything
    a = cands(100, seed=2, K=2, pred=np.arange(100) % 2)
    a['cand_contig'][0], a['cand_contig'][2] = 2, 65535
    rc, n, rows, out = fn(ctx, texts, a)
    assert (rc, rows) == (0, 50) and out[:n].tobytes() == svim_rows_ref.rows_of(texts + ['', ''], a)
    a = cands(10, seed=2, K=2, pred=1)
    refused([], a, 'contig count', cap=2000)                                             # n_contigs 0
    refused(['chr1', None], a, 'null CHROM text', cap=2000)
    for null in ('cand_contig', 'cand_type', 'cand_pos', 'cand_span', 'pred', 'ps'):
        refused(texts, a, 'null array', cap=2000, null=null)


def test_a_small_call_after_a_large_one_on_one_context(ctx):
    """the workspace is reused and the status words are stale"""
    texts = ['chr2', 'chr10']
    check_both(ctx, texts, cands(70000, seed=4, K=2, cand_pos=np.random.default_rng(1).integers(0, BIG, 70000)))
    check_both(ctx, texts, cands(5, seed=5, K=2, pred=[0, 1, 0, 2, 3], cand_pos=[9, 8, 7, 6, 5]))
    a = cands(5, seed=5, K=2, pred=4)
    assert host_rows(ctx, texts, a)[0] == _lib.DUET_ERR_INVALID
    check_both(ctx, texts, cands(300, seed=6, K=2))
    check_both(ctx, texts, cands(7, seed=7, K=2, pred=0))


def test_the_fused_run_and_the_product_path(ctx, tmp_path, monkeypatch):
    from duet_amd.devmem import DeviceSvim
    home = str(tmp_path / 'w')
    synth.write_svim_workdir(home, H.case_contigs('genome_small', 5), 5)
    chroms = init_chrom_list(False, home)
    texts = svim_mode.spelled_contigs(home, chroms)
    ing, got = NativeIngest.extract(home + '/snp_phasing/', chroms, thread=2, min_sv_size=50)
    assert ing is not None, got
    ing.close()
    ds = DeviceSvim(got, got['read_tag'], got['depth'], got['depth_off'], 1000, 50, 2, device='cuda:0')
    want = None
    for wait in (True, False):
        ds.run_fused(ctx, wait=wait)
        rows, n_rows = ds.phased_rows(ctx, texts)
        res = ds.fetch()
        want = svim_mode.rows_text(home, dict(res, chroms=chroms)).encode()
        assert rows.tobytes() == want and n_rows == int(np.count_nonzero(res['pred'])) > 100
    head = svim_mode.header_text(home, chroms).encode()

    def refuse(*a, **k):
        raise AssertionError('rows_text is not part of the product path')
    monkeypatch.setattr(svim_mode, 'rows_text', refuse)
    for flag in (False, True):
        svim_mode.sv_phasing_from_bams(home, 50, 2, 4, False, 0.9, 0, write_sv_calls=flag)
        assert open(home + '/phased_sv.vcf', 'rb').read() == head + want, flag
    # two ranks (plumbing mode: both on device 0) from a fresh interpreter: rank 0 formats the merged records on its context
    os.remove(home + '/phased_sv.vcf')
    r = fresh_interpreter('from duet_amd import svim_mode\nsvim_mode.sv_phasing_from_bams(%r, 50, 2, 4, False, 0.9, 0, gpus=2)\n' % home,
                          {'DUET_ONE_GPU': '1'})
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert open(home + '/phased_sv.vcf', 'rb').read() == head + want
