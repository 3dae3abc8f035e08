# coding=utf-8
"""-m gpu: the joined phase sets (duet_amd/csrc/duet_psjoin.hip) against tests/ps_join_ref.py, byte for byte: the remap of the read
tags and the change codes at the smallest shapes at which each can go wrong, the contracts of the four entries, the joined run
against the C oracle on the reference-remapped problem, and `duet --join_ps` in both modes.

pj_tags takes 256 reads per workgroup and copies a contig's slice of the table into LDS when the workgroup's reads lie in one
contig and the slice holds at most LDS_SLICE keys: the shapes below sit on both sides of each of those edges."""
import ctypes
import os
import shutil
import sys

import numpy as np
import pytest

from duet_amd import _lib, engine, ps_join, ps_links, svim_mode, synth, tune
from duet_amd.read_file import init_chrom_list
from oracle import c_oracle
from tests import helpers as H
from tests import pc_cap_ref, soa_fuzz, tune_ref
from tests import ps_join_ref as J
from tests import ps_links_ref as L

pytestmark = pytest.mark.gpu

BT = _lib.PS_BLOCK_DTYPE
UNTAGGED = J.UNTAGGED
LDS_SLICE = 2048                # kLdsSlice of duet_psjoin.hip
TILE = 256                      # kThreads
SEEDS = tuple(range(1, 9))
INVALID = _lib.DUET_ERR_INVALID


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def tag(hap, pc, ps):
    return (hap << 62) | (pc << 32) | ps


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros(8, dtype=torch.uint8, device='cuda:0')
    return torch.from_numpy(a.view(np.uint8).copy()).to('cuda:0')


def back(t, dtype, n):
    return t.cpu().numpy()[:n * np.dtype(dtype).itemsize].view(dtype).copy()


def check_tags(ctx, words, read_off, rows):
    """Reference against _host and _device, each into a second array and in place; -> (remapped words, n_changed)."""
    import torch
    words = np.ascontiguousarray(words, dtype=np.uint64)
    table = ps_join.table(rows)
    want, n_want = J.remap(words, read_off, rows)
    out, n = ctx.ps_join_tags_host(words, read_off, table)
    assert out.tobytes() == want.tobytes() and n == n_want
    same = words.copy()
    out, n = ctx.ps_join_tags_host(same, read_off, table, out=same)
    assert out is same and same.tobytes() == want.tobytes() and n == n_want
    src, dst = dev(words), dev(np.full(len(words), 0xABABABABABABABAB, dtype=np.uint64))
    n = ctx.ps_join_tags_device(src.data_ptr(), read_off, len(words), table, dst.data_ptr())
    torch.cuda.synchronize()
    assert back(dst, np.uint64, len(words)).tobytes() == want.tobytes() and n == n_want
    assert back(src, np.uint64, len(words)).tobytes() == words.tobytes()
    n = ctx.ps_join_tags_device(src.data_ptr(), read_off, len(words), table, src.data_ptr())
    torch.cuda.synchronize()
    assert back(src, np.uint64, len(words)).tobytes() == want.tobytes() and n == n_want
    return want, n_want


def random_words(rng, read_off, rows, ps_pool):
    """Tag words whose PS come from ps_pool (some in the table of their contig, some not), every hap, a few untagged."""
    R = int(read_off[-1])
    hap = rng.integers(0, 4, R).astype(np.uint64)
    pc = rng.integers(0, 1 << 30, R).astype(np.uint64)
    ps = np.asarray(ps_pool, dtype=np.uint64)[rng.integers(0, len(ps_pool), R)]
    words = (hap << np.uint64(62)) | (pc << np.uint64(32)) | ps
    words[rng.integers(0, 7, R) == 0] = UNTAGGED
    return words


POOL = (0, 1, 5, 20, 21, 22, 40000, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF)


def small_rows(K):
    rows = []
    for k in range(K):
        rows += [(k, 0, 0xFFFFFFFF, 1), (k, 5, 1 + k, 0), (k, 20, 5, 1), (k, 22, 5, 0), (k, 0x80000000, 0x7FFFFFFF, 1),
                 (k, 0xFFFFFFFF, 3, 1)][k % 2:]                          # (odd contigs lack the row of PS 0)
    return rows


# ---- the remap ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('R', [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_tags_one_contig(ctx, R):
    rng = np.random.default_rng(100 + R)
    words = random_words(rng, [0, R], small_rows(1), POOL)
    got, n = check_tags(ctx, words, [0, R], small_rows(1))
    if R >= 63:
        assert 0 < n < R
    for n_blocks in (0, 1):
        check_tags(ctx, words, [0, R], small_rows(1)[1:1 + n_blocks])


@pytest.mark.parametrize('read_off', [[0, 0, 300, 300, 700], [0, 130, 130, 600, 600], [0, 0, 0, 0, 257], [0, 1, 2, 3, 4],
                                      [0, 255, 256, 257, 1025], [0, 256, 512, 512, 768]])
def test_tags_four_contigs_empty_ones_and_straddled_tiles(ctx, read_off):
    """An empty first, middle and last contig; contig boundaries inside a tile of 256 reads and exactly on its edge."""
    rng = np.random.default_rng(sum(read_off))
    rows = small_rows(4)
    words = random_words(rng, read_off, rows, POOL)
    check_tags(ctx, words, read_off, rows)
    # one PS value on two contigs, with different blocks
    words[:] = tag(1, 7, 5)
    got, _ = check_tags(ctx, words, read_off, rows)
    for k in range(4):
        assert all(int(w) & 0xFFFFFFFF == 1 + k for w in got[read_off[k]:read_off[k + 1]])


@pytest.mark.parametrize('n_keys', [1, 2, LDS_SLICE - 1, LDS_SLICE, LDS_SLICE + 1])
def test_tags_slice_sizes_around_the_lds_threshold(ctx, n_keys):
    """Contig 1's slice holds n_keys keys 10, 20, 30, ..; its reads fill whole tiles (the LDS copy, or the bisection in global
    memory above the threshold) and share one tile with contig 0 and one with contig 2 (always global memory).  The reads ask for
    the first key, the last key, a value between two keys, one below the first and one above the last."""
    keys = [10 * (i + 1) for i in range(n_keys)]
    rows = [(0, 10, 9, 1)] + [(1, ps, ps // 10, i & 1) for i, ps in enumerate(keys)] + [(2, keys[-1], 1, 1)]
    read_off = [0, 100, 100 + 3 * TILE, 100 + 3 * TILE + 60]
    rng = np.random.default_rng(n_keys)
    asked = [keys[0], keys[-1], keys[n_keys // 2], keys[n_keys // 2] + 5, 5, keys[-1] + 5, 10]
    words = random_words(rng, read_off, rows, asked)
    got, n = check_tags(ctx, words, read_off, rows)
    assert n > 100


def test_tags_by_hand(ctx):
    rows = [(0, 20, 10, 1), (1, 20, 5, 0), (1, 0xFFFFFFFF, 7, 1)]
    pc = (1 << 30) - 2
    words = [tag(1, 3, 20), tag(2, pc, 20), tag(3, 9, 20), tag(0, 9, 20), tag(1, 3, 21), UNTAGGED,
             tag(1, 3, 20), tag(2, 0, 0xFFFFFFFF), UNTAGGED, tag(1, 3, 5)]
    got, n = check_tags(ctx, words, [0, 6, 10], rows)
    assert [int(x) for x in got] == [tag(2, 3, 10), tag(1, pc, 10), tag(3, 9, 10), tag(0, 9, 10), tag(1, 3, 21), UNTAGGED,
                                     tag(1, 3, 5), tag(1, 0, 7), UNTAGGED, tag(1, 3, 5)] and n == 6
    # PS 0 and PS 0xFFFFFFFF as keys and as blocks
    got, n = check_tags(ctx, [tag(1, 1, 0), tag(2, 1, 0xFFFFFFFF), UNTAGGED], [0, 3], [(0, 0, 0xFFFFFFFF, 1), (0, 0xFFFFFFFF, 0, 1)])
    assert [int(x) for x in got] == [tag(2, 1, 0xFFFFFFFF), tag(1, 1, 0), UNTAGGED] and n == 2


def tags_raw(ctx, words, read_off, K, R, table, out, n_blocks=None):
    n = ctypes.c_uint32(77)
    p = lambda a: None if a is None else a.ctypes.data
    rc = ctx.lib.duet_ps_join_tags_host(ctx.handle, p(words), p(read_off), K, R, p(table), len(table) if n_blocks is None else n_blocks,
                                        p(out), ctypes.byref(n))
    return rc, n.value


def test_tags_refusals_leave_the_output_untouched(ctx):
    import torch
    words = np.array([tag(1, 1, 20)] * 300, dtype=np.uint64)
    off = np.array([0, 100, 300], dtype=np.uint32)
    good = ps_join.table([(0, 20, 1, 0), (1, 20, 2, 1)])
    mark = np.full(300, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    bad_tables = [[(0, 20, 1, 0), (0, 20, 2, 0)],            # equal keys
                  [(1, 20, 1, 0), (0, 20, 2, 0)],            # contigs descend
                  [(0, 21, 1, 0), (0, 20, 2, 0)],            # PS descends inside a contig
                  [(0, 0x80000000, 1, 0), (0, 5, 2, 0)],     # ... as unsigned numbers
                  [(2, 20, 1, 0)],                           # contig >= K
                  [(0, 20, 1, 2)]]                           # flip > 1
    bad_offs = [[1, 100, 300], [0, 100, 299], [0, 301, 300], [0, 200, 100]]
    d_src, d_out = dev(words), dev(mark)
    for rows in bad_tables:
        out = mark.copy()
        assert tags_raw(ctx, words, off, 2, 300, ps_join.table(rows), out) == (INVALID, 0) and out.tobytes() == mark.tobytes()
        with pytest.raises(_lib.DuetLibraryError):
            ctx.ps_join_tags_device(d_src.data_ptr(), off, 300, ps_join.table(rows), d_out.data_ptr())
    for o in bad_offs:
        out = mark.copy()
        assert tags_raw(ctx, words, np.array(o, dtype=np.uint32), 2, 300, good, out) == (INVALID, 0) and out.tobytes() == mark.tobytes()
        with pytest.raises(_lib.DuetLibraryError):
            ctx.ps_join_tags_device(d_src.data_ptr(), o, 300, good, d_out.data_ptr())
    torch.cuda.synchronize()
    assert back(d_out, np.uint64, 300).tobytes() == mark.tobytes()
    out = mark.copy()
    assert tags_raw(ctx, words, off, 0, 300, good, out)[0] == INVALID                       # no contig
    assert tags_raw(ctx, words, None, 2, 300, good, out)[0] == INVALID
    assert tags_raw(ctx, None, off, 2, 300, good, out)[0] == INVALID
    assert tags_raw(ctx, words, off, 2, 300, good, None)[0] == INVALID
    assert tags_raw(ctx, words, off, 2, 300, None, out, n_blocks=2)[0] == INVALID           # rows announced, no table
    assert ctx.lib.duet_ps_join_tags_host(ctx.handle, words.ctypes.data, off.ctypes.data, 2, 300, good.ctypes.data, 2, out.ctypes.data,
                                          None) == INVALID
    assert out.tobytes() == mark.tobytes()
    # nothing to do: a copy, zero changed
    assert tags_raw(ctx, words, off, 2, 300, good[:0], out) == (0, 0) and out.tobytes() == words.tobytes()
    assert tags_raw(ctx, None, np.zeros(1, dtype=np.uint32), 0, 0, good[:0], None) == (0, 0)
    assert tags_raw(ctx, None, np.zeros(3, dtype=np.uint32), 2, 0, good, None) == (0, 0)


# ---- the change codes --------------------------------------------------------------------------------------------------------------

def check_diff(ctx, ctg_off, p0, s0, p1, s1, rows):
    """Reference against _host and _device in both contig forms -> (codes, counts)."""
    import torch
    K, C = len(ctg_off) - 1, len(p0)
    col = np.array(J.contig_column(ctg_off), dtype=np.uint16)
    table = ps_join.table(rows)
    want, want_counts = J.diff(col, p0, s0, p1, s1, rows)
    for kw in (dict(cand_ctg_off=ctg_off), dict(cand_contig=col)):
        change, counts = ctx.ps_join_diff_host(p0, s0, p1, s1, table, K, **kw)
        assert change.tobytes() == want.tobytes() and counts.tolist() == want_counts.tolist()
    d = [dev(np.ascontiguousarray(a, dtype=dt)) for a, dt in ((p0, np.uint8), (s0, np.uint32), (p1, np.uint8), (s1, np.uint32))]
    d_col = dev(col)
    for kw in (dict(cand_ctg_off=ctg_off), dict(cand_contig_ptr=d_col.data_ptr())):
        out = dev(np.full(C + 8, 0xAB, dtype=np.uint8))
        counts = ctx.ps_join_diff_device(C, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), table, K, out.data_ptr(), **kw)
        torch.cuda.synchronize()
        got = back(out, np.uint8, C + 8)
        assert got[:C].tobytes() == want.tobytes() and np.all(got[C:] == 0xAB) and counts.tolist() == want_counts.tolist()
    return want, want_counts


DIFF_ROWS = [(0, 20, 10, 1), (0, 30, 10, 0), (1, 4, 4, 0), (1, 20, 5, 0), (2, 0xFFFFFFFF, 0, 1)]
# (contig, p0, s0, p1, s1) -> the code's name
DIFF_CASES = [((0, 0, 0, 0, 0), 'none'), ((0, 0, 0, 3, 10), 'gained'), ((0, 0, 20, 1, 10), 'gained'), ((0, 2, 20, 0, 0), 'lost'),
              ((0, 1, 40, 1, 40), 'same'), ((1, 1, 4, 1, 4), 'same'), ((0, 1, 20, 2, 10), 'relabelled'), ((0, 3, 20, 3, 10), 'relabelled'),
              ((0, 2, 30, 2, 10), 'relabelled'), ((1, 1, 20, 1, 5), 'relabelled'), ((2, 2, 0xFFFFFFFF, 1, 0), 'relabelled'),
              ((1, 1, 20, 2, 10), 'other'), ((0, 3, 20, 1, 10), 'to_het'), ((2, 3, 40, 2, 40), 'to_het'), ((0, 1, 20, 3, 10), 'to_hom'),
              ((0, 1, 20, 1, 10), 'other'), ((2, 1, 40, 2, 40), 'other'), ((2, 3, 7, 3, 8), 'other')]


def test_diff_by_hand(ctx):
    cases = sorted(DIFF_CASES)                                       # (contigs ascend)
    k, p0, s0, p1, s1 = [np.array(x, dtype=np.int64) for x in zip(*[c for c, _ in cases])]
    ctg_off = [0] + [int((k <= i).sum()) for i in range(3)]
    codes, counts = check_diff(ctx, ctg_off, p0, s0, p1, s1, DIFF_ROWS)
    assert [J.NAMES[c] for c in codes] == [name for _, name in cases]
    assert all(counts > 0)                                           # each of the eight codes is hit


@pytest.mark.parametrize('C', [0, 1, 63, 64, 65, 257])
def test_diff_sizes(ctx, C):
    rng = np.random.default_rng(C)
    K = 4
    ctg_off = [0, 0, C // 3, C // 3, C]                              # an empty first and an empty middle contig
    rows = [(k, ps, 1 + k, ps & 1) for k in range(K) for ps in (2, 3, 5)]
    p0, p1 = rng.integers(0, 4, C), rng.integers(0, 4, C)
    s0 = rng.integers(1, 7, C)
    s1 = np.where(rng.integers(0, 2, C) == 0, s0, rng.integers(1, 7, C))
    # a third of the candidates keep their call under the table's own relabelling
    col = np.array(J.contig_column(ctg_off), dtype=np.int64)
    moved = (rng.integers(0, 3, C) == 0) & np.isin(s0, (2, 3, 5))
    p1 = np.where(moved, np.where((s0 & 1 == 1) & (p0 != 0) & (p0 != 3), 3 - p0, p0), p1)
    s1 = np.where(moved, 1 + col, s1)
    codes, counts = check_diff(ctx, ctg_off, p0, s0, p1, s1, rows)
    assert int(counts.sum()) == C
    if C >= 63:
        assert all(counts > 0)
    check_diff(ctx, ctg_off, p0, s0, p1, s1, [])                     # no table: nothing is relabelled


def test_diff_refusals(ctx):
    C, K = 70, 2
    p0, p1 = np.ones(C, dtype=np.uint8), np.full(C, 2, dtype=np.uint8)
    s0, s1 = np.full(C, 20, dtype=np.uint32), np.full(C, 10, dtype=np.uint32)
    off, col = np.array([0, 30, 70], dtype=np.uint32), np.array([0] * 30 + [1] * 40, dtype=np.uint16)
    table = ps_join.table([(0, 20, 10, 1)])
    mark = np.full(C, 0xAB, dtype=np.uint8)

    def raw(p0=p0, s0=s0, p1=p1, s1=s1, off=None, col=None, K=K, table=table, counts=True):
        change, cnt = mark.copy(), np.full(8, 9, dtype=np.uint32)
        p = lambda a: None if a is None else a.ctypes.data
        rc = ctx.lib.duet_ps_join_diff_host(ctx.handle, C, p(p0), p(s0), p(p1), p(s1), p(off), p(col), K, p(table), len(table), p(change),
                                            p(cnt) if counts else None)
        return rc, change, cnt

    rc, change, cnt = raw(off=off)
    assert rc == 0 and set(change[:30]) == {4} and set(change[30:]) == {7} and cnt.tolist() == [0, 0, 0, 0, 30, 0, 0, 40]
    untouched = lambda r: r[0] == INVALID and r[1].tobytes() == mark.tobytes() and not r[2].any()
    assert untouched(raw(off=off, col=col)) and untouched(raw())                         # both contig forms, neither
    bad = p1.copy()
    bad[C - 1] = 4
    assert untouched(raw(p1=bad, off=off)) and untouched(raw(p0=bad, col=col))           # pred above 3
    assert 'pred above 3' in ctx.last_error()
    far = col.copy()
    far[C - 1] = 2
    assert untouched(raw(col=far))                                                       # a contig the run does not have
    assert untouched(raw(off=np.array([0, 30, 69], dtype=np.uint32))) and untouched(raw(off=np.array([0, 71, 70], dtype=np.uint32)))
    assert untouched(raw(off=off, table=ps_join.table([(0, 20, 10, 2)])))
    assert untouched(raw(off=off, table=ps_join.table([(0, 20, 10, 1), (0, 20, 11, 1)])))
    assert untouched(raw(off=off, table=ps_join.table([(2, 20, 10, 1)])))
    assert untouched(raw(p0=None, off=off)) and untouched(raw(off=off, K=0))
    assert raw(off=off, counts=False)[0] == INVALID
    rc, _, cnt = raw(off=off)
    assert rc == 0 and cnt.tolist() == [0, 0, 0, 0, 30, 0, 0, 40]                        # a refusal leaves nothing behind


# ---- the joined run against the oracle ---------------------------------------------------------------------------------------------

def joined_on_the_device(ctx, soa, run, min_sv=2, cap=None):
    """The device links, blocks, the device remap, `run` on both tag tables, the device diff."""
    recs = ctx.ps_links_host(soa, 50, 2, pc_cap=cap)
    rows, _ = ps_links.blocks(recs, min_sv=min_sv)
    table = ps_join.table(rows)
    words, n_changed = ctx.ps_join_tags_host(soa.read_tag, soa.read_off, table)
    kw = {name: getattr(soa, name) for name, _ in engine.EfSoA.FIELDS}
    kw['read_tag'] = words
    base, joined = run(soa), run(engine.EfSoA(read_off=soa.read_off, **kw))
    change, counts = ctx.ps_join_diff_host(base[0], base[1], joined[0], joined[1], table, soa.n_contigs, cand_ctg_off=soa.cand_ctg_off)
    return dict(rows=rows, words=words, n_changed=n_changed, base=base, joined=joined, change=change, counts=counts)


@pytest.mark.parametrize('seed', SEEDS)
def test_joined_run_is_the_oracle_on_the_remapped_problem(ctx, seed):
    soa = soa_fuzz.random_soa(seed)
    got = joined_on_the_device(ctx, soa, lambda s: ctx.run_host(s, 50, 2))
    rows, _ = J.blocks_used(L.links(soa, 50, 2), 2)
    assert got['rows'] == rows
    want_words, want_changed = J.remap(soa.read_tag, soa.read_off, rows)
    assert got['words'].tobytes() == want_words.tobytes() and got['n_changed'] == want_changed and want_changed > 0
    rc0, p0, s0 = c_oracle.ef(soa, 50, 2)
    rc1, p1, s1 = c_oracle.ef(J.remapped_soa(soa, rows), 50, 2)
    assert (rc0, rc1) == (0, 0)
    assert np.array_equal(got['base'][0], p0) and np.array_equal(got['base'][1], s0)
    assert np.array_equal(got['joined'][0], p1) and np.array_equal(got['joined'][1], s1)
    codes, counts = J.diff(J.contig_column(soa.cand_ctg_off), p0, s0, p1, s1, rows)
    # the condition: the reference alone shows a candidate that gains a call or turns heterozygous
    assert counts[J.NAMES.index('gained')] + counts[J.NAMES.index('to_het')] >= 1
    assert got['change'].tobytes() == codes.tobytes() and got['counts'].tolist() == counts.tolist()


@pytest.mark.parametrize('cap', [None, 2400])
def test_joined_run_by_the_route_of_thresholds(ctx, cap):
    """--thresholds with the default vector, and --pc_cap 2400: the features under the cap plus one vector, on both tag tables."""
    soa, v = soa_fuzz.random_soa(2), tune.vector()
    got = joined_on_the_device(ctx, soa, lambda s: tune.apply(dict(feat=ctx.features_host(s, 50, 2, pc_cap=cap)), v, ctx=ctx), cap=cap)
    rows, _ = J.blocks_used(L.links(soa, 50, 2, L.PC_MAX if cap is None else cap), 2)
    assert got['rows'] == rows and len(rows) >= 2

    def calls(s):
        feat = pc_cap_ref.features(s, 50, 2, 8100 if cap is None else cap)
        return (np.array(tune_ref.preds_from_features(feat, v), dtype=np.uint8),
                np.array([f['ps'] if f['eligible'] else 0 for f in feat], dtype=np.uint32))
    (p0, s0), (p1, s1) = calls(soa), calls(J.remapped_soa(soa, rows))
    assert np.array_equal(got['base'][0], p0) and np.array_equal(got['joined'][0], p1)
    called = lambda p, s: np.where(p != 0, s, 0)
    assert np.array_equal(called(*got['base']), called(p0, s0)) and np.array_equal(called(*got['joined']), called(p1, s1))
    codes, counts = J.diff(J.contig_column(soa.cand_ctg_off), p0, called(p0, s0), p1, called(p1, s1), rows)
    dev_codes, dev_counts = ctx.ps_join_diff_host(p0, called(p0, s0), p1, called(p1, s1), ps_join.table(rows), soa.n_contigs,
                                                  cand_ctg_off=soa.cand_ctg_off)
    assert dev_codes.tobytes() == codes.tobytes() and dev_counts.tolist() == counts.tolist()
    assert counts[J.NAMES.index('gained')] + counts[J.NAMES.index('to_het')] >= 1


def test_nothing_of_ef_changes_after_a_join_call(ctx):
    soa = soa_fuzz.random_soa(3, n_contigs=4)
    before = (ctx.run_host(soa, 50, 2), ctx.features_host(soa, 50, 2), ctx.ps_links_host(soa, 50, 2))
    rng = np.random.default_rng(1)
    off = [0, 5000, 5000, 20000]
    rows = [(0, 10 * i, i, i & 1) for i in range(3000)] + [(2, 7, 7, 1)]
    check_tags(ctx, random_words(rng, off, rows, [10, 20, 30, 7, 8]), off, rows)
    check_diff(ctx, [0, 40, 100], rng.integers(0, 4, 100), rng.integers(0, 9, 100), rng.integers(0, 4, 100), rng.integers(0, 9, 100),
               [(0, 3, 1, 1), (1, 3, 2, 0)])
    check_tags(ctx, [tag(1, 1, 7)], [0, 1], [(0, 7, 6, 1)])
    after = (ctx.run_host(soa, 50, 2), ctx.features_host(soa, 50, 2), ctx.ps_links_host(soa, 50, 2))
    assert before[0][0].tobytes() == after[0][0].tobytes() and before[0][1].tobytes() == after[0][1].tobytes()
    assert before[1].tobytes() == after[1].tobytes() and before[2].tobytes() == after[2].tobytes()
    assert int((before[0][0] != 0).sum()) > 10


# ---- the product --------------------------------------------------------------------------------------------------------------------

def read(path):
    with open(path, 'rb') as f:
        return f.read()


def stub_stages(monkeypatch):
    from duet_amd import cli, stages
    for name in ('snp_calling', 'sv_calling', 'snp_phasing'):
        monkeypatch.setattr(stages, name, lambda *a: None)
    monkeypatch.setattr(cli, 'check_envs', lambda *a: None)
    monkeypatch.setattr(cli, 'set_logging', lambda *a: None)


def native_rows(soa, txt, feat, pred, ps):
    """The data rows of phased_sv.vcf for calls (pred, ps): built contig by contig and class by class (0, 1, 2) in callset order,
    then sorted stably by (CHROM, POS) and numbered (sv_phasing_fn.py:205-229).  feat: the reference's features (kept, cls)."""
    rows = []
    for k in range(soa.n_contigs):
        for want in (0, 1, 2):
            for c in range(int(soa.cand_ctg_off[k]), int(soa.cand_ctg_off[k + 1])):
                if feat[c]['kept'] and feat[c]['cls'] == want and pred[c]:
                    rows.append(c)
    rows.sort(key=lambda c: (txt['chrom'][c], int(soa.cand_pos[c])))
    return ''.join(tune.row_text(txt['chrom'][c], int(soa.cand_pos[c]), i + 1, txt['ref'][c], txt['alt'][c], int(soa.cand_svlen[c]),
                                 txt['svtype'][c], tune.HP_TEXT[int(pred[c])], int(ps[c])) for i, c in enumerate(rows))


def expected_files(soa, texts, head, rows_of, calls, cap=L.PC_MAX, min_sv=2, must_change=True):
    """The three files of --join_ps by the reference: calls(soa) -> (pred, ps) of the route; rows_of(soa, pred, ps) -> the data rows.
    must_change: the reference alone shows a candidate that gains a call or turns heterozygous."""
    rows, _ = J.blocks_used(L.links(soa, 50, 2, cap), min_sv)
    p0, s0 = calls(soa)
    joined = J.remapped_soa(soa, rows)
    p1, s1 = calls(joined)
    col = J.contig_column(soa.cand_ctg_off)
    codes, counts = J.diff(col, p0, s0, p1, s1, rows)
    assert not must_change or counts[J.NAMES.index('gained')] + counts[J.NAMES.index('to_het')] >= 1
    report =J.header() + J.report_text(texts, col, soa.cand_pos, soa.cand_svlen, codes, p0, s0, p1, s1)
    return ((head + rows_of(joined, p1, s1)).encode(), ('CHROM\tPS\tBLOCK\tFLIP\n' + L.blocks_text(rows, texts)).encode(), report.encode(),
            counts)


def join_paths(home):
    return ps_join.path_vcf(home), ps_join.path_blocks(home), ps_join.path_report(home)


def test_product_native_ingest(ctx, tmp_path_factory, monkeypatch, caplog):
    import logging
    from duet_amd import cli
    from duet_amd.sv_phasing import sv_phasing
    from tests.test_c_oracle import materialise_bams
    home = str(tmp_path_factory.mktemp('ps_join_golden') / 'w')
    shutil.copytree(os.path.join(H.GOLDEN, 'cases', 'fuzz_cutesv_s2'), home)
    materialise_bams(home)
    pinned = read(os.path.join(H.GOLDEN, 'cases', 'fuzz_cutesv_s2', 'phased_sv.vcf'))
    paths = join_paths(home)
    sv_phasing(home, 50, 2, 4, False)
    assert read(home + '/phased_sv.vcf') == pinned and not any(os.path.exists(p) for p in paths)      # no file without the flag
    soa, txt = tune._candidates(home, 50, 2, False, 2)
    texts = [txt['chrom'][int(soa.cand_ctg_off[k])] if soa.cand_ctg_off[k + 1] > soa.cand_ctg_off[k] else '?' for k in range(soa.n_contigs)]
    head = pinned[:pinned.index(b'#CHROM')].decode() + pinned[pinned.index(b'#CHROM'):].split(b'\n', 1)[0].decode() + '\n'

    def oracle_calls(s):
        rc, p, q = c_oracle.ef(s, 50, 2)
        assert rc == 0
        return p, q

    def vector_calls(v, cap):
        def calls(s):
            feat = pc_cap_ref.features(s, 50, 2, cap)
            p = np.array(tune_ref.preds_from_features(feat, v), dtype=np.uint8)
            return p, np.array([f['ps'] if f['eligible'] and q else 0 for f, q in zip(feat, p)], dtype=np.uint32)
        return calls

    rows_of = lambda cap: (lambda s, p, q: native_rows(s, txt, pc_cap_ref.features(s, 50, 2, cap), p, q))
    # (the builder of the expected rows states phased_sv.vcf itself)
    assert (head + rows_of(8100)(soa, *oracle_calls(soa))).encode() == pinned
    want = expected_files(soa, texts, head, rows_of(8100), oracle_calls)
    with caplog.at_level(logging.INFO):
        sv_phasing(home, 50, 2, 4, False, join_ps=True)
    assert read(home + '/phased_sv.vcf') == pinned
    assert tuple(read(p) for p in paths) == want[:3]
    assert want[0] != pinned and want[2].count(b'\n') > 1
    assert ps_join.summary_text(want[3]) in caplog.text
    # the one link of this input has three SVs on its winning side: --join_min_sv 3 still trusts it, 4 does not and the joined run
    # changes nothing; a vector of the caller's own and a cap take their route twice
    sv_phasing(home, 50, 2, 4, False, join_ps=True, join_min_sv=3)
    assert tuple(read(p) for p in paths) == want[:3]
    sv_phasing(home, 50, 2, 4, False, join_ps=True, join_min_sv=4)
    none = expected_files(soa, texts, head, rows_of(8100), oracle_calls, min_sv=4, must_change=False)
    assert tuple(read(p) for p in paths) == none[:3] and none[0] == pinned and none[2] == J.header().encode()
    v = tune.vector({'c1_max_ref_num': 3, 'c0_min_sv_num': 2})
    sv_phasing(home, 50, 2, 4, False, thresholds=v)
    other = read(home + '/phased_sv.vcf')
    sv_phasing(home, 50, 2, 4, False, thresholds=v, join_ps=True, ps_links=True)
    assert read(home + '/phased_sv.vcf') == other
    assert tuple(read(p) for p in paths) == expected_files(soa, texts, head, rows_of(8100), vector_calls(v, 8100))[:3]
    sv_phasing(home, 50, 2, 4, False, pc_cap=2400)
    capped = read(home + '/phased_sv.vcf')
    sv_phasing(home, 50, 2, 4, False, pc_cap=2400, join_ps=True)
    assert read(home + '/phased_sv.vcf') == capped
    # (under this cap the voters that remain tie nothing new to a call: the files are compared all the same)
    assert tuple(read(p) for p in paths) == expected_files(soa, texts, head, rows_of(2400), vector_calls(tune.vector(), 2400), cap=2400,
                                                           must_change=False)[:3]
    # the command
    stub_stages(monkeypatch)
    for p in paths:
        os.remove(p)
    monkeypatch.setattr(sys, 'argv', ['duet', 'in.bam', 'ref.fa', home])
    cli.main(None)
    assert read(home + '/phased_sv.vcf') == pinned and not any(os.path.exists(p) for p in paths)
    monkeypatch.setattr(sys, 'argv', ['duet', 'in.bam', 'ref.fa', home, '--join_ps'])
    cli.main(None)
    assert read(home + '/phased_sv.vcf') == pinned and tuple(read(p) for p in paths) == want[:3]


def test_a_joined_run_that_divides_by_zero_leaves_the_header_alone(tmp_path, monkeypatch):
    """phased_sv.vcf is written first and in full; the error of the second run propagates, phased_sv.joined.vcf keeps its header and
    no report is written.  (The run over the remapped tags is made to raise: no input of the suite divides by zero there alone.)"""
    from duet_amd.sv_phasing import sv_phasing
    from tests.test_c_oracle import materialise_bams
    home = str(tmp_path / 'w')
    shutil.copytree(os.path.join(H.GOLDEN, 'cases', 'fuzz_cutesv_s2'), home)
    materialise_bams(home)
    pinned = read(home + '/phased_sv.vcf')
    os.remove(home + '/phased_sv.vcf')
    real, seen = engine.run_ef, []

    def run_ef(soa, *args, **kw):
        seen.append(soa.read_tag.tobytes())
        if len(seen) > 1 and seen[-1] != seen[0]:
            raise ZeroDivisionError('division by zero')
        return real(soa, *args, **kw)
    monkeypatch.setattr(engine, 'run_ef', run_ef)
    with pytest.raises(ZeroDivisionError):
        sv_phasing(home, 50, 2, 4, False, join_ps=True)
    assert len(seen) == 2 and read(home + '/phased_sv.vcf') == pinned
    vcf, blocks, report = join_paths(home)
    assert read(vcf) == pinned[:pinned.index(b'\n', pinned.index(b'#CHROM')) + 1]
    assert read(blocks).count(b'\n') == 3 and not os.path.exists(report)


class SvimCase(object):
    """A synthetic work directory of the svim-gpu mode, the E/F problem its clustered candidates adapt to (read back from a copy's
    sv_calling/variants.vcf) and the builder of the expected rows."""

    def __init__(self, root):
        self.root = root
        self.home, copy = str(root / 'w'), str(root / 'copy')
        synth.write_svim_workdir(self.home, H.case_contigs('genome_small', 5), 5)
        shutil.copytree(self.home, copy)
        svim_mode.sv_phasing_from_bams(copy, 50, 2, 4, False, 0.9, 0, write_sv_calls=True)
        self.soa, txt = tune._candidates(copy, 50, 2, False, 4)
        self.chroms = init_chrom_list(False, self.home)
        self.texts = svim_mode.spelled_contigs(self.home, self.chroms)
        self.head = svim_mode.header_text(self.home, self.chroms)
        self.res = dict(chroms=self.chroms, cand_contig=np.array(J.contig_column(self.soa.cand_ctg_off), dtype=np.uint16),
                        cand_type=np.array([svim_mode.SV_TYPE_NAMES.index(t) for t in txt['svtype']], dtype=np.uint8))
        self.paths = join_paths(self.home)
        self.base = ['duet', 'in.bam', 'ref.fa', self.home, '-b', 'svim-gpu']

    def rows_of(self, s, p, q):
        return svim_mode.rows_text(self.home, dict(self.res, cand_pos=s.cand_pos, cand_span=s.cand_svlen, pred=p, ps=q))

    def run(self, monkeypatch, *flags):
        from duet_amd import cli
        stub_stages(monkeypatch)
        monkeypatch.setattr(sys, 'argv', self.base + list(flags))
        cli.main(None)
        return read(self.home + '/phased_sv.vcf')


@pytest.fixture(scope='module')
def svim_case(tmp_path_factory):
    return SvimCase(tmp_path_factory.mktemp('ps_join_svim'))


def oracle_calls(s):
    rc, p, q = c_oracle.ef(s, 50, 2)
    assert rc == 0
    return p, q


def test_product_svim_gpu(ctx, svim_case, monkeypatch):
    c = svim_case
    plain = c.run(monkeypatch)
    assert plain.count(b'\n') > 100 and not any(os.path.exists(p) for p in c.paths)
    assert (c.head + c.rows_of(c.soa, *oracle_calls(c.soa))).encode() == plain   # (the builder of the expected rows states the file)
    assert c.run(monkeypatch, '--join_ps') == plain
    want = expected_files(c.soa, c.texts, c.head, c.rows_of, oracle_calls)
    print('svim-gpu: change counts by the reference', want[3].tolist())
    assert tuple(read(p) for p in c.paths) == want[:3] and want[0] != plain
    for p in c.paths:
        os.remove(p)


def test_svim_run_joined_keeps_the_cluster_result_and_the_first_calls(ctx, svim_case):
    from duet_amd.devmem import DeviceSvim
    from duet_amd.native import NativeIngest
    c = svim_case
    ing, got = NativeIngest.extract(c.home + '/snp_phasing/', c.chroms, 4, 50, 20, 1000)
    ing.close()
    ds = DeviceSvim(got, got['read_tag'], got['depth'], got['depth_off'], 1000, 50, 2, max_dist=0.9)
    ds.run_fused(ctx)
    ctx.check()
    first = ds.fetch()
    plain_rows = ds.phased_rows(ctx, c.texts)[0].tobytes()
    rows, _ = ps_links.blocks(ds.ps_links(ctx), min_sv=2)
    table = ps_join.table(rows)
    j = ds.run_joined(ctx, table, got['read_off'])
    second = ds.fetch()
    assert all(first[k].tobytes() == second[k].tobytes() for k in first) and int((first['pred'] != 0).sum()) > 100
    N = len(first['pred'])
    pred1, ps1 = j['pred'][:N].cpu().numpy(), j['ps'][:N].cpu().numpy().view(np.uint32)
    codes, counts = J.diff(first['cand_contig'], first['pred'], first['ps'], pred1, ps1, rows)
    assert j['change'].tobytes() == codes.tobytes() and j['counts'].tolist() == counts.tolist()
    assert counts[J.NAMES.index('gained')] + counts[J.NAMES.index('to_het')] >= 1 and j['n_changed'] > 0
    assert ds.phased_rows(ctx, c.texts)[0].tobytes() == plain_rows
    joined_rows = ds.phased_rows(ctx, c.texts, pred=j['pred'], ps=j['ps'])[0].tobytes()
    assert joined_rows.decode() == svim_mode.rows_text(c.home, dict(c.res, cand_contig=first['cand_contig'], cand_type=first['cand_type'],
                                                                   cand_pos=first['cand_pos'], cand_span=first['cand_span'], pred=pred1,
                                                                   ps=ps1)) != plain_rows.decode()
    # by the route of --thresholds the same calls come out of the default vector
    t = ds.run_joined(ctx, table, got['read_off'], thresholds=tune.vector())
    assert t['pred'][:N].cpu().numpy().tobytes() == pred1.tobytes() and t['change'].tobytes() == j['change'].tobytes()
    assert ds.fetch()['pred'].tobytes() == first['pred'].tobytes()


def test_product_svim_gpu_under_a_cap(ctx, svim_case, monkeypatch):
    """Under a cap the route is that of --thresholds, twice, and the links are the cap's."""
    c = svim_case
    capped = c.run(monkeypatch, '--pc_cap', '2400')
    assert not any(os.path.exists(p) for p in c.paths)
    assert c.run(monkeypatch, '--pc_cap', '2400', '--join_ps') == capped

    def capped_calls(s):
        feat = pc_cap_ref.features(s, 50, 2, 2400)
        p = np.array(tune_ref.preds_from_features(feat, tune.vector()), dtype=np.uint8)
        return p, np.array([f['ps'] if f['eligible'] else 0 for f in feat], dtype=np.uint32)
    want = expected_files(c.soa, c.texts, c.head, c.rows_of, capped_calls, cap=2400, must_change=False)
    assert tuple(read(p) for p in c.paths) == want[:3]
    for p in c.paths:
        os.remove(p)


def test_product_refusals_leave_no_file(tmp_path, monkeypatch):
    from duet_amd import cli
    from duet_amd.sv_phasing import sv_phasing
    from tests.test_c_oracle import materialise_bams
    out = tmp_path / 'out'
    stub_stages(monkeypatch)
    for argv, text in ((['--join_ps', '--gpus', '2'], '--join_ps works on the single-GPU path only'),
                       (['--join_min_sv', '3'], '--join_min_sv needs --join_ps'),
                       (['--join_ps', '--join_min_sv', '0'], '--join_min_sv takes an integer >= 1')):
        monkeypatch.setattr(sys, 'argv', ['duet', 'in.bam', 'ref.fa', str(out)] + argv)
        with pytest.raises(SystemExit, match=text):
            cli.main(None)
    monkeypatch.setenv('DUET_FORCE_RANKS', '1')
    monkeypatch.setattr(sys, 'argv', ['duet', 'in.bam', 'ref.fa', str(out), '--join_ps'])
    with pytest.raises(SystemExit, match='--join_ps works on the single-GPU path only'):
        cli.main(None)
    monkeypatch.delenv('DUET_FORCE_RANKS')
    assert not out.exists()
    # an input the native ingest declines: refused before phased_sv.vcf is created
    home = str(tmp_path / 'w')
    shutil.copytree(os.path.join(H.GOLDEN, 'cases', 'fuzz_cutesv_s2'), home)
    materialise_bams(home)
    os.remove(home + '/phased_sv.vcf')
    monkeypatch.setenv('DUET_NATIVE_INGEST', '0')
    before = sorted(os.listdir(home))
    with pytest.raises(RuntimeError, match='--join_ps needs the native ingest'):
        sv_phasing(home, 50, 2, 4, False, join_ps=True)
    with pytest.raises(RuntimeError, match='--join_ps need the native ingest'):
        sv_phasing(home, 50, 2, 4, False, pc_cap=2400, join_ps=True)
    assert sorted(os.listdir(home)) == before
