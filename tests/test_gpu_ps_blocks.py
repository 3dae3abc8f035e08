# coding=utf-8
"""-m gpu: the blocks of the phase-set links built on the device (duet_amd/csrc/duet_psblocks.hip) against
duet_amd/ps_links.py: blocks, byte for byte -- rows, conflicts and counts through _host and _device -- and
duet_ps_join_links_device against duet_ps_join_tags_device on the table of blocks().

The unit defines one capacity of its own, 2^30 records (refused at once).  Its scans take 2048 and its sorts 4096 elements per
tile, over 2 * n_links node keys and n_links ranks: the sizes below sit on both sides of those edges."""
import ctypes

import numpy as np
import pytest

from duet_amd import _lib, ps_join, ps_links
from tests import ps_blocks_ref as B
from tests import ps_join_ref as J
from tests import soa_fuzz

pytestmark = pytest.mark.gpu

BT, LT = _lib.PS_BLOCK_DTYPE, _lib.PS_LINK_DTYPE
INVALID = _lib.DUET_ERR_INVALID
SEEDS = tuple(range(1, 9))


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros(8, dtype=torch.uint8, device='cuda:0')
    return torch.from_numpy(a.view(np.uint8).copy()).to('cuda:0')


def back(t, dtype, n):
    return t.cpu().numpy()[:n * np.dtype(dtype).itemsize].view(dtype).copy()


def expected(recs, min_sv):
    rows, conflicts = ps_links.blocks(recs, min_sv)
    trusted = sum(1 for r in recs if B.verdict(r) is not None and int(r['n_same' if B.verdict(r) == 0 else 'n_flip']) >= min_sv)
    counts = dict(n_rows=len(rows), n_trusted=trusted, n_conflicts=len(conflicts), n_components=len({(k, b) for k, _, b, _ in rows}))
    return B.table(rows), np.array(conflicts, dtype=np.uint32), counts


def check(ctx, recs, K, min_sv=1):
    """blocks() against _host and _device, the outputs exactly as large as promised to suffice; -> (rows, conflicts, counts)"""
    import torch
    recs = np.ascontiguousarray(recs, dtype=LT)
    n = len(recs)
    rows, conflicts, counts = expected(recs, min_sv)
    got = ctx.ps_blocks_host(recs, K, min_sv)
    assert got[2] == counts, (got[2], counts)
    assert got[0].tobytes() == rows.tobytes() and got[1].tobytes() == conflicts.tobytes()
    d_recs = dev(recs)
    d_rows, d_conf = dev(np.full(4 * (2 * n + 2), 0xABABABAB, dtype=np.uint32)), dev(np.full(n + 2, 0xABABABAB, dtype=np.uint32))
    c = ctx.ps_blocks_device(d_recs.data_ptr(), n, K, min_sv, d_rows.data_ptr(), 2 * n, d_conf.data_ptr(), n)
    torch.cuda.synchronize()
    assert c == counts
    r, f = back(d_rows, np.uint32, 4 * (2 * n + 2)), back(d_conf, np.uint32, n + 2)
    assert r[:4 * len(rows)].tobytes() == rows.tobytes() and np.all(r[4 * len(rows):] == 0xABABABAB)
    assert f[:len(conflicts)].tobytes() == conflicts.tobytes() and np.all(f[len(conflicts):] == 0xABABABAB)
    assert back(d_recs, LT, n).tobytes() == recs.tobytes()
    # no conflict buffer: the count alone
    assert ctx.ps_blocks_device(d_recs.data_ptr(), n, K, min_sv, d_rows.data_ptr(), 2 * n) == counts
    return rows, conflicts, counts


# ---- sizes -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_links', [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049])
def test_chain_sizes(ctx, n_links):
    """One chain with mixed verdicts: deep paths, parity along the path; tile edges of the scans (2 n = 2048) and sorts (4096)."""
    for min_sv in (1, 2):
        rows, conflicts, counts = check(ctx, B.chain(n_links), 1, min_sv)
    if n_links >= 63:
        assert counts['n_components'] > 1 and (rows['flip'] == 1).any() and (rows['block'] != rows['ps']).any()


def test_a_chain_that_hooks_into_one_path_in_the_first_round(ctx):
    """Strengths that descend along the chain: every phase set's best link is the one to its left, so round one builds a single
    path of 1,025 roots -- the deepest tree the jumps can meet -- and alternately the reverse."""
    for order in (lambda i: 2000 - i, lambda i: 10 + i):
        recs = B.records([dict(contig=0, ps_a=3 * i, ps_b=3 * i + 3, n_flip=order(i), w_flip=1, n_same=i % 2) for i in range(1024)])
        rows, _, counts = check(ctx, recs, 1)
        assert counts['n_components'] == 1 and rows['block'].max() == 0 and rows['flip'].tolist() == [i & 1 for i in range(1025)]


def test_a_star(ctx):
    recs = B.records([dict(contig=0, ps_a=7, ps_b=100 + i, n_same=1 + i % 3, n_flip=(i % 5) // 2, w_same=i % 4, w_flip=9) for i in range(300)])
    rows, _, counts = check(ctx, recs, 1)
    assert counts['n_components'] == 1
    recs = B.records([dict(contig=0, ps_a=i, ps_b=5000, n_flip=1 + i % 2, w_flip=i % 3) for i in range(300)])       # the hub is the largest PS
    check(ctx, recs, 1)


def test_cycles_closed_by_the_weakest_link(ctx):
    base = [dict(contig=0, ps_a=10, ps_b=20, n_same=5, w_same=5), dict(contig=0, ps_a=20, ps_b=30, n_flip=4, w_flip=5)]
    agree = B.records([base[0], dict(contig=0, ps_a=10, ps_b=30, n_flip=1, w_flip=1), base[1]])
    rows, conflicts, _ = check(ctx, agree, 1)
    assert len(conflicts) == 0 and rows['flip'].tolist() == [0, 0, 1]
    contradict = B.records([base[0], dict(contig=0, ps_a=10, ps_b=30, n_same=1, w_same=1), base[1]])
    rows, conflicts, _ = check(ctx, contradict, 1)
    assert conflicts.tolist() == [1] and rows['flip'].tolist() == [0, 0, 1]


def test_ties_broken_by_the_row_index_alone(ctx):
    """A complete graph on 12 phase sets whose links all have the same strength, the senses mixed: contradictions everywhere."""
    recs = B.records([dict(contig=0, ps_a=a, ps_b=b, n_same=2 * ((a * b) % 3 != 0), n_flip=2 * ((a * b) % 3 == 0), w_same=3 * ((a * b) % 3 != 0),
                           w_flip=3 * ((a * b) % 3 == 0)) for a in range(12) for b in range(a + 1, 12)])
    _, conflicts, _ = check(ctx, recs, 1)
    assert len(conflicts) > 5


def test_weights_that_differ_only_above_bit_32(ctx):
    recs = B.records([dict(contig=0, ps_a=1, ps_b=2, n_flip=1, w_flip=(1 << 32) + 5), dict(contig=0, ps_a=1, ps_b=3, n_flip=1, w_flip=(3 << 32) + 5),
                      dict(contig=0, ps_a=2, ps_b=3, n_flip=1, w_flip=(2 << 32) + 5)])
    rows, conflicts, _ = check(ctx, recs, 1)
    assert conflicts.tolist() == [0] and rows['flip'].tolist() == [0, 0, 1]
    recs['w_flip'][0] = (4 << 32) + 5                            # now the strongest: the conflict moves to the weakest
    _, conflicts, _ = check(ctx, recs, 1)
    assert conflicts.tolist() == [2]
    recs = B.records([dict(contig=0, ps_a=1, ps_b=2, n_same=1, n_flip=1, w_same=1 << 40, w_flip=(1 << 40) + 1)])      # the verdict itself
    rows, _, _ = check(ctx, recs, 1)
    assert rows['flip'].tolist() == [0, 1]


@pytest.mark.parametrize('min_sv', [1, 2, 3, 4])
def test_the_winning_side_at_and_below_min_sv(ctx, min_sv):
    recs = B.records([dict(contig=0, ps_a=1, ps_b=2, n_flip=min_sv - 1, w_flip=9, n_same=0), dict(contig=0, ps_a=2, ps_b=3, n_flip=min_sv, w_flip=1),
                      dict(contig=0, ps_a=3, ps_b=4, n_same=min_sv, n_flip=min_sv, w_same=7, w_flip=6)])
    rows, _, counts = check(ctx, recs, 1, min_sv)
    assert counts['n_trusted'] == 2 and rows['block'].tolist() == [1, 2, 2, 2] and rows['flip'].tolist() == [0, 0, 1, 1]


def test_records_without_a_verdict_keep_every_node_its_own_row(ctx):
    recs = B.records([dict(contig=0, ps_a=i, ps_b=i + 1 + i % 3, n_same=i % 3, n_flip=i % 3, w_same=i, w_flip=i, n_open=1) for i in range(100)])
    rows, conflicts, counts = check(ctx, recs, 1)
    assert counts['n_trusted'] == 0 and len(conflicts) == 0 and (rows['block'] == rows['ps']).all() and not rows['flip'].any()
    assert counts['n_components'] == counts['n_rows']


def test_the_smallest_ps_joins_last(ctx):
    """PS 1 hangs on the component by its weakest link, so no first-round choice goes through it, and an untrusted link names a
    still smaller PS that stays alone: the blocks are named after the re-rooting."""
    recs = B.records([dict(contig=0, ps_a=0, ps_b=50, n_same=1, n_flip=1, w_same=2, w_flip=2), dict(contig=0, ps_a=1, ps_b=40, n_flip=1, w_flip=1),
                      dict(contig=0, ps_a=20, ps_b=30, n_flip=9, w_flip=9), dict(contig=0, ps_a=30, ps_b=40, n_same=8, w_same=9),
                      dict(contig=0, ps_a=40, ps_b=50, n_flip=7, w_flip=9)])
    rows, _, _ = check(ctx, recs, 1)
    assert rows['block'].tolist() == [0, 1, 1, 1, 1, 1] and rows['flip'].tolist() == [0, 0, 0, 1, 1, 0]


def test_ps_zero_and_the_largest_ps(ctx):
    top = 0xFFFFFFFE
    recs = B.records([dict(contig=0, ps_a=0, ps_b=top, n_flip=2, w_flip=1), dict(contig=0, ps_a=0x7FFFFFFF, ps_b=0x80000000, n_same=1, w_same=1),
                      dict(contig=0, ps_a=0x80000000, ps_b=top, n_flip=1, w_flip=1)])
    rows, _, _ = check(ctx, recs, 1)
    assert rows['block'].tolist() == [0] * 4 and rows['flip'].tolist() == [0, 0, 0, 1]


def test_the_same_ps_on_two_contigs_and_empty_contigs(ctx):
    """Four contigs with links, between an empty first, middle and last one; PS 5 and 9 on all of them, joined differently."""
    recs = B.records([dict(contig=1, ps_a=5, ps_b=9, n_flip=1, w_flip=1), dict(contig=2, ps_a=5, ps_b=9, n_same=1, w_same=1),
                      dict(contig=4, ps_a=5, ps_b=9, n_open=3), dict(contig=4, ps_a=9, ps_b=11, n_flip=2, w_flip=1),
                      dict(contig=5, ps_a=4, ps_b=5, n_same=1, w_same=0)])
    rows, _, counts = check(ctx, recs, 7)
    assert rows['contig'].tolist() == [1, 1, 2, 2, 4, 4, 4, 5, 5] and rows['block'].tolist() == [5, 5, 5, 5, 5, 9, 9, 4, 4]
    assert rows['flip'].tolist() == [0, 1, 0, 0, 0, 0, 1, 0, 0] and counts['n_components'] == 5
    check(ctx, recs, 6)


@pytest.mark.parametrize('chunk', range(10))
def test_random_multigraphs(ctx, chunk):
    """The cases of tests/test_ps_blocks_host.py, 200 seeds."""
    with_conflicts = 0
    for seed in range(20 * chunk, 20 * chunk + 20):
        recs, K = B.random_records(seed)
        for min_sv in (1, 2, 3):
            with_conflicts += len(check(ctx, recs, K, min_sv)[1]) > 0
    assert with_conflicts >= 3


@pytest.mark.parametrize('seed', SEEDS)
def test_links_of_random_problems(ctx, seed):
    recs = ctx.ps_links_host(soa_fuzz.random_soa(seed), 50, 2)
    assert len(recs) >= 1
    for min_sv in (1, 2, 3):
        check(ctx, recs, 3, min_sv)


def test_contradicted_links_among_the_random_problems(ctx):
    n = sum(len(ps_links.blocks(ctx.ps_links_host(soa_fuzz.random_soa(seed), 50, 2), 1)[1]) > 0 for seed in SEEDS)
    assert n >= 3


# ---- contracts ---------------------------------------------------------------------------------------------------------------------

def raw_host(ctx, recs, n, K, min_sv, rows, rows_cap, conf, conf_cap):
    c = _lib.PsBlocksCounts(7, 7, 7, 7)
    p = lambda a: None if a is None else a.ctypes.data
    rc = ctx.lib.duet_ps_blocks_host(ctx.handle, p(recs), n, K, min_sv, p(rows), rows_cap, p(conf), conf_cap, ctypes.byref(c))
    return rc, c.as_dict()


ZERO = dict(n_rows=0, n_trusted=0, n_conflicts=0, n_components=0)


def test_refusals_leave_both_outputs_untouched(ctx):
    import torch
    good = B.records([dict(contig=0, ps_a=1, ps_b=2, n_same=3, w_same=1), dict(contig=0, ps_a=1, ps_b=3, n_same=1, w_same=1),
                      dict(contig=0, ps_a=2, ps_b=3, n_flip=2, w_flip=1), dict(contig=1, ps_a=1, ps_b=2, n_flip=2, w_flip=1)])

    def edited(i, **kw):
        r = good.copy()
        for k, v in kw.items():
            r[i][k] = v
        return r
    bad = [edited(1, ps_a=3),                                    # ps_a == ps_b
           edited(1, ps_a=4),                                    # ps_a > ps_b
           edited(0, ps_a=0x80000000, ps_b=5),                   # ... as unsigned numbers
           edited(3, contig=2),                                  # contig >= n_contigs
           edited(2, ps_a=1, ps_b=3),                            # equal keys
           edited(2, ps_a=1, ps_b=2),                            # ps_b descends
           edited(3, contig=0, ps_a=2, ps_b=9)[[3, 0, 1, 2]],    # contigs fine, the first record above the second
           edited(0, contig=1, ps_b=9)]                          # contigs descend
    mark_r, mark_c = np.full(8, 0x5A5A5A5A, dtype=np.uint32).repeat(4).view(BT), np.full(4, 0x5A5A5A5A, dtype=np.uint32)
    d_rows, d_conf = dev(mark_r), dev(mark_c)
    cases = [(r, 2, 1, 8, 4) for r in bad] + [(good, 2, 0, 8, 4),           # min_sv below 1
                                              (good, 2, 1, 4, 4),           # five rows, room for four
                                              (good, 2, 1, 8, 0),           # one conflict, a buffer without room
                                              (good, 0, 1, 8, 4)]           # no contig
    for recs, K, min_sv, rows_cap, conf_cap in cases:
        rows, conf = mark_r.copy(), mark_c.copy()
        assert raw_host(ctx, recs, len(recs), K, min_sv, rows, rows_cap, conf, conf_cap) == (INVALID, ZERO)
        assert rows.tobytes() == mark_r.tobytes() and conf.tobytes() == mark_c.tobytes()
        d_recs = dev(recs)
        with pytest.raises(_lib.DuetLibraryError):
            ctx.ps_blocks_device(d_recs.data_ptr(), len(recs), K, min_sv, d_rows.data_ptr(), rows_cap, d_conf.data_ptr(), conf_cap)
    torch.cuda.synchronize()
    assert back(d_rows, BT, 8).tobytes() == mark_r.tobytes() and back(d_conf, np.uint32, 4).tobytes() == mark_c.tobytes()
    rows, conf = mark_r.copy(), mark_c.copy()
    assert raw_host(ctx, None, 4, 2, 1, rows, 8, conf, 4)[0] == INVALID                     # records announced, none given
    assert raw_host(ctx, good, 4, 2, 1, None, 8, conf, 4)[0] == INVALID
    assert raw_host(ctx, good, 4, 2, 1, rows, 8, None, 4)[0] == INVALID
    assert raw_host(ctx, good, 1 << 30, 2, 1, rows, 8, conf, 4) == (INVALID, ZERO)          # the unit's capacity: refused before any read
    assert ctx.lib.duet_ps_blocks_host(ctx.handle, good.ctypes.data, 4, 2, 1, rows.ctypes.data, 8, conf.ctypes.data, 4, None) == INVALID
    assert rows.tobytes() == mark_r.tobytes() and conf.tobytes() == mark_c.tobytes()
    # nothing to do: no array is read
    assert raw_host(ctx, None, 0, 0, 1, None, 0, None, 0) == (0, ZERO)
    # a refusal leaves nothing behind; exactly enough room; no conflict buffer at all
    rc, c = raw_host(ctx, good, 4, 2, 1, rows, 5, conf, 1)
    assert rc == 0 and c == dict(n_rows=5, n_trusted=4, n_conflicts=1, n_components=2) and conf[0] == 1 and conf[1] == 0x5A5A5A5A
    assert rows[:5].tobytes() == expected(good, 1)[0].tobytes() and rows[5:].tobytes() == mark_r[5:].tobytes()
    assert raw_host(ctx, good, 4, 2, 1, rows, 5, None, 0) == (0, c)


def test_two_runs_give_identical_bytes(ctx):
    recs, K = B.chain(1025), 1
    a, b = ctx.ps_blocks_host(recs, K, 1), ctx.ps_blocks_host(recs, K, 1)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    recs = ctx.ps_links_host(soa_fuzz.random_soa(5), 50, 2)
    a, b = ctx.ps_blocks_host(recs, 3, 1), ctx.ps_blocks_host(recs, 3, 1)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


def test_nothing_of_ef_changes_after_a_blocks_call(ctx):
    soa = soa_fuzz.random_soa(3, n_contigs=4)
    before = (ctx.run_host(soa, 50, 2), ctx.features_host(soa, 50, 2), ctx.ps_links_host(soa, 50, 2))
    table = ps_join.table(ps_links.blocks(before[2], 2)[0])
    tags_before = ctx.ps_join_tags_host(soa.read_tag, soa.read_off, table)
    check(ctx, B.chain(3000), 1)
    check_join(ctx, B.chain(700), [0, 5000], 1, np.random.default_rng(2))
    check(ctx, B.chain(1), 1)
    after = (ctx.run_host(soa, 50, 2), ctx.features_host(soa, 50, 2), ctx.ps_links_host(soa, 50, 2))
    tags_after = ctx.ps_join_tags_host(soa.read_tag, soa.read_off, table)
    assert before[0][0].tobytes() == after[0][0].tobytes() and before[0][1].tobytes() == after[0][1].tobytes()
    assert before[1].tobytes() == after[1].tobytes() and before[2].tobytes() == after[2].tobytes()
    assert tags_before[0].tobytes() == tags_after[0].tobytes() and tags_before[1] == tags_after[1]
    assert int((before[0][0] != 0).sum()) > 10


# ---- links -> remapped tags ----------------------------------------------------------------------------------------------------------

def words_over(rng, recs, read_off):
    """Tag words whose PS come from the records' phase sets (of any contig) and a few others, every hap, some untagged."""
    R = int(read_off[-1])
    pool = np.unique(np.concatenate([recs['ps_a'], recs['ps_b'], np.array([0, 3, 0xFFFFFFFF], dtype=np.uint32)])).astype(np.uint64)
    words = (rng.integers(0, 4, R).astype(np.uint64) << np.uint64(62)) | (rng.integers(0, 1 << 30, R).astype(np.uint64) << np.uint64(32)) | \
        pool[rng.integers(0, len(pool), R)]
    words[rng.integers(0, 7, R) == 0] = J.UNTAGGED
    return words


def check_join(ctx, recs, read_off, min_sv, rng=None, words=None):
    """duet_ps_join_links_device against duet_ps_join_tags_device on the table of blocks(), into a second array and in place."""
    import torch
    recs = np.ascontiguousarray(recs, dtype=LT)
    K, R = len(read_off) - 1, int(read_off[-1])
    words = words_over(rng, recs, read_off) if words is None else np.ascontiguousarray(words, dtype=np.uint64)
    rows, _, counts = expected(recs, min_sv)
    d_recs, src, want_t, dst = dev(recs), dev(words), dev(np.zeros(R, dtype=np.uint64)), dev(np.full(R, 0xABABABABABABABAB, dtype=np.uint64))
    n_want = ctx.ps_join_tags_device(src.data_ptr(), read_off, R, rows, want_t.data_ptr())
    torch.cuda.synchronize()
    want = back(want_t, np.uint64, R)
    ref, n_ref = J.remap(words, read_off, [tuple(int(x) for x in r) for r in rows])
    assert want.tobytes() == ref.tobytes() and n_want == n_ref
    n, c = ctx.ps_join_links_device(d_recs.data_ptr(), len(recs), min_sv, src.data_ptr(), read_off, R, dst.data_ptr())
    torch.cuda.synchronize()
    assert (n, c) == (n_want, counts if len(recs) else ZERO)
    assert back(dst, np.uint64, R).tobytes() == want.tobytes() and back(src, np.uint64, R).tobytes() == words.tobytes()
    n, c = ctx.ps_join_links_device(d_recs.data_ptr(), len(recs), min_sv, src.data_ptr(), read_off, R, src.data_ptr())
    torch.cuda.synchronize()
    assert n == n_want and back(src, np.uint64, R).tobytes() == want.tobytes()
    return n_want


@pytest.mark.parametrize('seed', SEEDS)
def test_join_links_on_random_problems(ctx, seed):
    soa = soa_fuzz.random_soa(seed)
    recs = ctx.ps_links_host(soa, 50, 2)
    changed = [check_join(ctx, recs, soa.read_off, min_sv, words=soa.read_tag) for min_sv in (1, 2, 3)]
    assert changed[0] > 0


def test_join_links_on_the_chain_and_across_contigs(ctx):
    rng = np.random.default_rng(11)
    assert check_join(ctx, B.chain(1024), [0, 3000], 1, rng) > 1000
    # four contigs, the first, a middle and the last without reads or without links; tiles of 256 reads that straddle contigs
    recs = np.concatenate([B.chain(40, contig=1, first=5, step=2), B.chain(300, contig=2, first=0, step=1), B.chain(3, contig=4, first=5, step=2)])
    for off in ([0, 0, 300, 700, 700, 1000, 1000], [0, 100, 130, 600, 600, 601, 900], [0, 0, 0, 0, 0, 0, 0]):
        check_join(ctx, recs, off, 1, rng)
    check_join(ctx, recs[:0], [0, 10, 300], 1, rng)              # no links: a copy


def test_join_links_refusals(ctx):
    import torch
    recs = B.chain(10)
    words = np.full(50, (1 << 62) | 3, dtype=np.uint64)
    d_recs, src, dst = dev(recs), dev(words), dev(np.full(50, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64))
    for off, min_sv in (([0, 49], 1), ([1, 50], 1), ([0, 60, 50], 1), ([0, 50], 0)):
        with pytest.raises(_lib.DuetLibraryError):
            ctx.ps_join_links_device(d_recs.data_ptr(), 10, min_sv, src.data_ptr(), off, 50, dst.data_ptr())
    torch.cuda.synchronize()
    assert np.all(back(dst, np.uint64, 50) == 0x5A5A5A5A5A5A5A5A)
    # found on the device: the tags come out unchanged
    bad = recs.copy()
    bad[4]['ps_b'] = bad[4]['ps_a']
    d_bad = dev(bad)
    with pytest.raises(_lib.DuetLibraryError):
        ctx.ps_join_links_device(d_bad.data_ptr(), 10, 1, src.data_ptr(), [0, 50], 50, dst.data_ptr())
    torch.cuda.synchronize()
    assert back(dst, np.uint64, 50).tobytes() == words.tobytes()
