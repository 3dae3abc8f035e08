# coding=utf-8
"""CPU: every case of tests/cluster_cases.py sits on the edge it is named for -- shown from the input alone with the model of the
host driver's decisions in tests/cluster_model.py (the plan of duet_cluster_run, rule 2's partitions, the box expression in
binary64) -- and the oracle gives the answer the case is built for where the case fixes one.  Where a case depends on the box
test's outcome the outcome is decisive: at most half the threshold or at least twice it, so that the binary32 evaluation and its
1e-5 guard band cannot go the other way (the guard band itself: test_gpu_cluster.test_threshold_exactly_on_a_pair_distance)."""
import numpy as np
import pytest

from oracle import c_oracle
from tests import cluster_cases as C
from tests import cluster_model as Mo

_cache = {}


def get(name):
    if name not in _cache:
        _cache.clear()
        marks, kw = C.case(name)
        _cache[name] = (marks, kw, Mo.partitions(marks, kw.get('part_gap', 1000), kw.get('part_max', 100)))
    return _cache[name]


def oracle(name):
    marks, kw, _ = get(name)
    return c_oracle.cluster(marks['contig'], marks['type'], marks['pos'], marks['span'], **kw)


def cand_sizes(want):
    return np.diff(want['cand_off'].astype(np.int64))


def plans(marks, dbg, **kw):
    """the plan with and without hints: every case is built so that both agree on the key"""
    a, b = Mo.plan(marks, dbg, True, **kw), Mo.plan(marks, dbg, False, **kw)
    assert {k: v for k, v in a.items() if k != 'hinted'} == {k: v for k, v in b.items() if k != 'hinted'}
    return a


def outcomes(name):
    marks, kw, parts = get(name)
    out = Mo.box_outcomes(marks, parts, kw.get('max_dist', 0.9), kw.get('normalizer', 900.0))
    assert not np.any(out == 'undecided'), (name, np.nonzero(out == 'undecided')[0][:5])
    return out


# ---- every case ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', C.NAMES)
def test_every_case_is_shuffled_and_the_oracle_takes_it(name):
    marks, kw, parts = get(name)
    M = len(marks['pos'])
    assert all(len(v) == M for v in marks.values())
    if M > 3:
        assert not np.array_equal(parts['order'], np.arange(M)), 'the sort would be the identity'
    want = oracle(name)
    # the model's partitions are the oracle's: no candidate crosses a partition start, and the order is the sorted order within
    assert np.all(np.isin(parts['starts'], want['cand_off']))
    assert np.array_equal(np.sort(want['order']), np.arange(M))
    # (the large cases' subsets are lists of (hints, debug word))
    assert all(isinstance(h, bool) and isinstance(d, int) for h, d in C.SUBSET.get(name, ()))
    assert (name in C.SUBSET) == (M >= 65000)


def test_bits_for():
    assert [Mo.bits_for(v) for v in (0, 1, 2, 255, 256, (1 << 32) - 1, 1 << 32)] == [1, 1, 2, 8, 9, 32, 33]


# ---- A. the record sort's plan ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,M,rs_w', (('rs_one_pass_10', 16383, [10]), ('rs_one_pass_11', 16384, [11]),
                                         ('rs_one_pass_11_m32767', 32767, [11]), ('rs_two_pass_6_6', 32768, [6, 6])))
def test_rs_pass_plan_by_size(name, M, rs_w):
    marks = get(name)[0]
    for dbg in (Mo.RECSORT, Mo.LARGE):
        p = plans(marks, dbg)
        assert len(marks['pos']) == M and p['rec_mode'] and p['key_bits'] >= 30 and p['rs_w'] == rs_w and p['rs_lo'] == p['key_bits'] - sum(rs_w)
    assert not Mo.plan(marks, 0)['rec_mode']


def test_rs_wide_11_11():
    marks = get('rs_wide_11_11')[0]
    p = plans(marks, Mo.RECSORT)
    assert len(marks['pos']) == 3000 and (p['contig_bits'], p['type_bits'], p['idx_bits'], p['centre_bits']) == (16, 4, 12, 33)
    assert p['rec_mode'] and p['key_bits'] == 53 and p['T'] == 22 and p['rs_lo'] == 31 and p['rs_w'] == [11, 11]
    # the top 22 bits (contig, type, the centre's top two) take several values: both digits have something to order
    top = (marks['contig'].astype(np.int64) << 6) | (marks['type'].astype(np.int64) << 2) | (Mo.centres(marks) >> 31)
    assert len(np.unique(top & 2047)) > 8 and len(np.unique(top >> 11)) >= 4


def test_rs_wide_9_9_8():
    marks = get('rs_wide_9_9_8')[0]
    p = plans(marks, Mo.RECSORT)
    assert len(marks['pos']) == 200 and p['rec_mode'] and p['key_bits'] == 57 and p['T'] == 26 and p['rs_w'] == [9, 9, 8] and p['rs_lo'] == 31


@pytest.mark.parametrize('M', (7, 5000))
def test_rs_tiny_keys(M):
    marks = get('rs_tiny_keys_m%d' % M)[0]
    assert len(marks['pos']) == M and Mo.centres(marks).max() < 16 and marks['contig'].max() == 0 and marks['type'].max() == 0
    for hints in (True, False):
        p = Mo.plan(marks, Mo.RECSORT, hints)
        assert p['rec_mode'] and p['key_bits'] <= 6 and p['T'] == p['key_bits'] and p['rs_lo'] == 0 and p['rs_w'] == [p['key_bits']]


@pytest.mark.parametrize('M', (6147, 5))
def test_rs_dig_tail(M):
    marks = get('rs_dig_tail_m%d' % M)[0]
    p = plans(marks, Mo.RECSORT)
    assert len(marks['pos']) == M and p['rec_mode'] and p['rs_np'] >= 2 and M % 8 != 0
    assert p['contig_bits'] + p['type_bits'] + p['idx_bits'] == (32 if M == 6147 else 23)
    assert p['rs_w'] == ([11, 10] if M == 6147 else [11, 11])
    if M == 6147:                           # the tail lies in the second tile's second half (rs_hist_dig: 2,048 marks per round)
        assert p['nb_rs'] == 2 and (M - Mo.RS_TILE) // 2048 == 1 and (M - Mo.RS_TILE) % 2048 == 3
    else:
        assert M < 8


@pytest.mark.parametrize('M,nb_rs', ((4095, 1), (4096, 1), (4097, 2)))
def test_rs_tiles(M, nb_rs):
    marks = get('rs_tiles_%d' % M)[0]
    p = plans(marks, Mo.RECSORT)
    assert len(marks['pos']) == M and p['rec_mode'] and p['rs_np'] == 2 and p['nb_rs'] == nb_rs and p['rs_small']


@pytest.mark.parametrize('name,M,chunks', (('rs_chunks_16', 65536, 1), ('rs_chunks_17', 65537, 2)))
def test_rs_chunks(name, M, chunks):
    marks = get(name)[0]
    assert C.SUBSET[name] == ((True, Mo.LARGE), (True, Mo.RECSORT | Mo.LARGE))
    for _, dbg in C.SUBSET[name]:
        p = plans(marks, dbg)
        assert len(marks['pos']) == M and p['rec_mode'] and not p['rs_small'] and p['rs_chunks'] == chunks
        assert p['nb_rs'] == 16 + (chunks - 1) and p['box_applies'] and p['use_spine']


def test_rs_word():
    a, b = get('rs_word_32')[0], get('rs_word_33')[0]
    pa, pb = plans(a, Mo.RECSORT), plans(b, Mo.RECSORT)
    assert pa['contig_bits'] + pa['type_bits'] + pa['idx_bits'] == 32 and pa['rec_mode']
    assert pb['contig_bits'] + pb['type_bits'] + pb['idx_bits'] == 33 and not pb['rec_mode']
    assert 2000 < len(a['pos']) < 5000 and len(a['pos']) == len(b['pos'])


# ---- B. the key sort's switches -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kb,hybrid', ((24, False), (25, True), (47, True), (48, False)))
def test_ks_hybrid(kb, hybrid):
    marks = get('ks_kb%d' % kb)[0]
    for dbg in (0, Mo.KEYSORT):
        p = plans(marks, dbg)
        assert not p['rec_mode'] and p['idx_packed'] and p['key_bits'] == kb and p['hybrid'] == hybrid
        assert p['top_shift'] == (kb - 16 if hybrid else 0) and 2900 < len(marks['pos']) < 3100


def test_ks_idx():
    a, b = get('ks_idx_64')[0], get('ks_idx_65')[0]
    pa, pb = plans(a, 0), plans(b, 0)
    assert (len(a['pos']), len(b['pos'])) == (128, 129) and pa['key_bits'] == pb['key_bits'] == 57
    assert pa['key_bits'] + pa['idx_bits'] == 64 and pa['idx_packed'] and pb['key_bits'] + pb['idx_bits'] == 65 and not pb['idx_packed']
    assert not pa['hybrid'] and not pb['hybrid']


def test_ks_no_hints_zero_pos():
    marks = get('ks_no_hints_zero_pos')[0]
    assert marks['pos'].max() == 0 and marks['span'].min() > 0
    p = Mo.plan(marks, 0, True)
    assert not p['hinted'] and p['centre_bits'] == Mo.bits_for(int(marks['span'].max()) // 2)
    assert len(np.unique(Mo.centres(marks))) > 100


# ---- C. the partition scan ----------------------------------------------------------------------------------------------------

def test_gap():
    a, b = get('gap_1000')[2], get('gap_1001')[2]
    # centres exactly part_gap apart stay together, one more parts them; a type or contig change parts them either way
    assert a['sizes'].tolist() == [2, 2, 4, 1, 1, 1, 1] and b['sizes'].tolist() == [1] * 12
    ma = get('gap_1000')[0]
    c = np.sort(Mo.centres(ma)[(ma['contig'] == 0) & (ma['type'] == 0)])
    assert np.diff(c).tolist().count(1000) == 5
    mb = get('gap_1001')[0]
    c = np.sort(Mo.centres(mb)[(mb['contig'] == 0) & (mb['type'] == 0)])
    assert np.diff(c).tolist().count(1001) == 5
    assert cand_sizes(oracle('gap_1001')).tolist() == [1] * 12
    # ... and the cut decides the result: within a partition the marks 1,000 bp apart merge (d = 1.11, or 2.11 with spans 7 and 0, <= max_dist = 2.5)
    assert cand_sizes(oracle('gap_1000')).tolist() == [2, 2, 4, 1, 1, 1, 1]


@pytest.mark.parametrize('pm', (100, 128, 37, 1))
def test_cut(pm):
    marks, kw, parts = get('cut_pm%d' % pm)
    assert kw['part_max'] == pm
    assert parts['natural'][::2].tolist() == [pm, pm + 1, 2 * pm, 2 * pm + 1]
    sizes = []
    for n in parts['natural']:
        sizes += [pm] * (n // pm) + ([n % pm] if n % pm else [])
    assert parts['sizes'].tolist() == sizes
    if pm == 1:
        assert len(parts['starts']) == len(marks['pos'])


@pytest.mark.parametrize('at', (2047, 2048, 2049))
def test_head_at(at):
    marks, kw, parts = get('head_at_%d' % at)
    assert at in parts['heads'] and at - 1 not in parts['heads'] and at + 1 not in parts['heads']
    assert parts['tile'][np.searchsorted(parts['starts'], at)] == at // 2048 and Mo.plan(marks)['nb_sc'] == 2


def test_straddle_full_halo():
    marks, kw, parts = get('straddle_full_halo')
    j = np.searchsorted(parts['starts'], 2047)
    assert parts['starts'][j] == 2047 and parts['sizes'][j] == 128 == kw['part_max'] and parts['starts'][j + 1] == 2048 + Mo.BOX_HALO - 1
    assert len(marks['pos']) > 2048 + Mo.BOX_HALO


def test_tile_without_start():
    marks, kw, parts = get('tile_without_start')
    assert len(marks['pos']) == 2048 + 60 and Mo.plan(marks)['nb_sc'] == 2
    assert parts['starts'][-1] == 2000 and parts['sizes'][-1] == 108 and not np.any(parts['tile'] == 1)


@pytest.mark.parametrize('kind', ('first', 'last', 'none'))
def test_next_head_halo(kind):
    marks, kw, parts = get('next_head_halo_%s' % kind)
    pm = kw['part_max']
    assert Mo.plan(marks, Mo.LARGE)['nb_sc'] == 3 and Mo.plan(marks, Mo.LARGE)['box_applies']
    halo = parts['heads'][(parts['heads'] >= 2048) & (parts['heads'] < 2048 + Mo.BOX_HALO)]
    H = parts['heads'][parts['heads'] < 2048].max()                   # the natural start in force at tile 0's last position
    multiple = H + -(-(2048 - H) // pm) * pm
    last = parts['starts'][parts['starts'] < 2048].max()
    end = parts['starts'][np.searchsorted(parts['starts'], last) + 1]
    if kind == 'first':
        assert halo.min() == 2048 and multiple > 2048 and end == 2048
    elif kind == 'last':
        assert halo.tolist() == [2048 + Mo.BOX_HALO - 1] and last == 2047 and end == 2048 + Mo.BOX_HALO - 1
    else:
        assert len(halo) == 0 and end == multiple == 2100


@pytest.mark.parametrize('M', (1, 2, 3))
def test_first_mark_only(M):
    marks, kw, parts = get('first_mark_only_m%d' % M)
    assert len(marks['pos']) == M and parts['sizes'].tolist() == [1] * M


# ---- D. the box test ------------------------------------------------------------------------------------------------------------

def test_box_257_parts_in_tile():
    marks, kw, parts = get('box_257_parts_in_tile')
    assert (parts['tile'] == 0).sum() == 257 > Mo.BOX_THREADS and parts['starts'][256] == 2047
    assert sorted(set(parts['sizes'][:257].tolist())) == list(range(1, 17))
    out = outcomes('box_257_parts_in_tile')
    assert (out[:257] == 'open').sum() > 50 and (out[:257] == 'one').sum() > 100


def test_box_2048_singletons():
    marks, kw, parts = get('box_2048_singletons')
    assert len(marks['pos']) == 2049 and parts['sizes'].tolist() == [1] * 2049 and (parts['tile'] == 0).sum() == 2048
    assert np.all(np.diff(np.sort(Mo.centres(marks))) >= 1001)
    assert cand_sizes(oracle('box_2048_singletons')).tolist() == [1] * 2049


def test_box_n64_n65():
    for name, n in (('box_n64_one_cluster', 64), ('box_n65_same_shape', 65)):
        marks, kw, parts = get(name)
        assert parts['sizes'].tolist() == [4, n, 6] and outcomes(name).tolist() == ['one', 'one', 'open']
        assert cand_sizes(oracle(name)).tolist() == [4, n, 2, 2, 2]
        assert Mo.size_class(n) == (3 if n == 64 else 4)


def test_box_end_wraps():
    marks, kw, parts = get('box_end_wraps')
    assert parts['sizes'].tolist() == [6] * 6 and outcomes('box_end_wraps').tolist() == ['open'] * 6
    for j in range(6):
        pos, span = Mo.partition_rows(marks, parts, j)
        assert Mo.ends_wrap(pos, span) and not Mo.ends_wrap(pos[:3], span[:3])
        # in 32 bits the box is decisively tight, in truth decisively not
        assert Mo.box_value(pos, span, wrapped=True) <= 0.5 * kw['max_dist'] and Mo.box_value(pos, span) >= 2.0 * kw['max_dist']
    assert cand_sizes(oracle('box_end_wraps')).tolist() == [3] * 12


@pytest.mark.parametrize('n', (64, 128))
def test_box_mean_floor(n):
    marks, kw, parts = get('box_mean_floor_n%d' % n)
    pos, span = Mo.partition_rows(marks, parts, len(parts['starts']) - 1)
    assert len(pos) == n and not Mo.ends_wrap(pos, span) and pos.max() > (1 << 32) - 1000
    assert pos.sum() % n == n - n // 64 and span.sum() % n == n - n // 64           # the means: an integer minus 1 / 64
    assert outcomes('box_mean_floor_n%d' % n)[-1] == 'one'
    want = oracle('box_mean_floor_n%d' % n)
    assert cand_sizes(want)[-1] == n and want['cand_pos'][-1] == pos.sum() // n == pos.max() - 1 and want['cand_span'][-1] == 499


# ---- E. work lists and shards ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('counts', ((1, 3, 1, 1), (7, 4, 2, 1), (8, 5, 3, 1), (9, 3, 1, 1)))
def test_class_counts(counts):
    name = 'class_counts_%d' % counts[0]
    marks, kw, parts = get(name)
    out = outcomes(name)
    cls = np.array([Mo.size_class(n) for n in parts['sizes']])
    assert tuple(int(((out == 'open') & (cls == c)).sum()) for c in range(4)) == counts
    assert not np.any(cls == 4) and (out == 'one').sum() == sum(counts)
    open8 = parts['sizes'][(out == 'open') & (cls == 0)]
    assert open8.max() <= 8 and (counts[0] == 1 or 8 in open8)


def test_sizes():
    name = 'sizes_8_9_16_17_32_33_64_65_100_101_128'
    marks, kw, parts = get(name)
    out = outcomes(name)
    assert parts['sizes'][out == 'open'].tolist() == list(C.SIZES) and kw['part_max'] == 128
    want = cand_sizes(oracle(name))
    assert len(want) == 3 * len(C.SIZES) + len(C.SIZES)


def test_second_list_meets_first():
    marks, kw, parts = get('second_list_meets_first')
    M = len(marks['pos'])
    assert M == 2048 + 2047 and parts['sizes'].tolist() == [2] * 2047 + [1]
    assert (parts['tile'] == 0).sum() == 1024 == Mo.SCAN_TILE // 2 and (parts['tile'] == 1).sum() == 1024
    for j in (0, 1, 1023, 1024, 2046):
        pos, span = Mo.partition_rows(marks, parts, j)
        assert Mo.ends_wrap(pos, span)
    assert outcomes('second_list_meets_first')[:-1].tolist() == ['open'] * 2047
    for dbg in (Mo.TIERS, Mo.LARGE):
        p = Mo.plan(marks, dbg)
        assert p['tiers'] and p['tps'] == 1 and p['nb_sc'] == 2
    sizes = cand_sizes(oracle('second_list_meets_first'))
    assert (sizes == 2).sum() == 2047 - 683 and (sizes == 1).sum() == 2 * 683 + 1


def test_shards_tps2():
    marks, kw, parts = get('shards_tps2')
    M = len(marks['pos'])
    p = plans(marks, 0)
    assert M == 131073 and p['nb_sc'] == 65 and p['tps'] == 2 and (p['nb_sc'] + p['tps'] - 1) // p['tps'] == 33
    out = outcomes('shards_tps2')
    shard = parts['tile'] // p['tps']
    for s in (0, 16, 31):
        cls = {Mo.size_class(n) for n in parts['sizes'][(shard == s) & (out == 'open')]}
        assert cls == {0, 1, 2, 3, 4}, (s, cls)
    # the last shard is one tile of one mark: it belongs to a partition that starts in the tile before it (a single mark cannot be open)
    assert not np.any(shard == 32) and parts['starts'][-1] + parts['sizes'][-1] == M and parts['tile'][-1] == 63 and out[-1] == 'open'
    assert [d for _, d in C.SUBSET['shards_tps2']] == [0, Mo.TIERS, Mo.LARGE, Mo.RECSORT, 0x1800]


# ---- F. the agglomeration's arithmetic ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,n,merged', (('sum_2p38_merges', 64, True), ('sum_2p38_merges_md_90_900', 64, True),
                                           ('sum_2p38_plus_no_merge', 64, False), ('sum_2p38_plus_no_merge_md_90_900', 64, False),
                                           ('sum_32_32_merges', 32, True), ('sum_32_32_no_merge', 32, False),
                                           ('sum_50_50_merges', 50, True), ('sum_50_50_no_merge', 50, False)))
def test_sum_at_the_threshold(name, n, merged):
    marks, kw, parts = get(name)
    assert parts['sizes'].tolist() == [3, 2 * n, 7] and kw['part_max'] == (100 if n == 50 else 128)
    pos, span = Mo.partition_rows(marks, parts, 1)
    d = int(pos.max() - pos.min())
    assert d == (90 if merged else 91) and len(np.unique(pos)) == 2 and len(np.unique(span)) == 1
    # rule 3's fixed point of the pair distance: exactly the threshold 2^26 at 90 bp, above it at 91
    q = float(np.rint(float(d) * (1.0 / 900.0) * (67108864.0 / kw['max_dist'])))
    assert (q == Mo.Q_ONE) == merged and q >= Mo.Q_ONE
    if n == 64 and merged:
        assert n * n * int(q) == Mo.K_FAR
    assert cand_sizes(oracle(name)).tolist() == [3] + ([2 * n] if merged else [n, n]) + [3, 2, 2]
    assert Mo.plan(marks, 0, part_max=kw['part_max'])['cap100'] == (n == 50)


def test_cap100():
    a, b = get('cap100_pm100'), get('cap100_pm101')
    rows = lambda m: np.sort((m['pos'].astype(np.int64) << 20) | m['span'].astype(np.int64))
    assert np.array_equal(rows(a[0]), rows(b[0]))                      # the same marks (each case in a shuffle of its own)
    assert a[2]['sizes'].tolist() == [100, 100, 100, 10, 100, 1] and b[2]['sizes'].tolist() == [100, 101, 101, 8, 101]
    assert Mo.plan(a[0], Mo.WIDE_OFF, part_max=100)['cap100'] and not Mo.plan(b[0], Mo.WIDE_OFF, part_max=101)['cap100']
    assert not Mo.plan(a[0], Mo.WIDE_OFF)['wide'] and Mo.plan(a[0], 0)['wide']
    assert cand_sizes(oracle('cap100_pm100'))[0] == 100


def test_qcap_pair():
    marks, kw, parts = get('qcap_pair')
    assert parts['sizes'].tolist() == [3]
    d = 0.0 * (1.0 / 900.0) + 999999999.0 * (1.0 / 1000000000.0)
    assert np.rint(d * (67108864.0 / kw['max_dist'])) > float(1 << 41)
    assert sorted(cand_sizes(oracle('qcap_pair')).tolist()) == [1, 2]


@pytest.mark.parametrize('name,pm', (('all_singletons_in_full_partitions', 100), ('all_singletons_max_dist_negative', 128)))
def test_all_singletons(name, pm):
    marks, kw, parts = get(name)
    assert len(marks['pos']) == 2049 and parts['natural'].tolist() == [2049]
    assert parts['sizes'].tolist() == [pm] * (2049 // pm) + [2049 % pm]
    assert cand_sizes(oracle(name)).tolist() == [1] * 2049
    if pm == 100:
        assert outcomes(name)[:-1].tolist() == ['open'] * 20


def test_ties_smallest_index():
    marks, kw, parts = get('ties_smallest_index')
    assert parts['sizes'].tolist() == [12]
    pos, span = Mo.partition_rows(marks, parts, 0)
    assert np.diff(pos).tolist() == [10, 10, 80] * 3 + [10, 10] and len(np.unique(span)) == 1
    assert 10 / 900 < kw['max_dist'] < 15 / 900
    # of (0, 10) and (10, 20), exactly as far apart, the pair with the smaller first index merges; the third mark stays alone
    want = oracle('ties_smallest_index')
    assert cand_sizes(want).tolist() == [2, 1] * 4
    assert marks['pos'][want['order']].tolist() == pos.tolist()


# ---- G. candidate numbering -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', (63, 64, 65, 2047, 2048, 2049, 4097))
def test_parts(n):
    marks, kw, parts = get('parts_%d' % n)
    assert len(marks['pos']) == n and parts['sizes'].tolist() == [1] * n
    marks, kw, parts = get('parts_%d_multi' % n)
    assert len(parts['starts']) == n and parts['sizes'].tolist() == [2 * (1 + k % 3) for k in range(n)]
    sizes = cand_sizes(oracle('parts_%d_multi' % n))
    assert len(sizes) == sum(1 + k % 3 for k in range(n)) and np.all(sizes == 2)
    out = outcomes('parts_%d_multi' % n)
    assert np.array_equal(out == 'one', np.arange(n) % 3 == 0)
