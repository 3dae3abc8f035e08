# coding=utf-8
"""No GPU: the numpy reference of the device primitives (tests/prims_ref.py) on inputs small enough to type the answer out, and
every named case of tests/prims_cases.py has the shape it is named for -- tile counts, the launch plan it is meant to take, where
its groups sit relative to tile and window edges -- so that a case cannot silently stop hitting its edge."""
import numpy as np
import pytest

from tests import prims_cases as C
from tests import prims_ref as R

U64 = np.uint64


def u64(*v):
    return np.array(v, dtype=np.uint64)


def u32(*v):
    return np.array(v, dtype=np.uint32)


# -- the reference, by hand -------------------------------------------------------------------------
def test_sort_is_stable():
    keys, vals = R.sort_ref(u64(3, 1, 3, 0, 1, 3), u32(0, 1, 2, 3, 4, 5), key_bits=2)
    assert keys.tolist() == [0, 1, 1, 3, 3, 3]
    assert vals.tolist() == [3, 1, 4, 0, 2, 5]


def test_bits_above_key_bits_are_ignored_and_preserved():
    # key_bits = 4: the order is that of the low hexadecimal digit alone; the digits above it come along on their element
    keys, vals = R.sort_ref(u64(0xF2, 0x11, 0xA2, 0x01, 0x30), u32(10, 11, 12, 13, 14), key_bits=4)
    assert keys.tolist() == [0x30, 0x11, 0x01, 0xF2, 0xA2]
    assert vals.tolist() == [14, 11, 13, 10, 12]


def test_first_shift_leaves_the_bits_below_it_out():
    # bits [4, 8): the second hexadecimal digit; the first one neither orders nor is lost
    keys, vals = R.sort_ref(u64(0x2F, 0x10, 0x21, 0x1E, 0x105), u32(0, 1, 2, 3, 4), key_bits=8, first_shift=4)
    assert keys.tolist() == [0x105, 0x10, 0x1E, 0x2F, 0x21]
    assert vals.tolist() == [4, 1, 3, 0, 2]


def test_all_64_key_bits():
    top = 0xFFFFFFFFFFFFFFFF
    keys, _ = R.sort_ref(u64(top, 1 << 63, 0, (1 << 63) - 1, top), None, key_bits=64)
    assert keys.tolist() == [0, (1 << 63) - 1, 1 << 63, top, top]
    keys, _ = R.sort_ref(u64(top, 1 << 63, 0, (1 << 63) - 1), None, key_bits=63)       # bit 63 is payload now
    assert keys.tolist() == [1 << 63, 0, top, (1 << 63) - 1]


def test_keys_only_and_local_sort():
    assert R.sort_ref(u64(2, 0, 1), None, 8)[1] is None
    # the low 3 bits order, the index above them shows the ties kept their order
    got = R.local_sort_ref(u64(0 << 3 | 5, 1 << 3 | 2, 2 << 3 | 5, 3 << 3 | 2), key_bits=3)
    assert got.tolist() == [1 << 3 | 2, 3 << 3 | 2, 0 << 3 | 5, 2 << 3 | 5]


def test_exclusive_sum_wraps():
    out, total = R.scan_ref(u32(5, 0xFFFFFFFE, 3, 7), 0)
    assert out.tolist() == [0, 5, 3, 6]
    assert total == 13


def test_inclusive_max():
    out, total = R.scan_ref(u32(0, 4, 2, 0x80000000, 9, 0), 1)
    assert out.tolist() == [0, 4, 4, 0x80000000, 0x80000000, 0x80000000]
    assert total == 0x80000000


def test_n_dyn_clamps_and_leaves_the_rest_alone():
    P = C.PREFILL
    v = u32(1, 2, 3, C.BEHIND, C.BEHIND)
    assert R.scan_ref(v, 0, n_dyn=3)[0].tolist() == [0, 1, 3, P, P]
    assert R.scan_ref(v, 0, n_dyn=3)[1] == 6
    assert R.scan_ref(v, 1, n_dyn=2)[0].tolist() == [1, 2, P, P, P]
    assert R.scan_ref(v, 1, n_dyn=2)[1] == 2
    for op in (0, 1):
        out, total = R.scan_ref(v, op, n_dyn=0)
        assert out.tolist() == [P] * 5 and total == 0
    out, total = R.scan_ref(u32(1, 2, 3), 0, n_dyn=8)                              # a count above the bound: the bound holds
    assert out.tolist() == [0, 1, 3] and total == 6


# -- the cases' shapes ------------------------------------------------------------------------------
def test_the_table_of_cases_is_the_issue_s():
    assert len(set(C.SORT_NAMES + C.SORT_BIG_NAMES + C.SORT_CHAIN)) == len(C.SORT_NAMES) + 4 + 6
    assert len(C.SCAN_NAMES) == 2 * (11 + 3 + 12 + 1) + 4 and len(C.SCAN_HUGE_NAMES) == 2
    assert len(C.LOCAL_NAMES) == 2 * (8 + 2 * (2 + 7 + 9))


@pytest.mark.parametrize('name', C.SORT_NAMES + C.SORT_CHAIN)
def test_sort_case_shape(name):
    c = C.sort_case(name)
    keys, n = c['keys'], len(c['keys'])
    assert keys.dtype == np.uint64 and c['tiles'] == -(-n // C.RX_TILE)
    assert 1 <= c['key_bits'] <= 64 and c['first_shift'] < c['key_bits']
    assert c['plan'] == ('scan_spine' if c['force_scan'] else ('rx_offsets' if c['tiles'] <= C.RX_TOTALS_TILES else 'scan_self'))
    if 'kb' in name or 'shift' in name or name.startswith('sort_n'):
        # bits outside the sorted field are there, and differ: they must not order anything and must come back
        if c['key_bits'] < 64 and n > 64:
            assert len(np.unique(keys >> U64(c['key_bits']))) > 1
        if c['first_shift'] and n > 64:
            assert len(np.unique(keys & U64((1 << c['first_shift']) - 1))) > 1
    if n >= 4096 and c['dist'] != 'all_ones' and not name.startswith('sort_sorted') and not name.startswith('sort_reverse'):
        # keys tie in the sorted field (stability shows on the values, and on the bits above key_bits)
        field = (keys >> U64(c['first_shift'])) & U64((1 << (c['key_bits'] - c['first_shift'])) - 1)
        assert len(np.unique(field)) < n
    digits = (keys & U64(0xFF))
    if c['dist'] == 'all_ones':
        assert (keys == U64(0xFFFFFFFFFFFFFFFF)).all() and c['key_bits'] == 64
    if c['dist'] == 'all_equal':
        assert len(np.unique(keys & U64((1 << c['key_bits']) - 1))) == 1
    if c['dist'] == 'two_digits':
        assert sorted(np.unique(digits).tolist()) == [0x35, 0xCA] and (digits[:-1] != digits[1:]).all()
    if c['dist'] == 'uniform_digits':
        assert (np.bincount(digits.astype(np.int64), minlength=256) == n // 256).all() and n % 256 == 0
    if c['dist'] == 'sorted':
        assert (np.diff((keys & U64(0xFFFFFF)).astype(np.int64)) > 0).all()
    if c['dist'] == 'reverse':
        assert (np.diff((keys & U64(0xFFFFFF)).astype(np.int64)) < 0).all()
    if c['dist'] == 'dup256':
        assert 200 <= len(np.unique(keys & U64((1 << 40) - 1))) <= 256


def test_sort_sizes_and_partial_tiles():
    tiles = {n: C.sort_case('sort_n%d' % n)['tiles'] for n in C.SORT_SIZES}
    assert [tiles[n] for n in C.SORT_SIZES] == [1, 1, 1, 1, 1, 1, 1, 2, 8, 8, 10]          # around kDtotCopies = 8: 8 whole, 8 with a partial, 10
    assert any(n % 2 for n in C.SORT_SIZES) and any(n % 2 == 0 for n in C.SORT_SIZES)     # rx_hist loads two keys at a time
    for d in C.SORT_DISTS:
        sizes = [len(C.sort_case(n)['keys']) for n in C.SORT_NAMES if n.startswith('sort_%s_n' % d)]
        assert len(sizes) == 2 and sizes[0] == C.RX_TILE and sizes[1] > C.RX_TILE and sizes[1] % C.RX_TILE, d
    widths = [(kb - fs) % 8 for fs, kb in C.SORT_SHIFTS]
    assert sorted(set(fs for fs, _ in C.SORT_SHIFTS)) == [5, 11, 24] and widths.count(0) == 3 and len(widths) == 6
    assert [len(C.sort_case('sort_force_scan_n%d' % n)['keys']) for n in (1, 4097, 36865)] == [1, 4097, 36865]


def test_sort_tile_boundary_cases():
    """1024 tiles: rx_offsets from the digit totals; 1025: the generic scan over 256 * 1025 counts, 129 scan tiles, spine-less"""
    for kb in (16, 9):
        a, b = C._sort['sort_tiles1024_kb%d' % kb], C._sort['sort_tiles1025_kb%d' % kb]
        assert a[0] == 4194304 and b[0] == 4194305 and a[1] == b[1] == kb
        assert C.sort_plan(a[0], False) == 'rx_offsets' and C.sort_plan(b[0], False) == 'scan_self'
        assert -(-256 * 1025 // C.SCAN_TILE) == 129
    chain = [C._sort[n] for n in C.SORT_CHAIN]
    assert [-(-c[0] // C.RX_TILE) for c in chain] == [9, 3, 1025, 2, 5, 1]
    assert [C.sort_plan(c[0], c[3]) for c in chain] == ['rx_offsets', 'rx_offsets', 'scan_self', 'rx_offsets', 'scan_spine', 'rx_offsets']
    assert chain[2][1] == 16


@pytest.mark.parametrize('name', C.SCAN_NAMES + C.SCAN_HUGE_NAMES)
def test_scan_case_shape(name):
    c = C.scan_case(name, head_only=name in C.SCAN_HUGE_NAMES)
    n, nd = c['n'], c['n_dyn']
    assert c['tiles'] == -(-n // C.SCAN_TILE)
    assert ('force_spine' in name) == c['force_spine']
    assert c['path'] == ('spine' if c['force_spine'] or c['tiles'] > (C.SELF_SPINE_DYN if nd is not None else C.SELF_SPINE) else 'self')
    if name not in C.SCAN_HUGE_NAMES:
        v = c['values']
        assert v.dtype == np.uint32 and len(v) == n
        if nd is not None and nd < n:
            assert (v[nd:] == C.BEHIND).all()
    if name == 'scan_sum_wrap' or name.startswith('scan_sum_n') and n >= 7:
        assert int(c['values'].astype(np.uint64).sum()) >= 1 << 32
    if name == 'scan_max_bit31':
        v = c['values']
        assert (v == 0).any() and (v >= 0x80000000).any() and ((v == 0) | (v >= 0x80000000)).all()
    if name == 'scan_max_zeros':
        assert not c['values'].any()
    if name == 'scan_max_decreasing':
        assert (np.diff(c['values'].astype(np.int64)) < 0).all()
    if name.startswith('scan_max_n') and n > 64:                          # the running maximum changes in the last tile too
        assert len(np.unique(np.maximum.accumulate(c['values'])[-min(n, 2048):])) > 32


def test_scan_plan_boundaries():
    P = {n: C.scan_case(n, head_only=True) for n in C._scan if n.startswith('scan_sum')}
    assert [P['scan_sum_n%d' % n]['tiles'] for n in C.SCAN_SIZES] == [1, 1, 1, 1, 1, 1, 2, 257, 257, 2048, 2049]
    # the SELF carry loop (256 threads over the tiles in front) has a second round from tile 257 on
    assert P['scan_sum_n%d' % (2048 * 2048)]['path'] == 'self' and P['scan_sum_n%d' % (2048 * 2048 + 1)]['path'] == 'spine'
    big = P['scan_sum_force_spine_n%d' % (1025 * 2048 + 3)]
    assert big['tiles'] == 1026 and big['per'] == 2                       # scan_spine: two entries per thread, threads 513 .. 1023 own nothing
    assert 2 * 513 >= big['tiles'] > 2 * 512
    assert P['scan_sum_n%d' % (2048 * 2048 + 1)]['per'] == 3
    assert C.DYN_BOUND == 5 * 2048 + 9 and C.DYN_COUNTS == (0, 1, 2048, 2049, C.DYN_BOUND, C.DYN_BOUND + 5)
    for nd in C.DYN_COUNTS:
        assert P['scan_sum_dyn%d' % nd]['path'] == 'self' and P['scan_sum_force_spine_dyn%d' % nd]['path'] == 'spine'
    a, b = P['scan_sum_dyn_bound_2049_tiles'], P['scan_sum_dyn_bound_16385_tiles']
    assert (a['tiles'], a['path'], a['n_dyn']) == (2049, 'self', 5000)       # spine-less only because of n_dyn
    assert C.scan_path(a['n'], False, False) == 'spine'
    assert (b['tiles'], b['path'], b['n_dyn'], b['per']) == (16385, 'spine', 5000, 17)      # beyond kSelfSpineDyn; more than kHold entries per thread


def groups_of(sorted_keys, lo, key_bits):
    """(start, length) of the runs of keys that agree in the bits [lo, key_bits)"""
    g = (sorted_keys & U64((1 << key_bits) - 1)) >> U64(lo)
    starts = np.flatnonzero(np.concatenate(([True], g[1:] != g[:-1])))
    return list(zip(starts.tolist(), np.diff(np.concatenate((starts, [len(g)]))).tolist()))


@pytest.mark.parametrize('name', C.LOCAL_NAMES)
def test_local_case_shape(name):
    c = C.local_case(name)
    keys, n, lo, kb = c['keys'], len(c['keys']), c['lo'], c['key_bits']
    assert kb == lo + 9 and 1 <= lo < 32 and 1 <= c['cap'] <= C.LOC_HALO and c['threads'] in C.LOCAL_THREADS
    assert ((keys >> U64(kb)) == np.arange(n, dtype=np.uint64)).all()         # the payload: the input index
    want = R.local_sort_ref(keys, kb)
    groups = groups_of(want, lo, kb)
    assert groups == c['groups']                                              # the layout the case was built from is what the sort sees
    for claim in c['claims']:
        assert claim in groups, claim
    low = want & U64((1 << lo) - 1)
    assert len(np.unique(low)) <= 8                                           # a handful of low values: ties are the rule
    if n > 64:
        big = max(groups, key=lambda g: g[1])
        inside = low[big[0]:big[0] + big[1]]
        if big[1] > 8:
            assert len(np.unique(inside)) < len(inside)
        if lo > 20:                                                           # the split compare: values that agree in their low 20 bits
            assert len(np.unique(low & U64(0xFFFFF))) < len(np.unique(low))
    # the input is not already in order
    if n > 64:
        assert not np.array_equal(keys, want)


def test_local_group_lengths_and_placement():
    def case(fmt, lo=11, t=256):
        return C.local_case(fmt % (lo, t))
    for lo in C.LOCAL_LO:
        c = case('local_lo%d_cap256_t%d', lo)
        lengths = sorted(g[1] for g in c['claims'])
        assert lengths == sorted([256, 257, 255, 256, 257] + (list(C.LONG_GROUPS) if lo >= 8 else []))
        assert len(c['keys']) > (19000 if lo >= 8 else 7000)
        assert (lo <= 20) == (lo in (1, 8, 11, 16, 17, 20))
    assert [-(-lo // 8) for lo in C.LOCAL_LO] == [1, 1, 2, 2, 3, 3, 3, 4]         # rx_big's LSD passes; the last digit is partial but for 8 and 16
    for lo in (11, 21):
        for cap in (3, 128):
            lengths = [g[1] for g in case('local_lo%%d_cap%d_t%%d' % cap, lo)['claims']]
            assert cap in lengths and cap + 1 in lengths and 3000 in lengths
        for n in C.LOCAL_N:
            assert len(case('local_lo%%d_n%d_t%%d' % n, lo)['keys']) == n
        T, W = C.LOC_TILE, C.LOC_TILE + C.LOC_HALO
        assert case('local_lo%d_start0_len256_t%d', lo)['claims'] == [(0, 256)]
        assert case('local_lo%d_start2048_len200_t%d', lo)['claims'] == [(T, 200)]                  # window position 2048 of tile 0 = position 0 of tile 1
        c = case('local_lo%d_start2047_len128_cap128_t%d', lo)
        assert c['claims'] == [(T - 1, 128)] and c['cap'] == 128 and T < T - 1 + 128 < W           # a group of cap keys that ends inside the halo
        c = case('local_lo%d_start2047_len256_t%d', lo)
        assert c['claims'] == [(T - 1, 256)] and T - 1 + 256 == W - 1 == 2303                    # ... that ends at position 2303 of the window
        c = case('local_lo%d_start2047_len257_t%d', lo)
        assert c['claims'] == [(T - 1, 257)] and T - 1 + 257 == W                                # one more: its end is the window's last head
        assert case('local_lo%d_start4095_len256_t%d', lo)['claims'] == [(2 * T - 1, 256)]
        for fmt, length in (('local_lo%d_ends_at_n_len100_t%d', 100), ('local_lo%d_ends_at_n_len1500_t%d', 1500),
                            ('local_lo%d_last_single_t%d', 1)):
            c = case(fmt, lo)
            (start, got), = c['claims']
            assert got == length and start + length == len(c['keys']) and c['groups'][-1] == (start, length)
            assert len(c['keys']) % T
    # both thread counts see the same kinds of input
    assert sorted(n.replace('_t1024', '') for n in C.LOCAL_NAMES if n.endswith('_t1024')) == \
        sorted(n.replace('_t256', '') for n in C.LOCAL_NAMES if n.endswith('_t256'))
