# coding=utf-8
"""Named inputs for the device primitives of duet_amd/csrc/duet_prims.hip.h, one per plan boundary ("The primitives'
plan boundaries").  Every case is generated from a synth.SplitMix stream seeded by its name; tests/test_prims_ref_host.py shows on
the CPU that each has the shape it is named for, tests/test_gpu_prims.py runs every one of them on the device.

    sort_case(name)   -> dict(keys u64[n], key_bits, first_shift, force_scan, tiles)
    scan_case(name)   -> dict(values u32[n], op, n_dyn or None, force_spine, tiles, path, per)
    local_case(name)  -> dict(keys u64[n], key_bits, lo, cap, threads, groups [(start, length)] in sorted order, claims)
"""
import zlib

import numpy as np

from duet_amd.synth import SplitMix

# duet_prims.hip.h
RX_TILE, RX_TOTALS_TILES, DTOT_COPIES = 4096, 1024, 8
SCAN_TILE, SELF_SPINE, SELF_SPINE_DYN, SPINE_THREADS = 2048, 2048, 16384, 1024
LOC_TILE, LOC_HALO, BIG_LDS = 2048, 256, 1024
PREFILL, BEHIND = 0xA5A5A5A5, 0xFFFFFFFF          # out before the scan; in behind the real count


def _rng(name):
    return SplitMix(zlib.crc32(name.encode()))


def _high(rng, n, key_bits):
    """random bits above key_bits"""
    if key_bits >= 64:
        return np.zeros(n, dtype=np.uint64)
    return (rng.u64(n) >> np.uint64(key_bits)) << np.uint64(key_bits)


def _low_mask(key_bits):
    return np.uint64((1 << key_bits) - 1)


# ---------------------------------------------------------------------------------------------
# radix_sort_pairs
# ---------------------------------------------------------------------------------------------
SORT_SIZES = (1, 2, 63, 64, 65, 4095, 4096, 4097, 7 * 4096 + 5, 8 * 4096, 9 * 4096 + 1)
SORT_KEY_BITS = (1, 7, 8, 9, 16, 17, 33, 63, 64)
SORT_SHIFTS = ((5, 21), (5, 18), (11, 27), (11, 30), (24, 40), (24, 37))      # (first_shift, key_bits): 16 bits and not a multiple of 8
SORT_DISTS = ('all_equal', 'all_ones', 'two_digits', 'uniform_digits', 'sorted', 'reverse', 'dup256')

_sort = {}                                         # name -> (n, key_bits, first_shift, force_scan, dist)
for _n in SORT_SIZES:
    _sort['sort_n%d' % _n] = (_n, 20, 0, False, 'random')
for _kb in SORT_KEY_BITS:
    for _n in (4097, 9 * 4096 + 1):
        _sort['sort_kb%d_n%d' % (_kb, _n)] = (_n, _kb, 0, False, 'random' if _kb < 33 else 'pool')
for _fs, _kb in SORT_SHIFTS:
    _sort['sort_shift%d_kb%d' % (_fs, _kb)] = (9 * 4096 + 1, _kb, _fs, False, 'random')
for _n in (1, 4097, 9 * 4096 + 1):
    _sort['sort_force_scan_n%d' % _n] = (_n, 20, 0, True, 'random')
for _d in SORT_DISTS:
    for _n in (4096, 4352 if _d == 'uniform_digits' else 3 * 4096 + 1):      # a whole tile; a partial last tile
        _sort['sort_%s_n%d' % (_d, _n)] = (_n, {'all_equal': 24, 'all_ones': 64, 'two_digits': 8, 'uniform_digits': 8, 'sorted': 24,
                                                'reverse': 24, 'dup256': 40}[_d], 0, False, _d)
SORT_NAMES = tuple(_sort)
# the 1024-tile boundary (pairs only, in a test of their own)
for _t, _n in ((1024, 1024 * 4096), (1025, 1024 * 4096 + 1)):
    for _kb in (16, 9):
        _sort['sort_tiles%d_kb%d' % (_t, _kb)] = (_n, _kb, 0, False, 'random')
SORT_BIG_NAMES = tuple(n for n in _sort if n.startswith('sort_tiles'))
# one context, one sort after the other (the digit totals are zero between sorts whatever the plan of the last one)
_sort['sort_chain_9_tiles'] = (9 * 4096 - 7, 20, 0, False, 'random')
_sort['sort_chain_3_tiles'] = (2 * 4096 + 1, 12, 0, False, 'random')
_sort['sort_chain_1025_tiles'] = (1024 * 4096 + 9, 16, 0, False, 'random')
_sort['sort_chain_2_tiles'] = (4096 + 100, 17, 0, False, 'random')
_sort['sort_chain_5_tiles_force_scan'] = (4 * 4096 + 3, 20, 0, True, 'random')
_sort['sort_chain_1_tile'] = (777, 9, 0, False, 'random')
SORT_CHAIN = ('sort_chain_9_tiles', 'sort_chain_3_tiles', 'sort_chain_1025_tiles', 'sort_chain_2_tiles', 'sort_chain_5_tiles_force_scan',
              'sort_chain_1_tile')


def sort_plan(n, force_scan):
    """which launches give the tile offsets: 'rx_offsets' (digit totals), 'scan_self' or 'scan_spine' (the generic scan)"""
    tiles = (n + RX_TILE - 1) // RX_TILE
    if tiles <= RX_TOTALS_TILES and not force_scan:
        return 'rx_offsets'
    return 'scan_' + scan_path(256 * tiles, False, force_scan)


def sort_case(name):
    n, key_bits, first_shift, force_scan, dist = _sort[name]
    rng = _rng(name)
    high = _high(rng, n, key_bits)
    i = np.arange(n, dtype=np.uint64)
    if dist == 'random':
        keys = rng.u64(n)                                                      # (64 random bits: those above key_bits and below first_shift too)
        high = np.zeros(n, dtype=np.uint64)
    elif dist == 'pool':                                                       # wide keys that still tie: 1024 distinct values
        pool = rng.u64(1024) & _low_mask(key_bits)
        keys = pool[rng.below(n, 1024)]
    elif dist == 'all_equal':
        keys = np.full(n, 0x5A5A5A, dtype=np.uint64)
    elif dist == 'all_ones':
        keys = np.full(n, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    elif dist == 'two_digits':
        keys = np.where(i % np.uint64(2) == 0, np.uint64(0x35), np.uint64(0xCA))
    elif dist == 'uniform_digits':
        keys = np.argsort(rng.u64(256)).astype(np.uint64)[(i % np.uint64(256)).astype(np.int64)]
    elif dist == 'sorted':
        keys = i * np.uint64(3)
    elif dist == 'reverse':
        keys = (np.uint64(n - 1) - i) * np.uint64(3)
    else:
        assert dist == 'dup256', dist
        pool = rng.u64(256) & _low_mask(key_bits)
        keys = pool[rng.below(n, 256)]
    return dict(keys=(keys | high).astype(np.uint64), key_bits=key_bits, first_shift=first_shift, force_scan=force_scan, dist=dist,
                tiles=(n + RX_TILE - 1) // RX_TILE, plan=sort_plan(n, force_scan))


# ---------------------------------------------------------------------------------------------
# launch_scan
# ---------------------------------------------------------------------------------------------
OPS = ('sum', 'max')
SCAN_SIZES = (1, 7, 8, 9, 2047, 2048, 2049, 256 * 2048 + 1, 257 * 2048, 2048 * 2048, 2048 * 2048 + 1)
SCAN_SPINE_SIZES = (1, 2049, 1025 * 2048 + 3)
DYN_BOUND = 5 * 2048 + 9
DYN_COUNTS = (0, 1, 2048, 2049, DYN_BOUND, DYN_BOUND + 5)
DYN_HEAD = 5000                                                                # the real count of the two cases with a large bound

_scan = {}                                         # name -> (n, op, n_dyn, force_spine, dist)
for _op in OPS:
    for _n in SCAN_SIZES:
        _scan['scan_%s_n%d' % (_op, _n)] = (_n, _op, None, False, _op)
    for _n in SCAN_SPINE_SIZES:
        _scan['scan_%s_force_spine_n%d' % (_op, _n)] = (_n, _op, None, True, _op)
    for _nd in DYN_COUNTS:
        _scan['scan_%s_dyn%d' % (_op, _nd)] = (DYN_BOUND, _op, _nd, False, _op)
        _scan['scan_%s_force_spine_dyn%d' % (_op, _nd)] = (DYN_BOUND, _op, _nd, True, _op)
    _scan['scan_%s_dyn_bound_2049_tiles' % _op] = (2049 * 2048, _op, DYN_HEAD, False, _op)
_scan['scan_sum_wrap'] = (2 * 2048 + 5, 'sum', None, False, 'wrap')
_scan['scan_max_bit31'] = (2 * 2048 + 5, 'max', None, False, 'bit31')
_scan['scan_max_zeros'] = (2 * 2048 + 5, 'max', None, False, 'zeros')
_scan['scan_max_decreasing'] = (2 * 2048 + 5, 'max', None, False, 'decreasing')
SCAN_NAMES = tuple(_scan)
# a bound beyond kSelfSpineDyn tiles: 134 MB, filled once for both operations in a test of its own
for _op in OPS:
    _scan['scan_%s_dyn_bound_16385_tiles' % _op] = (16385 * 2048, _op, DYN_HEAD, False, _op)
SCAN_HUGE_NAMES = tuple(n for n in _scan if n.endswith('_16385_tiles'))


def scan_path(n, has_dyn, force_spine):
    """launch_scan's choice: 'self' (two launches, every block combines the tiles before it) or 'spine' (three)"""
    nb = (n + SCAN_TILE - 1) // SCAN_TILE
    if nb >= 1 and (nb <= SELF_SPINE or (has_dyn and nb <= SELF_SPINE_DYN)) and not force_spine:
        return 'self'
    return 'spine'


def scan_values(dist, n, rng):
    if dist == 'sum':                              # the whole range: the running total wraps about every other element
        return rng.u64(n).astype(np.uint32)
    if dist == 'max':                              # a noisy ramp: the running maximum keeps changing to the end
        return (np.arange(n, dtype=np.uint64) * np.uint64(8) + (rng.u64(n) & np.uint64(0xFFF))).astype(np.uint32)
    if dist == 'wrap':
        return (np.uint64(0x7FFFFFF0) + (rng.u64(n) & np.uint64(0x3F))).astype(np.uint32)
    if dist == 'bit31':                            # zeros, and values with bit 31 set that grow slowly
        v = np.uint64(0x80000000) + np.arange(n, dtype=np.uint64) * np.uint64(5) + (rng.u64(n) & np.uint64(0x1FF))
        return np.where(rng.chance(n, 1, 3), np.uint64(0), v).astype(np.uint32)
    if dist == 'zeros':
        return np.zeros(n, dtype=np.uint32)
    assert dist == 'decreasing', dist
    return (np.uint64(0xFFFFFFFF) - np.arange(n, dtype=np.uint64) * np.uint64(7)).astype(np.uint32)


def scan_case(name, head_only=False):
    """head_only: the elements in front of the real count only (the caller fills the rest of a large bound with BEHIND)"""
    n, op, n_dyn, force_spine, dist = _scan[name]
    rng = _rng(name)
    live = n if n_dyn is None else min(n, n_dyn)
    head = scan_values(dist, live, rng)
    values = head
    if not head_only and live < n:
        values = np.full(n, BEHIND, dtype=np.uint32)
        values[:live] = head
    nb = (n + SCAN_TILE - 1) // SCAN_TILE
    return dict(values=values, n=n, op=OPS.index(op), n_dyn=n_dyn, force_spine=force_spine, tiles=nb,
                path=scan_path(n, n_dyn is not None, force_spine), per=(nb + SPINE_THREADS - 1) // SPINE_THREADS)


# ---------------------------------------------------------------------------------------------
# global passes + rx_local + rx_big
# ---------------------------------------------------------------------------------------------
# A case is a LAYOUT: the lengths of its groups in sorted order.  key_bits = lo + 9, so a case has at most 512 groups; the
# fillers between the groups a case is about hold 1 .. 60 keys.
LOCAL_LO = (1, 8, 11, 16, 17, 20, 21, 31)          # <= 20: one packed compare per key; rx_big's 1, 1, 2, 2, 3, 3, 3, 4 LSD passes
LOCAL_CAPS = (3, 128, 256)
LOCAL_N = (1, 2047, 2048, 2049, 2304, 2305, 4097)
LOCAL_THREADS = (256, 1024)
LONG_GROUPS = (1023, 1024, 1025, 3000)             # with lo >= 8


def _fill(rng, total, longest=60):
    """group lengths of 1 .. longest that add up to total"""
    out = []
    while total > 0:
        g = min(total, 1 + rng.one(longest))
        out.append(g)
        total -= g
    return out


def _composed(rng, lo, cap):
    """every group length the kernels tell apart, fillers in between, about 20 k keys with the long groups"""
    named = [cap, cap + 1, 255, 256, 257] + (list(LONG_GROUPS) if lo >= 8 else [])
    order = np.argsort(rng.u64(len(named)))
    layout, claims = [], []
    for k in order:
        layout += _fill(rng, 1100 + rng.one(300))
        claims.append((sum(layout), named[k]))
        layout.append(named[k])
    layout += _fill(rng, 1100 + rng.one(300))
    return layout, claims


def _placed(rng, start, length, tail):
    """fillers up to `start`, a group of `length` keys there, `tail` keys of fillers behind it"""
    layout = _fill(rng, start)
    return layout + [length] + _fill(rng, tail), [(start, length)]


_local = {}                                        # name -> (lo, cap, threads, layout builder)
for _t in LOCAL_THREADS:
    for _lo in LOCAL_LO:
        _local['local_lo%d_cap256_t%d' % (_lo, _t)] = (_lo, 256, _t, lambda r, lo=_lo: _composed(r, lo, 256))
    for _lo in (11, 21):
        for _cap in (3, 128):
            _local['local_lo%d_cap%d_t%d' % (_lo, _cap, _t)] = (_lo, _cap, _t, lambda r, lo=_lo, cap=_cap: _composed(r, lo, cap))
        for _n in LOCAL_N:
            _local['local_lo%d_n%d_t%d' % (_lo, _n, _t)] = (_lo, 256, _t, lambda r, n=_n: (_fill(r, n), []))
        # where a group sits: at the start of a tile's window, on its last position, on the first position of the halo
        _local['local_lo%d_start0_len256_t%d' % (_lo, _t)] = (_lo, 256, _t, lambda r: _placed(r, 0, 256, 2100))
        _local['local_lo%d_start2048_len200_t%d' % (_lo, _t)] = (_lo, 256, _t, lambda r: _placed(r, 2048, 200, 2100))
        _local['local_lo%d_start2047_len128_cap128_t%d' % (_lo, _t)] = (_lo, 128, _t, lambda r: _placed(r, 2047, 128, 2100))   # ends inside the halo
        _local['local_lo%d_start2047_len256_t%d' % (_lo, _t)] = (_lo, 256, _t, lambda r: _placed(r, 2047, 256, 2100))          # ends at position 2303
        _local['local_lo%d_start2047_len257_t%d' % (_lo, _t)] = (_lo, 256, _t, lambda r: _placed(r, 2047, 257, 2100))          # ends on the window's end: rx_big's
        _local['local_lo%d_start4095_len256_t%d' % (_lo, _t)] = (_lo, 256, _t, lambda r: _placed(r, 4095, 256, 900))           # the same in the second tile
        _local['local_lo%d_ends_at_n_len100_t%d' % (_lo, _t)] = (_lo, 256, _t, lambda r: _placed(r, 2200, 100, 0))
        _local['local_lo%d_ends_at_n_len1500_t%d' % (_lo, _t)] = (_lo, 256, _t, lambda r: _placed(r, 2200, 1500, 0))           # rx_big's bisection ends at n
        _local['local_lo%d_last_single_t%d' % (_lo, _t)] = (_lo, 256, _t, lambda r: _placed(r, 2304, 1, 0))
LOCAL_NAMES = tuple(_local)


def low_values(lo):
    """the handful of low-bit values a case draws from (ties are the rule): both ends, values that differ above bit 20 only"""
    top = (1 << lo) - 1
    return sorted(set(v & top for v in (0, 1, top, top - 1, 1 << (lo - 1), 0x55555555, 3 << max(lo - 2, 0), 1 << max(lo - 11, 0))))


def local_case(name):
    lo, cap, threads, build = _local[name]
    rng = _rng(name)
    layout, claims = build(rng)
    n, groups = sum(layout), len(layout)
    assert groups <= 512, (name, groups)
    key_bits = lo + 9
    group_id = np.sort(np.argsort(rng.u64(512))[:groups]).astype(np.uint64)    # the groups' numbers: ascending, spread over the 9 bits
    top = np.repeat(group_id, layout)
    vals = np.array(low_values(lo), dtype=np.uint64)
    low = vals[rng.below(n, len(vals))]
    slot = np.argsort(rng.u64(n))                                              # input position i holds the key of sorted-order slot[i]
    index = np.arange(n, dtype=np.uint64)                                      # the payload above key_bits: the input index
    keys = (index << np.uint64(key_bits)) | (top[slot] << np.uint64(lo)) | low[slot]
    starts = np.concatenate(([0], np.cumsum(layout)[:-1])).astype(np.int64)
    return dict(keys=keys.astype(np.uint64), key_bits=key_bits, lo=lo, cap=cap, threads=threads,
                groups=list(zip(starts.tolist(), layout)), claims=claims)
