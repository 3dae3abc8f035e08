# coding=utf-8
"""-m gpu: the device primitives every unit is built on (duet_amd/csrc/duet_prims.hip.h) -- radix_sort_pairs, launch_scan, and the
local sort rx_local + rx_big behind global passes -- run on their own through the diagnostic entries of include/duet_ef.h and
compared, exactly, with numpy (tests/prims_ref.py) on every named case of tests/prims_cases.py: one per plan boundary
(tests/test_prims_ref_host.py shows on the CPU that each case sits on its edge).  One context serves the whole module, so every
sort also meets the digit totals as the sort before it left them, whatever its plan was."""
import numpy as np
import pytest

from duet_amd import _lib
from tests import prims_cases as C
from tests import prims_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def same(case, field, got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape and np.array_equal(got, want):
        return
    assert got.shape == want.shape, (case, field, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    raise AssertionError('%s: %s differs at %d of %d places, first at %s: got %s, expected %s' % (
        case, field, len(bad), len(want), bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist()))


# -- radix_sort_pairs ---------------------------------------------------------------------------------
def check_sort(ctx, name, pairs):
    c = C.sort_case(name)
    keys = c['keys']
    vals = np.arange(len(keys), dtype=np.uint32) if pairs else None
    want_keys, want_vals = R.sort_ref(keys, vals, c['key_bits'], c['first_shift'])
    got_keys, got_vals = ctx.prims_sort(keys, vals, c['key_bits'], c['first_shift'], c['force_scan'])
    case = '%s (%s)' % (name, 'pairs' if pairs else 'keys only')
    same(case, 'keys', got_keys, want_keys)
    if pairs:
        same(case, 'vals', got_vals, want_vals)
    else:
        assert got_vals is None


@pytest.mark.parametrize('mode', ('pairs', 'keys'))
@pytest.mark.parametrize('name', C.SORT_NAMES)
def test_sort(ctx, name, mode):
    check_sort(ctx, name, mode == 'pairs')


@pytest.mark.parametrize('name', C.SORT_BIG_NAMES)
def test_sort_at_the_1024_tile_boundary(ctx, name):
    check_sort(ctx, name, True)


def test_sorts_one_after_the_other_in_one_context():
    """9 tiles, 3, 1025, 2, 5 with the generic scan forced, 1: every plan finds the digit totals zero and leaves them so"""
    own = _lib.Context(0)
    try:
        for name in C.SORT_CHAIN:
            check_sort(own, name, True)
        for name in reversed(C.SORT_CHAIN):
            if name != 'sort_chain_1025_tiles':
                check_sort(own, name, False)
    finally:
        own.close()


# -- launch_scan ----------------------------------------------------------------------------------
def check_scan(ctx, name, c):
    want, want_total = R.scan_ref(c['values'], c['op'], c['n_dyn'], C.PREFILL)
    got, total, zero14 = ctx.prims_scan(c['values'], c['op'], c['n_dyn'], c['force_spine'], C.PREFILL)
    same(name, 'out', got, want)
    assert total == want_total, (name, 'total', total, want_total)
    same(name, 'zero14', zero14, np.zeros(14, dtype=np.uint32))


@pytest.mark.parametrize('name', C.SCAN_NAMES)
def test_scan(ctx, name):
    check_scan(ctx, name, C.scan_case(name))


def test_scan_with_a_bound_beyond_the_spine_less_reach(ctx):
    """16385 tiles of bound, 5000 real elements: the spine path although n_dyn is given.  One 134 MB input for both operations."""
    values = None
    for name in C.SCAN_HUGE_NAMES:
        c = C.scan_case(name, head_only=True)
        if values is None:
            values = np.full(c['n'], C.BEHIND, dtype=np.uint32)
        values[:len(c['values'])] = c['values']
        check_scan(ctx, name, dict(c, values=values))


# -- global passes, rx_local, rx_big --------------------------------------------------------------------
@pytest.mark.parametrize('name', C.LOCAL_NAMES)
def test_local_sort(ctx, name):
    c = C.local_case(name)
    want = R.local_sort_ref(c['keys'], c['key_bits'])
    got = ctx.prims_local_sort(c['keys'], c['key_bits'], c['lo'], c['cap'], c['threads'])
    same(name, 'keys', got, want)


# -- the entries' own argument checks: nothing is launched --------------------------------------------------
def test_empty_inputs_and_arguments_outside_the_preconditions(ctx):
    none64, none32 = np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32)
    keys, vals = ctx.prims_sort(none64, none32, 8)
    assert len(keys) == 0 and len(vals) == 0
    out, total, zero14 = ctx.prims_scan(none32, 0)
    assert len(out) == 0 and total == 0 and (zero14 == 1).all()              # n == 0: not even the 14 words are touched
    assert len(ctx.prims_local_sort(none64, 20, 11)) == 0
    k = np.arange(8, dtype=np.uint64)
    for bad in (dict(key_bits=0), dict(key_bits=65), dict(key_bits=8, first_shift=8), dict(key_bits=8, first_shift=40)):
        with pytest.raises(_lib.DuetLibraryError):
            ctx.prims_sort(k, None, **bad)
    with pytest.raises(_lib.DuetLibraryError):
        ctx.prims_scan(np.arange(8, dtype=np.uint32), 2)
    for bad in (dict(key_bits=20, lo=0), dict(key_bits=41, lo=32), dict(key_bits=11, lo=11), dict(key_bits=65, lo=11),
                dict(key_bits=20, lo=11, cap=0), dict(key_bits=20, lo=11, cap=257), dict(key_bits=20, lo=11, threads=512)):
        with pytest.raises(_lib.DuetLibraryError):
            ctx.prims_local_sort(k, **bad)
    lib, h = ctx.lib, ctx.handle
    assert lib.duet_prims_sort_host(h, None, None, 8, 8, 0, 0, k.ctypes.data, None) == _lib.DUET_ERR_INVALID
    assert lib.duet_prims_sort_host(h, k.ctypes.data, None, 8, 8, 0, 0, None, None) == _lib.DUET_ERR_INVALID
    assert lib.duet_prims_scan_host(h, None, 8, 0, 0xFFFFFFFF, 0, None, None, None) == _lib.DUET_ERR_INVALID
    assert lib.duet_prims_local_sort_host(h, None, 8, 20, 11, 256, 256, k.ctypes.data) == _lib.DUET_ERR_INVALID
    # the context still works
    same('after the refusals', 'keys', ctx.prims_sort(k[::-1].copy(), None, 8)[0], k)
