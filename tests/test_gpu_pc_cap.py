# coding=utf-8
"""-m gpu: the PC cap as a run parameter of the feature export (duet_amd/csrc/duet_tune_cap.hip: duet_ef_features_cap_*,
duet_svim_features_cap_*), of the sweep (tune.sweep_settings(pc_cap=..), `tune --pc_cap`) and of the single-GPU product run
(`duet --pc_cap`).  The reference is tests/pc_cap_ref.py: the oracle's own filter, classes, seed sets and vote with its PC_MAX set
per call; for caps at or below 8100 the product is also pinned to the unpatched oracle through demoted PC tags."""
import ctypes
import json
import math
import os
import re
import shutil
import sys

import numpy as np
import pytest

from duet_amd import _lib, engine, evaluation, svim_mode, synth, tune
from duet_amd.native import NativeIngest
from duet_amd.read_file import init_chrom_list
from tests import helpers as H
from tests import pc_cap_ref, soa_fuzz, tune_ref

pytestmark = pytest.mark.gpu

FIELDS = ('kept', 'eligible', 'cls', 'hap1', 'hap2', 'hap0', 'allhap', 't1', 't2', 'ps', 'deg', 'svread', 'refread')
VOTE = ('eligible', 'hap1', 'hap2', 'hap0', 'allhap', 't1', 't2', 'ps')
CAP_MAX = (1 << 30) - 3
CAPS = (0, 1, 972, 8099, 8100, 8101, 9720, CAP_MAX)
ABSENT = engine.MARK_ABSENT
SAT = (1 << 30) - 2                  # the saturated pc of the tag word: never votes


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


# ---- the four ways to a feature array, each with its status --------------------------------------------------------------------

def cap_host(ctx, soa, cap, s=0, r=0, fill=0):
    prob, keep = _lib.problem_from_arrays(soa, s, r)
    out = np.full(soa.n_cands * _lib.FEATURE_DTYPE.itemsize, fill, dtype=np.uint8).view(_lib.FEATURE_DTYPE)
    rc = ctx.lib.duet_ef_features_cap_host(ctx.handle, ctypes.byref(prob), ctypes.c_uint32(cap), _lib._ptr(out))
    del keep
    return rc, out


def plain_host(ctx, soa, s=0, r=0):
    prob, keep = _lib.problem_from_arrays(soa, s, r)
    out = np.zeros(soa.n_cands, dtype=_lib.FEATURE_DTYPE)
    rc = ctx.lib.duet_ef_features_host(ctx.handle, ctypes.byref(prob), _lib._ptr(out))
    del keep
    return rc, out


class Resident(object):
    """An EfSoA in HBM and a feature buffer behind it, for the _device entries."""

    def __init__(self, soa, s=0, r=0):
        import torch
        from duet_amd.devmem import DeviceProblem
        self.torch, self.soa = torch, soa
        self.dp = DeviceProblem(soa, s, r, device='cuda:0')
        self.size = max(soa.n_cands, 1) * _lib.FEATURE_DTYPE.itemsize
        self.buf = torch.zeros(self.size + 64, dtype=torch.uint8, device='cuda:0')

    def run(self, ctx, cap, fill=0):
        self.buf.fill_(fill)
        stream = self.torch.cuda.current_stream().cuda_stream
        if cap is None:
            rc = ctx.lib.duet_ef_features_device(ctx.handle, ctypes.byref(self.dp.problem), ctypes.c_void_p(self.buf.data_ptr()),
                                                 ctypes.c_void_p(stream))
        else:
            rc = ctx.lib.duet_ef_features_cap_device(ctx.handle, ctypes.byref(self.dp.problem), ctypes.c_uint32(cap),
                                                     ctypes.c_void_p(self.buf.data_ptr()), ctypes.c_void_p(stream))
        self.torch.cuda.synchronize()
        n = self.soa.n_cands * _lib.FEATURE_DTYPE.itemsize
        return rc, self.buf[:n].cpu().numpy().view(_lib.FEATURE_DTYPE).copy()


def assert_fields(got, want, what):
    for name in FIELDS:
        g = got[name].astype(np.int64)
        w = np.array([x[name] for x in want], dtype=np.int64)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, '%s: %s differs at %s: %s vs %s' % (what, name, bad[:5], g[bad[:5]], w[bad[:5]])


def status_of(want):
    return _lib.DUET_ERR_DIV_ZERO if any(w['eligible'] and w['svread'] + w['refread'] == 0 for w in want) else _lib.DUET_OK


def check_caps(ctx, soa, caps, s=0, r=0):
    """Both entries against the reference, field by field and status by status, for every cap -> {cap: records}."""
    res, out = Resident(soa, s, r), {}
    for cap in caps:
        want = pc_cap_ref.features(soa, s, r, cap)
        rc_h, host = cap_host(ctx, soa, cap, s, r)
        rc_d, dev = res.run(ctx, cap)
        assert_fields(host, want, 'cap %d, _host' % cap)
        assert host.tobytes() == dev.tobytes(), 'cap %d: _device differs from _host' % cap
        assert rc_h == rc_d == status_of(want), (cap, rc_h, rc_d, status_of(want))
        out[cap] = host
    return out


# ---- fuzz problems: against the existing entries at 8100, against the reference at every cap ----------------------------------------

FUZZ = [('fuzz%d' % s, dict(seed=s, n_contigs=4)) for s in range(6)] + [('divzero', dict(seed=47, n_contigs=2, allow_divzero=True))]


@pytest.fixture(scope='module')
def fuzz_soas():
    return {name: soa_fuzz.random_soa(**kw) for name, kw in FUZZ}


@pytest.mark.parametrize('name', [f[0] for f in FUZZ])
def test_cap_8100_equals_the_existing_entries_byte_for_byte(ctx, fuzz_soas, name):
    soa = fuzz_soas[name]
    res = Resident(soa)
    for s, r in ((50, 2), (0, 0)):
        res.dp.problem.svlen_thres, res.dp.problem.suppread_thres = s, r
        rc0, want = plain_host(ctx, soa, s, r)
        rc1, host = cap_host(ctx, soa, 8100, s, r)
        rc2, dev = res.run(ctx, 8100)
        rc3, dev0 = res.run(ctx, None)
        assert rc0 == rc1 == rc2 == rc3, (rc0, rc1, rc2, rc3)
        assert want.tobytes() == host.tobytes() == dev.tobytes() == dev0.tobytes()
        if name == 'divzero' and r == 0:
            assert rc0 == _lib.DUET_ERR_DIV_ZERO


@pytest.mark.parametrize('name', [f[0] for f in FUZZ])
def test_caps_on_fuzz_problems(ctx, fuzz_soas, name):
    soa = fuzz_soas[name]
    got = check_caps(ctx, soa, CAPS, 0, 0)
    # the caps are different problems
    assert got[0].tobytes() != got[8100].tobytes() and got[8099].tobytes() != got[8100].tobytes()
    assert got[9720].tobytes() != got[8100].tobytes()


@pytest.mark.parametrize('cap', [CAP_MAX + 1, 0xFFFFFFFF])
def test_a_cap_the_tag_word_cannot_hold_is_refused_and_nothing_is_written(ctx, fuzz_soas, cap):
    soa = fuzz_soas['fuzz0']
    rc, out = cap_host(ctx, soa, cap, fill=0xAB)
    assert rc == _lib.DUET_ERR_INVALID and 'pc_cap' in ctx.last_error()
    assert np.all(out.view(np.uint8) == 0xAB)
    rc, out = Resident(soa).run(ctx, cap, fill=0xAB)
    assert rc == _lib.DUET_ERR_INVALID and np.all(out.view(np.uint8) == 0xAB)
    for bad in (cap, -1, 8100.0, '8100', True):
        with pytest.raises(ValueError):
            ctx.features_host(soa, 0, 0, pc_cap=bad)
    # the largest legal cap, through the Python entry
    want = pc_cap_ref.features(soa, 0, 0, CAP_MAX)
    assert_fields(ctx.features_host(soa, 0, 0, pc_cap=CAP_MAX), want, 'Context.features_host')


# ---- hand-built problems ---------------------------------------------------------------------------------------------------------

def cand(pos, marks, svlen=100, svread=5, refread=5, gt=1):
    """marks: (hap, pc, ps), None for a mark without a tag, or ('raw', read index)."""
    return dict(pos=pos, marks=marks, svlen=svlen, svread=svread, refread=refread, gt=gt)


def build(contigs):
    """contigs: one list of cand() per contig.  Every tagged mark gets a read of its own."""
    tags, marks, off, ctg_off = [], [], [0], [0]
    cols = dict(pos=[], svlen=[], svread=[], refread=[], gt=[])
    for cs in contigs:
        for c in cs:
            for m in c['marks']:
                if m is None:
                    marks.append(ABSENT)
                else:
                    marks.append(len(tags))
                    tags.append(m)
            off.append(len(marks))
            for k in cols:
                cols[k].append(c[k])
        ctg_off.append(len(cols['pos']))
    t = np.array(tags, dtype=np.int64).reshape(-1, 3)
    return engine.EfSoA(cand_ctg_off=ctg_off, read_tag=engine.pack_tags(t[:, 0], t[:, 1], t[:, 2]), cand_pos=cols['pos'],
                        cand_svlen=cols['svlen'], cand_svread=cols['svread'], cand_refread=cols['refread'], cand_gt_ok=cols['gt'],
                        cand_off=off, mark_read=np.array(marks, dtype=np.uint32))


V = (1, 100, 7)                        # a voter under any cap >= 100, phase set 7
HAND_CAPS = (0, 99, 100, 101, 4999, 5000, 8100, 8999, 9000, CAP_MAX)


def seeded(ps, pc=100, pos=10, n=1):
    """n class-1 candidates whose marks all carry `ps` and vote from cap `pc` on."""
    return [cand(pos + i, [(1 + i % 2, pc, ps), (2, pc, ps)]) for i in range(n)]


def test_no_candidate_and_one_candidate(ctx):
    empty = build([[]])
    assert empty.n_cands == 0
    for cap in (0, 8100, CAP_MAX):
        rc, out = cap_host(ctx, empty, cap)
        assert rc == _lib.DUET_OK and len(out) == 0
        assert Resident(empty).run(ctx, cap)[0] == _lib.DUET_OK
    assert cap_host(ctx, empty, CAP_MAX + 1)[0] == _lib.DUET_ERR_INVALID
    got = check_caps(ctx, build([[cand(5, [V])]]), HAND_CAPS)
    assert got[99]['eligible'][0] == 0 and got[100]['eligible'][0] == 1 and got[100]['ps'][0] == 7


@pytest.mark.parametrize('K,empty', [(1, ()), (2, (0,)), (2, (1,)), (65, (0, 31, 32, 64)), (65, tuple(range(1, 64)))])
def test_contig_counts_and_empty_contigs(ctx, K, empty):
    contigs = [[] if k in empty else seeded(1000 + k, pc=100 if k % 2 else 5000, pos=50 * k, n=1 + k % 3) +
               [cand(50 * k + 7, [None]), cand(50 * k + 9, [(1, 100, 1000 + k), (2, 100, 3)])] for k in range(K)]
    got = check_caps(ctx, build(contigs), HAND_CAPS)
    e99, e100, e5000 = (int(got[cap]['eligible'].sum()) for cap in (99, 100, 5000))
    assert 0 == e99 <= e100 <= e5000 and e5000 > 0
    if K - len(empty) > 2:
        assert 0 < e100 < e5000


def test_a_contig_loses_its_only_seed_below_a_cap_and_gains_its_first_above_8100(ctx):
    """Contig 0's only seed votes from 5000 on, contig 1's from 9000 on, contig 2 keeps one throughout.  Below its cap every
    candidate of a contig is ineligible: its vote fields read zero (kept, cls, deg, svread and refread are the candidate's own,
    as in the records of the existing entry)."""
    soa = build([seeded(11, pc=5000) + [cand(40, [None], svread=9, refread=1), cand(60, [(1, 50, 11), (2, 60, 12)])],
                 seeded(21, pc=9000) + [cand(45, [None]), cand(70, [(1, 50, 21), (2, 50, 22)])],
                 seeded(31, pc=0) + [cand(80, [None])]])
    got = check_caps(ctx, soa, HAND_CAPS)
    c0, c1 = slice(0, 3), slice(3, 6)
    for cap in HAND_CAPS:
        for sl, first in ((c0, 5000), (c1, 9000)):
            f = got[cap][sl]
            if cap < first:
                assert all(not f[n].any() for n in VOTE), (cap, first)
                assert f['kept'].all() and list(f['deg']) == [2, 1, 2] and list(f['cls']) == [1, 0, 2]
            else:
                assert f['eligible'].all(), (cap, first)
        assert got[cap][6:]['eligible'].all()
    assert got[8100][c1]['eligible'].sum() == 0 and got[9000][c1]['eligible'].sum() == 3


def test_the_same_ps_as_a_seed_of_two_contigs_and_300_candidates_sharing_one(ctx):
    soa = build([seeded(77, n=300) + [cand(5, [None])], seeded(77) + seeded(78) + [cand(1 << 20, [None])], seeded(5000000, n=3)])
    got = check_caps(ctx, soa, (99, 100, 8100))
    assert got[100]['ps'][300] == 77 and got[100]['ps'][303] == 78 and got[100]['eligible'].all()


@pytest.mark.parametrize('n', [1, 2, 255, 256, 257, 2049])
def test_distinct_seeds_in_a_contig(ctx, n):
    """n seeds 1000, 1010, ..: class-0 candidates take the nearest (a tie goes to the larger), class-2 candidates vote among
    those of their PS values that are seeds.  Half of the seeds appear only from cap 5000 on."""
    ps = [1000 + 10 * i for i in range(n)]
    cs = []
    for i in reversed(range(n)):                                            # (descending: the sort has work to do)
        cs += seeded(ps[i], pc=100 if i % 2 == 0 else 5000, pos=i)
    cs += [cand(p, [None]) for p in (0, 999, 1005, 1004, 1006, ps[-1], ps[-1] + 5, ps[-1] + 6, ps[n // 2] + 5, 1 << 31)]
    cs += [cand(3, [(1, 100, ps[n // 2]), (1, 100, ps[n // 2]), (2, 100, ps[-1]), (2, 100, 5)]),
           cand(4, [(1, 100, 4), (2, 100, 6)])]
    got = check_caps(ctx, build([cs, seeded(1)]), (99, 100, 4999, 5000, CAP_MAX))
    assert int(got[5000]['eligible'].sum()) == len(cs) + 1
    if n >= 2:
        assert got[5000]['ps'][n + 2] == 1010 and got[100]['ps'][n + 2] == 1000       # pos 1005: the tie goes to the larger


def test_class_one_voters_first_and_last_and_none(ctx):
    soa = build([[cand(10, [(1, 9000, 7), (2, 5000, 7), None, (1, 100, 7)]),      # the first tagged mark is above the cap, the last votes
                  cand(20, [(1, 9000, 100), (2, SAT, 100)]),                      # class 1, never a voter below 9000: no seed from it
                  cand(150, [(1, SAT, 300)]),                                     # class 1 without any voter, ever
                  cand(30, [(2, 100, 200)])]])
    got = check_caps(ctx, soa, HAND_CAPS)
    f = got[100]
    assert list(f['cls']) == [1, 1, 1, 1] and f['eligible'].all()
    assert (f['hap1'][0], f['hap2'][0], f['t1'][0], f['ps'][0]) == (1, 0, 100, 7)
    # seeds {7, 200}: candidate 2 at 150 has no voter and takes the nearest seed; from 9000 on the seeds are {7, 100, 200} and
    # 150 lies between 100 and 200: the larger
    assert f['ps'][2] == 200 and got[9000]['ps'][2] == 200 and got[9000]['hap1'][1] == 1
    assert got[CAP_MAX]['allhap'][2] == 0 and got[CAP_MAX]['allhap'][1] == 1      # a saturated pc never votes
    assert not got[99]['eligible'].any()


@pytest.mark.parametrize('deg', [1, 63, 64, 65, 1024, 1025, 2049])
def test_degrees_with_the_only_voter_first_or_last(ctx, deg):
    other = [(2, 9000, 7)] * (deg - 1)
    multi = [(2, 9000, 8 + i % 3) for i in range(deg - 1)]
    soa = build([[cand(10, [V] + other), cand(20, other + [V]), cand(30, [V] + multi), cand(40, multi + [V]),
                  cand(50, [None] * (deg - 1) + [V]), cand(60, [(1, 100, 9)] + [None] * (deg - 1))]])
    got = check_caps(ctx, soa, (99, 100, 8999, 9000))
    assert got[100]['eligible'].all() and list(got[100]['hap1']) == [1] * 6 and list(got[100]['deg']) == [deg] * 6


def test_pc_equal_to_the_cap_and_one_above(ctx):
    for P in (0, 972, 8100, CAP_MAX):
        soa = build([[cand(10, [(1, P, 7), (2, P + 1, 7)]), cand(20, [(2, P + 1, 7), (2, P + 1, 7)]), cand(30, [(1, P, 8), (2, P + 1, 9)])]])
        got = check_caps(ctx, soa, [c for c in (P - 1, P, P + 1) if 0 <= c <= CAP_MAX])
        f = got[P]
        assert (f['hap1'][0], f['hap2'][0], f['t1'][0], f['t2'][0]) == (1, 0, P, 0) and f['allhap'][1] == 0 and f['allhap'][2] == 1


def test_class_two(ctx):
    """Seeds 7, 8 (from 100), 9 (from 5000).  Candidate a: PS 7 has two voters from 100 on, PS 9 three from 5000 on -- the winner
    changes.  b: one voter each of 8 and 7 -- a tie, the first seen (8) wins.  c: voters whose PS (50, 60) is no seed -- hap0
    stays 0 and ps is the nearest seed.  d: hap 3 beside hap 1 in class 1."""
    soa = build([seeded(7, pos=7) + seeded(8, pos=8) + seeded(9, pc=5000, pos=9) + [
        cand(100, [(1, 100, 7), (2, 100, 7), (2, 5000, 9), (2, 5000, 9), (1, 5000, 9), None]),
        cand(200, [(1, 100, 8), (2, 100, 7), (2, 9000, 7)]),
        cand(8, [(1, 100, 50), (2, 100, 60), (1, 100, 50)]),
        cand(300, [(3, 100, 7), (1, 100, 7), (3, 5000, 7)])]])
    got = check_caps(ctx, soa, HAND_CAPS)
    a, b, c, d = 3, 4, 5, 6
    assert got[100]['ps'][a] == 7 and got[5000]['ps'][a] == 9 and got[5000]['hap0'][a] == 2 and got[5000]['allhap'][a] == 5
    assert got[100]['ps'][b] == 8 and got[9000]['ps'][b] == 7
    assert got[100]['hap0'][c] == 0 and got[100]['allhap'][c] == 3 and got[100]['ps'][c] == 8
    assert (got[5000]['hap1'][d], got[5000]['hap2'][d], got[5000]['allhap'][d]) == (1, 0, 1)


def test_absent_marks_reads_past_the_table_and_extreme_ps(ctx):
    big = (1 << 32) - 2
    soa = build([[cand(10, [None, (1, 100, 0), None]), cand(20, [(2, 100, big), None]), cand((1 << 31) + 10, [None, None]),
                  cand(30, [(1, 100, 0), (2, 100, big)]), cand(40, [(1, 100, 5), None])]])
    want = {cap: pc_cap_ref.features(soa, 0, 0, cap) for cap in (99, 100)}
    # a read index at and past n_reads counts as a mark without a tag (the reference's candidates were built with None there)
    soa.mark_read[np.nonzero(soa.mark_read == ABSENT)[0][[0, 3]]] = [soa.n_reads, 0xFFFFFFFE]
    res = Resident(soa)
    for cap in (99, 100):
        rc_h, host = cap_host(ctx, soa, cap)
        rc_d, dev = res.run(ctx, cap)
        assert rc_h == rc_d == _lib.DUET_OK
        assert_fields(host, want[cap], 'cap %d' % cap)
        assert host.tobytes() == dev.tobytes()
    assert sorted(set(int(x) for x in host['ps'])) == [0, 5, big] and host['ps'][2] == big


def test_div_zero_depends_on_the_cap(ctx):
    """The candidate with svread + refread == 0 sits on a contig whose only seed votes from 5000 on: DUET_OK below, and
    DUET_ERR_DIV_ZERO -- with the records written -- from there on."""
    soa = build([seeded(7, pc=5000) + [cand(50, [None], svread=0, refread=0)], seeded(9)])
    got = check_caps(ctx, soa, HAND_CAPS)                   # (the statuses are compared with the reference's in there)
    assert cap_host(ctx, soa, 4999)[0] == _lib.DUET_OK and cap_host(ctx, soa, 5000)[0] == _lib.DUET_ERR_DIV_ZERO
    assert got[5000]['eligible'][1] == 1 and got[4999]['eligible'][1] == 0 and got[4999]['eligible'][2] == 1
    with pytest.raises(ZeroDivisionError):
        ctx.features_host(soa, 0, 0, pc_cap=5000)
    assert ctx.features_host(soa, 0, 0, pc_cap=4999).tobytes() == got[4999].tobytes()


# ---- one context, many calls ---------------------------------------------------------------------------------------------------

def test_cap_calls_leave_the_context_as_they_found_it(ctx, fuzz_soas):
    large = soa_fuzz.random_soa(11, n_contigs=6, cands_per_contig=(800, 1500))
    small, third = fuzz_soas['fuzz1'], fuzz_soas['fuzz2']
    fresh = _lib.Context(0)
    try:
        want_large = cap_host(fresh, large, 300)
        want_small = cap_host(fresh, small, 9720)
    finally:
        fresh.close()
    fresh = _lib.Context(0)
    try:
        want_ef = fresh.run_host(third, 0, 0)
        want_seeds = [fresh.seed_ps(k) for k in range(third.n_contigs)]
    finally:
        fresh.close()
    one = _lib.Context(0)
    try:
        a = cap_host(one, large, 300)
        b = cap_host(one, small, 9720)
        ef = one.run_host(third, 0, 0)
        seeds = [one.seed_ps(k) for k in range(third.n_contigs)]
        c = cap_host(one, large, 300)
        seeds_after = [one.seed_ps(k) for k in range(third.n_contigs)]
        plain_after = plain_host(one, third)
    finally:
        one.close()
    for got, want in ((a, want_large), (b, want_small), (c, want_large)):
        assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes()
    assert np.array_equal(ef[0], want_ef[0]) and np.array_equal(ef[1], want_ef[1])
    assert sum(len(s) for s in want_seeds) > 0
    for k in range(third.n_contigs):
        assert np.array_equal(seeds[k], want_seeds[k]) and np.array_equal(seeds_after[k], want_seeds[k]), k
    rc, want_plain = plain_host(ctx, third)
    assert plain_after[0] == rc and plain_after[1].tobytes() == want_plain.tobytes()


# ---- the fused pipeline's entries ----------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def svim_home(tmp_path_factory):
    """A work directory of BAMs only, its raw marks, and the E/F problem the fused pipeline adapts from them at -c 0.9, -s 50, -r 2:
    the callset the product run writes, read back (as tests/test_gpu_tune_grid.py obtains it)."""
    root = tmp_path_factory.mktemp('pc_cap_svim')
    home, copy = str(root / 'w'), str(root / 'copy')
    synth.write_svim_workdir(home, H.case_contigs('genome_small', 5), 5)
    shutil.copytree(home, copy)
    svim_mode.sv_phasing_from_bams(copy, 50, 2, 4, False, 0.9, 0, write_sv_calls=True)
    soa, _ = tune._candidates(copy, 50, 2, False, 4)
    ing, got = NativeIngest.extract(home + '/snp_phasing/', init_chrom_list(False, home), 4, 50, 20, 1000)
    assert ing is not None, got
    ing.close()
    return dict(home=home, copy=copy, soa=soa, marks=got, plain=open(copy + '/phased_sv.vcf', 'rb').read(),
                plain_calls=open(svim_mode.callset_path(copy), 'rb').read())


def svim_device(ctx, got, cap):
    import torch
    from duet_amd.devmem import DeviceSvim
    ds = DeviceSvim(got, got['read_tag'], got['depth'], got['depth_off'], 1000, 50, 2, max_dist=0.9, device='cuda:0')
    buf = torch.zeros(len(got['pos']) * _lib.FEATURE_DTYPE.itemsize + 64, dtype=torch.uint8, device='cuda:0')
    n = ds.run_features(ctx, buf.data_ptr(), pc_cap=cap)
    return buf[:n * _lib.FEATURE_DTYPE.itemsize].cpu().numpy().view(_lib.FEATURE_DTYPE).copy(), ds.fetch()


def test_svim_entries(ctx, svim_home):
    got, soa = svim_home['marks'], svim_home['soa']
    args = (got, got['read_tag'], got['depth'], got['depth_off'], 1000, 50, 2)
    plain = ctx.svim_features_host(*args, max_dist=0.9)
    assert len(plain['feat']) == soa.n_cands and int(plain['feat']['eligible'].sum()) > 100
    plain_dev, plain_res = svim_device(ctx, got, None)
    assert plain_dev.tobytes() == plain['feat'].tobytes()
    seen = {}
    for cap in (8100, 300, 9720):
        host = ctx.svim_features_host(*args, max_dist=0.9, pc_cap=cap)
        dev, res = svim_device(ctx, got, cap)
        assert host['feat'].tobytes() == dev.tobytes(), cap
        for k in ('cand_off', 'cand_contig', 'cand_type', 'cand_pos', 'cand_span'):      # the clustering does not see the cap
            assert np.array_equal(host[k], plain[k]) and np.array_equal(res[k], plain_res[k]), (cap, k)
        if cap == 8100:
            assert host['feat'].tobytes() == plain['feat'].tobytes()
        else:
            assert_fields(host['feat'], pc_cap_ref.features(soa, 50, 2, cap), 'svim, cap %d' % cap)
        seen[cap] = host['feat']
    assert seen[300].tobytes() != seen[8100].tobytes() != seen[9720].tobytes()
    for bad in (CAP_MAX + 1, -1):
        with pytest.raises(ValueError):
            ctx.svim_features_host(*args, max_dist=0.9, pc_cap=bad)
    p, r, out, _, n, keep = ctx._svim_host_problem(*args, 0.9, 1000, 100, 900.0, False)
    feat = np.full(len(got['pos']) * _lib.FEATURE_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    rc = ctx.lib.duet_svim_features_cap_host(ctx.handle, ctypes.byref(p), ctypes.byref(r), ctypes.c_uint32(CAP_MAX + 1), _lib._ptr(feat))
    assert rc == _lib.DUET_ERR_INVALID and np.all(feat == 0xAB)


# ---- command lines -----------------------------------------------------------------------------------------------------------

def read(path):
    with open(path, 'rb') as f:
        return f.read()


def evaluate(truth, called):
    """The unmodified evaluator's ten numbers -- an exception of its own stays an exception here."""
    return evaluation.evaluation(evaluation.parse_vcf(truth, False, ''), evaluation.parse_vcf(called, False, ''), 1000, 0.0)


def demoted_copy(src, dst, cap):
    """A copy of a work directory whose `samtools view` texts have every PC:i: value in (cap, 8100] rewritten to 8101."""
    shutil.copytree(src, dst)
    d = os.path.join(dst, 'snp_phasing')
    n = 0
    for name in sorted(os.listdir(d)):
        if name.endswith('.bam'):
            os.remove(os.path.join(d, name))
            continue

        def sub(m):
            nonlocal n
            hit = cap < int(m.group(1)) <= 8100
            n += hit
            return 'PC:i:8101' if hit else m.group(0)

        with open(os.path.join(d, name)) as f:
            text = re.sub(r'PC:i:(\d+)', sub, f.read())
        with open(os.path.join(d, name), 'w') as f:
            f.write(text)
    return n


@pytest.fixture(scope='module')
def golden_home(tmp_path_factory):
    from tests.test_c_oracle import materialise_bams
    home = str(tmp_path_factory.mktemp('pc_cap_golden') / 'w')
    shutil.copytree(os.path.join(H.GOLDEN, 'cases', 'fuzz_cutesv_s2'), home)
    materialise_bams(home)
    return home


def test_tune_command_with_caps(ctx, golden_home, tmp_path):
    from tests.test_gpu_tune_grid import write_truth
    home = golden_home
    soa, txt = tune._candidates(home, 50, 2, False, 2)
    truth = str(tmp_path / 'truth.vcf')
    write_truth(dict(pos=soa.cand_pos, svlen=soa.cand_svlen, **txt), truth, 3)
    grid = [{}, {'c1_max_ref_num': 3}, {'c2_min_sv_ratio': 0.6, 'c0_min_sv_num': 2, 'c1_twohap_sv_ratio_1': 0.2}]
    with open(str(tmp_path / 'g.json'), 'w') as f:
        json.dump(grid, f)
    out = lambda name: str(tmp_path / name)
    tune.main([home, truth, '--grid', out('g.json'), '--out', out('plain.tsv')])
    tune.main([home, truth, '--grid', out('g.json'), '--out', out('caps.tsv'), '--pc_cap', '2400,8100'])
    plain = [ln.split('\t') for ln in read(out('plain.tsv')).decode().splitlines()]
    caps = [ln.split('\t') for ln in read(out('caps.tsv')).decode().splitlines()]
    assert caps[0] == ['pc_cap'] + plain[0] and [r[0] for r in caps[1:]] == ['2400'] * 3 + ['8100'] * 3
    assert [r[1:] for r in caps[4:]] == plain[1:]                          # 8100: the run without the flag, minus the column
    called = out('called.vcf')
    for g, row, row_8100 in zip(grid, caps[1:4], caps[4:]):
        v = tune.vector(g)
        for cap, r in ((2400, row), (8100, row_8100)):
            with open(called, 'w') as f:
                f.write(pc_cap_ref.phased_text(home, 50, 2, v, cap))
            want = evaluate(truth, called)                                   # numbers, not an exception, at both caps
            assert not any(math.isnan(x) for x in want), (cap, want)
            assert tune_ref.same_floats([float(x) for x in r[1 + len(tune.NAMES):]], [float(x) for x in want]), (cap, g, want, r)
        assert row[1:] != row_8100[1:]


def test_product_run_with_a_cap_native_ingest(golden_home, tmp_path):
    """`duet --pc_cap 2400` against the pinned oracle, with no patched constant: its text on a copy of the work directory whose
    PC tags in (2400, 8100] read 8101."""
    from duet_amd.sv_phasing import sv_phasing
    from oracle import ef_oracle as O
    home = golden_home
    sv_phasing(home, 50, 2, 4, False)
    plain = read(home + '/phased_sv.vcf')
    sv_phasing(home, 50, 2, 4, False, pc_cap=8100)
    assert read(home + '/phased_sv.vcf') == plain
    demoted = str(tmp_path / 'demoted')
    assert demoted_copy(home, demoted, 2400) > 20
    want = O.sv_phasing_text(demoted, 50, 2)
    sv_phasing(home, 50, 2, 4, False, pc_cap=2400)
    got = read(home + '/phased_sv.vcf')
    assert got == want.encode() and got != plain
    # with a vector, and with the cap taken from the thresholds file the way the command takes it (the flag wins)
    v = tune.vector({'c1_max_ref_num': 3, 'c0_min_sv_num': 2})
    sv_phasing(home, 50, 2, 4, False, thresholds=v, pc_cap=2400)
    assert read(home + '/phased_sv.vcf').decode() == pc_cap_ref.phased_text(home, 50, 2, v, 2400)
    sv_phasing(home, 50, 2, 4, False)
    assert read(home + '/phased_sv.vcf') == plain


def test_duet_command_takes_the_cap_from_the_flag_or_the_thresholds_file(golden_home, tmp_path, monkeypatch):
    """cli.main up to the last stage: the external stages and the input checks are replaced, SV phasing runs."""
    from duet_amd import cli, stages
    home = golden_home
    for name in ('snp_calling', 'sv_calling', 'snp_phasing'):
        monkeypatch.setattr(stages, name, lambda *a: None)
    monkeypatch.setattr(cli, 'check_envs', lambda *a: None)
    monkeypatch.setattr(cli, 'set_logging', lambda *a: None)
    vec = str(tmp_path / 'v.json')
    with open(vec, 'w') as f:
        json.dump({'c1_max_ref_num': 3, 'pc_cap': 2400}, f)
    v = tune.vector({'c1_max_ref_num': 3})
    for extra, want in ((['--pc_cap', '2400'], pc_cap_ref.phased_text(home, 50, 2, tune.vector(), 2400)),
                        (['--thresholds', vec], pc_cap_ref.phased_text(home, 50, 2, v, 2400)),
                        (['--thresholds', vec, '--pc_cap', '972'], pc_cap_ref.phased_text(home, 50, 2, v, 972))):
        monkeypatch.setattr(sys, 'argv', ['duet', 'in.bam', 'ref.fa', home] + extra)
        cli.main(None)
        assert read(home + '/phased_sv.vcf').decode() == want, extra


def test_product_run_with_a_cap_svim_gpu(ctx, svim_home):
    """`duet -b svim-gpu --pc_cap P [--write_sv_calls]`: 8100 is the run without the flag; 2400 gives the rows svim_mode.rows_text
    writes for the reference's (pred, ps) on the adapted problem."""
    copy, soa = svim_home['copy'], svim_home['soa']
    for calls in (False, True):
        svim_mode.sv_phasing_from_bams(copy, 50, 2, 4, False, 0.9, 0, write_sv_calls=calls, pc_cap=8100)
        assert read(copy + '/phased_sv.vcf') == svim_home['plain']
        if calls:
            assert read(svim_mode.callset_path(copy)) == svim_home['plain_calls']
    want_feat = pc_cap_ref.features(soa, 50, 2, 2400)
    v = tune.vector()
    pred = np.array([tune_ref.decide_vec(w['cls'], w['svread'], w['refread'], w['deg'], w['hap1'], w['hap2'], w['hap0'], w['allhap'],
                                         w['t1'], w['t2'], v) if w['eligible'] else 0 for w in want_feat], dtype=np.uint8)
    res = ctx.svim_features_host(svim_home['marks'], svim_home['marks']['read_tag'], svim_home['marks']['depth'],
                                 svim_home['marks']['depth_off'], 1000, 50, 2, max_dist=0.9)
    chroms = init_chrom_list(False, copy)
    rows = svim_mode.rows_text(copy, dict(chroms=chroms, cand_contig=res['cand_contig'], cand_type=res['cand_type'],
                                          cand_pos=res['cand_pos'], cand_span=res['cand_span'], pred=pred,
                                          ps=np.array([w['ps'] if w['eligible'] else 0 for w in want_feat], dtype=np.uint32)))
    want = (svim_mode.header_text(copy, chroms) + rows).encode()
    assert want != svim_home['plain'] and rows.count('\n') > 100
    for calls in (False, True):
        svim_mode.sv_phasing_from_bams(copy, 50, 2, 4, False, 0.9, 0, write_sv_calls=calls, pc_cap=2400)
        assert read(copy + '/phased_sv.vcf') == want
        assert read(svim_mode.callset_path(copy)) == svim_home['plain_calls']           # the cap does not touch the calls
    svim_mode.sv_phasing_from_bams(copy, 50, 2, 4, False, 0.9, 0, write_sv_calls=True)
    assert read(copy + '/phased_sv.vcf') == svim_home['plain']
