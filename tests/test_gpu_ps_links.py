# coding=utf-8
"""-m gpu: the phase-set links (duet_amd/csrc/duet_pslinks.hip) against tests/ps_links_ref.py, record for record and bit for bit
(np.array_equal on the structured array): the smallest shapes at which each stage can go wrong, the contracts of the four
entries, and `duet --write_ps_links` in both modes.

The random problems are the five soa_fuzz.random_soa calls of RANDOM.  At -s 50 -r 2 and the reference's cap each of them must
yield at least one link, the first two all three kinds each, and the five together all three kinds: a generator change cannot
empty them unnoticed.  (A single problem cannot be asked for all three kinds at every setting: the last one holds ONE candidate
and so one link, and cap 0 leaves next to no voter anywhere.)"""
import ctypes
import os
import shutil
import sys

import numpy as np
import pytest

from duet_amd import _lib, ps_links, svim_mode, synth, tune
from duet_amd.read_file import init_chrom_list
from oracle import c_oracle
from tests import helpers as H
from tests import ps_links_ref as R
from tests import soa_fuzz, svim_fuzz, svim_ref

pytestmark = pytest.mark.gpu

DT = _lib.PS_LINK_DTYPE
ABSENT = 0xFFFFFFFF
CAP_MAX = (1 << 30) - 3


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


class Soa(object):
    """The arrays of one problem without engine.EfSoA's validation: what the entries have to survive (a read index beyond the tag
    table, candidates without marks) can be stated here."""

    def __init__(self, **kw):
        for name, dt in (('cand_ctg_off', np.uint32), ('read_tag', np.uint64), ('cand_pos', np.uint32), ('cand_svlen', np.uint32),
                         ('cand_svread', np.uint32), ('cand_refread', np.uint32), ('cand_gt_ok', np.uint8), ('cand_off', np.uint32),
                         ('mark_read', np.uint32)):
            setattr(self, name, np.ascontiguousarray(kw[name], dtype=dt))

    n_contigs = property(lambda self: len(self.cand_ctg_off) - 1)
    n_cands = property(lambda self: len(self.cand_pos))
    n_marks = property(lambda self: len(self.mark_read))
    n_reads = property(lambda self: len(self.read_tag))


def tag(hap, pc, ps):
    return (hap << 62) | (pc << 32) | ps


def build(contigs, n_reads=None):
    """contigs: a list of candidate lists; a candidate is dict(marks=[...], pos=, svlen=, svread=, gt=); a mark is (hap, pc, ps) --
    a read of its own --, ('again', i) -- the read of the candidate's i-th mark once more --, 'absent', 'untagged' (a read whose
    tag word is all-ones) or ('raw', index)."""
    tags, marks, off, cols, ctg_off = [], [], [0], dict(pos=[], svlen=[], svread=[], gt=[]), [0]
    for cands in contigs:
        for c in cands:
            mine = []
            for m in c['marks']:
                if m == 'absent':
                    mine.append(ABSENT)
                elif m == 'untagged':
                    tags.append(R.UNTAGGED)
                    mine.append(len(tags) - 1)
                elif m[0] == 'again':
                    mine.append(mine[m[1]])
                elif m[0] == 'raw':
                    mine.append(m[1])
                else:
                    tags.append(tag(*m))
                    mine.append(len(tags) - 1)
            marks += mine
            off.append(len(marks))
            cols['pos'].append(c.get('pos', 1000))
            cols['svlen'].append(c.get('svlen', 100))
            cols['svread'].append(c.get('svread', 5))
            cols['gt'].append(c.get('gt', 1))
        ctg_off.append(len(cols['pos']))
    if n_reads is not None:
        tags = (tags + [tag(1, 0, 1)] * n_reads)[:n_reads]
    C = len(cols['pos'])
    return Soa(cand_ctg_off=ctg_off, read_tag=np.array(tags, dtype=np.uint64), cand_pos=cols['pos'], cand_svlen=cols['svlen'],
               cand_svread=cols['svread'], cand_refread=np.zeros(C), cand_gt_ok=cols['gt'], cand_off=off,
               mark_read=np.array(marks, dtype=np.uint32))


def check(ctx, soa, s=50, r=2, cap=None):
    """The device's records equal the reference's, bit for bit -> the records."""
    got = ctx.ps_links_host(soa, s, r, pc_cap=cap)
    want = R.records(R.links(soa, s, r, R.PC_MAX if cap is None else cap), DT)
    assert got.dtype == DT and got.tobytes() == want.tobytes(), (got, want)
    assert np.array_equal(got, want)
    return got


def one(marks, **kw):
    return build([[dict(marks=marks, **kw)]])


def fields(rec):
    return tuple(int(rec[f]) for f in ('contig', 'ps_a', 'ps_b', 'n_sv', 'n_same', 'n_flip', 'n_open', 'w_same', 'w_flip', 'pos_min', 'pos_max'))


# ---- empty problems ----------------------------------------------------------------------------------------------------------------

def test_empty_problems(ctx):
    none = build([[]])
    assert none.n_cands == 0 and len(check(ctx, none)) == 0
    assert len(check(ctx, build([[], [], []]))) == 0
    no_marks = build([[dict(marks=[]), dict(marks=[])]])
    assert no_marks.n_cands == 2 and no_marks.n_marks == 0 and len(check(ctx, no_marks)) == 0
    single = build([[dict(marks=[(1, 0, 7), (2, 0, 7), (1, 0, 7)]), dict(marks=[(1, 0, 9)])], [dict(marks=['absent'])]])
    assert len(check(ctx, single)) == 0                                        # voters, but no candidate with two phase sets


# ---- one candidate, two marks in two phase sets --------------------------------------------------------------------------------------

def test_same_flip_open(ctx):
    got = check(ctx, one([(1, 0, 10), (1, 0, 20)], pos=77))
    assert [fields(x) for x in got] == [(0, 10, 20, 1, 1, 0, 0, 1, 0, 77, 77)]
    got = check(ctx, one([(2, 0, 20), (2, 0, 10)]))                            # both haplotype 2: the same sign
    assert [fields(x) for x in got] == [(0, 10, 20, 1, 1, 0, 0, 1, 0, 1000, 1000)]
    got = check(ctx, one([(1, 0, 10), (2, 0, 20)]))
    assert [fields(x) for x in got] == [(0, 10, 20, 1, 0, 1, 0, 0, 1, 1000, 1000)]
    got = check(ctx, one([(1, 0, 10), (2, 0, 10), (1, 0, 20)]))                # a tie inside the first group
    assert [fields(x) for x in got] == [(0, 10, 20, 1, 0, 0, 1, 0, 0, 1000, 1000)]
    got = check(ctx, one([(1, 0, 10), (2, 0, 20), (1, 0, 20)]))                # ... inside the second
    assert [fields(x)[3:9] for x in got] == [(1, 0, 0, 1, 0, 0)]
    assert got['reserved'].tolist() == [0]


def test_who_votes(ctx):
    assert len(check(ctx, one([(1, 0, 10), (3, 0, 20)]))) == 0                 # the second group's only voter has hap 3
    assert len(check(ctx, one([(1, 0, 10), (0, 0, 20)]))) == 0                 # (hap field 0 is no haplotype either)
    assert len(check(ctx, one([(1, 0, 10), (3, 0, 20), (2, 0, 20)]))) == 1     # hap 3 beside a voter: the voter counts
    assert len(check(ctx, one([(1, 0, 10), 'absent']))) == 0
    assert len(check(ctx, one([(1, 0, 10), 'absent', (1, 0, 20)]))) == 1
    assert len(check(ctx, one([(1, 0, 10), 'untagged']))) == 0
    assert len(check(ctx, one([(1, 0, 10), 'untagged', (1, 0, 20)]))) == 1
    soa = one([(1, 0, 10), ('raw', 1), (1, 0, 20)])                            # read 1 is the third mark's: two groups
    assert len(check(ctx, soa)) == 1
    for beyond in (1, 2, 0xFFFFFFFE):                                          # a read index that is not in the tag table
        soa = one([(1, 0, 10), ('raw', beyond)])
        assert soa.n_reads == 1 and len(check(ctx, soa)) == 0
        soa = one([(1, 0, 10), ('raw', max(beyond, 2)), (1, 0, 20)])
        assert soa.n_reads == 2 and len(check(ctx, soa)) == 1
    got = check(ctx, one([(1, 0, 10), ('again', 0), (2, 0, 20)]))              # one read marked twice counts twice: d = 2, -1
    assert [fields(x)[3:9] for x in got] == [(1, 0, 1, 0, 0, 1)]
    got = check(ctx, one([(1, 0, 10), ('again', 0), (1, 0, 20), ('again', 2), ('again', 2)]))
    assert [fields(x)[3:9] for x in got] == [(1, 1, 0, 0, 2, 0)]


@pytest.mark.parametrize('P', [0, 8100, CAP_MAX])
def test_pc_at_the_cap_and_one_above(ctx, P):
    at = one([(1, P, 10), (1, P, 20)])
    above = one([(1, P, 10), (1, P + 1, 20)])
    assert len(check(ctx, at, cap=P)) == 1 and len(check(ctx, above, cap=P)) == 0
    if P == 8100:
        assert len(check(ctx, at)) == 1 and len(check(ctx, above)) == 0        # no cap given: the reference's
    if P:
        assert len(check(ctx, at, cap=P - 1)) == 0


def test_the_three_filter_terms(ctx):
    marks = [(1, 0, 10), (2, 0, 20)]
    assert len(check(ctx, one(marks, svlen=50, svread=2), 50, 2)) == 1
    assert len(check(ctx, one(marks, svlen=49, svread=2), 50, 2)) == 0
    assert len(check(ctx, one(marks, svlen=50, svread=1), 50, 2)) == 0
    assert len(check(ctx, one(marks, svlen=50, svread=2, gt=0), 50, 2)) == 0
    assert len(check(ctx, one(marks, svlen=0, svread=0), 0, 0)) == 1
    assert len(check(ctx, one(marks, svlen=0, svread=0, gt=0), 0, 0)) == 0


# ---- groups per candidate, degree ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('G', [1, 2, 3, 63, 64, 65, 129])
def test_groups_per_candidate(ctx, G):
    rng = np.random.default_rng(G)
    pss = np.unique(rng.integers(0, 2 ** 32 - 1, 4 * G).astype(np.uint64))[:G]
    rng.shuffle(pss)
    assert len(pss) == G
    marks = [(int(rng.integers(1, 3)), 0, int(ps)) for ps in pss for _ in range(int(rng.integers(1, 4)))]
    rng.shuffle(marks)
    before = dict(marks=[(1, 0, 5), (1, 0, 6)], pos=3)
    got = check(ctx, build([[before, dict(marks=[tuple(m) for m in marks], pos=9)]]))
    mine = got[got['pos_min'] == 9]
    assert len(mine) == G - 1 and len(got) == G
    order = np.sort(pss)
    assert np.array_equal(mine['ps_a'], order[:-1]) and np.array_equal(mine['ps_b'], order[1:])       # neighbours only
    assert np.all(mine['n_sv'] == 1)


def test_degrees(ctx):
    """Candidates of every degree at which the walk changes (one lane's share, one step of the wavefront, several), light ones and
    heavy ones side by side in two contigs."""
    rng = np.random.default_rng(5)
    degs = [1, 2, 63, 64, 65, 1023, 1024, 1025, 3000]
    cands = []
    for d in degs + [3, 1, 3000, 2, 64, 5, 65, 1]:
        pss = [100, 200, 300][:min(d, int(rng.integers(2, 4)))]
        marks = [(int(rng.integers(1, 3)), int(rng.integers(0, 9000)), pss[int(rng.integers(0, len(pss)))]) for _ in range(d)]
        if d >= 2:
            marks[0], marks[-1] = (1, 0, pss[0]), (2, 0, pss[1])              # (the first and the last mark vote, in two phase sets)
        cands.append(dict(marks=marks, pos=int(rng.integers(1, 10 ** 6))))
    soa = build([cands[:9], cands[9:]])
    got = check(ctx, soa)
    assert int(got['n_sv'].sum()) >= len([d for d in degs if d >= 2]) and len(got) >= 2
    check(ctx, soa, cap=0)
    check(ctx, soa, cap=9000)


# ---- PS values and contigs ----------------------------------------------------------------------------------------------------------

def test_ps_values_are_unsigned_and_contigs_stay_apart(ctx):
    vals = [2 ** 31, 0, 2 ** 32 - 2, 1, 2 ** 31 - 1]
    c = dict(marks=[(1, 0, v) for v in vals])
    got = check(ctx, build([[c], [c]]))
    assert got['contig'].tolist() == [0] * 4 + [1] * 4
    assert got['ps_a'].tolist() == [0, 1, 2 ** 31 - 1, 2 ** 31] * 2 and got['ps_b'].tolist() == [1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2] * 2
    # two candidates of one contig on one link, a third on a link that shares only ps_a
    got = check(ctx, build([[dict(marks=[(1, 0, 2 ** 31), (1, 0, 2 ** 32 - 2)]), dict(marks=[(1, 0, 2 ** 31), (2, 0, 2 ** 32 - 2)]),
                             dict(marks=[(1, 0, 2 ** 31), (2, 0, 2 ** 31 + 1)])]]))
    assert [fields(x)[:7] for x in got] == [(0, 2 ** 31, 2 ** 31 + 1, 1, 0, 1, 0), (0, 2 ** 31, 2 ** 32 - 2, 2, 1, 1, 0)]


@pytest.mark.parametrize('K', [1, 2, 300])
def test_contig_counts_with_empty_contigs(ctx, K):
    rng = np.random.default_rng(K)
    contigs = []
    for k in range(K):
        empty = K > 2 and (k in (0, 1, K - 1, K - 2) or k % 3 == 0)
        contigs.append([] if empty else [dict(marks=[(1, 0, 10), (int(rng.integers(1, 3)), 0, 20)] + [(1, 0, 30)] * (k % 2), pos=k + 1)
                                         for _ in range(int(rng.integers(1, 4)))])
    got = check(ctx, build(contigs))
    full = [k for k in range(K) if contigs[k]]
    assert sorted(set(got['contig'].tolist())) == full and np.all(np.diff(got['contig'].astype(np.int64)) >= 0)
    assert np.array_equal(got['pos_min'], got['contig'] + 1)


# ---- one link fed by N candidates; many links ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('N', [1, 63, 64, 65, 257, 5000])
def test_one_link_fed_by_n_candidates(ctx, N):
    rng = np.random.default_rng(N)
    cands, want = [], dict(same=[0, 0], flip=[0, 0], open=[0, 0])
    pos = rng.permutation(N) * 7 + 11                                           # out of order
    for i in range(N):
        a1, a2, b1, b2 = (int(x) for x in rng.integers(0, 5, 4))
        if a1 + a2 == 0:
            a1 = 1
        if b1 + b2 == 0:
            b2 = 1
        cands.append(dict(marks=[(1, 0, 100)] * a1 + [(2, 0, 200)] * b2 + [(2, 0, 100)] * a2 + [(1, 0, 200)] * b1, pos=int(pos[i])))
        da, db = a1 - a2, b1 - b2
        kind = 'open' if da == 0 or db == 0 else ('same' if (da > 0) == (db > 0) else 'flip')
        want[kind][0] += 1
        want[kind][1] += min(abs(da), abs(db))
    got = check(ctx, build([[], cands, []]))
    assert len(got) == 1
    assert fields(got[0]) == (1, 100, 200, N, want['same'][0], want['flip'][0], want['open'][0], want['same'][1], want['flip'][1],
                              11, 11 + 7 * (N - 1))
    if N >= 63:
        assert min(want['same'][0], want['flip'][0], want['open'][0]) > 0


def test_many_links_of_one_observation_each(ctx):
    rng = np.random.default_rng(8)
    order = rng.permutation(5000)
    cands = [dict(marks=[(1, 0, 10 * int(i) + 2), (1 + int(i) % 2, 0, 10 * int(i) + 1)], pos=int(i) + 1) for i in order]
    got = check(ctx, build([cands[:2500], cands[2500:]]))
    assert len(got) == 5000 and np.all(got['n_sv'] == 1)
    assert np.array_equal(got['pos_min'], got['ps_a'] // 10 + 1)


# ---- random problems ----------------------------------------------------------------------------------------------------------------

RANDOM = (((1,), {}),
          ((3,), dict(n_contigs=2, cands_per_contig=(300, 300), n_ps=(3, 6), big_deg=1500, reads_per_contig=(200, 300))),
          ((4,), dict(n_contigs=5, n_ps=(60, 90), reads_per_contig=(250, 300), deg=(100, 200), cands_per_contig=(20, 40))),
          ((5,), dict(n_contigs=40, cands_per_contig=(1, 13), n_ps=(1, 3), deg=(1, 6))),
          ((2,), dict(n_contigs=1, cands_per_contig=(1, 1), reads_per_contig=(4, 4), n_ps=(2, 2), deg=(4, 4), empty_contig_rate=0,
                      no_seed_contig_rate=0, absent_rate=0)))
_soa = {}


def random_problem(i):
    if i not in _soa:
        _soa[i] = soa_fuzz.random_soa(*RANDOM[i][0], **RANDOM[i][1])
    return _soa[i]


def kinds(recs):
    return tuple(sum(int(r[f]) for r in recs) for f in ('n_same', 'n_flip', 'n_open'))


def test_the_random_problems_exercise_the_rule():
    per = [R.links(random_problem(i), 50, 2) for i in range(len(RANDOM))]
    assert [len(p) for p in per] == [14, 3, 47, 23, 1]                         # (the generator's output at these seeds: pinned)
    assert all(len(p) >= 1 for p in per)
    assert kinds(per[0]) == (50, 77, 17) and kinds(per[1]) == (56, 52, 6) and kinds(per[3])[2] == 15
    assert all(min(kinds(p)) > 0 for p in per[:2]) and min(kinds([r for p in per for r in p])) > 0


@pytest.mark.parametrize('cap', [0, 8100, 12000])
@pytest.mark.parametrize('sr', [(50, 2), (0, 0)])
@pytest.mark.parametrize('i', range(len(RANDOM)))
def test_random_problems(ctx, i, sr, cap):
    got = check(ctx, random_problem(i), sr[0], sr[1], cap)
    if cap == 8100 and sr == (50, 2):
        assert len(got) >= 1


# ---- contracts ----------------------------------------------------------------------------------------------------------------------

def raw_host(ctx, soa, cap, out, out_cap, s=50, r=2):
    prob, keep = _lib.problem_from_arrays(soa, s, r)
    n = ctypes.c_uint32(0xDEAD)
    rc = ctx.lib.duet_ps_links_host(ctx.handle, ctypes.byref(prob), cap, out.ctypes.data if out is not None else None, out_cap, ctypes.byref(n))
    return rc, n.value


def test_out_cap_exact_and_one_short(ctx):
    soa = random_problem(0)
    want = R.records(R.links(soa, 50, 2), DT)
    L = len(want)
    out = np.full((L + 2) * DT.itemsize, 0xAB, dtype=np.uint8)
    rc, n = raw_host(ctx, soa, 8100, out, L)
    assert rc == _lib.DUET_OK and n == L and out[:L * DT.itemsize].tobytes() == want.tobytes() and np.all(out[L * DT.itemsize:] == 0xAB)
    out[:] = 0xAB
    rc, n = raw_host(ctx, soa, 8100, out, L - 1)
    assert rc == _lib.DUET_ERR_INVALID and n == L and np.all(out == 0xAB) and 'too small' in ctx.last_error()
    rc, n = raw_host(ctx, soa, 8100, None, 0)
    assert rc == _lib.DUET_ERR_INVALID and n == L
    assert _lib.ps_links_room(soa.n_marks) >= L


def test_pc_cap_and_argument_refusals(ctx):
    soa = random_problem(0)
    out = np.full(64 * DT.itemsize, 0xAB, dtype=np.uint8)
    for cap in (CAP_MAX + 1, 1 << 30, 0xFFFFFFFF):
        rc, n = raw_host(ctx, soa, cap, out, 64)
        assert rc == _lib.DUET_ERR_INVALID and n == 0 and 'pc_cap' in ctx.last_error() and np.all(out == 0xAB)
    assert raw_host(ctx, soa, CAP_MAX, out, 64)[0] == _lib.DUET_OK
    out[:] = 0xAB
    with pytest.raises(ValueError, match='pc_cap'):
        ctx.ps_links_host(soa, 50, 2, pc_cap=CAP_MAX + 1)
    prob, keep = _lib.problem_from_arrays(soa, 50, 2)
    n = ctypes.c_uint32(5)
    assert ctx.lib.duet_ps_links_host(ctx.handle, None, 8100, out.ctypes.data, 64, ctypes.byref(n)) == _lib.DUET_ERR_INVALID and n.value == 0
    assert ctx.lib.duet_ps_links_host(ctx.handle, ctypes.byref(prob), 8100, None, 64, ctypes.byref(n)) == _lib.DUET_ERR_INVALID
    assert ctx.lib.duet_ps_links_host(ctx.handle, ctypes.byref(prob), 8100, out.ctypes.data, 64, None) == _lib.DUET_ERR_INVALID
    # what duet_ef_run_host refuses is refused here: offsets that do not end at n_cands, a null array
    bad = Soa(**{k: getattr(soa, k) for k in ('cand_ctg_off', 'read_tag', 'cand_pos', 'cand_svlen', 'cand_svread', 'cand_refread',
                                               'cand_gt_ok', 'cand_off', 'mark_read')})
    bad.cand_ctg_off = bad.cand_ctg_off.copy()
    bad.cand_ctg_off[-1] -= 1
    rc, count = raw_host(ctx, bad, 8100, out, 64)
    assert rc == _lib.DUET_ERR_INVALID and count == 0 and 'cand_ctg_off' in ctx.last_error()
    with pytest.raises(_lib.DuetLibraryError):
        ctx.run_host(bad, 50, 2)
    prob.cand_svread = None
    assert ctx.lib.duet_ps_links_host(ctx.handle, ctypes.byref(prob), 8100, out.ctypes.data, 64, ctypes.byref(n)) == _lib.DUET_ERR_INVALID
    assert np.all(out == 0xAB)


def test_device_form_agrees_and_two_runs_are_identical(ctx):
    import torch
    from duet_amd.devmem import DeviceProblem
    for i, cap in ((0, None), (1, 12000), (2, 8100), (3, 0)):
        soa = random_problem(i)
        want = ctx.ps_links_host(soa, 50, 2, pc_cap=cap)
        assert want.tobytes() == ctx.ps_links_host(soa, 50, 2, pc_cap=cap).tobytes()
        dp = DeviceProblem(soa, 50, 2)
        room = _lib.ps_links_room(soa.n_marks)
        runs = []
        for _ in range(2):
            out = torch.full((room * DT.itemsize + 64,), 0xAB, dtype=torch.uint8, device='cuda:0')
            n = ctx.ps_links_device(dp.problem, out.data_ptr(), room, pc_cap=cap)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert np.all(got[n * DT.itemsize:] == 0xAB)
            runs.append(got[:n * DT.itemsize].tobytes())
        assert runs[0] == runs[1] == want.tobytes()
        if len(want):
            out = torch.full((room * DT.itemsize + 64,), 0xAB, dtype=torch.uint8, device='cuda:0')
            n = ctypes.c_uint32(0)
            rc = ctx.lib.duet_ps_links_device(ctx.handle, ctypes.byref(dp.problem), 8100 if cap is None else cap, ctypes.c_void_p(out.data_ptr()),
                                              len(want) - 1, ctypes.byref(n), None)
            torch.cuda.synchronize()
            assert rc == _lib.DUET_ERR_INVALID and n.value == len(want) and bool((out == 0xAB).all())


def test_nothing_of_ef_changes_after_a_large_and_a_small_call(ctx):
    soa = soa_fuzz.random_soa(3, n_contigs=4)
    before = (ctx.run_host(soa, 0, 0), ctx.features_host(soa, 0, 0))
    check(ctx, random_problem(2))                                              # a large call, then a small one
    check(ctx, one([(1, 0, 10), (2, 0, 20)]))
    check(ctx, random_problem(1), cap=12000)
    after = (ctx.run_host(soa, 0, 0), ctx.features_host(soa, 0, 0))
    assert np.array_equal(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1])
    assert before[1].tobytes() == after[1].tobytes()
    assert int((before[0][0] != 0).sum()) > 10


# ---- the svim form ------------------------------------------------------------------------------------------------------------------

def svim_case(seed, G, K):
    rng = synth.SplitMix(7100 + seed)
    g_contig = np.sort(rng.below(G, K)) if G else np.zeros(0, dtype=np.int64)
    return svim_fuzz.build('ps_links_%d' % seed, seed, g_contig, svim_fuzz.n_sizes(rng, G, 2, 24) if G else np.zeros(0, dtype=np.int64), K)


@pytest.mark.parametrize('seed,G,K', [(1, 60, 3), (2, 150, 5), (3, 0, 2)])
def test_svim_entries(ctx, seed, G, K):
    from duet_amd.devmem import DeviceSvim
    c = svim_case(seed, G, K)
    args = (c.marks, c.read_tag, c.depth, c.depth_off, c.depth_bin, c.svlen_thres, c.suppread_thres)
    if G:
        cl = c_oracle.cluster(c.marks['contig'], c.marks['type'], c.marks['pos'], c.marks['span'], **c.kw)
        soa = svim_ref.adapt(cl, c.marks, c.read_tag, c.depth, c.depth_off, c.depth_bin)[0]
    else:
        soa = build([[] for _ in range(K)])                                    # no mark: no candidate
    phase = ctx.svim_host(*args, **c.kw)
    for cap in (None, 2400):
        want = R.records(R.links(soa, c.svlen_thres, c.suppread_thres, R.PC_MAX if cap is None else cap), DT)
        got = ctx.svim_ps_links_host(*args, pc_cap=cap, **c.kw)
        assert got['links'].tobytes() == want.tobytes()
        for k in ('cand_off', 'cand_contig', 'cand_type', 'cand_pos', 'cand_span'):
            assert np.array_equal(got[k], phase[k]), k                         # the cluster result left behind is the fused run's
        ds = DeviceSvim(*args, device='cuda:0', **c.kw)
        assert ds.ps_links(ctx, pc_cap=cap).tobytes() == want.tobytes()
        left = ds.fetch()
        for k in ('cand_off', 'cand_contig', 'cand_type', 'cand_pos', 'cand_span'):
            assert np.array_equal(left[k], phase[k]), k
    if G:
        assert len(want) >= 1 and soa.n_cands >= G // 2
    else:
        assert len(want) == 0 and len(phase['cand_pos']) == 0


def test_svim_refusals(ctx):
    c = svim_case(1, 60, 3)
    with pytest.raises(ValueError, match='pc_cap'):
        ctx.svim_ps_links_host(c.marks, c.read_tag, c.depth, c.depth_off, c.depth_bin, 50, 2, pc_cap=CAP_MAX + 1)
    p, res, out, _, n, keep = ctx._svim_host_problem(c.marks, c.read_tag, c.depth, c.depth_off, c.depth_bin, 50, 2, 0.9, 1000, 100, 900.0, False)
    links = np.full(DT.itemsize, 0xAB, dtype=np.uint8)
    nl = ctypes.c_uint32(7)
    rc = ctx.lib.duet_svim_ps_links_host(ctx.handle, ctypes.byref(p), ctypes.byref(res), CAP_MAX + 1, links.ctypes.data, 1, ctypes.byref(nl))
    assert rc == _lib.DUET_ERR_INVALID and nl.value == 0 and 'pc_cap' in ctx.last_error()
    rc = ctx.lib.duet_svim_ps_links_host(ctx.handle, ctypes.byref(p), ctypes.byref(res), 8100, links.ctypes.data, 1, ctypes.byref(nl))
    assert rc == _lib.DUET_ERR_INVALID and nl.value > 1 and np.all(links == 0xAB)       # one record of room: the count is exact
    assert nl.value == len(ctx.svim_ps_links_host(c.marks, c.read_tag, c.depth, c.depth_off, c.depth_bin, 50, 2)['links'])


# ---- the product --------------------------------------------------------------------------------------------------------------------

def read(path):
    with open(path, 'rb') as f:
        return f.read()


def vcf_chroms(home):
    return set(ln.split(b'\t')[0].decode() for ln in read(home + '/phased_sv.vcf').splitlines() if ln and not ln.startswith(b'#'))


def tables(recs, texts):
    recs = R.records(recs, DT)
    return ((R.header() + R.rows_text(recs, texts)).encode(),
            ('CHROM\tPS\tBLOCK\tFLIP\n' + R.blocks_text(R.blocks(recs)[0], texts)).encode())


@pytest.fixture(scope='module')
def golden_home(tmp_path_factory):
    from tests.test_c_oracle import materialise_bams
    home = str(tmp_path_factory.mktemp('ps_links_golden') / 'w')
    shutil.copytree(os.path.join(H.GOLDEN, 'cases', 'fuzz_cutesv_s2'), home)
    materialise_bams(home)
    return home


def stub_stages(monkeypatch):
    from duet_amd import cli, stages
    for name in ('snp_calling', 'sv_calling', 'snp_phasing'):
        monkeypatch.setattr(stages, name, lambda *a: None)
    monkeypatch.setattr(cli, 'check_envs', lambda *a: None)
    monkeypatch.setattr(cli, 'set_logging', lambda *a: None)


def test_product_native_ingest(golden_home, monkeypatch):
    from duet_amd import cli
    from duet_amd.sv_phasing import sv_phasing
    home = golden_home
    pinned = read(os.path.join(H.GOLDEN, 'cases', 'fuzz_cutesv_s2', 'phased_sv.vcf'))
    paths = (ps_links.links_path(home), ps_links.blocks_path(home))
    sv_phasing(home, 50, 2, 4, False)
    assert read(home + '/phased_sv.vcf') == pinned and not any(os.path.exists(p) for p in paths)      # no file without the flag
    soa, txt = tune._candidates(home, 50, 2, False, 2)
    texts = [txt['chrom'][int(soa.cand_ctg_off[k])] if soa.cand_ctg_off[k + 1] > soa.cand_ctg_off[k] else '?' for k in range(soa.n_contigs)]

    def expect(cap=R.PC_MAX):
        recs = R.links(soa, 50, 2, cap)
        assert len(recs) >= 1
        assert set(texts[r['contig']] for r in recs) <= vcf_chroms(home) | set(txt['chrom'])
        return tables(recs, texts)

    sv_phasing(home, 50, 2, 4, False, ps_links=True)
    assert read(home + '/phased_sv.vcf') == pinned
    assert (read(paths[0]), read(paths[1])) == expect()
    first = read(paths[0])
    # with a vector of the caller's own the decision changes, the links do not; under a cap the voters are the cap's
    v = tune.vector({'c1_max_ref_num': 3, 'c0_min_sv_num': 2})
    sv_phasing(home, 50, 2, 4, False, thresholds=v)
    other = read(home + '/phased_sv.vcf')
    for p in paths:
        os.remove(p)
    sv_phasing(home, 50, 2, 4, False, thresholds=v, ps_links=True)
    assert read(home + '/phased_sv.vcf') == other and read(paths[0]) == first
    sv_phasing(home, 50, 2, 4, False, pc_cap=2400)
    capped = read(home + '/phased_sv.vcf')
    sv_phasing(home, 50, 2, 4, False, pc_cap=2400, ps_links=True)
    assert read(home + '/phased_sv.vcf') == capped
    assert (read(paths[0]), read(paths[1])) == expect(2400) and read(paths[0]) != first
    # the command
    stub_stages(monkeypatch)
    for p in paths:
        os.remove(p)
    monkeypatch.setattr(sys, 'argv', ['duet', 'in.bam', 'ref.fa', home])
    cli.main(None)
    assert read(home + '/phased_sv.vcf') == pinned and not any(os.path.exists(p) for p in paths)
    monkeypatch.setattr(sys, 'argv', ['duet', 'in.bam', 'ref.fa', home, '--write_ps_links'])
    cli.main(None)
    assert read(home + '/phased_sv.vcf') == pinned and (read(paths[0]), read(paths[1])) == expect()


def test_product_svim_gpu(ctx, tmp_path_factory, monkeypatch):
    from duet_amd import cli
    root = tmp_path_factory.mktemp('ps_links_svim')
    home, copy = str(root / 'w'), str(root / 'copy')
    synth.write_svim_workdir(home, H.case_contigs('genome_small', 5), 5)
    shutil.copytree(home, copy)
    svim_mode.sv_phasing_from_bams(copy, 50, 2, 4, False, 0.9, 0, write_sv_calls=True)
    soa, _ = tune._candidates(copy, 50, 2, False, 4)                          # the E/F problem the fused pipeline adapts, read back
    texts = svim_mode.spelled_contigs(home, init_chrom_list(False, home))
    paths = (ps_links.links_path(home), ps_links.blocks_path(home))
    stub_stages(monkeypatch)
    base = ['duet', 'in.bam', 'ref.fa', home, '-b', 'svim-gpu']
    monkeypatch.setattr(sys, 'argv', base)
    cli.main(None)
    plain = read(home + '/phased_sv.vcf')
    assert plain.count(b'\n') > 100 and not any(os.path.exists(p) for p in paths)
    monkeypatch.setattr(sys, 'argv', base + ['--write_ps_links'])
    cli.main(None)
    assert read(home + '/phased_sv.vcf') == plain
    recs = R.links(soa, 50, 2)
    assert (read(paths[0]), read(paths[1])) == tables(recs, texts)
    assert vcf_chroms(home) <= set(texts) and len(recs) >= 1
    monkeypatch.setattr(sys, 'argv', base + ['--pc_cap', '2400'])
    cli.main(None)
    capped = read(home + '/phased_sv.vcf')
    monkeypatch.setattr(sys, 'argv', base + ['--pc_cap', '2400', '--write_ps_links', '--thresholds', str(root / 'v.json')])
    with open(str(root / 'v.json'), 'w') as f:
        f.write('{}')
    cli.main(None)
    assert read(home + '/phased_sv.vcf') == capped
    assert (read(paths[0]), read(paths[1])) == tables(R.links(soa, 50, 2, 2400), texts)
