# coding=utf-8
"""-m gpu: the planned tags from other SVs (duet_amd/csrc/duet_svtags_plan.hip: duet_sv_tags_plan_*, duet_sv_tags_apply_*) against
tests/sv_tags_ref.py, byte for byte on out_tag, the identity index and the counters, through both entries of each: the problems of
tests/test_gpu_sv_tags.py with their own pred under mask = NULL and mask = pred != 0, the smallest shapes at which the new kernels
can go wrong, no stale state between vectors, the fourth counter, the refusals, and the resident second runs of five vectors."""
import numpy as np
import pytest

from duet_amd import _lib, tune
from tests import cap_line_ref
from tests import pc_cap_ref
from tests import read_tags_cases as RK
from tests import sv_tags_cases as K
from tests import sv_tags_ref as S

pytestmark = pytest.mark.gpu

ABSENT, UN = S.ABSENT, S.UNTAGGED
tag = S.tag
FILL = 0xABABABABABABABAB
IFILL = 0xABABABAB
# the grid of tests/test_gpu_tune_sv_tags.py: the default vector and the four of the condition (tests/test_sv_tags_plan_host.py)
GRID = [{}, {'c1_max_ref_num': 3, 'c0_min_sv_num': 2}, {'c1_twohap_sv_ratio_2': 0.7, 'c1_max_ref_num': 1000},
        {'c1_onehap_sv_ratio_hi': 0.6}, {'c1_hapread_ratio': 0.4}]


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


def cand(pred, ps, marks, pos=1000):
    return dict(pred=pred, ps=ps, marks=marks, pos=pos)


def host_arrays(p):
    kw = p.arrays()
    kw.pop('cand_pos')
    kw.pop('pred')
    return kw


class Resident(object):
    """A problem uploaded, with out_tag and out_index starting as FILL."""

    def __init__(self, p):
        M, C = len(p.mark_read), len(p.pred)
        self.M, self.C = M, C
        self.keep = dict(cand_off=dev(np.array(p.cand_off, dtype=np.uint32)), mark_read=dev(np.array(p.mark_read, dtype=np.uint32)),
                         mark_name=dev(np.array(p.mark_name, dtype=np.uint32)), ps=dev(np.array(p.ps, dtype=np.uint32)),
                         read_tag=dev(np.array(p.read_tag, dtype=np.uint64)))
        if p.mark_order is not None:
            self.keep['mark_order'] = dev(np.array(p.mark_order, dtype=np.uint32))
        if p.cand_contig is not None:
            self.keep['cand_contig'] = dev(np.array(p.cand_contig, dtype=np.uint16))
        self.prob = prob = _lib.ReadTagsProblem()
        prob.n_cands, prob.n_marks, prob.n_reads, prob.n_names = C, M, len(p.read_tag), p.n_names
        for k, t in self.keep.items():
            setattr(prob, k, t.data_ptr())
        if p.cand_ctg_off is not None:
            self.off = np.array(p.cand_ctg_off, dtype=np.uint32)
            prob.cand_ctg_off, prob.n_contigs = self.off.ctypes.data, len(self.off) - 1
        self.out, self.index = dev(np.full(max(M, 1), FILL, dtype=np.uint64)), dev(np.full(max(M, 1), IFILL, dtype=np.uint32))
        self.counts = dev(np.full(4, IFILL, dtype=np.uint32))

    def plan(self, ctx, mask=None, **kw):
        import torch
        self.mask = None if mask is None else dev(np.array(mask, dtype=np.uint8))
        try:
            return ctx.sv_tags_plan_device(self.prob, self.out.data_ptr(), self.index.data_ptr(),
                                           cand_mask_ptr=None if mask is None else self.mask.data_ptr(), **kw)
        finally:
            torch.cuda.synchronize()

    def apply(self, ctx, pred, **kw):
        import torch
        d_pred = dev(np.array(pred, dtype=np.uint8))
        try:
            ctx.sv_tags_apply_device(d_pred.data_ptr(), self.out.data_ptr(), self.counts.data_ptr(), **kw)
        finally:
            torch.cuda.synchronize()
        return self.words(), tuple(int(x) for x in back(self.counts, np.uint32, 4))

    def words(self):
        return back(self.out, np.uint64, self.M)

    def indices(self):
        return back(self.index, np.uint32, self.M)


def base_words(p):
    return np.array([int(p.read_tag[r]) if S.has_tag(p, int(r)) else UN for r in p.mark_read], dtype=np.uint64)


def masks_of(p):
    return (None, [1 if int(x) else 0 for x in p.pred])


def check(ctx, p, min_votes=1, pc_new=0, masks=None):
    """Plan and apply through both entries, under each mask, equal the reference byte for byte -> (out_tag as a list, counts)."""
    want, _, counts = S.sv_tags(p, min_votes, pc_new)
    M = len(p.mark_read)
    for mask in (masks_of(p) if masks is None else masks):
        if want is None:                                                       # no candidate or no mark: nothing is written
            r = Resident(p)
            assert r.plan(ctx, mask) == dict(n_untagged=0, n_records=0, n_runs=0, n_contributing=0)
            words, got = r.apply(ctx, p.pred, min_votes=min_votes, pc_new=pc_new)
            assert (words == FILL).all() and (r.indices() == IFILL).all() and got == (0, 0, 0, 0)
            out, idx, info = ctx.sv_tags_plan_host(cand_mask=mask, out_tag=np.full(M, FILL, dtype=np.uint64),
                                                   out_index=np.full(M, IFILL, dtype=np.uint32), **host_arrays(p))
            assert (out == FILL).all() and (idx == IFILL).all() and info['n_untagged'] == 0
            assert ctx.sv_tags_apply_host(p.pred, out, min_votes, pc_new)[1] == (0, 0, 0, 0) and (out == FILL).all()
            continue
        want_bytes, base = np.array(want, dtype=np.uint64).tobytes(), base_words(p)
        r = Resident(p)
        info = r.plan(ctx, mask)
        assert r.words().tobytes() == base.tobytes() and r.indices().tobytes() == np.arange(M, dtype=np.uint32).tobytes()
        assert info['n_untagged'] == counts[0] and info['n_records'] <= info['n_runs'] <= info['n_contributing'] <= M
        words, got = r.apply(ctx, p.pred, min_votes=min_votes, pc_new=pc_new)
        assert (words.tobytes(), got) == (want_bytes, counts + (0,)), (mask is None, 'device')
        out, idx, info_h = ctx.sv_tags_plan_host(cand_mask=mask, out_tag=np.full(M, FILL, dtype=np.uint64),
                                                 out_index=np.full(M, IFILL, dtype=np.uint32), **host_arrays(p))
        assert out.tobytes() == base.tobytes() and idx.tobytes() == np.arange(M, dtype=np.uint32).tobytes() and info_h == info
        out, got = ctx.sv_tags_apply_host(p.pred, out, min_votes, pc_new)
        assert (out.tobytes(), got) == (want_bytes, counts + (0,)), (mask is None, 'host')
    return want, counts


# ---- the problems of tests/test_gpu_sv_tags.py ------------------------------------------------------------------------------------------

def sized(M, C, seed, form='off', permute=0):
    """tests/test_gpu_sv_tags.py: sized -- C candidates over M marks, reads shared between neighbours, a third of the reads tagged."""
    rng = np.random.RandomState(seed)
    cuts = np.sort(rng.choice(np.arange(1, M), C - 1, replace=False)) if C > 1 and M > 1 else np.zeros(0, dtype=np.int64)
    off = [0] + [int(x) for x in cuts] + [M] * (C - len(cuts))
    n_reads = max(M // 3, 1)
    tags = [tag(1 + int(rng.randint(2)), int(rng.randint(9000)), 7 + int(rng.randint(3))) if rng.randint(3) == 0 else UN for _ in range(n_reads)]
    half = max(C // 2, 1) if n_reads >= 2 else C
    cands = []
    for c in range(C):
        lo, hi = (0, max(n_reads // 2, 1)) if c < half else (n_reads // 2, n_reads)
        marks = [(int(r), int(r)) for r in rng.randint(lo, hi, off[c + 1] - off[c])]
        cands.append(cand(int(rng.randint(4)), 7 + int(rng.randint(3)), marks, pos=c))
    return RK.problem([cands[:half], [], cands[half:]], tags, n_names=n_reads, form=form, permute=permute)


@pytest.mark.parametrize('M', [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_mark_counts(ctx, M):
    for form, permute in (('off', 0), ('contig', 5)):
        p = sized(M, min(max(M // 7, 1), max(M, 1)), 100 + M, form, permute) if M else RK.problem([[cand(1, 7, [])]], form=form)
        _, counts = check(ctx, p)
        assert M < 63 or counts[1] > 0


@pytest.mark.parametrize('C', [1, 63, 64, 65, 257])
def test_candidate_counts(ctx, C):
    for form, permute in (('off', 3), ('contig', 0)):
        _, counts = check(ctx, sized(3 * C + 1, C, 200 + C, form, permute))
        assert C < 63 or counts[1] > 0


def test_empty_problems(ctx):
    assert check(ctx, RK.problem([[]]))[1] == (0, 0, 0)
    assert check(ctx, RK.problem([[], [], []], form='contig'))[1] == (0, 0, 0)
    out, counts = check(ctx, RK.problem([[cand(0, 0, [(0, ABSENT)]), cand(3, 0, [(0, ABSENT), (1, 0)])]], [tag(1, 0, 7)]))
    assert out == [UN, UN, tag(1, 0, 7)] and counts == (2, 0, 0)               # pred all 0 or 3: no het candidate at all


@pytest.mark.parametrize('read', [ABSENT, 2, 3, 1 << 31, 1])
def test_every_spelling_of_no_tag(ctx, read):
    p = RK.problem([[cand(1, 7, [(0, read)]), cand(3, 0, [(0, read)])]], [tag(1, 0, 5), UN])
    out, counts = check(ctx, p, pc_new=77)
    assert out == [UN, tag(1, 77, 7)] and counts == (2, 1, 1)


def test_tagged_words_are_copied_whatever_they_hold(ctx):
    words = [tag(0, 3, 7), tag(3, 8101, 7), tag(1, (1 << 30) - 2, 9), tag(2, 0, 0), tag(3, (1 << 30) - 1, 0xFFFFFFFE)]
    marks = [(i, i) for i in range(5)] + [(5, ABSENT)]
    p = RK.problem([[cand(1, 7, marks), cand(2, 9, marks)]], words)
    for cap in (0, 8100, S.CAP_MAX):                                           # (the cap of the run the tags are made for: not read)
        out, _, _ = ctx.sv_tags_plan_host(pc_cap=cap, **host_arrays(p))
        out, counts = ctx.sv_tags_apply_host(p.pred, out)
        assert out.tolist() == words + [tag(2, 0, 9)] + words + [tag(1, 0, 7)] and counts == (2, 2, 0, 0)
        r = Resident(p)
        r.plan(ctx, pc_cap=cap)
        assert r.apply(ctx, p.pred)[0].tolist() == out.tolist()
    out, counts = check(ctx, p)
    assert out == words + [tag(2, 0, 9)] + words + [tag(1, 0, 7)] and counts == (2, 2, 0)


@pytest.mark.parametrize('n_ps', [1, 2, 3, 5, 65])
def test_a_name_with_so_many_records(ctx, n_ps):
    cands = [cand(1, 10 * i, [(0, ABSENT)] * (i + 1), pos=i) for i in range(n_ps)] + [cand(0, 0, [(0, ABSENT), (1, ABSENT)])]
    out, counts = check(ctx, RK.problem([cands]))
    assert out[-2] == tag(1, 0, 10 * (n_ps - 1)) and out[-1] == UN
    assert out[-3] == (UN if n_ps == 1 else tag(1, 0, 10 * (n_ps - 2)))


def test_ties_extreme_ps_and_zero_after_removal(ctx):
    ask = cand(0, 0, [(0, ABSENT)])
    out, _ = check(ctx, RK.problem([[cand(1, 0xFFFFFFFE, [(0, ABSENT)] * 2), cand(2, 0, [(0, ABSENT)] * 2), ask]]))
    assert out[-1] == tag(2, 0, 0)                                             # equal |d|: the smaller PS, here 0
    out, _ = check(ctx, RK.problem([[cand(2, 0x80000000, [(0, ABSENT)]), cand(1, 5, [(0, ABSENT)]), ask]]))
    assert out[-1] == tag(1, 0, 5)                                             # compared as unsigned 32-bit numbers
    out, _ = check(ctx, RK.problem([[cand(2, 0x80000000, [(0, ABSENT)]), cand(1, 0xFFFFFFF0, [(0, ABSENT)]), ask]]))
    assert out[-1] == tag(2, 0, 0x80000000)                                    # a tie between two phase sets with PS >= 2^31
    out, counts = check(ctx, RK.problem([[cand(1, 7, [(0, ABSENT)] * 3), ask]]))
    assert out == [UN] * 3 + [tag(1, 0, 7)] and counts == (4, 1, 3)            # d exactly 0 after the own removal: own_only
    for mv in (1, 3):
        for n in (mv - 1, mv):                                                 # |d| + 1 == min_votes, |d| == min_votes
            out, _ = check(ctx, RK.problem([[cand(2, 7, [(0, ABSENT)] * n + [(1, ABSENT)]), ask]]), min_votes=mv)
            assert out[-1] == (tag(2, 0, 7) if n >= mv else UN)


@pytest.mark.parametrize('k', [2, 3, 64, 65, 257])
def test_a_candidate_lists_a_read_k_times(ctx, k):
    filler = [(1 + i, ABSENT) for i in range(70)]
    X = cand(1, 7, filler[:30] + [(0, ABSENT)] * k + filler[30:])
    Y, Z, W = cand(2, 7, [(0, ABSENT)] * k), cand(2, 9, [(0, ABSENT)] * (k + 1)), cand(3, 0, [(0, ABSENT)])
    out, counts = check(ctx, RK.problem([[cand(1, 5, filler), X, Y, Z, W]]))
    assert out[-1] == tag(2, 0, 9)
    assert out[70 + 30] == tag(2, 0, 9) and out[70 + 70 + k] == tag(2, 0, 9)


def test_k_two_against_two_and_three(ctx):
    X = cand(1, 7, [(0, ABSENT)] * 2 + [(1, ABSENT)])
    for n, want in ((2, UN), (3, tag(2, 0, 7))):
        out, _ = check(ctx, RK.problem([[X, cand(2, 7, [(0, ABSENT)] * n), cand(0, 0, [(0, ABSENT)])]]))
        assert out[-1] == want and out[0] == out[1] == tag(2, 0, 7) and out[2] == UN


@pytest.mark.parametrize('kw', RK.RANDOM, ids=lambda kw: 'seed%d' % kw['seed'])
def test_random_problems_in_every_form(ctx, kw):
    p = RK.random_problem(**kw)
    check(ctx, p)
    for q in RK.same_in_other_forms(p):                                        # cand_contig, mark_order as a permutation, both
        check(ctx, q, masks=(None,))


def test_a_fuzz_problem_with_the_oracle_calls(ctx):
    soa = K.untagged_soa(2)
    _, counts = check(ctx, K.problem_of(soa, *K.oracle_calls(soa)))
    assert counts == K.PINNED[2][0]


# ---- the smallest shapes of the new kernels ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('U', [0, 1, 255, 256, 257])
def test_untagged_mark_counts(ctx, U):
    """A workgroup of sa_marks is 256 untagged marks: X (1|0) lists the first names, W (1|1) the same ones again, every other mark
    is tagged."""
    a = (U + 1) // 2
    X = cand(1, 7, [(i, ABSENT) for i in range(a)] + [(a + 1, 0)])
    W = cand(3, 0, [(i, ABSENT) for i in range(U - a)] + [(a + 1, 0), (a + 2, 1)])
    out, counts = check(ctx, RK.problem([[X, W]], [tag(2, 5, 9), tag(1, 6, 7)]))
    assert counts == (U, U - a, a)                                             # W's marks get X's haplotype; X's own see nobody


@pytest.mark.parametrize('n', [1, 8, 9, 63, 64, 65, 257])
def test_a_record_of_so_many_runs(ctx, n):
    """n het candidates of one phase set list the name once each: one record of n runs (kLight = 8 of them are summed by one lane),
    beside a record of one run in the same wavefront of sa_records."""
    cands = [cand(1 if i % 3 else 2, 7, [(0, ABSENT)], pos=i) for i in range(n)]
    cands += [cand(1, 9, [(1, ABSENT)]), cand(0, 0, [(0, ABSENT), (1, ABSENT)])]
    out, counts = check(ctx, RK.problem([cands]))
    n2 = len(range(0, n, 3))
    d = (n - n2) - n2
    assert out[-2] == (UN if d == 0 else tag(1 if d > 0 else 2, 0, 7)) and out[-1] == tag(1, 0, 9)


def test_many_long_records_in_one_wavefront(ctx):
    """Five names of 9 .. 70 runs each next to short ones: the ballot of sa_records names several long records in one wavefront."""
    cands, pos = [], 0
    for name, n in ((0, 9), (1, 1), (2, 70), (3, 2), (4, 65), (5, 10), (6, 64)):
        for i in range(n):
            cands.append(cand(1 if (i + name) % 4 else 2, 7 + 2 * (i % 2 if name == 5 else 0), [(name, ABSENT)], pos=pos))
            pos += 1
    cands.append(cand(0, 0, [(name, ABSENT) for name in range(8)]))
    check(ctx, RK.problem([cands], n_names=8))


def test_one_run_of_70000(ctx):
    n = 70000
    p = RK.problem([[cand(1, 7, [(0, ABSENT)] * n), cand(0, 0, [(0, ABSENT)])]])
    r = Resident(p)
    info = r.plan(ctx)
    assert info == dict(n_untagged=n + 1, n_records=2, n_runs=2, n_contributing=n + 1)          # (mask NULL: the asker is a run too)
    words, counts = r.apply(ctx, p.pred)
    assert counts == (n + 1, 1, n, 0) and words[-1] == tag(1, 0, 7) and (words[:-1] == UN).all()
    r = Resident(p)
    assert r.plan(ctx, [1, 0])['n_runs'] == 1
    assert r.apply(ctx, p.pred)[0].tobytes() == words.tobytes()
    out, _, _ = ctx.sv_tags_plan_host(**host_arrays(p))
    assert ctx.sv_tags_apply_host(p.pred, out)[0].tobytes() == words.tobytes()


def test_masks_of_nobody_and_of_one(ctx):
    X, Y, W = cand(1, 7, [(0, ABSENT), (1, ABSENT)]), cand(2, 9, [(0, ABSENT)]), cand(0, 0, [(0, ABSENT), (2, 0)])
    p = RK.problem([[X, Y, W]], [tag(1, 0, 5)])
    none = S.R.Problem(**dict(p.__dict__, pred=[0, 0, 0]))
    out, counts = check(ctx, none, masks=(None, [0, 0, 0], [0, 1, 0]))         # pred all 0 under every mask; V == 0
    assert out == [UN] * 4 + [tag(1, 0, 5)] and counts == (4, 0, 0)
    r = Resident(p)
    assert r.plan(ctx, [0, 0, 0]) == dict(n_untagged=4, n_records=0, n_runs=0, n_contributing=0)
    only_y = S.R.Problem(**dict(p.__dict__, pred=[0, 2, 3]))
    out, counts = check(ctx, only_y, masks=([0, 1, 0], [0, 1, 1]))
    assert out == [tag(2, 0, 9), UN, UN, tag(2, 0, 9), tag(1, 0, 5)] and counts == (4, 2, 1)


# ---- no stale state -----------------------------------------------------------------------------------------------------------------

def fuzz_problem(seed=2):
    soa = K.untagged_soa(seed)
    return K.problem_of(soa, *K.oracle_calls(soa))


def with_pred(p, pred):
    return S.R.Problem(**dict(p.__dict__, pred=[int(x) for x in pred]))


def test_vectors_a_b_a_on_one_plan(ctx):
    p = fuzz_problem()
    A = np.array(p.pred, dtype=np.uint8)
    het = np.flatnonzero((A == 1) | (A == 2))
    B = A.copy()
    B[het[::2]] = 0                                                            # B's het set is a strict subset of A's
    assert 0 < int(((B == 1) | (B == 2)).sum()) < len(het)
    want = {k: S.sv_tags(with_pred(p, v)) for k, v in (('A', A), ('B', B))}
    assert want['A'][0] != want['B'][0]
    r = Resident(p)
    r.plan(ctx, [1 if x else 0 for x in A])
    got = [r.apply(ctx, v) for v in (A, B, A)]
    for (words, counts), k in zip(got, 'ABA'):
        assert words.tobytes() == np.array(want[k][0], dtype=np.uint64).tobytes() and counts == want[k][2] + (0,)
    assert got[0][0].tobytes() == got[2][0].tobytes() and got[0][1] == got[2][1]
    # the host entry, on one array
    out, _, _ = ctx.sv_tags_plan_host(cand_mask=(A != 0).astype(np.uint8), **host_arrays(p))
    for v, k in zip((A, B, A), 'ABA'):
        out, counts = ctx.sv_tags_apply_host(v, out)
        assert out.tobytes() == np.array(want[k][0], dtype=np.uint64).tobytes() and counts == want[k][2] + (0,)


@pytest.mark.parametrize('name, values', [('min_votes', (1, 3, 1)), ('pc_new', (0, 7, 0))])
def test_settings_a_b_a_on_one_plan(ctx, name, values):
    p = fuzz_problem()
    r = Resident(p)
    r.plan(ctx)
    got = []
    for v in values:
        want, _, counts = S.sv_tags(p, **{name: v})
        got.append(r.apply(ctx, p.pred, **{name: v}))
        assert got[-1][0].tobytes() == np.array(want, dtype=np.uint64).tobytes() and got[-1][1] == counts + (0,)
    assert got[0][0].tobytes() == got[2][0].tobytes() != got[1][0].tobytes()


# ---- the fourth counter, refusals -----------------------------------------------------------------------------------------------------

def test_the_fourth_counter(ctx):
    X, Y, W = cand(1, 7, [(0, ABSENT), (1, 0)]), cand(2, 9, [(0, ABSENT)]), cand(0, 0, [(0, ABSENT), (2, 0)])
    p = RK.problem([[X, Y, W]], [tag(1, 3, 5)])
    base = base_words(p)
    tagged = base != UN
    r = Resident(p)
    r.plan(ctx, [1, 0, 0])
    words, counts = r.apply(ctx, [1, 0, 0])
    assert counts[3] == 0
    words, counts = r.apply(ctx, [1, 2, 0])                                    # a het call outside the mask
    assert counts[3] == 1 and np.array_equal(words[tagged], base[tagged])
    words, counts = r.apply(ctx, [1, 0, 4])                                    # pred above 3
    assert counts[3] == 1 and np.array_equal(words[tagged], base[tagged])
    words, counts = r.apply(ctx, [1, 3, 3])                                    # a hom call outside the mask is no het call
    assert counts[3] == 0
    r.plan(ctx)                                                                # mask NULL: only pred above 3 counts
    assert r.apply(ctx, [1, 2, 0])[1][3] == 0 and r.apply(ctx, [4, 2, 4])[1][3] == 2
    out, _, _ = ctx.sv_tags_plan_host(cand_mask=[1, 0, 0], **host_arrays(p))
    out, counts = ctx.sv_tags_apply_host([1, 2, 0], out)
    assert counts[3] == 1 and np.array_equal(out[tagged], base[tagged])


def refused(ctx, p, match, mask=None, **kw):
    """Both plan entries refuse with `match`, leave out_tag and the index untouched, and leave no plan."""
    M = len(p.mark_read)
    out, idx = np.full(M, FILL, dtype=np.uint64), np.full(M, IFILL, dtype=np.uint32)
    with pytest.raises(_lib.DuetLibraryError, match=match):
        ctx.sv_tags_plan_host(cand_mask=mask, out_tag=out, out_index=idx, **dict(host_arrays(p), **kw))
    assert (out == FILL).all() and (idx == IFILL).all()
    with pytest.raises(_lib.DuetLibraryError, match='without a plan'):
        ctx.sv_tags_apply_host(p.pred, out)
    if (p.cand_ctg_off is None) != (p.cand_contig is None):                    # (Resident states one contig form)
        r = Resident(p)
        with pytest.raises(_lib.DuetLibraryError, match=match):
            r.plan(ctx, mask, **kw)
        assert (r.words() == FILL).all() and (r.indices() == IFILL).all()


def test_refusals_leave_the_outputs_untouched(ctx):
    p = RK.problem([[cand(1, 7, [(0, ABSENT), (1, ABSENT)]), cand(2, 7, [(0, ABSENT)])]])
    refused(ctx, p, 'pc_cap', pc_cap=S.CAP_MAX + 1)
    refused(ctx, RK.problem([[cand(0, 7, [(2, ABSENT)])]], n_names=2), 'mark_name not below n_names')
    refused(ctx, S.R.Problem(**dict(p.__dict__, cand_off=[0, 3, 1])), 'cand_off does not ascend')
    refused(ctx, S.R.Problem(**dict(p.__dict__, cand_off=[0, 2, 4])), 'cand_off does not ascend')
    refused(ctx, S.R.Problem(**dict(p.__dict__, mark_order=[0, 3, 1])), 'mark_order not below n_marks')
    refused(ctx, S.R.Problem(**dict(p.__dict__, mark_order=[0, 1, 1])), 'names a raw mark twice')
    refused(ctx, S.R.Problem(**dict(p.__dict__, cand_contig=[0, 0])), 'exactly one of')
    refused(ctx, S.R.Problem(**dict(p.__dict__, cand_ctg_off=None)), 'exactly one of')
    refused(ctx, S.R.Problem(**dict(p.__dict__, cand_ctg_off=[0, 1])), 'cand_ctg_off')
    refused(ctx, S.R.Problem(**dict(p.__dict__, cand_ctg_off=[0, 2, 1, 2])), 'cand_ctg_off')
    refused(ctx, RK.problem([[cand(1, 7, [(0, ABSENT)])], [cand(1, 9, [(0, ABSENT)])]]), 'two contigs')
    refused(ctx, RK.problem([[cand(1, 7, [(0, 0)]), cand(1, 9, [(0, 1)])]], [tag(1, 0, 7)] * 2), 'two read indices')
    big = RK.problem([[cand(1, 7, [(0, ABSENT), (1, ABSENT)]), cand(0, 0, [(1, ABSENT)])], [cand(2, 9, [(0, ABSENT)])]], form='contig')
    refused(ctx, big, 'two contigs', mask=[1, 0, 1])
    check(ctx, p)                                                             # the context works on


def test_the_plan_is_stricter_about_masked_candidates(ctx):
    """Two 1|1 calls share a name across two contigs: duet_sv_tags_* looks at het calls only and accepts, the plan looks at every
    masked candidate and refuses; with the two left out of the mask it accepts."""
    p = RK.problem([[cand(3, 7, [(0, ABSENT)]), cand(1, 5, [(1, ABSENT)])], [cand(3, 9, [(0, ABSENT)])]])
    want, _, counts = S.sv_tags(p)
    out, _, got = ctx.sv_tags_host(**dict(host_arrays(p), pred=p.pred))
    assert out.tobytes() == np.array(want, dtype=np.uint64).tobytes() and got == counts
    refused(ctx, p, 'two contigs')
    refused(ctx, p, 'two contigs', mask=[1, 0, 1])
    check(ctx, p, masks=([0, 1, 0],))


def test_apply_without_a_plan_and_with_bad_settings():
    c = _lib.Context(0)
    try:
        p = RK.problem([[cand(1, 7, [(0, ABSENT)]), cand(0, 0, [(0, ABSENT)])]])
        r = Resident(p)
        for go in (lambda: r.apply(c, p.pred), lambda: c.sv_tags_apply_host(p.pred, np.full(2, UN, dtype=np.uint64))):
            with pytest.raises(_lib.DuetLibraryError, match='without a plan'):
                go()
        r.plan(c)
        base = r.words().copy()
        for kw, text in ((dict(min_votes=0), 'min_votes'), (dict(pc_new=S.CAP_MAX + 1), 'pc_new')):
            with pytest.raises(_lib.DuetLibraryError, match=text):
                r.apply(c, p.pred, **kw)
            with pytest.raises(_lib.DuetLibraryError, match=text):
                c.sv_tags_apply_host(p.pred, base.copy(), **kw)
            four = np.full(4, IFILL, dtype=np.uint32)                           # the entry itself: a refused call writes no counter
            h_pred, words = np.array(p.pred, dtype=np.uint8), base.copy()
            rc = c.lib.duet_sv_tags_apply_host(c.handle, h_pred.ctypes.data, kw.get('min_votes', 1), kw.get('pc_new', 0),
                                               words.ctypes.data, four.ctypes.data)
            assert rc != 0 and (four == IFILL).all() and words.tobytes() == base.tobytes()
        assert r.words().tobytes() == base.tobytes()
        assert r.apply(c, p.pred, pc_new=S.CAP_MAX)[1] == (2, 1, 1, 0)
    finally:
        c.close()


# ---- the second runs of five vectors, resident ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('seed', sorted(K.PINNED))
def test_resident_second_runs_of_five_vectors(ctx, seed):
    """Nothing leaves the device between the runs: the features under the cap, the first-run pred of the five grid vectors and the
    phase sets (duet_tune_sweep_device), ONE plan with mask = eligible, five applies, and per vector the features call on the same
    problem pointed at out_tag and the identity index -- against the reference's records on the reference's expanded problem."""
    import torch
    from duet_amd.devmem import DeviceProblem, upload
    soa, cap = K.untagged_soa(seed), 8100
    vecs = tune.expand_grid(GRID)
    C, M, V = soa.n_cands, soa.n_marks, len(vecs)
    feat0 = pc_cap_ref.features(K.oracle_form(soa), 50, 2, cap)
    dp = DeviceProblem(soa, 50, 2)
    st = torch.cuda.current_stream(dp.device).cuda_stream
    rec = _lib.FEATURE_DTYPE.itemsize
    feat = torch.zeros(C * rec, dtype=torch.uint8, device=dp.device)
    feat2 = torch.zeros(C * rec, dtype=torch.uint8, device=dp.device)
    ctx.features_device(dp.problem, feat.data_ptr(), st, pc_cap=cap)
    d_vec = upload(torch, dp.device, vecs, np.float64)
    pred, ps = torch.zeros(V * C, dtype=torch.uint8, device=dp.device), torch.zeros(C, dtype=torch.int32, device=dp.device)
    ctx.sweep_device(feat.data_ptr(), C, d_vec.data_ptr(), V, None, 0, st, out_pred_ptr=pred.data_ptr(), out_ps_ptr=ps.data_ptr())
    mask = feat.view(C, rec)[:, _lib.FEATURE_DTYPE.fields['eligible'][1]].contiguous()
    names, n_names = K.mark_names(soa)
    d_names = upload(torch, dp.device, names, np.uint32)
    ef = dp.problem
    p = _lib.ReadTagsProblem()
    p.n_cands, p.n_marks, p.n_reads, p.n_names, p.n_contigs = C, M, soa.n_reads, n_names, soa.n_contigs
    p.cand_off, p.mark_read, p.read_tag, p.mark_name = ef.cand_off, ef.mark_read, ef.read_tag, d_names.data_ptr()
    p.cand_ctg_off, p.ps = soa.cand_ctg_off.ctypes.data, ps.data_ptr()
    out, index = dev(np.full(M, FILL, dtype=np.uint64)), dev(np.full(M, IFILL, dtype=np.uint32))
    counts = torch.zeros(4 * V, dtype=torch.int32, device=dp.device)
    ctx.sv_tags_plan_device(p, out.data_ptr(), index.data_ptr(), cand_mask_ptr=mask.data_ptr(), pc_cap=cap, stream=st)
    second = _lib.EfProblem.from_buffer_copy(ef)
    second.read_tag, second.mark_read, second.n_reads = out.data_ptr(), index.data_ptr(), M
    got_pred = pred.cpu().numpy().reshape(V, C)
    distinct = set()
    for v in range(V):
        ctx.sv_tags_apply_device(pred.data_ptr() + v * C, out.data_ptr(), counts.data_ptr() + 16 * v, stream=st)
        ctx.features_device(second, feat2.data_ptr(), st, pc_cap=cap)
        p0 = np.array(tune_ref_preds(feat0, vecs[v]), dtype=np.uint8)
        assert np.array_equal(got_pred[v], p0)
        s0 = [f['ps'] if f['eligible'] else 0 for f in feat0]
        want_tags, _, want_counts = S.sv_tags(K.problem_of(soa, p0, s0))
        assert back(out, np.uint64, M).tobytes() == np.array(want_tags, dtype=np.uint64).tobytes()
        want = cap_line_ref.records(pc_cap_ref.features(K.oracle_form(K.expanded_soa(soa, want_tags)), 50, 2, cap))
        got = back(feat2, _lib.FEATURE_DTYPE, C)
        for name in ('eligible', 'kept', 'cls', 'hap1', 'hap2', 'hap0', 'allhap', 't1', 't2'):
            assert np.array_equal(got[name], want[name]), (v, name)
        el = want['eligible'] != 0
        assert np.array_equal(got['ps'][el], want['ps'][el])
        assert tuple(counts.cpu().numpy()[4 * v:4 * v + 4].tolist()) == want_counts + (0,)
        distinct.add(np.array(want_tags, dtype=np.uint64).tobytes())
    assert len(distinct) >= 2                                                  # the tags do depend on the vector
    assert back(index, np.uint32, M).tobytes() == np.arange(M, dtype=np.uint32).tobytes()


def tune_ref_preds(feat, vec):
    from tests import tune_ref
    return tune_ref.preds_from_features(feat, vec)
