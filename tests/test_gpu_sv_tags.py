# coding=utf-8
"""-m gpu: the tags from other SVs (duet_amd/csrc/duet_svtags.hip) against tests/sv_tags_ref.py, byte for byte on out_tag, the
identity index and the three counters, through both entries: the smallest shapes at which each stage can go wrong, the contracts,
the second run against the C oracle on the reference's expanded problem, and `duet --vote_sv_tags` in both modes."""
import logging
import os
import shutil
import sys
import time

import numpy as np
import pytest

from duet_amd import _lib, engine, sv_tags, svim_mode, synth, tune
from duet_amd.read_file import init_chrom_list
from tests import helpers as H
from tests import pc_cap_ref, soa_fuzz, tune_ref
from tests import read_tags_cases as RK
from tests import sv_tags_cases as K
from tests import sv_tags_ref as S

pytestmark = pytest.mark.gpu

ABSENT, UN = S.ABSENT, S.UNTAGGED
tag = S.tag
FILL = 0xABABABABABABABAB


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


def arrays(p):
    kw = p.arrays()
    kw.pop('cand_pos')
    return kw


def device_call(ctx, p, raises=None, **settings):
    """duet_sv_tags_device on uploaded arrays -> (out_tag, out_index, counts); the outputs start as FILL.  raises: the call must be
    refused with that text; the buffers are read back all the same and counts is None."""
    import torch
    M, C = len(p.mark_read), len(p.pred)
    keep = dict(cand_off=dev(np.array(p.cand_off, dtype=np.uint32)), mark_read=dev(np.array(p.mark_read, dtype=np.uint32)),
                mark_name=dev(np.array(p.mark_name, dtype=np.uint32)), pred=dev(np.array(p.pred, dtype=np.uint8)),
                ps=dev(np.array(p.ps, dtype=np.uint32)), read_tag=dev(np.array(p.read_tag, dtype=np.uint64)))
    if p.mark_order is not None:
        keep['mark_order'] = dev(np.array(p.mark_order, dtype=np.uint32))
    if p.cand_contig is not None:
        keep['cand_contig'] = dev(np.array(p.cand_contig, dtype=np.uint16))
    prob = _lib.ReadTagsProblem()
    prob.n_cands, prob.n_marks, prob.n_reads, prob.n_names = C, M, len(p.read_tag), p.n_names
    for k, t in keep.items():
        setattr(prob, k, t.data_ptr())
    off = None
    if p.cand_ctg_off is not None:
        off = np.array(p.cand_ctg_off, dtype=np.uint32)
        prob.cand_ctg_off, prob.n_contigs = off.ctypes.data, len(off) - 1
    out, index = dev(np.full(max(M, 1), FILL, dtype=np.uint64)), dev(np.full(max(M, 1), 0xABABABAB, dtype=np.uint32))
    counts = None
    try:
        if raises is None:
            counts = ctx.sv_tags_device(prob, out.data_ptr(), index.data_ptr(), **settings)
        else:
            with pytest.raises(_lib.DuetLibraryError, match=raises):
                ctx.sv_tags_device(prob, out.data_ptr(), index.data_ptr(), **settings)
    finally:
        torch.cuda.synchronize()
    return back(out, np.uint64, M), back(index, np.uint32, M), counts


def check(ctx, p, min_votes=1, pc_new=0):
    """Both entries equal the reference byte for byte -> (out_tag as a list, counts)."""
    want, index, counts = S.sv_tags(p, min_votes, pc_new)
    M = len(p.mark_read)
    if want is None:                                                           # no candidate or no mark: nothing is written
        want_bytes, index_bytes = np.full(M, FILL, dtype=np.uint64).tobytes(), np.full(M, 0xABABABAB, dtype=np.uint32).tobytes()
    else:
        want_bytes, index_bytes = np.array(want, dtype=np.uint64).tobytes(), np.arange(M, dtype=np.uint32).tobytes()
    out, idx, got = ctx.sv_tags_host(min_votes=min_votes, pc_new=pc_new, out_tag=np.full(M, FILL, dtype=np.uint64),
                                     out_index=np.full(M, 0xABABABAB, dtype=np.uint32), **arrays(p))
    assert (out.tobytes(), idx.tobytes(), got) == (want_bytes, index_bytes, counts)
    out, idx, got = device_call(ctx, p, min_votes=min_votes, pc_new=pc_new)
    assert (out.tobytes(), idx.tobytes(), got) == (want_bytes, index_bytes, counts)
    return want, counts


def refused(ctx, p, match, **settings):
    """Both entries refuse with `match` and leave out_tag and the index untouched."""
    M = len(p.mark_read)
    with pytest.raises(S.Refused):
        S.sv_tags(p, settings.get('min_votes', 1), settings.get('pc_new', 0), settings.get('pc_cap', 8100))
    out, idx = np.full(M, FILL, dtype=np.uint64), np.full(M, 0xABABABAB, dtype=np.uint32)
    with pytest.raises(_lib.DuetLibraryError, match=match):
        ctx.sv_tags_host(out_tag=out, out_index=idx, **dict(arrays(p), **settings))
    assert (out == FILL).all() and (idx == 0xABABABAB).all()
    if (p.cand_ctg_off is None) != (p.cand_contig is None):                    # (device_call states one contig form)
        out, idx, _ = device_call(ctx, p, raises=match, **settings)
        assert len(out) == M and (out == FILL).all() and (idx == 0xABABABAB).all()


def cand(pred, ps, marks, pos=1000):
    return dict(pred=pred, ps=ps, marks=marks, pos=pos)


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------

def sized(M, C, seed, form='off', permute=0):
    """C candidates over M marks (C <= M or M == 0), reads shared between neighbours, a third of the reads tagged."""
    rng = np.random.RandomState(seed)
    cuts = np.sort(rng.choice(np.arange(1, M), C - 1, replace=False)) if C > 1 and M > 1 else np.zeros(0, dtype=np.int64)
    off = [0] + [int(x) for x in cuts] + [M] * (C - len(cuts))
    n_reads = max(M // 3, 1)
    tags = [tag(1 + int(rng.randint(2)), int(rng.randint(9000)), 7 + int(rng.randint(3))) if rng.randint(3) == 0 else UN for _ in range(n_reads)]
    # (a read belongs to one contig: the first half of the candidates draws from the first half of the reads)
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
    assert out == [UN, UN, tag(1, 0, 7)] and counts == (2, 0, 0)               # no het candidate at all


# ---- the spellings of no-tag, and tagged words ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('read', [ABSENT, 2, 3, 1 << 31, 1])
def test_every_spelling_of_no_tag(ctx, read):
    p = RK.problem([[cand(1, 7, [(0, read)]), cand(3, 0, [(0, read)])]], [tag(1, 0, 5), UN])
    out, counts = check(ctx, p, pc_new=77)
    assert out == [UN, tag(1, 77, 7)] and counts == (2, 1, 1)


def test_tagged_words_are_copied_whatever_they_hold(ctx):
    words = [tag(0, 3, 7), tag(3, 8101, 7), tag(1, (1 << 30) - 2, 9), tag(2, 0, 0), tag(3, (1 << 30) - 1, 0xFFFFFFFE)]
    marks = [(i, i) for i in range(5)] + [(5, ABSENT)]
    for cap in (0, 8100, S.CAP_MAX):
        p = RK.problem([[cand(1, 7, marks), cand(2, 9, marks)]], words)
        out, _, counts = ctx.sv_tags_host(pc_cap=cap, **arrays(p))
        assert out.tolist() == words + [tag(2, 0, 9)] + words + [tag(1, 0, 7)] and counts == (2, 2, 0)
    check(ctx, p)


# ---- the records of one name ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_ps', [1, 2, 3, 65])
def test_one_name_in_many_phase_sets(ctx, n_ps):
    # phase set 10 * i holds i + 1 marks of 1|0 calls (two candidates each beyond the first); the asker lists the name once
    cands = [cand(1, 10 * i, [(0, ABSENT)] * (i + 1), pos=i) for i in range(n_ps)] + [cand(0, 0, [(0, ABSENT), (1, ABSENT)])]
    out, counts = check(ctx, RK.problem([cands]))
    assert out[-2] == tag(1, 0, 10 * (n_ps - 1)) and out[-1] == UN
    # the largest phase set's own marks see it empty: with one phase set nothing, else the runner-up
    assert out[-3] == (UN if n_ps == 1 else tag(1, 0, 10 * (n_ps - 2)))


def test_ties_extreme_ps_and_zero_after_removal(ctx):
    ask = cand(0, 0, [(0, ABSENT)])
    out, _ = check(ctx, RK.problem([[cand(1, 0xFFFFFFFE, [(0, ABSENT)] * 2), cand(2, 0, [(0, ABSENT)] * 2), ask]]))
    assert out[-1] == tag(2, 0, 0)                                             # equal |d|: the smaller PS, here 0
    out, _ = check(ctx, RK.problem([[cand(2, 0x80000000, [(0, ABSENT)]), cand(1, 5, [(0, ABSENT)]), ask]]))
    assert out[-1] == tag(1, 0, 5)                                             # compared as unsigned 32-bit numbers
    out, counts = check(ctx, RK.problem([[cand(1, 7, [(0, ABSENT)] * 3), ask]]))
    assert out == [UN] * 3 + [tag(1, 0, 7)] and counts == (4, 1, 3)            # d exactly 0 after the own removal
    for mv in (1, 3):
        for n in (mv - 1, mv):
            out, _ = check(ctx, RK.problem([[cand(2, 7, [(0, ABSENT)] * n + [(1, ABSENT)]), ask]]), min_votes=mv)
            assert out[-1] == (tag(2, 0, 7) if n >= mv else UN)


# ---- duplicates inside a candidate -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('k', [2, 3, 64, 65, 257])
def test_a_candidate_lists_a_read_k_times(ctx, k):
    # X lists name 0 k times among other names, so its run straddles wavefront and tile edges of the sorted order; Y brings k and
    # k + 1 marks of the other haplotype in two phase sets
    filler = [(1 + i, ABSENT) for i in range(70)]
    X = cand(1, 7, filler[:30] + [(0, ABSENT)] * k + filler[30:])
    Y, Z, W = cand(2, 7, [(0, ABSENT)] * k), cand(2, 9, [(0, ABSENT)] * (k + 1)), cand(3, 0, [(0, ABSENT)])
    out, counts = check(ctx, RK.problem([[cand(1, 5, filler), X, Y, Z, W]]))
    assert out[-1] == tag(2, 0, 9)                                             # W: 0 in PS 7, k + 1 in PS 9
    assert out[70 + 30] == tag(2, 0, 9) and out[70 + 70 + k] == tag(2, 0, 9)   # X's own: k against k + 1; Y's own: k against k + 1


def test_k_two_against_two_and_three(ctx):
    X = cand(1, 7, [(0, ABSENT)] * 2 + [(1, ABSENT)])
    for n, want in ((2, UN), (3, tag(2, 0, 7))):
        out, _ = check(ctx, RK.problem([[X, cand(2, 7, [(0, ABSENT)] * n), cand(0, 0, [(0, ABSENT)])]]))
        assert out[-1] == want and out[0] == out[1] == tag(2, 0, 7) and out[2] == UN


def test_one_candidate_of_70000_marks_under_one_name(ctx):
    """The run rule is not quadratic: one run of 70,000, crossing every tile of the sort and the scans."""
    n = 70000
    p = RK.problem([[cand(1, 7, [(0, ABSENT)] * n), cand(2, 7, [(0, ABSENT)] * 5), cand(0, 0, [(0, ABSENT)])]])
    want, _, counts = S.sv_tags(p)
    kw = arrays(p)
    ctx.sv_tags_host(**kw)
    t0 = time.perf_counter()
    out, idx, got = ctx.sv_tags_host(**kw)
    dt = time.perf_counter() - t0
    print('70,000 marks under one name: %.1f ms' % (1e3 * dt))
    assert out.tobytes() == np.array(want, dtype=np.uint64).tobytes() and got == counts == (n + 6, n + 6, 0)
    assert out[0] == tag(2, 0, 7) and out[-1] == tag(1, 0, 7) and dt < 1.0


# ---- refusals, determinism, side effects -----------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched(ctx):
    p = RK.problem([[cand(1, 7, [(0, ABSENT), (1, ABSENT)]), cand(2, 7, [(0, ABSENT)])]])
    refused(ctx, p, 'min_votes', min_votes=0)
    refused(ctx, p, 'pc_new', pc_new=S.CAP_MAX + 1)
    refused(ctx, p, 'pc_cap', pc_cap=S.CAP_MAX + 1)
    refused(ctx, RK.problem([[cand(1, 7, [(0, ABSENT)]), cand(4, 7, [(1, ABSENT)])]]), 'pred above 3')
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
    # (refused() runs the device entry too and reads its buffers back: the round-trip-1 refusals -- pred, order, duplicate, name --
    # and the round-trip-3 ones, found after the words were staged.)  A contradiction beside marks that would get a tag:
    big = RK.problem([[cand(1, 7, [(0, ABSENT), (1, ABSENT)]), cand(0, 0, [(1, ABSENT)])], [cand(2, 9, [(0, ABSENT)])]], form='contig')
    refused(ctx, big, 'two contigs')
    check(ctx, p)                                                             # the context works on


def test_two_calls_give_identical_bytes(ctx):
    p = K.problem_of(K.untagged_soa(2), *K.oracle_calls(K.untagged_soa(2)))
    a, b = ctx.sv_tags_host(**arrays(p)), ctx.sv_tags_host(**arrays(p))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] == K.PINNED[2][0]
    assert device_call(ctx, p)[0].tobytes() == a[0].tobytes()


def test_nothing_of_ef_changes_after_a_call(ctx):
    soa = soa_fuzz.random_soa(3, n_contigs=4)
    before = (ctx.run_host(soa, 50, 2), ctx.features_host(soa, 50, 2), ctx.ps_links_host(soa, 50, 2))
    u = K.untagged_soa(5)
    check(ctx, K.problem_of(u, *K.oracle_calls(u)))
    check(ctx, sized(1025, 100, 9, 'contig', 4))
    after = (ctx.run_host(soa, 50, 2), ctx.features_host(soa, 50, 2), ctx.ps_links_host(soa, 50, 2))
    assert before[0][0].tobytes() == after[0][0].tobytes() and before[0][1].tobytes() == after[0][1].tobytes()
    assert before[1].tobytes() == after[1].tobytes() and before[2].tobytes() == after[2].tobytes()
    assert int((before[0][0] != 0).sum()) > 10


# ---- the second run against the oracle ---------------------------------------------------------------------------------------------------

def second_run_on_the_device(ctx, soa, run):
    p0, s0 = run(soa)
    p = K.problem_of(soa, p0, s0)
    out, idx, counts = ctx.sv_tags_host(**arrays(p))
    kw = {name: getattr(soa, name) for name, _ in engine.EfSoA.FIELDS}
    kw['read_tag'], kw['mark_read'] = out, idx
    p1, s1 = run(engine.EfSoA(read_off=soa.cand_off[soa.cand_ctg_off], **kw))
    change, n = ctx.ps_join_diff_host(p0, s0, p1, s1, np.zeros(0, dtype=_lib.PS_BLOCK_DTYPE), soa.n_contigs, cand_ctg_off=soa.cand_ctg_off)
    return dict(p0=p0, s0=s0, out=out, counts=counts, p1=p1, s1=s1, change=change, n=n)


@pytest.mark.parametrize('seed', sorted(K.PINNED))
def test_second_run_is_the_oracle_on_the_expanded_problem(ctx, seed):
    soa = K.untagged_soa(seed)
    got = second_run_on_the_device(ctx, soa, lambda s: ctx.run_host(s, 50, 2))
    want = K.second_run(soa, K.oracle_calls)
    assert np.array_equal(got['p0'], want['p0']) and np.array_equal(got['s0'], want['s0'])
    assert got['out'].tobytes() == np.array(want['out_tag'], dtype=np.uint64).tobytes() and got['counts'] == want['counts'] == K.PINNED[seed][0]
    assert np.array_equal(got['p1'], want['p1']) and np.array_equal(got['s1'], want['s1'])
    assert [_lib.JOIN_CHANGE_NAMES[int(c)] for c in got['change']] == want['codes']
    assert got['n'].tolist() == [want['codes'].count(n) for n in S.CHANGE] and want['codes'].count('gained') == K.PINNED[seed][1]
    host = sv_tags.change_codes(want['p0'], want['s0'], want['p1'], want['s1'])
    assert host[0].tobytes() == got['change'].tobytes() and host[1].tolist() == got['n'].tolist()


@pytest.mark.parametrize('seed', sorted(K.PINNED))
def test_resident_second_run_is_the_oracle_on_the_expanded_problem(ctx, seed):
    """Nothing leaves the device between the two runs: duet_ef_run_device on the resident problem, duet_sv_tags_device on its
    resident calls, duet_ef_run_device again on the same problem pointed at out_tag and the identity index -- against the C oracle
    on the reference's expanded problem."""
    import torch
    from duet_amd.devmem import DeviceProblem, upload
    soa = K.untagged_soa(seed)
    want = K.second_run(soa, K.oracle_calls)
    dp = DeviceProblem(soa, 50, 2, n_out=2)
    dp.run(ctx, slot=0)
    ctx.check()
    first = dp.results(0)
    assert np.array_equal(first[0], want['p0']) and np.array_equal(first[1], want['s0'])
    names, n_names = K.mark_names(soa)
    d_names = upload(torch, dp.device, names, np.uint32)
    M, ef, blk = soa.n_marks, dp.problem, dp.out_blocks[0]
    p = _lib.ReadTagsProblem()
    p.n_cands, p.n_marks, p.n_reads, p.n_names, p.n_contigs = soa.n_cands, M, soa.n_reads, n_names, soa.n_contigs
    p.cand_off, p.mark_read, p.read_tag, p.mark_name = ef.cand_off, ef.mark_read, ef.read_tag, d_names.data_ptr()
    p.cand_ctg_off = soa.cand_ctg_off.ctypes.data
    p.ps, p.pred = blk.data_ptr(), blk.data_ptr() + 4 * dp.n_max
    out, index = dev(np.full(M, FILL, dtype=np.uint64)), dev(np.full(M, 0xABABABAB, dtype=np.uint32))
    counts = ctx.sv_tags_device(p, out.data_ptr(), index.data_ptr())
    assert counts == want['counts'] == K.PINNED[seed][0]
    second = _lib.EfProblem.from_buffer_copy(ef)
    second.read_tag, second.mark_read, second.n_reads = out.data_ptr(), index.data_ptr(), M
    blk2 = dp.out_blocks[1]
    ctx.run_device(second, blk2.data_ptr() + 4 * dp.n_max, blk2.data_ptr(), torch.cuda.current_stream(dp.device).cuda_stream)
    ctx.check()
    p1, s1 = dp.results(1)
    assert back(out, np.uint64, M).tobytes() == np.array(want['out_tag'], dtype=np.uint64).tobytes()
    assert back(index, np.uint32, M).tobytes() == np.arange(M, dtype=np.uint32).tobytes()
    assert np.array_equal(p1, want['p1']) and np.array_equal(s1, want['s1'])
    assert not np.array_equal(p1, first[0])                                    # the second run is another run
    codes = [S.change(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(first[0], first[1], p1, s1)]
    assert codes == want['codes'] and codes.count('gained') == K.PINNED[seed][1]
    again = dp.results(0)
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])


@pytest.mark.parametrize('cap', [None, 2400])
def test_second_run_by_the_route_of_thresholds(ctx, cap):
    """--thresholds with the default vector, and --pc_cap 2400: the features under the cap plus one vector, on both problems."""
    soa, v = K.untagged_soa(2), tune.vector()
    got = second_run_on_the_device(ctx, soa, lambda s: tune.apply(dict(feat=ctx.features_host(s, 50, 2, pc_cap=cap)), v, ctx=ctx))

    def calls(s):
        feat = pc_cap_ref.features(K.oracle_form(s), 50, 2, 8100 if cap is None else cap)
        p = np.array(tune_ref.preds_from_features(feat, v), dtype=np.uint8)
        return p, np.array([f['ps'] if f['eligible'] else 0 for f in feat], dtype=np.uint32)
    p0, s0 = calls(soa)
    assert np.array_equal(got['p0'], p0) and np.array_equal(np.where(p0 != 0, got['s0'], 0), np.where(p0 != 0, s0, 0))
    # (the phase set of a candidate without a call is not part of the contract: the tags are derived from the device's own calls)
    want, _, counts = S.sv_tags(K.problem_of(soa, got['p0'], got['s0']))
    assert got['out'].tobytes() == np.array(want, dtype=np.uint64).tobytes() and got['counts'] == counts and counts[1] > 0
    p1, s1 = calls(K.expanded_soa(soa, want))
    called = lambda p, s: np.where(p != 0, s, 0)
    assert np.array_equal(got['p1'], p1) and np.array_equal(called(got['p1'], got['s1']), called(p1, s1))
    codes = [S.change(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(p0, called(p0, got['s0']), p1, called(p1, s1))]
    assert codes.count('gained') >= 1


# ---- the product ---------------------------------------------------------------------------------------------------------------------

def read(path):
    with open(path, 'rb') as f:
        return f.read()


def stub_stages(monkeypatch):
    from duet_amd import cli, stages
    for name in ('snp_calling', 'sv_calling', 'snp_phasing'):
        monkeypatch.setattr(stages, name, lambda *a: None)
    monkeypatch.setattr(cli, 'check_envs', lambda *a: None)
    monkeypatch.setattr(cli, 'set_logging', lambda *a: None)


def paths(home):
    return sv_tags.path_vcf(home), sv_tags.path_report(home)


def golden_home(root):
    from tests.test_c_oracle import materialise_bams
    home = str(root / 'w')
    shutil.copytree(os.path.join(H.GOLDEN, 'cases', 'fuzz_cutesv_s2'), home)
    materialise_bams(home)
    return home


def test_product_native_ingest(ctx, tmp_path, monkeypatch, caplog):
    """A golden work dir as it is (its untagged reads are the reads missing from the BAM text).  The expected files: the ingest's
    own problem and names, the reference's tags, the C oracle on the expanded problem, the ingest's row writer."""
    from duet_amd import cli
    from duet_amd import sv_phasing as sp
    home = golden_home(tmp_path)
    pinned = read(home + '/phased_sv.vcf')
    sp.sv_phasing(home, 50, 2, 4, False)
    assert read(home + '/phased_sv.vcf') == pinned and not any(os.path.exists(p) for p in paths(home))   # no file without the flag
    ing, chrom_list = sp.load_native(home, 4, False, home + '/sv_calling/variants.vcf', log=False, names=True)
    try:
        soa, nm = ing.soa, ing.mark_names()
        head = ing.header(False)
        p0, s0 = K.oracle_calls(soa)
        off = [int(x) for x in soa.cand_ctg_off]
        prob = S.R.Problem([int(x) for x in soa.cand_off], [int(x) for x in soa.mark_read], [int(x) for x in nm['mark_name']],
                           len(nm['name_off']) - 1, p0, s0, soa.cand_pos, [int(t) for t in soa.read_tag], cand_ctg_off=off)
        tags, _, counts = S.sv_tags(prob)
        p1, s1 = K.oracle_calls(K.expanded_soa(soa, tags))
        want_vcf = head + ing.emit_rows(p1, s1)
        codes = [S.change(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(p0, s0, p1, s1)]
        texts = sp.contig_texts(ing, chrom_list, '--vote_sv_tags')
        contig = np.repeat(np.arange(soa.n_contigs), np.diff(soa.cand_ctg_off.astype(np.int64)))
        change = np.array([S.CHANGE.index(c) for c in codes], dtype=np.uint8)
        want_report = (sv_tags.report_header() + sv_tags.report_text(texts, contig, soa.cand_pos, soa.cand_svlen, change, p0, s0, p1, s1)).encode()
    finally:
        ing.close()
    print('native golden: marks', counts, 'changes', {c: codes.count(c) for c in set(codes)})
    # the reference alone, pinned: the input is not degenerate
    assert counts == (747, 86, 30) and (codes.count('gained'), codes.count('lost')) == (3, 1)
    with caplog.at_level(logging.INFO):
        sp.sv_phasing(home, 50, 2, 4, False, vote_sv_tags=True)
    assert read(home + '/phased_sv.vcf') == pinned
    assert (read(paths(home)[0]), read(paths(home)[1])) == (want_vcf, want_report)
    assert sv_tags.summary_text(counts, [codes.count(n) for n in S.CHANGE]) in caplog.text
    # by the route of --pc_cap the first file stays the cap's
    sp.sv_phasing(home, 50, 2, 4, False, pc_cap=2400)
    capped = read(home + '/phased_sv.vcf')
    sp.sv_phasing(home, 50, 2, 4, False, pc_cap=2400, vote_sv_tags=True, sv_tag_min=2, sv_tag_pc=100)
    assert read(home + '/phased_sv.vcf') == capped and read(paths(home)[0]).startswith(head)
    # the command
    stub_stages(monkeypatch)
    for p in paths(home):
        os.remove(p)
    monkeypatch.setattr(sys, 'argv', ['duet', 'in.bam', 'ref.fa', home])
    cli.main(None)
    assert read(home + '/phased_sv.vcf') == pinned and not any(os.path.exists(p) for p in paths(home))
    monkeypatch.setattr(sys, 'argv', ['duet', 'in.bam', 'ref.fa', home, '--vote_sv_tags'])
    cli.main(None)
    assert read(home + '/phased_sv.vcf') == pinned and (read(paths(home)[0]), read(paths(home)[1])) == (want_vcf, want_report)


def test_a_second_run_that_divides_by_zero_leaves_the_header_alone(tmp_path, monkeypatch):
    """phased_sv.vcf is written first and in full; the error of the second run propagates, phased_sv.sv_tags.vcf keeps its header
    and no report is written.  (The run on the expanded problem is made to raise: no input of the suite divides by zero there
    alone.)"""
    from duet_amd.sv_phasing import sv_phasing
    home = golden_home(tmp_path)
    pinned = read(home + '/phased_sv.vcf')
    os.remove(home + '/phased_sv.vcf')
    real, seen = engine.run_ef, []

    def run_ef(soa, *args, **kw):
        seen.append(soa.n_reads)
        if soa.n_reads == soa.n_marks and len(seen) > 1:
            raise ZeroDivisionError('division by zero')
        return real(soa, *args, **kw)
    monkeypatch.setattr(engine, 'run_ef', run_ef)
    with pytest.raises(ZeroDivisionError):
        sv_phasing(home, 50, 2, 4, False, vote_sv_tags=True)
    assert read(home + '/phased_sv.vcf') == pinned
    vcf, report = paths(home)
    assert read(vcf) == pinned[:pinned.index(b'\n', pinned.index(b'#CHROM')) + 1] and not os.path.exists(report)


def test_product_svim_gpu(ctx, tmp_path, monkeypatch):
    from duet_amd import cli
    from duet_amd.devmem import DeviceSvim
    from duet_amd.native import NativeIngest
    home = str(tmp_path / 'w')
    synth.write_svim_workdir(home, H.case_contigs('genome_small', 5), 5)
    stub_stages(monkeypatch)
    base = ['duet', 'in.bam', 'ref.fa', home, '-b', 'svim-gpu']
    monkeypatch.setattr(sys, 'argv', base)
    cli.main(None)
    plain = read(home + '/phased_sv.vcf')
    assert plain.count(b'\n') > 100 and not any(os.path.exists(p) for p in paths(home))
    monkeypatch.setattr(sys, 'argv', base + ['--vote_sv_tags'])
    cli.main(None)
    assert read(home + '/phased_sv.vcf') == plain
    # an independent reference: a copy writes its clustered calls, the native ingest reads them back as an E/F problem with the
    # marks' names, the reference makes the tags and the C oracle runs on the expanded problem
    from duet_amd import sv_phasing as sp
    copy = str(tmp_path / 'copy')
    shutil.copytree(home, copy)
    svim_mode.sv_phasing_from_bams(copy, 50, 2, 4, False, 0.9, 0, write_sv_calls=True)
    _, txt = tune._candidates(copy, 50, 2, False, 4)
    ing, _ = sp.load_native(copy, 4, False, copy + '/sv_calling/variants.vcf', log=False, names=True)
    try:
        kw = {name: getattr(ing.soa, name).copy() for name, _ in engine.EfSoA.FIELDS}
        soa, mark_name = engine.EfSoA(read_off=ing.soa.read_off.copy(), **kw), [int(x) for x in ing.mark_names()['mark_name']]
        n_names = len(ing.mark_names()['name_off']) - 1
    finally:
        ing.close()
    p0, s0 = K.oracle_calls(soa)
    ref = S.R.Problem([int(x) for x in soa.cand_off], [int(x) for x in soa.mark_read], mark_name, n_names, p0, s0, soa.cand_pos,
                      [int(t) for t in soa.read_tag], cand_ctg_off=[int(x) for x in soa.cand_ctg_off])
    ref_tags, _, ref_counts = S.sv_tags(ref)
    r1, q1 = K.oracle_calls(K.expanded_soa(soa, ref_tags))
    ref_codes = [S.change(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(p0, s0, r1, q1)]
    col = np.repeat(np.arange(soa.n_contigs), np.diff(soa.cand_ctg_off.astype(np.int64))).astype(np.uint16)
    shape = dict(chroms=init_chrom_list(False, home), cand_contig=col,
                 cand_type=np.array([svim_mode.SV_TYPE_NAMES.index(t) for t in txt['svtype']], dtype=np.uint8),
                 cand_pos=soa.cand_pos, cand_span=soa.cand_svlen)
    head = svim_mode.header_text(home, shape['chroms'])
    assert (head + svim_mode.rows_text(home, dict(shape, pred=p0, ps=s0))).encode() == plain     # (the builder states the first file)
    assert read(paths(home)[0]) == (head + svim_mode.rows_text(home, dict(shape, pred=r1, ps=q1))).encode() != plain
    assert ref_codes.count('gained') >= 1 and ref_counts[1] > 0
    # the same on the resident arrays: the entry against the reference, the cluster result and the first calls kept
    chroms = init_chrom_list(False, home)
    texts = svim_mode.spelled_contigs(home, chroms)
    ing, got = NativeIngest.extract(home + '/snp_phasing/', chroms, 4, 50, 20, 1000, names=True)
    ing.close()
    ds = DeviceSvim(got, got['read_tag'], got['depth'], got['depth_off'], 1000, 50, 2, max_dist=0.9)
    ds.run_fused(ctx)
    ctx.check()
    first = ds.fetch()
    second = ds.run_sv_tags(ctx, got)
    again = ds.fetch()
    assert all(first[k].tobytes() == again[k].tobytes() for k in first)
    prob = S.R.Problem(first['cand_off'], got['read'], got['mark_name'], len(got['name_off']) - 1, first['pred'], first['ps'],
                       first['cand_pos'], [int(t) for t in got['read_tag']], cand_contig=first['cand_contig'], mark_order=first['order'])
    want, _, counts = S.sv_tags(prob)
    assert second['marks'] == counts
    N = len(first['pred'])
    p1, s1 = second['pred'][:N].cpu().numpy(), second['ps'][:N].cpu().numpy().view(np.uint32)
    codes, n = sv_tags.change_codes(first['pred'], first['ps'], p1, s1)
    assert second['change'].tobytes() == codes.tobytes() and second['counts'].tolist() == n.tolist()
    print('svim-gpu: marks', counts, 'changes', n.tolist())
    assert counts == ref_counts and np.array_equal(p1, r1) and [_lib.JOIN_CHANGE_NAMES[int(x)] for x in codes] == ref_codes
    rows = ds.phased_rows(ctx, texts, pred=second['pred'], ps=second['ps'])[0].tobytes()
    assert read(paths(home)[0]) == svim_mode.header_text(home, chroms).encode() + rows
    res = dict(cand_contig=first['cand_contig'], cand_pos=first['cand_pos'], cand_span=first['cand_span'])
    report = sv_tags.report_text(texts, res['cand_contig'], res['cand_pos'], res['cand_span'], codes, first['pred'], first['ps'], p1, s1)
    assert read(paths(home)[1]) == (sv_tags.report_header() + report).encode()
    # by the route of --thresholds the same calls come out of the default vector
    t = ds.run_sv_tags(ctx, got, thresholds=tune.vector())
    assert t['pred'][:N].cpu().numpy().tobytes() == p1.tobytes() and t['marks'] == counts


def test_product_refusals_leave_no_file(tmp_path, monkeypatch):
    from duet_amd import cli
    from duet_amd.sv_phasing import sv_phasing
    out = tmp_path / 'out'
    stub_stages(monkeypatch)
    for argv, text in ((['--vote_sv_tags', '--gpus', '2'], '--vote_sv_tags works on the single-GPU path only'),
                       (['--vote_sv_tags', '--join_ps'], 'do not work together'),
                       (['--sv_tag_min', '3'], 'need --vote_sv_tags'),
                       (['--vote_sv_tags', '--sv_tag_min', '0'], '--sv_tag_min takes an integer >= 1'),
                       (['--vote_sv_tags', '--sv_tag_pc', str((1 << 30) - 2)], '--sv_tag_pc takes an integer')):
        monkeypatch.setattr(sys, 'argv', ['duet', 'in.bam', 'ref.fa', str(out)] + argv)
        with pytest.raises(SystemExit, match=text):
            cli.main(None)
    assert not out.exists()
    home = golden_home(tmp_path)
    os.remove(home + '/phased_sv.vcf')
    monkeypatch.setenv('DUET_NATIVE_INGEST', '0')
    before = sorted(os.listdir(home))
    with pytest.raises(RuntimeError, match='--vote_sv_tags needs the native ingest'):
        sv_phasing(home, 50, 2, 4, False, vote_sv_tags=True)
    with pytest.raises(RuntimeError, match='--vote_sv_tags need the native ingest'):
        sv_phasing(home, 50, 2, 4, False, pc_cap=2400, vote_sv_tags=True)
    assert sorted(os.listdir(home)) == before
