# coding=utf-8
"""-m gpu: the read tags from phased SVs (duet_amd/csrc/duet_readtags.hip) against tests/read_tags_ref.py: the records byte for
byte (tobytes() on the structured array), the rows text byte for byte; the smallest shapes at which each stage can go wrong and
the contracts of the four entries.

The random problems are the five of read_tags_cases.RANDOM; tests/test_read_tags_host.py checks without a GPU that each yields a
record and the five together every status but other_ps, which has hand-built cases here."""
import ctypes

import numpy as np
import pytest

from duet_amd import _lib
from tests import read_tags_cases as K
from tests import read_tags_ref as R
from tests import soa_fuzz

pytestmark = pytest.mark.gpu

DT = _lib.READ_TAG_DTYPE
ABSENT = R.ABSENT
CAP_MAX = (1 << 30) - 3
tag = K.tag


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def n_contigs(p):
    return len(p.cand_ctg_off) - 1 if p.cand_ctg_off is not None else max(list(p.cand_contig) + [0]) + 1


def check(ctx, p, cap=None, texts=None, chroms=None):
    """The device's records and rows equal the reference's, byte for byte -> the records."""
    want = R.read_tags(p, R.PC_MAX if cap is None else cap)
    got = ctx.read_tags_host(pc_cap=cap, **p.arrays())
    assert got.dtype == DT and got.tobytes() == R.records(want, DT).tobytes(), (got, want)
    chroms = chroms or ['chr%d' % (k + 1) for k in range(n_contigs(p))]
    texts = texts or K.default_names(p.n_names)[0]
    off, pool = K.pool_of(texts)
    text = ctx.read_tags_rows_host(got, off, pool, chroms, p.read_tag)
    assert text == R.rows_text(want, texts, chroms, p.read_tag).encode()
    return got


def refused(ctx, p, match, cap=None, out_cap=None):
    """The call is refused with `match` in the message and nothing written -> the record count it reports."""
    with pytest.raises(_lib.DuetLibraryError, match=match) as e:
        ctx.read_tags_host(pc_cap=cap, out_cap=out_cap, **p.arrays())
    assert not e.value.out.view(np.uint8).any()
    return e.value.n_recs


def status(recs):
    return [R.STATUS[int(s)] for s in recs['status']]


def one_read(calls, tags, read=0):
    return K.problem([[dict(pred=pr, ps=ps, pos=100 * (i + 1), marks=[(0, read)]) for i, (pr, ps) in enumerate(calls)]], tags)


# ---- empty problems ----------------------------------------------------------------------------------------------------------------

def test_empty_problems(ctx):
    none = K.problem([[]])
    assert len(none.pred) == 0 and len(check(ctx, none)) == 0
    assert len(check(ctx, K.problem([[], [], []], form='contig'))) == 0
    no_marks = K.problem([[dict(marks=[]), dict(pred=2, marks=[])]])
    assert len(no_marks.pred) == 2 and len(no_marks.mark_read) == 0 and len(check(ctx, no_marks)) == 0
    no_het = K.problem([[dict(pred=0, marks=[(0, ABSENT)]), dict(pred=3, marks=[(0, ABSENT), (1, ABSENT)])]])
    assert len(check(ctx, no_het)) == 0
    got = check(ctx, K.problem([[dict(pred=2, ps=9, pos=77, marks=[(0, ABSENT)])]]))
    assert [tuple(int(x) for x in r) for r in got] == [(0, 0, 9, ABSENT, 0, 1, 77, 77, R.STATUS.index('new'), 0)]


# ---- the tiles of the sort and the scans ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('V', [4095, 4096, 4097])
def test_sort_tile_edges(ctx, V):
    # one het candidate of V marks over 1000 names, a dropped one in front and a 1|1 call behind
    p = K.problem([[dict(pred=0, marks=[(5, ABSENT)] * 3), dict(pred=2, marks=[((i * 7) % 1000, ABSENT) for i in range(V)]),
                    dict(pred=3, marks=[(6, ABSENT)])]])
    got = check(ctx, p)
    assert len(got) == 1000 and int(got['n_h2'].sum()) == V


@pytest.mark.parametrize('C', [2047, 2048, 2049])
def test_scan_tile_edges(ctx, C):
    # C het candidates of one mark each, every mark a read of its own: C records
    p = K.problem([[dict(pred=1 + (c & 1), ps=c % 3, pos=c, marks=[((c * 5) % C if C % 5 else c, ABSENT)]) for c in range(C)]])
    assert len(set(p.mark_name)) == C
    assert len(check(ctx, p)) == C


def test_candidate_sizes(ctx):
    cands, nxt = [], 1
    for n in (1, 63, 64, 65, 129, 5000):
        cands.append(dict(pred=1 + (n & 1), ps=7, pos=n, marks=[(0, 0)] + [(nxt + i, ABSENT) for i in range(n - 1)]))
        cands.append(dict(pred=3, ps=7, marks=[(0, 0)]))
        nxt += n - 1
    got = check(ctx, K.problem([cands], [tag(1, 0, 7)]))
    assert (int(got['n_h1'][0]), int(got['n_h2'][0]), int(got['pos_min'][0]), int(got['pos_max'][0])) == (2, 4, 1, 5000)
    assert len(got) == nxt


# ---- placement -----------------------------------------------------------------------------------------------------------------------

def test_placement_and_the_four_forms(ctx):
    het = lambda name, **kw: dict(pred=kw.pop('pred', 1), marks=[(name, ABSENT), (name + 1, ABSENT)], **kw)
    quiet = lambda name: dict(pred=0, marks=[(name, ABSENT)])
    p = K.problem([[], [], [het(0), quiet(2), quiet(3), het(4, pred=2), quiet(6)], [], [], [quiet(7), het(8), het(10, ps=9)], []])
    got = check(ctx, p)
    assert [(int(r['name']), int(r['contig'])) for r in got] == [(0, 2), (1, 2), (4, 2), (5, 2), (8, 5), (9, 5), (10, 5), (11, 5)]
    for q in K.same_in_other_forms(p):
        assert check(ctx, q).tobytes() == got.tobytes()
    first_last = K.problem([[het(0), quiet(2), het(3)]])
    assert len(check(ctx, first_last)) == 4
    built = K.problem([[het(0), quiet(2)], [het(3)]], form='contig', permute=5)
    assert built.mark_order is not None and built.cand_contig == [0, 0, 1]
    assert [int(k) for k in check(ctx, built)['contig']] == [0, 0, 1, 1]


# ---- read multiplicity ---------------------------------------------------------------------------------------------------------------

def test_read_multiplicity(ctx):
    twice = check(ctx, K.problem([[dict(pred=2, marks=[(0, 0), (1, ABSENT), (0, 0)])]], [tag(2, 0, 7)]))
    assert [(int(r['n_h1']), int(r['n_h2'])) for r in twice] == [(0, 2), (0, 1)] and status(twice) == ['agree', 'new']
    many = check(ctx, K.problem([[dict(pred=1 + (c % 3 == 0), ps=7, pos=10 + c, marks=[(0, 0)]) for c in range(5000)]], [tag(1, 0, 7)]))
    assert len(many) == 1 and (int(many['n_h1'][0]), int(many['n_h2'][0])) == (3333, 1667)
    assert (int(many['pos_min'][0]), int(many['pos_max'][0])) == (10, 5009) and status(many) == ['agree']
    three = check(ctx, one_read([(1, 0xFFFFFFFE), (2, 0), (1, 5), (1, 5)], [], read=ABSENT))
    assert [int(x) for x in three['ps']] == [0, 5, 0xFFFFFFFE] and status(three) == ['new'] * 3


# ---- value ranges --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_names', [1, 2, 257, 65537])
def test_name_and_ps_ranges(ctx, n_names):
    top = n_names - 1
    marks = [(0, ABSENT), (top, 0 if top else ABSENT), (top // 2, ABSENT if top // 2 in (0, top) else 1)]
    p = K.problem([[dict(pred=1, ps=0, marks=marks), dict(pred=2, ps=0xFFFFFFFE, marks=marks[::-1])]],
                  [tag(1, 0, 0), tag(2, 0, 0xFFFFFFFE)], n_names=n_names)
    got = check(ctx, p)
    assert set(int(x) for x in got['name']) == {0, top // 2, top} and set(int(x) for x in got['ps']) == {0, 0xFFFFFFFE}
    refused(ctx, K.problem([[dict(marks=[(n_names, ABSENT)])]], n_names=n_names), 'mark_name not below n_names')


# ---- what the status reads -----------------------------------------------------------------------------------------------------------

def test_status_inputs(ctx):
    assert status(check(ctx, one_read([(1, 7), (1, 7), (2, 7)], [tag(1, 10, 7)]))) == ['agree']
    assert status(check(ctx, one_read([(2, 7)], [tag(1, 10, 7)]))) == ['disagree']
    assert status(check(ctx, one_read([(1, 7), (2, 7)], [tag(1, 10, 7)]))) == ['tie']
    assert status(check(ctx, one_read([(1, 7)], [tag(3, 10, 7)]))) == ['new']                         # hap 3
    assert status(check(ctx, one_read([(1, 7)], [R.UNTAGGED]))) == ['new']                            # the all-ones word
    assert status(check(ctx, one_read([(1, 7)], [tag(1, 10, 7)], read=1))) == ['new']                 # an index at n_reads
    assert status(check(ctx, one_read([(1, 7)], [tag(1, 10, 9)]))) == ['other_ps']
    assert status(check(ctx, one_read([(1, 7), (2, 7)], [tag(2, 10, 9)]))) == ['other_ps']
    for cap in (None, 0, 2400, CAP_MAX):
        at = R.PC_MAX if cap is None else cap
        p = K.problem([[dict(pred=1, marks=[(0, 0), (1, 1)])]], [tag(1, at, 7), tag(1, at + 1, 7)])
        assert status(check(ctx, p, cap=cap)) == ['agree', 'new']                                     # pc at the cap and one above
    assert refused(ctx, one_read([(1, 7)], [tag(1, 0, 7)]), 'pc_cap', cap=CAP_MAX + 1) == 0


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_contradictions_are_refused_and_nothing_is_written(ctx):
    lone = lambda name, read, **kw: dict(marks=[(name, read)], **kw)
    tags = [tag(1, 0, 7)] * 2
    for p in (K.problem([[lone(0, ABSENT)], [lone(0, ABSENT)]]),                                        # inside one record
              K.problem([[lone(0, ABSENT)], [lone(0, ABSENT, ps=9)]]),                                  # across two records of the name
              K.problem([[lone(1, ABSENT), lone(0, ABSENT)], [], [lone(2, ABSENT), lone(0, ABSENT, ps=9)]], form='contig')):
        with pytest.raises(R.Refused, match='two contigs'):
            R.read_tags(p)
        assert refused(ctx, p, 'two contigs') == 0
    for p in (K.problem([[lone(0, 0), lone(0, 1)]], tags), K.problem([[lone(0, 0), lone(0, 1, ps=9)]], tags),
              K.problem([[lone(0, 0), lone(0, ABSENT, ps=9), lone(0, 0, ps=11)]], tags)):
        with pytest.raises(R.Refused, match='two read indices'):
            R.read_tags(p)
        assert refused(ctx, p, 'two read indices') == 0
    # only contributing marks are looked at
    assert len(check(ctx, K.problem([[lone(0, 0, pred=3)], [lone(0, 1, pred=0), lone(0, 1)]], tags))) == 1


def test_argument_refusals(ctx):
    assert refused(ctx, K.problem([[dict(marks=[(0, ABSENT)]), dict(pred=4, marks=[(1, ABSENT)])]]), 'pred above 3') == 0
    p = K.problem([[dict(marks=[(0, ABSENT)])]])
    both, neither = R.Problem(**dict(p.__dict__, cand_contig=[0])), R.Problem(**dict(p.__dict__, cand_ctg_off=None))
    assert refused(ctx, both, 'exactly one of') == 0 and refused(ctx, neither, 'exactly one of') == 0
    short = R.Problem(**dict(p.__dict__, cand_ctg_off=[0, 0]))
    assert refused(ctx, short, 'cand_ctg_off') == 0
    far = R.Problem(**dict(p.__dict__, mark_order=[1]))
    assert refused(ctx, far, 'mark_order') == 0


def test_out_cap_exact_and_one_short(ctx):
    p = K.random_problem(**K.RANDOM[0])
    want = R.records(R.read_tags(p), DT)
    assert len(want) > 10
    assert refused(ctx, p, 'too small', out_cap=len(want) - 1) == len(want)
    assert ctx.read_tags_host(out_cap=len(want), **p.arrays()).tobytes() == want.tobytes()
    assert refused(ctx, p, 'too small', out_cap=0) == len(want)


# ---- the rows writer -----------------------------------------------------------------------------------------------------------------

def test_rows_name_and_chrom_lengths(ctx):
    texts = ['', 'a', 'b' * 63, 'c' * 64, 'd' * 65, 'e' * 300, 'f/1;x,y']
    chroms = ['1', 'K' * 40]
    tags = [tag(1, 10, 7), tag(2, 0xFFFFFF, 0xFFFFFFFE), tag(3, 1, 1)]
    p = K.problem([[dict(pred=1 + (i & 1), ps=7, pos=4000000000 + i, marks=[(i, i if i < 3 else ABSENT), (6, ABSENT)]) for i in range(6)],
                   [dict(pred=2, ps=0xFFFFFFFE, marks=[(7, 1)])]], tags)
    got = check(ctx, p, texts=texts + ['g'], chroms=chroms)
    assert len(got) == 8 and status(got)[6] == 'tie'
    # the text buffer exact and one byte short
    off, pool = K.pool_of(texts + ['g'])
    text = ctx.read_tags_rows_host(got, off, pool, chroms, tags)
    assert ctx.read_tags_rows_host(got, off, pool, chroms, tags, cap=len(text)) == text
    with pytest.raises(_lib.DuetLibraryError, match='too small') as e:
        ctx.read_tags_rows_host(got, off, pool, chroms, tags, cap=len(text) - 1)
    assert e.value.out_len == len(text) and not e.value.out.any()
    assert len(text) <= _lib.read_tags_bound(len(got), off, chroms)


def test_rows_refusals(ctx):
    off, pool = K.pool_of(['a', 'b'])
    rec = lambda **kw: R.records([dict(dict(name=0, contig=0, ps=1, read=ABSENT, n_h1=1, n_h2=0, pos_min=1, pos_max=1, status=3,
                                           reserved=0), **kw)], DT)
    assert ctx.read_tags_rows_host(rec(), off, pool, ['c'], []) == b'c\ta\t1\t1\t1\t0\t1\t.\t.\t.\tnew\t1\t1\n'
    for bad, match in ((rec(name=2), 'name'), (rec(contig=1), 'contig'), (rec(status=5), 'status')):
        with pytest.raises(_lib.DuetLibraryError, match=match) as e:
            ctx.read_tags_rows_host(bad, off, pool, ['c'], [])
        assert e.value.out_len == 0 and not e.value.out.any()
    assert ctx.read_tags_rows_host(rec()[:0], off, pool, ['c'], []) == b''


# ---- workspace and side effects ------------------------------------------------------------------------------------------------------

def test_device_form_agrees_and_two_runs_are_identical(ctx):
    import torch
    p = K.random_problem(**K.RANDOM[1])
    want = ctx.read_tags_host(**p.arrays())
    assert want.tobytes() == ctx.read_tags_host(**p.arrays()).tobytes() and len(want) > 10
    dev = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt).view(np.uint8)).to('cuda:0')
    held = dict(cand_off=dev(p.cand_off, np.uint32), mark_read=dev(p.mark_read, np.uint32), mark_name=dev(p.mark_name, np.uint32),
                pred=dev(p.pred, np.uint8), ps=dev(p.ps, np.uint32), cand_pos=dev(p.cand_pos, np.uint32),
                read_tag=dev(p.read_tag, np.uint64))
    ctg_off = np.ascontiguousarray(p.cand_ctg_off, dtype=np.uint32)
    prob = _lib.ReadTagsProblem()
    prob.n_cands, prob.n_marks, prob.n_reads, prob.n_names = len(p.pred), len(p.mark_read), len(p.read_tag), p.n_names
    prob.n_contigs, prob.cand_ctg_off = len(ctg_off) - 1, ctg_off.ctypes.data
    for k, t in held.items():
        setattr(prob, k, t.data_ptr())
    room = prob.n_marks
    runs = []
    for _ in range(2):
        out = torch.full((room * DT.itemsize + 64,), 0xAB, dtype=torch.uint8, device='cuda:0')
        n = ctx.read_tags_device(prob, out.data_ptr(), room)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.all(got[n * DT.itemsize:] == 0xAB)
        runs.append(got[:n * DT.itemsize].tobytes())
    assert runs[0] == runs[1] == want.tobytes()
    out = torch.full((room * DT.itemsize + 64,), 0xAB, dtype=torch.uint8, device='cuda:0')
    n = ctypes.c_uint32(0)
    rc = ctx.lib.duet_read_tags_device(ctx.handle, ctypes.byref(prob), 8100, ctypes.c_void_p(out.data_ptr()), len(want) - 1, ctypes.byref(n),
                                       None)
    torch.cuda.synchronize()
    assert rc == _lib.DUET_ERR_INVALID and n.value == len(want) and bool((out == 0xAB).all())
    # the rows of the resident records
    texts, off, pool = K.default_names(p.n_names)
    chroms = ['chr%d' % (k + 1) for k in range(prob.n_contigs)]
    keep = [dev(off, np.uint64), dev(np.frombuffer(pool, dtype=np.uint8), np.uint8)]
    names = _lib.callset_names(0, keep[0].data_ptr(), keep[1].data_ptr(), chroms, keep)
    names.n_names = p.n_names
    recs = dev(want.view(np.uint8), np.uint8)
    expect = R.rows_text(R.read_tags(p), texts, chroms, p.read_tag).encode()
    text = torch.full((len(expect) + 64,), 0xAB, dtype=torch.uint8, device='cuda:0')
    size = ctx.read_tags_rows_device(recs.data_ptr(), len(want), names, held['read_tag'].data_ptr(), prob.n_reads, text.data_ptr(),
                                     len(expect))
    torch.cuda.synchronize()
    got = text.cpu().numpy()
    assert size == len(expect) and got[:size].tobytes() == expect and np.all(got[size:] == 0xAB)


def test_nothing_of_ef_changes_after_a_large_a_small_and_a_large_call(ctx):
    soa = soa_fuzz.random_soa(3, n_contigs=4)
    before = (ctx.run_host(soa, 0, 0), ctx.features_host(soa, 0, 0), ctx.ps_links_host(soa, 0, 0))
    large = K.random_problem(**K.RANDOM[2])
    first = check(ctx, large)
    check(ctx, K.problem([[dict(pred=2, marks=[(0, ABSENT)])]]))
    assert check(ctx, large).tobytes() == first.tobytes()
    after = (ctx.run_host(soa, 0, 0), ctx.features_host(soa, 0, 0), ctx.ps_links_host(soa, 0, 0))
    assert np.array_equal(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1])
    assert before[1].tobytes() == after[1].tobytes() and before[2].tobytes() == after[2].tobytes()
    assert int((before[0][0] != 0).sum()) > 10


# ---- random problems -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('i,cap', [(0, None), (1, 2400), (2, None), (3, 0), (4, 12000)])
def test_random_problems(ctx, i, cap):
    p = K.random_problem(**K.RANDOM[i])
    got = check(ctx, p, cap=cap)
    assert len(got) >= 1
    for q in K.same_in_other_forms(p, seed=20 + i):
        assert check(ctx, q, cap=cap).tobytes() == got.tobytes()


# ---- the product --------------------------------------------------------------------------------------------------------------------

def read(path):
    with open(path, 'rb') as f:
        return f.read()


def host_arrays(home, numbered=None):
    """The Python host path's arrays of <home>: the E/F problem, the marks' names interned per contig in order of first mark, and the
    CHROM text the rows carry per contig.  numbered = (texts, {(contig, text): index}): the names are numbered by that table."""
    from duet_amd import sv_phasing_fn as F
    tab, soa = F.generate_callinfo(home + '/sv_calling/variants.vcf', F.read_hap_bam(home + '/snp_phasing/', 4, False), False)
    texts, mark_name, chroms = ([], [], []) if numbered is None else (numbered[0], [], [])
    for k in range(soa.n_contigs):
        a, b = int(soa.cand_ctg_off[k]), int(soa.cand_ctg_off[k + 1])
        seen = {}
        for c in range(a, b):
            for name in tab.names[c]:
                if numbered is not None:
                    seen[name] = numbered[1][(k, name)]
                elif name not in seen:
                    seen[name] = len(texts)
                    texts.append(name)
                mark_name.append(seen[name])
        chroms.append(tab.chrom[a] if b > a else '?')
    return soa, mark_name, texts, chroms


def expected_table(soa, mark_name, texts, chroms, pred, ps, cap=R.PC_MAX):
    p = R.Problem(soa.cand_off, soa.mark_read, mark_name, max(len(texts), 1), pred, ps, soa.cand_pos, [int(t) for t in soa.read_tag],
                  cand_ctg_off=soa.cand_ctg_off)
    recs = R.read_tags(p, cap)
    assert len(recs) >= 1
    return (R.header() + R.rows_text(recs, texts, chroms, p.read_tag)).encode(), recs


def stub_stages(monkeypatch):
    from duet_amd import cli, stages
    for name in ('snp_calling', 'sv_calling', 'snp_phasing'):
        monkeypatch.setattr(stages, name, lambda *a: None)
    monkeypatch.setattr(cli, 'check_envs', lambda *a: None)
    monkeypatch.setattr(cli, 'set_logging', lambda *a: None)


def test_product_native_ingest(ctx, tmp_path_factory, monkeypatch, caplog):
    import logging
    import os
    import shutil
    import sys
    from duet_amd import cli, read_tags, tune
    from duet_amd.sv_phasing import sv_phasing
    from tests import helpers as H
    from tests.test_c_oracle import materialise_bams
    home = str(tmp_path_factory.mktemp('read_tags_golden') / 'w')
    shutil.copytree(os.path.join(H.GOLDEN, 'cases', 'fuzz_cutesv_s2'), home)
    materialise_bams(home)
    pinned = read(os.path.join(H.GOLDEN, 'cases', 'fuzz_cutesv_s2', 'phased_sv.vcf'))
    path = read_tags.path(home)
    sv_phasing(home, 50, 2, 4, False)
    assert read(home + '/phased_sv.vcf') == pinned and not os.path.exists(path)                        # no file without the flag
    soa, mark_name, texts, chroms = host_arrays(home)
    pred, ps = ctx.run_host(soa, 50, 2)
    want, recs = expected_table(soa, mark_name, texts, chroms, pred, ps)
    assert R.summary(recs)['new'] >= 1
    with caplog.at_level(logging.INFO):
        sv_phasing(home, 50, 2, 4, False, read_tags=True)
    assert read(home + '/phased_sv.vcf') == pinned and read(path) == want
    counts = R.summary(recs)
    assert '%d read tag records: %s' % (len(recs), ', '.join('%s %d' % (s, counts[s]) for s in R.STATUS)) in caplog.text
    # a vector of the caller's own changes the calls and with them the table; under a cap the status uses the cap
    v = tune.vector({'c1_max_ref_num': 3, 'c0_min_sv_num': 2})
    sv_phasing(home, 50, 2, 4, False, thresholds=v)
    other = read(home + '/phased_sv.vcf')
    os.remove(path)
    sv_phasing(home, 50, 2, 4, False, thresholds=v, read_tags=True)
    pred_v, ps_v = tune.apply(dict(feat=ctx.features_host(soa, 50, 2)), v, ctx=ctx)
    assert read(home + '/phased_sv.vcf') == other and read(path) == expected_table(soa, mark_name, texts, chroms, pred_v, ps_v)[0]
    sv_phasing(home, 50, 2, 4, False, pc_cap=2400)
    capped = read(home + '/phased_sv.vcf')
    sv_phasing(home, 50, 2, 4, False, pc_cap=2400, read_tags=True)
    pred_c, ps_c = tune.apply(dict(feat=ctx.features_host(soa, 50, 2, pc_cap=2400)), tune.vector(), ctx=ctx)
    assert read(home + '/phased_sv.vcf') == capped
    assert read(path) == expected_table(soa, mark_name, texts, chroms, pred_c, ps_c, 2400)[0] and read(path) != want
    # the command
    stub_stages(monkeypatch)
    os.remove(path)
    monkeypatch.setattr(sys, 'argv', ['duet', 'in.bam', 'ref.fa', home])
    cli.main(None)
    assert read(home + '/phased_sv.vcf') == pinned and not os.path.exists(path)
    monkeypatch.setattr(sys, 'argv', ['duet', 'in.bam', 'ref.fa', home, '--write_read_tags'])
    cli.main(None)
    assert read(home + '/phased_sv.vcf') == pinned and read(path) == want


def test_product_svim_gpu(ctx, tmp_path_factory, monkeypatch):
    import os
    import shutil
    import sys
    from duet_amd import cli, read_tags, svim_mode, synth, tune
    from duet_amd.read_file import init_chrom_list
    from tests import helpers as H
    root = tmp_path_factory.mktemp('read_tags_svim')
    home, copy = str(root / 'w'), str(root / 'copy')
    synth.write_svim_workdir(home, H.case_contigs('genome_small', 5), 5)
    shutil.copytree(home, copy)
    svim_mode.sv_phasing_from_bams(copy, 50, 2, 4, False, 0.9, 0, write_sv_calls=True)
    # the clustered calls, read back with their READS= lists; the names numbered as the extraction numbers them
    from duet_amd.native import NativeIngest
    ing, got = NativeIngest.extract(home + '/snp_phasing/', init_chrom_list(False, home), 4, 50, names=True)
    ing.close()
    pool = [t.decode() for t in read_tags.names_of(got['name_off'], got['name_pool'])]
    numbered = (pool, {(int(k), pool[int(j)]): int(j) for k, j in zip(got['contig'], got['mark_name'])})
    soa, mark_name, texts, _ = host_arrays(copy, numbered)
    chroms = svim_mode.spelled_contigs(home, init_chrom_list(False, home))
    path = read_tags.path(home)
    stub_stages(monkeypatch)
    base = ['duet', 'in.bam', 'ref.fa', home, '-b', 'svim-gpu']
    monkeypatch.setattr(sys, 'argv', base)
    cli.main(None)
    plain = read(home + '/phased_sv.vcf')
    assert plain.count(b'\n') > 100 and not os.path.exists(path)
    monkeypatch.setattr(sys, 'argv', base + ['--write_read_tags'])
    cli.main(None)
    pred, ps = ctx.run_host(soa, 50, 2)
    want, recs = expected_table(soa, mark_name, texts, chroms, pred, ps)
    assert read(home + '/phased_sv.vcf') == plain and read(path) == want
    monkeypatch.setattr(sys, 'argv', base + ['--pc_cap', '2400'])
    cli.main(None)
    capped = read(home + '/phased_sv.vcf')
    with open(str(root / 'v.json'), 'w') as f:
        f.write('{}')
    monkeypatch.setattr(sys, 'argv', base + ['--pc_cap', '2400', '--write_read_tags', '--thresholds', str(root / 'v.json')])
    cli.main(None)
    pred_c, ps_c = tune.apply(dict(feat=ctx.features_host(soa, 50, 2, pc_cap=2400)), tune.vector(), ctx=ctx)
    assert read(home + '/phased_sv.vcf') == capped
    assert read(path) == expected_table(soa, mark_name, texts, chroms, pred_c, ps_c, 2400)[0]


def test_product_refusals_leave_no_file(tmp_path, monkeypatch):
    import os
    import shutil
    import sys
    from duet_amd import cli, svim_mode
    from duet_amd.sv_phasing import sv_phasing
    from tests import helpers as H
    from tests.test_c_oracle import materialise_bams
    out = tmp_path / 'out'
    stub_stages(monkeypatch)
    monkeypatch.setattr(sys, 'argv', ['duet', 'in.bam', 'ref.fa', str(out), '--write_read_tags', '--gpus', '2'])
    with pytest.raises(SystemExit, match='--write_read_tags works on the single-GPU path only'):
        cli.main(None)
    assert not out.exists()
    monkeypatch.setenv('DUET_FORCE_RANKS', '1')
    monkeypatch.setattr(sys, 'argv', ['duet', 'in.bam', 'ref.fa', str(out), '--write_read_tags'])
    with pytest.raises(SystemExit, match='--write_read_tags works on the single-GPU path only'):
        cli.main(None)
    for fn, args in ((sv_phasing, (str(out), 50, 2, 4, False)), (svim_mode.sv_phasing_from_bams, (str(out), 50, 2, 4, False))):
        with pytest.raises(ValueError, match='read_tags: single-GPU path only'):
            fn(*args, read_tags=True)
        monkeypatch.delenv('DUET_FORCE_RANKS', raising=False)
        with pytest.raises(ValueError, match='read_tags: single-GPU path only'):
            fn(*args, gpus=2, read_tags=True)
        monkeypatch.setenv('DUET_FORCE_RANKS', '1')
    monkeypatch.delenv('DUET_FORCE_RANKS')
    assert not out.exists()
    # an input the native ingest declines: refused before phased_sv.vcf is created
    home = str(tmp_path / 'w')
    shutil.copytree(os.path.join(H.GOLDEN, 'cases', 'fuzz_cutesv_s2'), home)
    materialise_bams(home)
    os.remove(home + '/phased_sv.vcf')
    monkeypatch.setenv('DUET_NATIVE_INGEST', '0')
    before = sorted(os.listdir(home))
    with pytest.raises(RuntimeError, match='--write_read_tags needs the native ingest'):
        sv_phasing(home, 50, 2, 4, False, read_tags=True)
    with pytest.raises(RuntimeError, match='--write_read_tags need the native ingest'):
        sv_phasing(home, 50, 2, 4, False, pc_cap=2400, read_tags=True)
    assert sorted(os.listdir(home)) == before
