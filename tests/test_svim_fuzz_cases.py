# coding=utf-8
"""The named cases of tests/svim_fuzz.py still bite: for every case the CPU reference (tests/svim_ref.py) is run and the
case's own coverage predicate asserted on its result -- the structural property the case is named for holds exactly, the
phasing cases reach every prediction, and where an adapter rule has a natural wrong variant the reference computed with
that variant gives other (pred, ps) on the case's input.  No GPU: tests/test_gpu_fused_edges.py runs the same cases on
the device against the same reference."""
import numpy as np
import pytest

from duet_amd import engine
from tests import svim_fuzz, svim_ref

_ref = {}
# exempt from "20 candidates of each prediction": all marks absent, no read table, no marks (they assert pred == 0 everywhere), and
# the cases too small to hold 60 candidates that pass the support filter
SILENT = ('all_marks_absent', 'no_reads', 'marks_0')
EXEMPT = ('parts_1', 'marks_1', 'marks_2', 'marks_63', 'marks_64', 'marks_65')


def reference(name, variant=None):
    if (name, variant) not in _ref:
        c = svim_fuzz.case(name)
        _ref[(name, variant)] = svim_ref.fused(c.marks, c.read_tag, c.depth, c.depth_off, c.depth_bin, c.svlen_thres,
                                               c.suppread_thres, variant=variant, **c.kw)
    return _ref[(name, variant)]


def phase_sets_per_candidate(c, r):
    """distinct PS values among each candidate's tagged marks"""
    read = c.marks['read'][r['order']].astype(np.int64)
    cand = np.repeat(np.arange(len(r['support'])), r['support'])
    live = read != engine.MARK_ABSENT
    ps = (c.read_tag[read[live]] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return np.bincount(np.unique(cand[live] << 32 | ps) >> 32, minlength=len(r['support']))


@pytest.mark.parametrize('name', svim_fuzz.NAMES)
def test_case_has_the_property_it_is_named_for(name):
    c, r = svim_fuzz.case(name), reference(name)
    e = c.expect
    assert r['rc'] == 0
    N, M = len(r['pred']), c.M
    support, pred = r['support'], r['pred']
    counts = np.bincount(pred, minlength=4)
    assert len(c.marks['contig']) == M and (M == 0 or int(c.marks['contig'].max()) < c.K)
    assert int(support.sum()) == M and len(r['ctg_off']) == c.K + 1
    kw = dict(dict(part_gap=1000, part_max=100), **{k: v for k, v in c.kw.items() if k in ('part_gap', 'part_max')})
    n_parts, pid = svim_fuzz.partitions(c.marks, **kw)
    # -- predictions
    assert e['silent'] == (name in SILENT) and e['phasing'] == (name not in SILENT + EXEMPT)
    if e['silent']:
        assert counts[1:].sum() == 0
    elif e['phasing']:
        assert min(counts[1:]) >= 20, counts
        used = c.read_tag[c.marks['read'][c.marks['read'] != engine.MARK_ABSENT]]
        assert ((used >> np.uint64(62)) == 3).any(), 'hap code 3'
        pc = (used >> np.uint64(32)) & np.uint64(0x3FFFFFFF)
        assert (pc == 8100).any() and (pc == 8101).any() and (pc < 8100).any() and (pc > 8101).any()
        d = r['depth_at']
        for delta in (-1, 0, 1):
            assert (d == support + delta).any() or 'lot_over' in e, 'depth = support %+d' % delta
        if N >= 600 and c.suppread_thres <= 2 and 'lot_over' not in e:
            nps = phase_sets_per_candidate(c, r)
            assert min((nps == 1).sum(), (nps == 2).sum(), (nps > 2).sum()) >= 20, 'candidates over 1, 2, > 2 phase sets'
    else:
        # the named exemptions: cases that cannot hold 20 candidates of each prediction (svim_fuzz: _parts, _sized)
        assert name in EXEMPT and e['exempt']
        if e.get('some'):
            assert counts[1:].sum() > 0
    # -- structure
    if 'n_parts' in e:
        assert n_parts == e['n_parts']
    if 'n_cands' in e:
        assert N == e['n_cands']
    if 'n_marks' in e:
        assert M == e['n_marks']
    if 'min_marks' in e:
        assert M >= e['min_marks']
    if 'K' in e:
        assert c.K == e['K']
    occupied = np.unique(r['cand_contig']).astype(np.int64)
    if 'occupied' in e:
        assert len(occupied) == e['occupied']
    if 'singles' in e:
        assert (np.bincount(r['cand_contig'])[occupied] == 1).sum() >= 10, 'contigs of exactly one candidate'
    if 'empty_front' in e:
        gaps = np.diff(np.concatenate([[-1], occupied, [c.K]])) - 1
        assert gaps[0] >= e['empty_front'] and gaps[-1] >= e['empty_behind'] and (gaps[1:-1] >= e['empty_run']).any()
    if 'opens' in e:
        opens = r['ctg_off'][occupied[1:]] % 64
        for x in e['opens']:
            assert (opens == x).any(), (x, r['ctg_off'][occupied])
        assert np.bincount(r['cand_contig'])[e['single']] == 1
    if 'supports' in e:
        for x in e['supports']:
            assert (support == x).any(), x
        assert int(support.max()) == e['part_max']
        assert c.suppread_thres in (1, 2, 128) and (support >= c.suppread_thres).any()
        big = support >= min(63, e['part_max'] - 1)
        assert big.sum() >= 20 and min(np.bincount(pred[big], minlength=4)[1:]) >= 1, 'large clusters with every prediction'
        assert (r['ps'][big] != 0).any()
    if 'lot_over' in e:
        first_part = pid[r['order'][r['cand_off'][:-1].astype(np.int64)]]
        assert np.array_equal(first_part, np.sort(first_part))
        assert int(np.bincount(first_part // 64).max()) > e['lot_over']
        assert N > n_parts
    if 'no_bins' in e:
        nb = np.diff(c.depth_off.astype(np.int64))
        for k in e['no_bins']:
            on = r['cand_contig'] == k
            assert nb[k] == 0 and on.sum() >= 10 and (r['refread'][on] == 0).all()
    if 'beyond' in e:
        nb = np.diff(c.depth_off.astype(np.int64))[r['cand_contig']]
        assert int((r['cand_pos'].astype(np.int64) // c.depth_bin >= nb).sum()) >= e['beyond']
    if 'depth_max' in e:
        assert (r['depth_at'] == 0xFFFFFFFF).sum() >= 10
    if name.startswith('depth_bin_'):
        assert c.depth_bin == {'depth_bin_1': 1, 'depth_bin_max': 0xFFFFFFFF}[name]
    if 'span_at' in e:
        s = e['span_at']
        assert (r['cand_span'] == s).sum() >= 10 and (r['cand_span'] == s - 1).sum() >= 10
        assert c.svlen_thres in (s - 1, s, s + 1)
    if 'dup' in e:
        read = c.marks['read'][r['order']].astype(np.int64)
        cand = np.repeat(np.arange(N), support)
        live = read != engine.MARK_ABSENT
        assert len(np.unique(cand[live] << 32 | read[live])) < int(live.sum()) - 100
    if 'not_the_defaults' in e:
        for drop in ('part_gap', 'normalizer'):
            other = svim_ref.fused(c.marks, c.read_tag, c.depth, c.depth_off, c.depth_bin, c.svlen_thres, c.suppread_thres,
                                   **{k: v for k, v in c.kw.items() if k != drop})
            assert not np.array_equal(other['cand_off'], r['cand_off']), drop
    if name == 'no_reads':
        assert len(c.read_tag) == 0
    if name == 'all_marks_absent':
        assert len(c.read_tag) > 0 and (c.marks['read'] == engine.MARK_ABSENT).all()
    if name == 'suppread_thres_1':
        assert c.suppread_thres == 1 and ((support == 1) & (pred != 0)).any()


def differs(name, variant):
    a, b = reference(name), reference(name, variant)
    return not (np.array_equal(a['pred'], b['pred']) and np.array_equal(a['ps'], b['ps']))


# (case, wrong variant): the input tells the contract from the mistake in the (pred, ps) the device tests compare
WRONG = [('beyond_the_last_bin', 'no_clamp'),
         ('contigs_2', 'refread_wrap'), ('depth_bin_max', 'refread_wrap'),
         # (told apart where contig 0 has candidates: in front of empty contigs `<=` only renumbers the contigs)
         ('contigs_2', 'ctg_off_le'), ('contig_opens_at_0_and_63', 'ctg_off_le'), ('contigs_65', 'ctg_off_le'),
         ('svlen_thres_on_a_mean_+0', 'round_mean'), ('svlen_thres_on_a_mean_+1', 'round_mean'),
         ('repeated_reads', 'dedup_support'), ('contigs_1', 'dedup_support')]


@pytest.mark.parametrize('name,variant', WRONG)
def test_input_tells_the_wrong_variant_from_the_contract(name, variant):
    assert differs(name, variant)


def test_strict_comparison_in_refread_is_the_same_function():
    """`depth > support ? depth - support : 0` and the same with `>=` agree everywhere (both give 0 at depth == support), so no
    input can tell them apart; the mistake that the depth = support - 1 / support / support + 1 inputs do catch at this place is
    the missing floor (refread_wrap above)."""
    d, s = np.meshgrid(np.arange(0, 70), np.arange(1, 70))
    assert np.array_equal(np.where(d > s, d - s, 0), np.where(d >= s, d - s, 0))
    assert np.array_equal(np.where(d > s, d - s, 0), np.maximum(d - s, 0))


def test_every_named_case_is_listed_once():
    assert len(set(svim_fuzz.NAMES)) == len(svim_fuzz.NAMES) >= 40
    assert all(svim_fuzz.case(n).name == n for n in svim_fuzz.NAMES if n.startswith('marks_'))
