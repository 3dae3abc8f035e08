# coding=utf-8
"""No GPU: the rule of the read tags (tests/read_tags_ref.py) on hand-stated cases, duet_amd/read_tags.py's text against the
reference's, what the random problems of the GPU tests must yield, and the compile remarks of duet_readtags.hip."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from duet_amd import _lib, read_tags
from tests import read_tags_cases as K
from tests import read_tags_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABSENT = R.ABSENT
tag = K.tag


def one_read(calls, tags, read=0, cap=R.PC_MAX):
    """The records of one read (name 0) listed once in each candidate (pred, ps) of `calls`."""
    p = K.problem([[dict(pred=pr, ps=ps, pos=100 * (i + 1), marks=[(0, read)]) for i, (pr, ps) in enumerate(calls)]], tags)
    return R.read_tags(p, cap)


def status(rec):
    return R.STATUS[rec['status']]


# ---- the rule --------------------------------------------------------------------------------------------------------------------

def test_one_case_per_status():
    agree = one_read([(1, 7), (1, 7), (2, 7)], [tag(1, 10, 7)])
    assert [(r['name'], r['contig'], r['ps'], r['read'], r['n_h1'], r['n_h2'], r['pos_min'], r['pos_max'], status(r), r['reserved'])
            for r in agree] == [(0, 0, 7, 0, 2, 1, 100, 300, 'agree', 0)]
    assert [status(r) for r in one_read([(2, 7)], [tag(1, 10, 7)])] == ['disagree']
    assert [status(r) for r in one_read([(1, 7), (2, 7)], [tag(1, 10, 7)])] == ['tie']
    assert [status(r) for r in one_read([(1, 7), (2, 7)], [], read=ABSENT)] == ['tie']               # for any tag
    assert [status(r) for r in one_read([(2, 7)], [], read=ABSENT)] == ['new']
    assert [status(r) for r in one_read([(1, 7)], [tag(1, 10, 9)])] == ['other_ps']
    assert [status(r) for r in one_read([(1, 7), (2, 7)], [tag(1, 10, 9)])] == ['other_ps']           # ... before the tie


def test_what_makes_a_tag_usable():
    assert [status(r) for r in one_read([(1, 7)], [R.UNTAGGED])] == ['new']
    assert [status(r) for r in one_read([(1, 7)], [tag(3, 10, 7)])] == ['new']                        # hap 3
    assert [status(r) for r in one_read([(1, 7)], [tag(3, 10, 9)])] == ['new']                        # ... whatever its PS
    assert [status(r) for r in one_read([(1, 7)], [tag(1, 10, 7)], read=1)] == ['new']                # an index at n_reads
    assert [status(r) for r in one_read([(1, 7)], [tag(1, 8100, 7)])] == ['agree']                    # pc at the cap
    assert [status(r) for r in one_read([(1, 7)], [tag(1, 8101, 7)])] == ['new']                      # ... and one above
    assert [status(r) for r in one_read([(1, 7)], [tag(1, 0, 7)], cap=0)] == ['agree']
    assert [status(r) for r in one_read([(1, 7)], [tag(1, 1, 7)], cap=0)] == ['new']
    top = (1 << 30) - 3
    assert [status(r) for r in one_read([(2, 7)], [tag(2, top, 7)], cap=top)] == ['agree']
    with pytest.raises(R.Refused):
        one_read([(1, 7)], [tag(1, 0, 7)], cap=top + 1)


def test_who_contributes_and_how_records_are_keyed():
    p = K.problem([[dict(pred=0, ps=7, marks=[(0, ABSENT)]), dict(pred=3, ps=7, marks=[(0, ABSENT)])]])
    assert R.read_tags(p) == []                                         # a dropped candidate and a 1|1 call say nothing
    twice = K.problem([[dict(pred=2, ps=7, marks=[(0, ABSENT), (1, ABSENT), (0, ABSENT)])]])
    assert [(r['name'], r['n_h1'], r['n_h2']) for r in R.read_tags(twice)] == [(0, 0, 2), (1, 0, 1)]   # a read twice counts twice
    three = one_read([(1, 0xFFFFFFFE), (2, 0), (1, 5), (1, 5)], [], read=ABSENT)
    assert [(r['ps'], r['n_h1'], r['n_h2'], r['pos_min'], r['pos_max']) for r in three] == \
        [(0, 0, 1, 200, 200), (5, 2, 0, 300, 400), (0xFFFFFFFE, 1, 0, 100, 100)]                      # PS as an unsigned number
    contigs = K.problem([[], [dict(marks=[(0, ABSENT)])], [], [dict(marks=[(1, ABSENT)]), dict(marks=[(2, ABSENT)])], []])
    assert [(r['name'], r['contig']) for r in R.read_tags(contigs)] == [(0, 1), (1, 3), (2, 3)]
    for q in K.same_in_other_forms(contigs):
        assert R.read_tags(q) == R.read_tags(contigs)


def test_the_refusals():
    two_contigs = K.problem([[dict(marks=[(0, ABSENT)])], [dict(marks=[(0, ABSENT)])]])
    with pytest.raises(R.Refused, match='two contigs'):
        R.read_tags(two_contigs)
    two_reads = K.problem([[dict(ps=7, marks=[(0, 0)]), dict(ps=9, marks=[(0, 1)])]], [tag(1, 0, 7)] * 2)
    with pytest.raises(R.Refused, match='two read indices'):
        R.read_tags(two_reads)
    quiet = K.problem([[dict(pred=3, marks=[(0, ABSENT)])], [dict(pred=0, marks=[(0, 0)])]], [tag(1, 0, 7)])
    assert R.read_tags(quiet) == []                                     # (only contributing marks are looked at)
    with pytest.raises(R.Refused):
        R.read_tags(K.problem([[dict(pred=4, marks=[(0, ABSENT)])]]))
    with pytest.raises(R.Refused):
        R.read_tags(K.problem([[dict(marks=[(1, ABSENT)])]], n_names=1))
    p = K.problem([[dict(marks=[(0, ABSENT)])]])
    p.cand_contig = [0]
    with pytest.raises(R.Refused):
        R.read_tags(p)                                                  # both contig forms
    p.cand_contig = p.cand_ctg_off = None
    with pytest.raises(R.Refused):
        R.read_tags(p)                                                  # neither


# ---- the host side's text -----------------------------------------------------------------------------------------------------------

def test_text_equals_the_references():
    tags = [tag(1, 10, 7), tag(2, 9000, 7), tag(3, 5, 7), R.UNTAGGED, tag(2, 0, 9)]
    p = K.problem([[dict(pred=1, ps=7, pos=5, marks=[(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, ABSENT), (6, 9)]),
                    dict(pred=2, ps=7, pos=4000000000, marks=[(0, 0), (5, ABSENT)])],
                   [dict(pred=2, ps=0xFFFFFFFE, pos=9, marks=[(7, ABSENT)])]], tags)
    recs = R.read_tags(p)
    arr = R.records(recs, _lib.READ_TAG_DTYPE)
    assert arr.dtype.itemsize == 40
    names, chroms = ['read/%d' % i for i in range(8)], ['chr1', 'chrUn_long_name']
    want = R.rows_text(recs, names, chroms, tags)
    assert read_tags.rows_text(arr, names, chroms, np.array(tags, dtype=np.uint64)) == want
    assert read_tags.rows_text(arr, [n.encode() for n in names], [c.encode() for c in chroms], tags) == want
    assert want.splitlines()[0] == 'chr1\tread/0\t7\t2\t1\t1\t.\t1\t7\t10\ttie\t5\t4000000000'
    assert want.splitlines()[1] == 'chr1\tread/1\t7\t1\t1\t0\t1\t2\t7\t9000\tnew\t5\t5'                 # its own tag, whatever the cap
    assert want.splitlines()[2] == 'chr1\tread/2\t7\t1\t1\t0\t1\t.\t7\t5\tnew\t5\t5'                     # hap 3
    assert want.splitlines()[3] == 'chr1\tread/3\t7\t1\t1\t0\t1\t.\t.\t.\tnew\t5\t5'
    assert want.splitlines()[4] == 'chr1\tread/4\t7\t1\t1\t0\t1\t2\t9\t0\tother_ps\t5\t5'
    assert want.splitlines()[7] == 'chrUn_long_name\tread/7\t4294967294\t1\t0\t1\t2\t.\t.\t.\tnew\t9\t9'
    assert read_tags.header() == R.header() and read_tags.header().count('\t') == want.splitlines()[0].count('\t')
    assert read_tags.summary(arr) == R.summary(recs) == dict(agree=0, disagree=0, tie=2, new=5, other_ps=1)
    assert read_tags.summary_text(arr) == '8 read tag records: agree 0, disagree 0, tie 2, new 5, other_ps 1'
    assert read_tags.summary(read_tags.empty()) == dict.fromkeys(R.STATUS, 0)
    off, pool = K.pool_of(names)
    assert read_tags.names_of(off, pool) == [n.encode() for n in names]


def test_write(tmp_path):
    read_tags.write(str(tmp_path), b'a\tb\n')
    assert (tmp_path / 'phased_sv.read_tags.tsv').read_bytes() == R.header().encode() + b'a\tb\n'


def test_bound_and_layout():
    assert ctypes.sizeof(_lib.ReadTagsProblem) == 6 * 4 + 10 * 8
    assert _lib.READ_TAG_DTYPE.names == R.FIELDS and _lib.READ_TAG_STATUS_NAMES == R.STATUS and _lib.READ_TAG_COLUMNS == R.COLUMNS
    # the longest row: every number at its widest, the two eight-letter statuses
    top = 0xFFFFFFFF
    rec = dict(name=0, contig=0, ps=top, read=0, n_h1=top, n_h2=top - 1, pos_min=top, pos_max=top, status=R.STATUS.index('disagree'),
               reserved=0)
    row = R.rows_text([rec], ['n' * 30], ['c' * 40], [tag(2, (1 << 30) - 1, top)])
    off, _ = K.pool_of(['n' * 30, 'x'])
    assert len(row) == 40 + 30 + 103 and _lib.read_tags_bound(1, off, ['c' * 40, 'c']) == 40 + 30 + 104
    assert _lib.read_tags_bound(0, off[:1], []) == 0


# ---- what the GPU tests rely on ------------------------------------------------------------------------------------------------------

def test_random_problems_yield_what_the_gpu_tests_need():
    seen = dict.fromkeys(R.STATUS, 0)
    for kw in K.RANDOM:
        recs = R.read_tags(K.random_problem(**kw))
        assert len(recs) >= 1, kw
        for s, n in R.summary(recs).items():
            seen[s] += n
    assert all(seen[s] > 0 for s in ('agree', 'disagree', 'tie', 'new')), seen


# ---- the unit's compile remarks --------------------------------------------------------------------------------------------------------

HIPCC = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)


@pytest.mark.skipif(HIPCC is None, reason='hipcc not found')
def test_readtags_kernels_use_no_scratch_and_make_no_call(tmp_path):
    csrc = os.path.join(REPO, 'duet_amd', 'csrc')
    asm = str(tmp_path / 'duet_readtags.s')
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fvisibility=hidden',
           '-Wno-unused-function', '-I' + os.path.join(REPO, 'include'), '--cuda-device-only', '-S',
           '-Rpass-analysis=kernel-resource-usage', os.path.join(csrc, 'duet_readtags.hip'), '-o', asm]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    found = re.findall(r'Function Name: (\S+) \[.*?\n(?:.*\n){0,8}?.*ScratchSize \[bytes/lane\]: (\d+)', r.stderr)
    kernels = {n: int(v) for n, v in found}
    # its own six and everything it instantiates of the shared scans and the sort
    for own in ('rt_count', 'rt_keys', 'rt_reduce', 'rr_len', 'rr_write', 'scan_spine_u64'):
        assert sum(own in n for n in kernels) == 1, (own, sorted(kernels))
    assert len(kernels) >= 12, sorted(kernels)
    assert all(v == 0 for v in kernels.values()), kernels
    with open(asm) as f:
        assert 's_swappc' not in f.read()
