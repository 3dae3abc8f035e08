# coding=utf-8
"""No GPU: the reference of the phase-set links (tests/ps_links_ref.py) against cases worked by hand, the host side of
duet_amd/ps_links.py (verdict, the two tables, the blocks) against it, the record layout, and the refusals of --write_ps_links
that need no device."""
import ctypes
import os
import sys

import numpy as np
import pytest

from duet_amd import _lib, engine, ps_links
from tests import ps_links_ref as R
from tests import soa_fuzz

DT = _lib.PS_LINK_DTYPE


def soa_of(contigs):
    """contigs: lists of candidates; a candidate is (pos, svlen, svread, gt, [(hap, pc, ps) per mark, or None: absent])."""
    tags, marks, off, cols, ctg = [], [], [0], [], [0]
    for cands in contigs:
        for pos, svlen, svread, gt, ms in cands:
            for m in ms:
                if m is None:
                    marks.append(0xFFFFFFFF)
                else:
                    tags.append(engine.pack_tags([m[0]], [m[1]], [m[2]])[0])
                    marks.append(len(tags) - 1)
            off.append(len(marks))
            cols.append((pos, svlen, svread, gt))
        ctg.append(len(cols))
    col = lambda i: [c[i] for c in cols]
    return engine.EfSoA(cand_ctg_off=ctg, read_tag=np.array(tags, dtype=np.uint64), cand_pos=col(0), cand_svlen=col(1), cand_svread=col(2),
                        cand_refread=[0] * len(cols), cand_gt_ok=col(3), cand_off=off, mark_read=np.array(marks, dtype=np.uint32))


def rec(contig, a, b, n_same=0, n_flip=0, n_open=0, w_same=0, w_flip=0, pos_min=0, pos_max=0):
    return dict(w_same=w_same, w_flip=w_flip, contig=contig, ps_a=a, ps_b=b, n_sv=n_same + n_flip + n_open, n_same=n_same, n_flip=n_flip,
                n_open=n_open, pos_min=pos_min, pos_max=pos_max, reserved=0)


def records(*recs):
    return R.records(list(recs), DT)


# ---- the reference against hand-worked cases ----------------------------------------------------------------------------------------

def test_reference_hand_worked():
    # candidate 1: PS 10 has h1 = 3, h2 = 1 (d = +2); PS 20 has h2 = 3 (d = -3); PS 30 has h1 = 1, h2 = 1 (d = 0)
    #   -> (10, 20) flip with w = min(2, 3) = 2; (20, 30) open; NOT (10, 30): only neighbours pair
    # candidate 2: PS 10 d = +1, PS 20 d = +4 -> (10, 20) same, w = 1
    # candidate 3 (other contig): PS 10 d = -2, PS 20 d = -1 -> same, w = 1, on its own record
    c1 = (500, 100, 5, 1, [(1, 0, 10)] * 3 + [(2, 0, 10)] + [(2, 0, 20)] * 3 + [(1, 0, 30), (2, 0, 30)])
    c2 = (200, 100, 5, 1, [(1, 0, 20)] * 4 + [(1, 0, 10)])
    c3 = (900, 100, 5, 1, [(2, 0, 10)] * 2 + [(2, 0, 20)])
    got = R.links(soa_of([[c1, c2], [], [c3]]), 50, 2)
    assert got == [rec(0, 10, 20, n_same=1, n_flip=1, w_same=1, w_flip=2, pos_min=200, pos_max=500),
                   rec(0, 20, 30, n_open=1, pos_min=500, pos_max=500),
                   rec(2, 10, 20, n_same=1, w_same=1, pos_min=900, pos_max=900)]


def test_reference_who_takes_part():
    two = [(1, 0, 10), (2, 0, 20)]
    assert len(R.links(soa_of([[(1, 50, 2, 1, two)]]), 50, 2)) == 1
    assert R.links(soa_of([[(1, 49, 2, 1, two)]]), 50, 2) == []                 # the three filter terms
    assert R.links(soa_of([[(1, 50, 1, 1, two)]]), 50, 2) == []
    assert R.links(soa_of([[(1, 50, 2, 0, two)]]), 50, 2) == []
    assert R.links(soa_of([[(1, 50, 2, 1, [(1, 0, 10), (3, 0, 20)])]]), 50, 2) == []          # hap 3 does not vote
    assert R.links(soa_of([[(1, 50, 2, 1, [(1, 0, 10), None])]]), 50, 2) == []                # an absent mark
    assert len(R.links(soa_of([[(1, 50, 2, 1, [(1, 8100, 10), (1, 8100, 20)])]]), 50, 2)) == 1   # pc == cap votes
    assert R.links(soa_of([[(1, 50, 2, 1, [(1, 8100, 10), (1, 8101, 20)])]]), 50, 2) == []
    assert len(R.links(soa_of([[(1, 50, 2, 1, [(1, 8100, 10), (1, 8101, 20)])]]), 50, 2, 8101)) == 1
    # PS values order as unsigned numbers
    got = R.links(soa_of([[(1, 50, 2, 1, [(1, 0, 2 ** 31), (1, 0, 1), (1, 0, 2 ** 32 - 2)])]]), 50, 2)
    assert [(r['ps_a'], r['ps_b']) for r in got] == [(1, 2 ** 31), (2 ** 31, 2 ** 32 - 2)]
    # an untagged read (all-ones tag word)
    soa = soa_of([[(1, 50, 2, 1, two)]])
    soa.read_tag[1] = R.UNTAGGED
    assert R.links(soa, 50, 2) == []


def test_the_generator_exercises_the_rule():
    """The five random problems of tests/test_gpu_ps_links.py at -s 50 -r 2 and the reference's cap, with the figures the
    generator gave when the rule was written: each yields a link; the first two hold all three kinds."""
    from tests.test_gpu_ps_links import RANDOM, kinds
    per = [R.links(soa_fuzz.random_soa(*a, **k), 50, 2) for a, k in RANDOM]
    assert [len(p) for p in per] == [14, 3, 47, 23, 1]
    assert [sum(r['n_sv'] for r in p) for p in per[:2]] == [144, 114]
    assert kinds(per[0]) == (50, 77, 17) and kinds(per[1]) == (56, 52, 6) and kinds(per[3])[2] == 15
    assert min(kinds([r for p in per for r in p])) > 0


# ---- verdict and text ---------------------------------------------------------------------------------------------------------------

def test_verdict_with_ties():
    v = lambda **kw: ps_links.verdict(records(rec(0, 1, 2, **kw))[0])
    assert v(n_same=2, n_flip=1) == 'same' and v(n_same=1, n_flip=2) == 'flip'
    assert v(n_same=1, n_flip=1, w_same=3, w_flip=2) == 'same'                  # counts tie: the weights decide
    assert v(n_same=1, n_flip=1, w_same=2, w_flip=3) == 'flip'
    assert v(n_same=1, n_flip=1, w_same=2, w_flip=2) == '.'
    assert v(n_open=5) == '.'
    assert v(n_same=1, n_flip=2, w_same=100, w_flip=1) == 'flip'                # the count goes first
    for kw in (dict(n_same=2, n_flip=1), dict(n_same=1, n_flip=1, w_same=2, w_flip=3), dict(n_open=1)):
        assert v(**kw) == R.verdict(rec(0, 1, 2, **kw))


def test_header_and_rows_text():
    assert ps_links.header() == 'CHROM\tPS_A\tPS_B\tN_SV\tN_SAME\tN_FLIP\tN_OPEN\tW_SAME\tW_FLIP\tPOS_MIN\tPOS_MAX\tVERDICT\n' == R.header()
    assert ps_links.blocks_header() == 'CHROM\tPS\tBLOCK\tFLIP\n'
    recs = records(rec(0, 10, 20, n_same=1, n_flip=1, w_same=1, w_flip=2, pos_min=200, pos_max=500),
                   rec(2, 0, 2 ** 32 - 2, n_same=2 ** 32 - 1, w_same=2 ** 64 - 1, pos_max=2 ** 32 - 1), rec(2, 5, 6, n_open=3))
    text = ps_links.rows_text(recs, ['chr1', 'chr2', b'X'])
    assert text == ('chr1\t10\t20\t2\t1\t1\t0\t1\t2\t200\t500\tflip\n'
                    'X\t0\t4294967294\t4294967295\t4294967295\t0\t0\t18446744073709551615\t0\t0\t4294967295\tsame\n'
                    'X\t5\t6\t3\t0\t0\t3\t0\t0\t0\t0\t.\n')
    assert text == R.rows_text(recs, ['chr1', 'chr2', 'X'])
    assert ps_links.rows_text(recs[:0], []) == ''


# ---- blocks -------------------------------------------------------------------------------------------------------------------------

def both(recs):
    got = ps_links.blocks(recs)
    assert got == R.blocks(recs)
    return got


def test_blocks_chain_and_composition():
    rows, conflicts = both(records(rec(0, 10, 20, n_same=3, w_same=3), rec(0, 20, 30, n_flip=2, w_flip=2)))
    assert rows == [(0, 10, 10, 0), (0, 20, 10, 0), (0, 30, 10, 1)] and conflicts == []
    rows, conflicts = both(records(rec(0, 10, 20, n_flip=1, w_flip=1), rec(0, 20, 30, n_flip=1, w_flip=1)))   # flip . flip = same
    assert rows == [(0, 10, 10, 0), (0, 20, 10, 1), (0, 30, 10, 0)] and conflicts == []
    # the later components merge through their larger members: the block is still the smallest PS, flips relative to it
    rows, conflicts = both(records(rec(0, 5, 9, n_flip=9, w_flip=9), rec(0, 20, 30, n_same=8, w_same=8), rec(0, 9, 30, n_flip=1, w_flip=1)))
    assert rows == [(0, 5, 5, 0), (0, 9, 5, 1), (0, 20, 5, 0), (0, 30, 5, 0)] and conflicts == []
    # a link without a verdict joins nothing, but its phase sets are listed
    rows, conflicts = both(records(rec(0, 10, 20, n_open=4), rec(0, 20, 30, n_same=1, n_flip=1, w_same=2, w_flip=2)))
    assert rows == [(0, 10, 10, 0), (0, 20, 20, 0), (0, 30, 30, 0)] and conflicts == []
    assert both(records()) == ([], [])


def test_blocks_triangle_with_a_contradicting_weakest_link():
    tri = records(rec(0, 10, 30, n_same=1, w_same=1),          # the weakest: contradicts same . flip = flip
                  rec(0, 10, 20, n_same=5, w_same=9), rec(0, 20, 30, n_flip=4, w_flip=4))
    rows, conflicts = both(tri)
    assert conflicts == [0]
    assert rows == both(tri[1:])[0] == [(0, 10, 10, 0), (0, 20, 10, 0), (0, 30, 10, 1)]         # it changes nothing
    agree = tri.copy()
    agree[0] = records(rec(0, 10, 30, n_flip=1, w_flip=1))[0]
    assert both(agree) == (rows, [])
    # the order is (-n_win, -w_win, row index): with the strengths swapped the other two win and (20, 30) is the conflict
    swapped = records(rec(0, 10, 30, n_same=9, w_same=1), rec(0, 10, 20, n_same=5, w_same=9), rec(0, 20, 30, n_flip=4, w_flip=4))
    assert both(swapped) == ([(0, 10, 10, 0), (0, 20, 10, 0), (0, 30, 10, 0)], [2])
    # equal counts: the weight decides; equal both: the earlier row
    tie = records(rec(0, 10, 30, n_same=2, w_same=5), rec(0, 10, 20, n_same=2, w_same=5), rec(0, 20, 30, n_flip=2, w_flip=6))
    assert both(tie)[1] == [1]
    tie['w_flip'][2] = 5
    assert both(tie)[1] == [2]


def test_blocks_contigs_stay_apart():
    rows, conflicts = both(records(rec(0, 10, 20, n_same=1, w_same=1), rec(1, 10, 20, n_flip=1, w_flip=1), rec(1, 20, 30, n_flip=1, w_flip=1)))
    assert rows == [(0, 10, 10, 0), (0, 20, 10, 0), (1, 10, 10, 0), (1, 20, 10, 1), (1, 30, 10, 0)] and conflicts == []
    assert ps_links.blocks_text(rows, ['a', b'b']) == 'a\t10\t10\t0\na\t20\t10\t0\nb\t10\t10\t0\nb\t20\t10\t1\nb\t30\t10\t0\n' == \
        R.blocks_text(rows, ['a', 'b'])


def test_blocks_on_random_records():
    for a, k in ((1,), {}), ((4,), dict(n_contigs=5, n_ps=(60, 90), reads_per_contig=(250, 300), deg=(100, 200), cands_per_contig=(20, 40))):
        for cap in (8100, 12000):
            recs = R.records(R.links(soa_fuzz.random_soa(*a, **k), 0, 0, cap), DT)
            rows, conflicts = both(recs)
            assert len(recs) >= 10 and len(rows) >= 3
            assert [r[:2] for r in rows] == sorted(set([(int(r['contig']), int(r[f])) for r in recs for f in ('ps_a', 'ps_b')]))
            assert all(block <= ps for _, ps, block, _ in rows)


def test_write_both_tables(tmp_path):
    recs = records(rec(0, 10, 20, n_same=3, w_same=3), rec(0, 20, 30, n_flip=2, w_flip=2))
    home = str(tmp_path)
    assert ps_links.write(home, recs, ['chr9']) == (2, 3, 0)
    assert open(ps_links.links_path(home)).read() == ps_links.header() + 'chr9\t10\t20\t3\t3\t0\t0\t3\t0\t0\t0\tsame\nchr9\t20\t30\t2\t0\t2\t0\t0\t2\t0\t0\tflip\n'
    assert open(ps_links.blocks_path(home)).read() == 'CHROM\tPS\tBLOCK\tFLIP\nchr9\t10\t10\t0\nchr9\t20\t10\t0\nchr9\t30\t10\t1\n'
    assert ps_links.links_path(home).endswith('/phased_sv.ps_links.tsv') and ps_links.blocks_path(home).endswith('/phased_sv.ps_blocks.tsv')


# ---- the record and the bindings ----------------------------------------------------------------------------------------------------

def test_record_layout():
    assert DT.itemsize == 56 == ctypes.sizeof(_lib.PsLink)
    want = dict(w_same=0, w_flip=8, contig=16, ps_a=20, ps_b=24, n_sv=28, n_same=32, n_flip=36, n_open=40, pos_min=44, pos_max=48, reserved=52)
    assert {n: DT.fields[n][1] for n in DT.names} == want
    assert {n: getattr(_lib.PsLink, n).offset for n, _ in _lib.PsLink._fields_} == want
    assert DT.names == R.FIELDS
    for name in ('duet_ps_links_device', 'duet_ps_links_host', 'duet_svim_ps_links_device', 'duet_svim_ps_links_host'):
        assert name in _lib.EXPORTS
    assert _lib.ps_links_room(0) == 0 and _lib.ps_links_room(1) == 0 and _lib.ps_links_room(10) == 9
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'duet_ef.h')).read()
    assert 'typedef struct duet_ps_link {' in header and 'THREE host round trips' in header


# ---- the flag's refusals ------------------------------------------------------------------------------------------------------------

def test_flag_is_declared_and_refused_on_the_sharded_paths(monkeypatch, tmp_path):
    from duet_amd import cli, utils
    from duet_amd.sv_phasing import sv_phasing
    from duet_amd.svim_mode import sv_phasing_from_bams
    a = utils.build_parser().parse_args(['in.bam', 'ref.fa', 'out', '--write_ps_links'])
    assert a.write_ps_links is True and utils.build_parser().parse_args(['in.bam', 'ref.fa', 'out']).write_ps_links is False
    out = str(tmp_path / 'never')
    for argv, env in ((['--gpus', '2'], None), (['-b', 'svim-gpu', '--gpus', '3'], None), ([], '1'), (['-b', 'svim-gpu'], '1')):
        monkeypatch.setattr(sys, 'argv', ['duet', 'in.bam', 'ref.fa', out, '--write_ps_links'] + argv)
        if env:
            monkeypatch.setenv('DUET_FORCE_RANKS', env)
        else:
            monkeypatch.delenv('DUET_FORCE_RANKS', raising=False)
        with pytest.raises(SystemExit) as e:
            cli.main(None)
        assert '--write_ps_links works on the single-GPU path only' in str(e.value)
        assert not os.path.exists(out)                                         # refused before anything is created
    monkeypatch.delenv('DUET_FORCE_RANKS', raising=False)
    for fn, args in ((sv_phasing, (out, 50, 2, 4, False)), (sv_phasing_from_bams, (out, 50, 2, 4, False))):
        with pytest.raises(ValueError, match='ps_links: single-GPU path only'):
            fn(*args, gpus=2, ps_links=True)
        monkeypatch.setenv('DUET_FORCE_RANKS', '1')
        with pytest.raises(ValueError, match='ps_links: single-GPU path only'):
            fn(*args, ps_links=True)
        monkeypatch.delenv('DUET_FORCE_RANKS', raising=False)
    assert not os.path.exists(out)


def test_flag_is_refused_where_the_native_ingest_declines(monkeypatch, tmp_path):
    """The refusal comes from the ingest, before any context or kernel is needed: DUET_NATIVE_INGEST=0 declines every input."""
    from duet_amd import sv_phasing as sp
    home = str(tmp_path)
    os.makedirs(home + '/sv_calling')
    os.makedirs(home + '/snp_phasing')
    monkeypatch.setenv('DUET_NATIVE_INGEST', '0')
    with pytest.raises(RuntimeError, match='--write_ps_links needs the native ingest'):
        sp._native(home, 50, 2, 4, False, home + '/sv_calling/variants.vcf', home + '/phased_sv.vcf', None, ps_links=True)
    with pytest.raises(RuntimeError, match='--write_ps_links need the native ingest'):
        sp._native_thresholds(home, 50, 2, 4, False, home + '/sv_calling/variants.vcf', home + '/phased_sv.vcf', None, None, ps_links=True)
    assert sp._native(home, 50, 2, 4, False, home + '/sv_calling/variants.vcf', home + '/phased_sv.vcf', None) is False
    assert not os.path.exists(home + '/phased_sv.vcf') and not os.path.exists(ps_links.links_path(home))
