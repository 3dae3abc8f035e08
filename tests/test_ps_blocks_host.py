# coding=utf-8
"""No GPU: the round-based build of the blocks (tests/ps_blocks_ref.py -- what duet_amd/csrc/duet_psblocks.hip does on the device)
against duet_amd/ps_links.py: blocks, the normative text, on seeded random multigraph records; and the binding against the
header."""
import ctypes
import json
import os
import re

import pytest

from duet_amd import _lib, ps_links, tune
from tests import ps_blocks_ref as B

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SEEDS = 1500


def same(records, min_sv):
    want_rows, want_conflicts = ps_links.blocks(records, min_sv)
    rows, conflicts, rounds = B.blocks(records, min_sv)
    assert [tuple(r) for r in want_rows] == rows and list(want_conflicts) == conflicts
    return conflicts, rounds


def test_rounds_select_what_kruskal_selects():
    """min_sv 1..3; at least a tenth of the cases with a contradicting link and a tenth with a tie in (n_win, w_win): otherwise the
    comparison would show little."""
    cases = with_conflict = with_tie = max_rounds = 0
    for seed in range(N_SEEDS):
        records, _ = B.random_records(seed)
        for min_sv in (1, 2, 3):
            conflicts, rounds = same(records, min_sv)
            cases += 1
            with_conflict += len(conflicts) > 0
            with_tie += B.has_tie(records, min_sv)
            max_rounds = max(max_rounds, rounds)
    assert with_conflict * 10 >= cases and with_tie * 10 >= cases, (cases, with_conflict, with_tie)
    assert max_rounds >= 3


def test_the_chain_of_1025_phase_sets():
    for min_sv in (1, 2):
        _, rounds = same(B.chain(1024), min_sv)
        assert rounds >= 2
    # every phase set's best link is the one to its left: one round, one path
    records = B.records([dict(contig=0, ps_a=3 * i, ps_b=3 * i + 3, n_flip=2000 - i, w_flip=1) for i in range(1024)])
    assert same(records, 1) == ([], 1)


def test_rounds_stay_within_what_the_device_launches():
    """The device fixes its rounds on the host: one for every r with (2 * n_links) >> r >= 2."""
    for seed in range(200):
        records, _ = B.random_records(seed)
        if len(records):
            launched = sum(1 for r in range(40) if (2 * len(records)) >> r >= 2)
            assert B.blocks(records, 1)[2] <= launched


def test_the_reference_tells_a_wrong_build_apart():
    """The same records with one strength changed give another table: the comparison above is not vacuous."""
    records = B.records([dict(contig=0, ps_a=1, ps_b=2, n_flip=1, w_flip=1), dict(contig=0, ps_a=1, ps_b=3, n_flip=1, w_flip=3),
                         dict(contig=0, ps_a=2, ps_b=3, n_flip=1, w_flip=2)])
    assert B.blocks(records, 1)[1] == [0]
    records['w_flip'][0] = 9
    assert B.blocks(records, 1)[1] == [2]
    assert B.blocks(records, 2)[:2] == ([(0, 1, 1, 0), (0, 2, 2, 0), (0, 3, 3, 0)], [])


def header_text():
    with open(os.path.join(REPO, 'include', 'duet_ef.h')) as f:
        return f.read()


def test_header_against_bindings():
    text = re.sub(r'/\*.*?\*/', '', header_text(), flags=re.S)
    m = re.search(r'typedef struct duet_ps_blocks_counts \{(.*?)\} duet_ps_blocks_counts;', text, flags=re.S)
    fields = [n.strip() for n in m.group(1).replace('uint32_t', '').replace(';', '').split(',')]
    assert fields == [n for n, _ in _lib.PsBlocksCounts._fields_] and ctypes.sizeof(_lib.PsBlocksCounts) == 16
    for name in ('duet_ps_blocks_device', 'duet_ps_blocks_host', 'duet_ps_join_links_device'):
        assert name in _lib.EXPORTS
        args = re.search(r'DUET_API int %s\((.*?)\);' % name, text, flags=re.S).group(1)
        assert len(args.split(',')) == len(getattr(_lib.load(), name).argtypes)
    assert '#define DUET_ABI_VERSION 1' in header_text()


def test_tune_arguments():
    base = ['w', 't.vcf', '--grid', 'g.json']
    assert tune.parse_args(base).join is None
    assert tune.parse_args(base + ['--join_ps']).join == [2]
    assert tune.parse_args(base + ['--join_ps', '--join_min_sv', '0,1,2,3']).join == [0, 1, 2, 3]
    assert tune.parse_args(['w', 't.vcf', '--fit', 'hp_f1', '--fit_cap', '--join_ps', '--join_min_sv', '1,2']).join == [1, 2]
    for bad in (['--join_min_sv', '2'], ['--join_ps', '--join_min_sv', '-1'], ['--join_ps', '--join_min_sv', '1,x'],
                ['--join_ps', '--join_min_sv', '']):
        with pytest.raises(SystemExit):
            tune.parse_args(base + bad)
    for bad in ([], [-1], [1.5], [True], 'x'):
        with pytest.raises((ValueError, TypeError)):
            tune._join_list(bad)
    assert tune._join_list(None) is None and tune._join_list(2) == [2] and tune._join_list((0, 3)) == [0, 3]
    # the setting columns and the names of --features
    assert tune.LEAD[-1] == 'join_min_sv' and list(tune._lead(None, 50, 2, 8100, 0)) == ['pc_cap', 'svlen_thres', 'suppread_thres', 'join_min_sv']
    assert list(tune._lead(None, 50, 2)) == ['svlen_thres', 'suppread_thres']
    assert tune.features_path('f.tsv', tune._lead(0.9, 50, 2, 2400, 2)) == 'f.c0.9.s50.r2.p2400.j2.tsv'
    assert tune.features_path('f.tsv', tune._lead(None, 50, 2)) == 'f.s50.r2.tsv'


def test_load_vector_with_the_new_key(tmp_path):
    path = str(tmp_path / 'v.json')

    def write(obj):
        with open(path, 'w') as f:
            json.dump(obj, f)
    write({'c1_max_ref_num': 3, 'pc_cap': 2400, 'join_min_sv': 3})
    want = tune.vector({'c1_max_ref_num': 3})
    # the call forms there were return what they returned
    assert tune.load_vector(path).tolist() == want.tolist()
    vec, cap = tune.load_vector(path, with_cap=True)
    assert vec.tolist() == want.tolist() and cap == 2400
    vec, cap, join = tune.load_vector(path, with_cap=True, with_join=True)
    assert vec.tolist() == want.tolist() and (cap, join) == (2400, 3)
    vec, join = tune.load_vector(path, with_join=True)
    assert join == 3
    write({'c1_max_ref_num': 3})
    assert tune.load_vector(path, with_cap=True, with_join=True)[1:] == (None, None)
    for bad in (0, -1, 1.5, '2', True):
        write({'join_min_sv': bad})
        with pytest.raises(ValueError):
            tune.load_vector(path)
