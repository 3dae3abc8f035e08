# coding=utf-8
"""No GPU: the reference of the joined phase sets (tests/ps_join_ref.py) against cases worked by hand, the host side of
duet_amd/ps_join.py against it, the bindings, the refusals of --join_ps that need no device, and -- with the C oracle -- that the
rule changes calls on the project's own random problems."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from duet_amd import _lib, ps_join, ps_links
from oracle import c_oracle
from tests import ps_join_ref as J
from tests import ps_links_ref as L
from tests import soa_fuzz
from tests.test_ps_links_host import rec, records

SEEDS = tuple(range(1, 9))


def tag(hap, pc, ps):
    return (hap << 62) | (pc << 32) | ps


# ---- the reference against hand-worked cases ----------------------------------------------------------------------------------------

def test_reference_remap_by_hand():
    rows = [(0, 20, 10, 1), (1, 20, 5, 0), (1, 0xFFFFFFFF, 7, 1)]
    pc = (1 << 30) - 2
    words = [tag(1, 3, 20), tag(2, pc, 20), tag(3, 9, 20), tag(0, 9, 20), tag(1, 3, 21), J.UNTAGGED,     # contig 0
             tag(1, 3, 20), tag(2, 0, 0xFFFFFFFF), J.UNTAGGED, tag(1, 3, 5)]                             # contig 1
    got, n = J.remap(np.array(words, dtype=np.uint64), [0, 6, 10], rows)
    want = [tag(2, 3, 10), tag(1, pc, 10), tag(3, 9, 10), tag(0, 9, 10), tag(1, 3, 21), J.UNTAGGED,
            tag(1, 3, 5), tag(1, 0, 7), J.UNTAGGED, tag(1, 3, 5)]
    assert [int(x) for x in got] == want and n == 6
    # the all-ones word is hap 3, pc 2^30 - 1, ps 0xFFFFFFFF: the row (1, 0xFFFFFFFF) leaves it alone
    assert J.remap(np.array([J.UNTAGGED], dtype=np.uint64), [0, 0, 1], rows) == (np.array([J.UNTAGGED], dtype=np.uint64), 0)
    # a block that maps a phase set to itself changes nothing
    assert J.remap(np.array([tag(1, 1, 4)], dtype=np.uint64), [0, 1], [(0, 4, 4, 0)])[1] == 0


def test_reference_change_codes_by_hand():
    tab = J.as_dict([(0, 20, 10, 1), (0, 30, 10, 0), (1, 20, 5, 0)])
    code = lambda k, p0, s0, p1, s1: J.NAMES[J.change_code(k, p0, s0, p1, s1, tab)]
    assert code(0, 0, 0, 0, 0) == 'none'
    assert code(0, 0, 0, 3, 10) == 'gained' and code(0, 0, 7, 1, 7) == 'gained'
    assert code(0, 2, 20, 0, 0) == 'lost'
    assert code(0, 1, 40, 1, 40) == 'same'
    assert code(0, 1, 10, 1, 10) == 'same'
    assert code(0, 1, 20, 2, 10) == 'relabelled'             # flipped into block 10
    assert code(0, 3, 20, 3, 10) == 'relabelled'             # 1|1 has no side to flip
    assert code(0, 2, 30, 2, 10) == 'relabelled'
    assert code(1, 1, 20, 1, 5) == 'relabelled' and code(1, 1, 20, 2, 10) == 'other'        # the key holds the contig
    assert code(0, 3, 20, 1, 10) == 'to_het' and code(0, 3, 40, 2, 40) == 'to_het'
    assert code(0, 1, 20, 3, 10) == 'to_hom'
    assert code(0, 1, 20, 1, 10) == 'other' and code(0, 1, 40, 1, 41) == 'other' and code(0, 1, 40, 2, 40) == 'other'
    # precedence: `same` before `relabelled` (a row that maps a phase set to itself), `gained` before everything
    assert J.NAMES[J.change_code(0, 1, 4, 1, 4, J.as_dict([(0, 4, 4, 0)]))] == 'same'
    assert code(0, 0, 20, 1, 10) == 'gained'
    codes, counts = J.diff([0, 0, 1], [0, 1, 1], [0, 20, 20], [0, 2, 1], [0, 10, 5], [(0, 20, 10, 1), (1, 20, 5, 0)])
    assert codes.tolist() == [0, 4, 4] and counts.tolist() == [1, 0, 0, 0, 2, 0, 0, 0]


def test_reference_report_by_hand():
    text = J.report_text(['chr1', 'chr2'], [0, 0, 1, 1], [5, 6, 7, 8], [50, 60, 70, 80], [1, 4, 5, 2], [0, 1, 3, 2], [0, 20, 30, 9],
                         [1, 2, 2, 0], [10, 10, 30, 0])
    assert text == 'chr1\t5\t50\tgained\t.\t.\t1|0\t10\nchr2\t7\t70\tto_het\t1|1\t30\t0|1\t30\nchr2\t8\t80\tlost\t0|1\t9\t.\t.\n'
    assert J.header() == 'CHROM\tPOS\tSVLEN\tCHANGE\tHP\tPS\tHP_JOINED\tPS_JOINED\n'


# ---- duet_amd/ps_join.py and ps_links.blocks(min_sv) ---------------------------------------------------------------------------------

def fuzz_records(seed):
    return L.records(L.links(soa_fuzz.random_soa(seed), 50, 2), _lib.PS_LINK_DTYPE)


def test_blocks_min_sv_1_is_what_it_was():
    for seed in SEEDS:
        recs = fuzz_records(seed)
        assert ps_links.blocks(recs, min_sv=1) == ps_links.blocks(recs) == L.blocks(recs)
    assert any(len(fuzz_records(seed)) > 3 for seed in SEEDS)


def test_select_at_the_threshold():
    recs = records(rec(0, 1, 2, n_same=2, n_flip=1), rec(0, 2, 3, n_flip=3, n_same=1), rec(0, 3, 4, n_same=1, n_flip=1),
                   rec(0, 4, 5, n_same=1), rec(0, 5, 6, n_open=4))
    pick = lambda n: [(int(r['ps_a']), int(r['ps_b'])) for r in ps_join.select(recs, n)]
    assert pick(1) == [(1, 2), (2, 3), (4, 5)]                      # a tie and an open link have no verdict
    assert pick(2) == [(1, 2), (2, 3)]                              # N_win == min_sv stays, min_sv - 1 goes
    assert pick(3) == [(2, 3)] and pick(4) == []
    assert [tuple(recs[i][f] for f in ('ps_a', 'ps_b')) for i in J.select(recs, 2)] == pick(2)
    for n in (1, 2, 3, 4):
        rows, conflicts = ps_links.blocks(recs, min_sv=n)
        assert (rows, conflicts) == J.blocks_used(recs, n)
        joined = [r for r in rows if r[1] != r[2]]
        assert joined == [r for r in ps_links.blocks(ps_join.select(recs, n))[0] if r[1] != r[2]]
    assert ps_links.blocks(recs, min_sv=2)[0] == [(0, 1, 1, 0), (0, 2, 1, 0), (0, 3, 1, 1), (0, 4, 4, 0), (0, 5, 5, 0), (0, 6, 6, 0)]
    for seed in SEEDS:
        recs = fuzz_records(seed)
        for n in (1, 2, 3):
            assert ps_links.blocks(recs, min_sv=n) == J.blocks_used(recs, n)
    with pytest.raises(ValueError):
        ps_join.check_min_sv(0)
    with pytest.raises(ValueError):
        ps_join.check_min_sv(1.5)
    assert ps_join.check_min_sv(3) == 3


def test_table_and_texts():
    rows = [(0, 20, 10, 1), (2, 0xFFFFFFFF, 7, 0)]
    t = ps_join.table(rows)
    assert t.dtype == _lib.PS_BLOCK_DTYPE and t.tolist() == rows and ps_join.table([]).shape == (0,)
    args = (['chr1', b'chr2'], [0, 0, 1, 1], [5, 6, 7, 8], [50, 60, 70, 80], [1, 4, 5, 2], [0, 1, 3, 2], [0, 20, 30, 9], [1, 2, 2, 0],
            [10, 10, 30, 0])
    assert ps_join.report_text(*args) == J.report_text(['chr1', 'chr2'], *args[1:])
    assert ps_join.report_header() == J.header()
    assert ps_join.report_text(['a'], [], [], [], [], [], [], [], []) == ''
    line = ps_join.summary_text([1, 2, 3, 4, 5, 6, 7, 8], 9, 10)
    assert line == ('none 1, gained 2, lost 3, same 4, relabelled 5, to_het 6, to_hom 7, other 8; 9 read tags remapped; '
                    '10 phase sets in the table')
    assert ps_join.path_vcf('h') == 'h/phased_sv.joined.vcf' and ps_join.path_report('h') == 'h/phased_sv.join_report.tsv'
    assert ps_join.path_blocks('h') == 'h/phased_sv.join_blocks.tsv'


def test_header_and_bindings_agree():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'duet_ef.h')).read()
    assert 'Joined phase sets' in header and 'typedef struct duet_ps_block {' in header
    assert _lib.PS_BLOCK_DTYPE.itemsize == 16 and _lib.PS_BLOCK_DTYPE.names == ('contig', 'ps', 'block', 'flip')
    names = re.search(r'#define DUET_PS_JOIN_CHANGE_NAMES \{(.*)\}', header).group(1)
    assert tuple(n.strip().strip('"') for n in names.split(',')) == _lib.JOIN_CHANGE_NAMES == J.NAMES
    for i, n in enumerate(J.NAMES):
        assert re.search(r'#define DUET_PS_JOIN_%s %du\n' % (n.upper(), i), header)
    for name in ('duet_ps_join_tags_device', 'duet_ps_join_tags_host', 'duet_ps_join_diff_device', 'duet_ps_join_diff_host'):
        assert name in _lib.EXPORTS and re.search(r'DUET_API int %s\(' % name, header)
    for m in ('ps_join_tags_host', 'ps_join_tags_device', 'ps_join_diff_host', 'ps_join_diff_device'):
        assert callable(getattr(_lib.Context, m))
    assert tuple(ps_join.REPORTED) == tuple(J.NAMES.index(n) for n in J.REPORTED)
    assert '#define DUET_ABI_VERSION 1\n' in header


# ---- the flag's refusals ------------------------------------------------------------------------------------------------------------

def test_flags_are_declared_and_refused(monkeypatch, tmp_path):
    from duet_amd import cli, utils
    from duet_amd.sv_phasing import sv_phasing
    from duet_amd.svim_mode import sv_phasing_from_bams
    parse = lambda *argv: utils.build_parser().parse_args(['in.bam', 'ref.fa', 'out'] + list(argv))
    assert parse().join_ps is False and parse().join_min_sv is None
    assert parse('--join_ps').join_ps is True and parse('--join_ps', '--join_min_sv', '3').join_min_sv == 3
    with pytest.raises(SystemExit):
        parse('--join_ps', '--join_min_sv', 'two')
    out = str(tmp_path / 'never')
    cases = ((['--join_ps', '--gpus', '2'], None, '--join_ps works on the single-GPU path only'),
             (['--join_ps', '-b', 'svim-gpu', '--gpus', '3'], None, '--join_ps works on the single-GPU path only'),
             (['--join_ps'], '1', '--join_ps works on the single-GPU path only'),
             (['--join_ps', '-b', 'svim-gpu'], '1', '--join_ps works on the single-GPU path only'),
             (['--join_min_sv', '2'], None, '--join_min_sv needs --join_ps'),
             (['--join_ps', '--join_min_sv', '0'], None, '--join_min_sv takes an integer >= 1'),
             (['--join_ps', '--join_min_sv', '-1', '-b', 'svim-gpu'], None, '--join_min_sv takes an integer >= 1'))
    for argv, env, text in cases:
        monkeypatch.setattr(sys, 'argv', ['duet', 'in.bam', 'ref.fa', out] + argv)
        if env:
            monkeypatch.setenv('DUET_FORCE_RANKS', env)
        else:
            monkeypatch.delenv('DUET_FORCE_RANKS', raising=False)
        with pytest.raises(SystemExit) as e:
            cli.main(None)
        assert text in str(e.value)
        assert not os.path.exists(out)                                         # refused before anything is created
    monkeypatch.delenv('DUET_FORCE_RANKS', raising=False)
    for fn, args in ((sv_phasing, (out, 50, 2, 4, False)), (sv_phasing_from_bams, (out, 50, 2, 4, False))):
        with pytest.raises(ValueError, match='join_ps: single-GPU path only'):
            fn(*args, gpus=2, join_ps=True)
        with pytest.raises(ValueError, match='join_min_sv: an integer >= 1'):
            fn(*args, join_ps=True, join_min_sv=0)
        monkeypatch.setenv('DUET_FORCE_RANKS', '1')
        with pytest.raises(ValueError, match='join_ps: single-GPU path only'):
            fn(*args, join_ps=True)
        monkeypatch.delenv('DUET_FORCE_RANKS', raising=False)
    assert not os.path.exists(out)


def test_flag_is_refused_where_the_native_ingest_declines(monkeypatch, tmp_path):
    from duet_amd import sv_phasing as sp
    home = str(tmp_path)
    os.makedirs(home + '/sv_calling')
    os.makedirs(home + '/snp_phasing')
    monkeypatch.setenv('DUET_NATIVE_INGEST', '0')
    with pytest.raises(RuntimeError, match='--join_ps needs the native ingest'):
        sp._native(home, 50, 2, 4, False, home + '/sv_calling/variants.vcf', home + '/phased_sv.vcf', None, join_min_sv=2)
    with pytest.raises(RuntimeError, match='--join_ps need the native ingest'):
        sp._native_thresholds(home, 50, 2, 4, False, home + '/sv_calling/variants.vcf', home + '/phased_sv.vcf', None, None, join_min_sv=2)
    assert sorted(os.listdir(home)) == ['snp_phasing', 'sv_calling']


# ---- the unit's compile remarks --------------------------------------------------------------------------------------------------------

HIPCC = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)


@pytest.mark.skipif(HIPCC is None, reason='hipcc not found')
def test_psjoin_kernels_are_integer_only_without_scratch_or_calls(tmp_path):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(repo, 'duet_amd', 'csrc')
    asm = str(tmp_path / 'duet_psjoin.s')
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fvisibility=hidden',
           '-Wno-unused-function', '-I' + os.path.join(repo, 'include'), '--cuda-device-only', '-S',
           '-Rpass-analysis=kernel-resource-usage', os.path.join(csrc, 'duet_psjoin.hip'), '-o', asm]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    found = re.findall(r'Function Name: (\S+) \[.*?\n(?:.*\n){0,8}?.*ScratchSize \[bytes/lane\]: (\d+)', r.stderr)
    kernels = {n: int(v) for n, v in found}
    assert len(kernels) == 2 and sum('pj_tags' in n for n in kernels) == 1 and sum('pj_diff' in n for n in kernels) == 1, sorted(kernels)
    assert all(v == 0 for v in kernels.values()), kernels
    lds = dict(re.findall(r'Function Name: (\S+) \[.*?\n(?:.*\n){0,12}?.*LDS Size \[bytes/block\]: (\d+)', r.stderr))
    assert sorted(int(v) for v in lds.values()) == [0, 8192], lds                 # the slice copy of pj_tags: 2048 keys
    with open(asm) as f:
        code = [ln.split(';')[0] for ln in f if ln.startswith('\t') and not ln.startswith('\t.')]
    assert len(code) > 100
    assert not any('s_swappc' in ln or 's_call' in ln for ln in code)
    assert not any(re.search(r'_f(16|32|64)\b', ln) for ln in code), [ln for ln in code if re.search(r'_f(16|32|64)\b', ln)][:5]


# ---- the rule does something on the project's own problems (the condition of tests/test_gpu_ps_join.py, pinned on the CPU) -----------

def joined_by_the_oracle(seed, min_sv=2):
    soa = soa_fuzz.random_soa(seed)
    recs = L.links(soa, 50, 2)
    rows, conflicts = J.blocks_used(recs, min_sv)
    rc0, p0, s0 = c_oracle.ef(soa, 50, 2)
    rc1, p1, s1 = c_oracle.ef(J.remapped_soa(soa, rows), 50, 2)
    codes, counts = J.diff(J.contig_column(soa.cand_ctg_off), p0, s0, p1, s1, rows)
    return dict(soa=soa, rows=rows, conflicts=conflicts, rc=(rc0, rc1), base=(p0, s0), joined=(p1, s1), codes=codes, counts=counts)


def test_the_rule_changes_calls_on_every_seed():
    per = [joined_by_the_oracle(seed) for seed in SEEDS]
    name = J.NAMES.index
    for r in per:
        assert r['rc'] == (0, 0)                                                # neither run divides by zero
        assert r['counts'][name('gained')] + r['counts'][name('to_het')] >= 1
        assert 20 <= r['counts'][name('gained')] <= 177
    assert [seed for seed, r in zip(SEEDS, per) if r['counts'][name('to_het')]] == [1, 2, 5, 6, 7, 8]
    assert sum(1 for r in per if r['conflicts']) >= 5
