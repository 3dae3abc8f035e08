# coding=utf-8
"""Tags from other SVs without a GPU: the reference (tests/sv_tags_ref.py) on hand cases, the header against the bindings and the
library's symbols, the flags and their refusals, the unit's compile remarks, and the CPU condition -- the reference's tags through
the C oracle on the expanded problem, with the per-seed counts pinned."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from duet_amd import _lib, sv_tags
from tests import read_tags_cases as RK
from tests import sv_tags_cases as K
from tests import sv_tags_ref as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABSENT, UN = S.ABSENT, S.UNTAGGED
tag = S.tag


def cand(pred, ps, marks):
    return dict(pred=pred, ps=ps, marks=marks)


# ---- the reference on hand cases -----------------------------------------------------------------------------------------------------

def test_the_central_case():
    """Het call X (1|0, PS 7) lists untagged read r; candidate Y of class 0 lists r too."""
    X, Y = cand(1, 7, [(0, ABSENT)]), cand(0, 0, [(0, ABSENT)])
    out, index, counts = S.sv_tags(RK.problem([[X, Y]]), min_votes=1, pc_new=5)
    assert out == [UN, tag(1, 5, 7)] and index == [0, 1]                      # X's own mark gets nothing, Y's gets hap 1 / PS 7
    assert counts == (2, 1, 1)                                                # ... and X's mark is what leave-one-out took away
    # a second het call Z listing r: X's mark gets Z's evidence only
    Z = cand(2, 9, [(0, ABSENT)])
    out, _, counts = S.sv_tags(RK.problem([[X, Y, Z]]))
    assert out == [tag(2, 0, 9), tag(1, 0, 7), tag(1, 0, 7)] and counts == (3, 3, 0)
    #   (Y sees |d| = 1 in PS 7 and in PS 9: the smaller PS wins; Z's own mark sees X alone)
    # in Z's own phase set the two calls cancel for Y, and each het call sees the other alone
    Z7 = cand(2, 7, [(0, ABSENT)])
    out, _, counts = S.sv_tags(RK.problem([[X, Y, Z7]]))
    assert out == [tag(2, 0, 7), UN, tag(1, 0, 7)] and counts == (3, 2, 0)


def test_tagged_marks_keep_their_word_whatever_it_holds():
    words = [tag(0, 3, 7), tag(3, 8101, 7), tag(1, (1 << 30) - 2, 9), tag(2, 0, 0)]
    X = cand(1, 7, [(i, i) for i in range(4)] + [(4, ABSENT)])
    Y = cand(2, 9, [(i, i) for i in range(4)] + [(4, ABSENT)])
    out, _, counts = S.sv_tags(RK.problem([[X, Y]], words))
    assert out[:4] == words and out[5:9] == words and counts == (2, 2, 0)
    assert out[4] == tag(2, 0, 9) and out[9] == tag(1, 0, 7)


def test_every_spelling_of_no_tag():
    X = cand(1, 7, [(0, ABSENT)])
    for read, names in ((ABSENT, 0), (2, 0), (3, 0), (1 << 31, 0), (1, 0)):     # absent, n_reads, n_reads + 1, 2^31, an all-ones word
        Y = cand(3, 0, [(names, read)])
        p = RK.problem([[X, Y]], [tag(1, 0, 5), UN])
        p.mark_read[0] = read                                                  # (one name, one read index)
        out, _, counts = S.sv_tags(p)
        assert out == [UN, tag(1, 0, 7)] and counts == (2, 1, 1)


def test_duplicates_inside_a_candidate_and_min_votes():
    # a het candidate with k = 2 against another call's evidence of exactly 2 (tie -> no tag) and of 3
    X = cand(1, 7, [(0, ABSENT)] * 2 + [(1, ABSENT)])
    for n, want in ((2, UN), (3, tag(2, 0, 7))):
        Y = cand(2, 7, [(0, ABSENT)] * n)
        W = cand(0, 0, [(0, ABSENT)])
        out, _, counts = S.sv_tags(RK.problem([[X, Y, W]]))
        assert out[-1] == want                                                 # W: 2 against n
        assert out[0] == out[1] == tag(2, 0, 7) and out[2] == UN               # X's own marks of name 0 see Y alone; name 1 nobody
    # |d| at min_votes - 1 and at min_votes
    for mv in (1, 3):
        for n in (mv - 1, mv):
            p = RK.problem([[cand(1, 7, [(0, ABSENT)] * n + [(1, ABSENT)]), cand(3, 0, [(0, ABSENT)])]])
            out, _, _ = S.sv_tags(p, min_votes=mv)
            assert out[-1] == (tag(1, 0, 7) if n >= mv else UN)


def test_refusals_of_the_reference():
    p = RK.problem([[cand(1, 7, [(0, ABSENT)])]])
    for kw in (dict(min_votes=0), dict(pc_new=S.CAP_MAX + 1), dict(pc_cap=S.CAP_MAX + 1)):
        with pytest.raises(S.Refused):
            S.sv_tags(p, **kw)
    for bad in (RK.problem([[cand(4, 7, [(0, ABSENT)])]]), RK.problem([[cand(1, 7, [(1, ABSENT)])]], n_names=1),
                S.R.Problem(**dict(p.__dict__, mark_order=[1])), S.R.Problem(**dict(p.__dict__, cand_contig=[0])),
                S.R.Problem(**dict(p.__dict__, cand_ctg_off=None)), S.R.Problem(**dict(p.__dict__, cand_ctg_off=[0, 0])),
                RK.problem([[cand(1, 7, [(0, ABSENT)])], [cand(1, 7, [(0, ABSENT)])]]),
                RK.problem([[cand(1, 7, [(0, 0)]), cand(1, 9, [(0, 1)])]], [tag(1, 0, 7)] * 2)):
        with pytest.raises(S.Refused):
            S.sv_tags(bad)
    assert S.sv_tags(RK.problem([[]])) == (None, None, (0, 0, 0))
    out, _, counts = S.sv_tags(RK.problem([[cand(0, 0, [(0, ABSENT)]), cand(3, 0, [(0, ABSENT), (1, 0)])]], [tag(1, 0, 7)]))
    assert out == [UN, UN, tag(1, 0, 7)] and counts == (2, 0, 0)               # no het candidate: every untagged mark stays all-ones


def test_change_codes_on_the_host_are_the_reference():
    rng = np.random.RandomState(3)
    p0, p1 = rng.randint(0, 4, 500), rng.randint(0, 4, 500)
    s0, s1 = rng.randint(0, 3, 500), rng.randint(0, 3, 500)
    change, counts = sv_tags.change_codes(p0, s0, p1, s1)
    want = [S.change(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(p0, s0, p1, s1)]
    assert [_lib.JOIN_CHANGE_NAMES[int(x)] for x in change] == want and set(want) == set(S.CHANGE) - {'relabelled'}
    assert counts.tolist() == [want.count(n) for n in S.CHANGE]


# ---- header, bindings, symbols -------------------------------------------------------------------------------------------------------

def header_text():
    with open(os.path.join(REPO, 'include', 'duet_ef.h')) as f:
        return f.read()


def test_header_declares_the_two_entries_under_their_section():
    text = header_text()
    at = text.index('Tags from other SVs (duet_svtags.hip')
    assert text.index('duet_sv_tags_device(') > at and text.index('duet_sv_tags_host(') > at
    assert '#define DUET_ABI_VERSION 1\n' in text
    assert 'duet_sv_tags_device' in _lib.EXPORTS and 'duet_sv_tags_host' in _lib.EXPORTS
    proto = re.search(r'duet_sv_tags_device\((.*?)\);', text, flags=re.S).group(1)
    assert len(proto.split(',')) == 9                                          # ctx, prob, three settings, three outputs, stream


def test_library_exports_the_two_entries():
    import __graft_entry__
    __graft_entry__.build()
    out = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    names = set(l.split()[-1] for l in out.splitlines() if l.split())
    assert {'duet_sv_tags_device', 'duet_sv_tags_host'} <= names
    assert not any('svtags' in n or n.startswith('st_') for n in names)         # nothing else of the unit is visible
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'duet_sv_tags_host')
    assert len(_lib.load().duet_sv_tags_device.argtypes) == 9 and len(_lib.load().duet_sv_tags_host.argtypes) == 8


# ---- flags ---------------------------------------------------------------------------------------------------------------------------

def test_flags_and_refusals(monkeypatch, tmp_path):
    from duet_amd import cli, utils
    from duet_amd.sv_phasing import sv_phasing
    from duet_amd.svim_mode import sv_phasing_from_bams
    parse = lambda *argv: utils.build_parser().parse_args(['in.bam', 'ref.fa', 'out'] + list(argv))
    a = parse()
    assert a.vote_sv_tags is False and a.sv_tag_min is None and a.sv_tag_pc is None
    a = parse('--vote_sv_tags', '--sv_tag_min', '3', '--sv_tag_pc', '8100')
    assert a.vote_sv_tags is True and a.sv_tag_min == 3 and a.sv_tag_pc == 8100
    with pytest.raises(SystemExit):
        parse('--vote_sv_tags', '--sv_tag_min', 'two')
    assert sv_tags.check_settings(True, None, None) == (1, 0) and sv_tags.check_settings(False, None, None) is None
    out = str(tmp_path / 'never')
    one_gpu = '--vote_sv_tags works on the single-GPU path only'
    cases = ((['--vote_sv_tags', '--gpus', '2'], None, one_gpu),
             (['--vote_sv_tags', '-b', 'svim-gpu', '--gpus', '3'], None, one_gpu),
             (['--vote_sv_tags'], '1', one_gpu),
             (['--vote_sv_tags', '-b', 'svim-gpu'], '1', one_gpu),
             (['--vote_sv_tags', '--join_ps'], None, '--vote_sv_tags and --join_ps do not work together'),
             (['--sv_tag_min', '2'], None, '--sv_tag_min and --sv_tag_pc need --vote_sv_tags'),
             (['--sv_tag_pc', '2'], None, '--sv_tag_min and --sv_tag_pc need --vote_sv_tags'),
             (['--vote_sv_tags', '--sv_tag_min', '0'], None, '--sv_tag_min takes an integer >= 1'),
             (['--vote_sv_tags', '--sv_tag_pc', str((1 << 30) - 2), '-b', 'svim-gpu'], None, '--sv_tag_pc takes an integer in 0 ..'),
             (['--vote_sv_tags', '--sv_tag_pc', '-1'], None, '--sv_tag_pc takes an integer in 0 ..'))
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
        with pytest.raises(ValueError, match='vote_sv_tags: single-GPU path only'):
            fn(*args, gpus=2, vote_sv_tags=True)
        with pytest.raises(ValueError, match='vote_sv_tags: not together with join_ps'):
            fn(*args, vote_sv_tags=True, join_ps=True)
        with pytest.raises(ValueError, match='sv_tag_min: an integer >= 1'):
            fn(*args, vote_sv_tags=True, sv_tag_min=0)
        with pytest.raises(ValueError, match='sv_tag_pc: an integer in 0'):
            fn(*args, vote_sv_tags=True, sv_tag_pc=(1 << 30) - 2)
        with pytest.raises(ValueError, match='need vote_sv_tags'):
            fn(*args, sv_tag_min=2)
        monkeypatch.setenv('DUET_FORCE_RANKS', '1')
        with pytest.raises(ValueError, match='vote_sv_tags: single-GPU path only'):
            fn(*args, vote_sv_tags=True)
        monkeypatch.delenv('DUET_FORCE_RANKS', raising=False)
    assert not os.path.exists(out)


def test_flag_is_refused_where_the_native_ingest_declines(monkeypatch, tmp_path):
    from duet_amd import sv_phasing as sp
    home = str(tmp_path)
    os.makedirs(home + '/sv_calling')
    os.makedirs(home + '/snp_phasing')
    monkeypatch.setenv('DUET_NATIVE_INGEST', '0')
    with pytest.raises(RuntimeError, match='--vote_sv_tags needs the native ingest'):
        sp._native(home, 50, 2, 4, False, home + '/sv_calling/variants.vcf', home + '/phased_sv.vcf', None, sv_tags=(1, 0))
    with pytest.raises(RuntimeError, match='--vote_sv_tags need the native ingest'):
        sp._native_thresholds(home, 50, 2, 4, False, home + '/sv_calling/variants.vcf', home + '/phased_sv.vcf', None, None,
                              sv_tags=(1, 0))
    assert sorted(os.listdir(home)) == ['snp_phasing', 'sv_calling']


def test_report_and_log_line():
    text = sv_tags.report_text(['chr1', 'chr2'], [0, 0, 1], [10, 20, 30], [50, 60, 70], [1, 3, 6], [0, 1, 2], [0, 7, 9], [1, 1, 3], [7, 7, 9])
    assert text == 'chr1\t10\t50\tgained\t.\t.\t1|0\t7\nchr2\t30\t70\tto_hom\t0|1\t9\t1|1\t9\n'
    assert sv_tags.report_header() == 'CHROM\tPOS\tSVLEN\tCHANGE\tHP\tPS\tHP_NEW\tPS_NEW\n'
    line = sv_tags.summary_text((5, 3, 1), [4, 1, 0, 2, 0, 0, 1, 0])
    assert line == '5 marks untagged, 3 marks given, 1 marks own_only; none 4, gained 1, lost 0, same 2, to_het 0, to_hom 1, other 0'
    assert sv_tags.path_vcf('o') == 'o/phased_sv.sv_tags.vcf' and sv_tags.path_report('o') == 'o/phased_sv.sv_tags_report.tsv'


# ---- the unit's compile remarks ------------------------------------------------------------------------------------------------------

HIPCC = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)
OWN = ('st_count', 'st_owner', 'st_owner_check', 'st_keys', 'st_runs', 'st_reduce', 'st_derive', 'st_iota')


@pytest.mark.skipif(HIPCC is None, reason='hipcc not found')
def test_svtags_kernels_are_integer_only_without_scratch_or_calls(tmp_path):
    csrc = os.path.join(REPO, 'duet_amd', 'csrc')
    asm = str(tmp_path / 'duet_svtags.s')
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fvisibility=hidden',
           '-Wno-unused-function', '-I' + os.path.join(REPO, 'include'), '--cuda-device-only', '-S',
           '-Rpass-analysis=kernel-resource-usage', os.path.join(csrc, 'duet_svtags.hip'), '-o', asm]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    found = re.findall(r'Function Name: (\S+) \[.*?\n(?:.*\n){0,8}?.*ScratchSize \[bytes/lane\]: (\d+)', r.stderr)
    kernels = {n: int(v) for n, v in found}
    for name in OWN:
        assert sum(1 for n in kernels if re.search(r'\d%s[A-Z]' % name, n)) == 1, (name, sorted(kernels))
    assert len(kernels) > len(OWN) and all(v == 0 for v in kernels.values()), kernels      # the shared sort and scans included
    with open(asm) as f:
        code = [ln.split(';')[0] for ln in f if ln.startswith('\t') and not ln.startswith('\t.')]
    assert len(code) > 100
    assert not any('s_swappc' in ln or 's_call' in ln for ln in code)
    assert not any(re.search(r'_f(16|32|64)\b', ln) for ln in code), [ln for ln in code if re.search(r'_f(16|32|64)\b', ln)][:5]


# ---- the CPU condition: the feature matters on the project's own problems -------------------------------------------------------------

@pytest.mark.parametrize('seed', sorted(K.PINNED))
def test_the_reference_gains_calls_through_the_oracle(seed):
    """soa_fuzz.random_soa(seed) with a third of each contig's tag words turned to all-ones (K.SHARE), names = read indices: the
    reference's tags, then the C oracle on the expanded problem.  All of seeds 1..8 qualify at this share."""
    soa = K.untagged_soa(seed)
    r = K.second_run(soa, K.oracle_calls)                                      # (raises K.DivZero where either run divides by zero)
    counts, gained = K.PINNED[seed]
    assert r['counts'] == counts and r['codes'].count('gained') == gained
    assert gained >= 1 and counts[2] >= 1 and counts[1] + counts[2] <= counts[0]
    assert counts[0] == sum(1 for m in soa.mark_read if not S.has_tag(K.problem_of(soa, r['p0'], r['s0']), int(m)))
    assert 'relabelled' not in r['codes']


def test_all_of_seeds_one_to_eight_are_pinned():
    assert sorted(K.PINNED) == list(range(1, 9))
