# coding=utf-8
"""The evidence table without a GPU: its reference (tests/evidence_ref.py) tied to what is already pinned -- the phased_sv.vcf of
the golden work directories, the oracle's kept / eligible, the preds the unmodified predict_hp recorded -- the names the binding,
the header and the reference share, and the refusals of the flag."""
import collections
import os
import re
import shutil
import sys

import numpy as np
import pytest

from duet_amd import _lib, cli, sv_phasing, svim_mode, tune, utils
from oracle import ef_oracle as O
from tests import cap_line_ref, evidence_ref, tune_ref
from tests import helpers as H
from tests.test_c_oracle import materialise_bams

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_names_agree():
    assert _lib.EVIDENCE_COLUMNS == evidence_ref.COLUMNS and len(_lib.EVIDENCE_COLUMNS) == 17
    assert (_lib.LEAF_NO_SEED, _lib.LEAF_FILTERED) == (evidence_ref.NO_SEED, evidence_ref.FILTERED) == (0xFD, 0xFE)
    with open(os.path.join(REPO, 'include', 'duet_ef.h')) as f:
        text = f.read()
    body = re.search(r'#define DUET_EVIDENCE_COLUMNS(.*?)\}', text, flags=re.S).group(1)
    assert tuple(re.findall(r'"([A-Z0-9]+)"', body)) == _lib.EVIDENCE_COLUMNS
    assert int(re.search(r'#define DUET_TUNE_LEAF_NO_SEED (\w+)u', text).group(1), 16) == _lib.LEAF_NO_SEED
    assert int(re.search(r'#define DUET_TUNE_LEAF_FILTERED (\w+)u', text).group(1), 16) == _lib.LEAF_FILTERED
    for sym in ('duet_tune_leaves_device', 'duet_tune_leaves_host', 'duet_evidence_rows_device', 'duet_evidence_rows_host'):
        assert sym in _lib.EXPORTS
    assert _lib.evidence_header().decode() == evidence_ref.header()
    # the bound of the header comment: every number at its full width, the longest rule name
    f = np.zeros(1, dtype=_lib.FEATURE_DTYPE)
    for n in ('hap1', 'hap2', 'hap0', 'allhap', 'deg', 'svread', 'refread', 'ps'):
        f[n] = 0xFFFFFFFF
    f['t1'] = f['t2'] = 0xFFFFFFFFFFFFFFFF
    f['kept'] = f['eligible'] = 1
    f['cls'] = 255
    longest = max(range(18), key=lambda i: len(_lib.LEAF_NAMES[i]))
    assert len(evidence_ref.row_text('', 0xFFFFFFFF, '', 0xFFFFFFFF, f[0], longest, 3)) <= _lib.EVIDENCE_ROW_MAX
    assert _lib.evidence_bound(7, 5, 3) == 7 * (5 + 3 + 180)


def reference_table(home, s, r):
    soa, txt = tune._candidates(home, s, r, False, 2)
    want = tune_ref.oracle_features(soa, s, r)
    feat = cap_line_ref.records(want)
    leaf, pred = evidence_ref.leaves(feat, tune.vector())
    return soa, want, feat, leaf, pred, evidence_ref.rows_text(txt['chrom'], soa.cand_pos, txt['svtype'], soa.cand_svlen, feat, leaf, pred)


@pytest.mark.parametrize('name,src,params', H.full_cases(), ids=[c[0] for c in H.full_cases()])
def test_reference_on_the_golden_work_directories(name, src, params, tmp_path):
    """The called rows of the reference's table are the data rows of the pinned phased_sv.vcf, as a multiset of (CHROM, POS, HP,
    PS); filtered / no_seed are the oracle's kept / eligible."""
    home = str(tmp_path / name)
    shutil.copytree(src, home)
    materialise_bams(home)
    soa, want, feat, leaf, pred, text = reference_table(home, params['svlen_thres'], params['suppread_thres'])
    rows = [ln.split('\t') for ln in text.splitlines()]
    assert len(rows) == soa.n_cands and all(len(r) == len(evidence_ref.COLUMNS) for r in rows)
    col = {n: i for i, n in enumerate(evidence_ref.COLUMNS)}
    called = collections.Counter((r[col['CHROM']], r[col['POS']], r[col['HP']], r[col['PS']]) for r in rows if r[col['HP']] != '.')
    with open(os.path.join(src, 'phased_sv.vcf')) as f:
        data = [ln.split('\t') for ln in f.read().splitlines() if ln and not ln.startswith('#')]
    pinned = collections.Counter((d[0], d[1]) + tuple(d[-1].split(':')) for d in data)
    assert called == pinned
    for w, r, code in zip(want, rows, leaf):
        assert (r[col['RULE']] == 'filtered') == (not w['kept']) == (code == evidence_ref.FILTERED)
        assert (r[col['RULE']] == 'no_seed') == bool(w['kept'] and not w['eligible']) == (code == evidence_ref.NO_SEED)
        assert (r[col['CLASS']] == '.') == (not w['kept'])
        assert (r[col['PS']] == '.') == (not w['eligible']) == (r[col['VOTERS']] == '.')
        if r[col['HP']] != '.':
            assert w['eligible'] and code < 18


def test_reference_gives_the_recorded_pred(golden_dir):
    with np.load(os.path.join(golden_dir, 'kat_random.npz')) as zf:
        z = {k: zf[k] for k in zf.files}
    off = z['off']
    sets = [set(int(x) for x in z['oneps_val'][z['oneps_off'][s]:z['oneps_off'][s + 1]]) for s in range(len(z['oneps_off']) - 1)]
    n = len(z['cls'])
    feat = np.zeros(n, dtype=_lib.FEATURE_DTYPE)
    for i in range(n):
        cd = O.Candidate()
        cd.pos, cd.svread, cd.refread = int(z['pos'][i]), int(z['svread'][i]), int(z['refread'][i])
        a, b = off[i], off[i + 1]
        cd.marks = [(int(h), int(p), int(c)) if t else None
                    for t, h, p, c in zip(z['m_tagged'][a:b], z['m_hap'][a:b], z['m_ps'][a:b], z['m_pc'][a:b])]
        cls = int(z['cls'][i])
        hap1, hap2, hap0, allhap, t1, t2, ps = O.vote(cd, cls, sets[int(z['oneps_set'][i])])
        feat[i] = (t1, t2, hap1, hap2, hap0, allhap, len(cd.marks), cd.svread, cd.refread, int(ps), 1, 1, cls, 0, 0)
    leaf, pred = evidence_ref.leaves(feat, tune.vector())
    assert np.array_equal(pred, z['pred'].astype(np.uint8))
    nominal = np.array(_lib.LEAF_PRED)[leaf]
    assert np.all((pred == nominal) | ((nominal == 1) & (pred == 2)))
    text = evidence_ref.rows_text(['c'] * n, z['pos'], ['INS'] * n, np.zeros(n, dtype=np.int64), feat, leaf, pred)
    assert [ln.split('\t')[-1] for ln in text.splitlines()] == [evidence_ref.HP_TEXT[int(p)] for p in z['pred']]
    assert [ln.split('\t')[7] for ln in text.splitlines()] == [_lib.LEAF_NAMES[int(x)] for x in leaf]


def test_states_of_the_reference():
    feat = np.zeros(3, dtype=_lib.FEATURE_DTYPE)
    feat['deg'], feat['svread'], feat['refread'] = 4, 9, 0
    feat['kept'] = (0, 1, 1)
    feat['eligible'] = (0, 0, 1)
    leaf, pred = evidence_ref.leaves(feat, tune.vector())
    assert leaf.tolist() == [evidence_ref.FILTERED, evidence_ref.NO_SEED, 0] and pred.tolist() == [0, 0, 3]
    text = evidence_ref.rows_text(['a', 'b', 'c'], [1, 2, 3], ['INS', '', 'DEL'], [5, 6, 7], feat, leaf, pred)
    assert text == ('a\t1\tINS\t5\t9\t0\t4\tfiltered\t.\t.\t.\t.\t.\t.\t.\t.\t.\n'
                    'b\t2\t\t6\t9\t0\t4\tno_seed\t0\t.\t.\t.\t.\t.\t.\t.\t.\n'
                    'c\t3\tDEL\t7\t9\t0\t4\tc0_call\t0\t0\t0\t0\t0\t0\t0\t0\t1|1\n')
    with pytest.raises(IndexError):
        evidence_ref.rule_text(18)


# ---- the flag ---------------------------------------------------------------------------------------------------------------------

def test_command_line_argument():
    duet = ['in.bam', 'ref.fa', 'out']
    assert utils.build_parser().parse_args(duet).write_evidence is False
    assert utils.build_parser().parse_args(duet + ['--write_evidence']).write_evidence is True
    assert utils.build_parser().parse_args(duet + ['--write_evidence', '-b', 'svim-gpu', '--pc_cap', '2400']).write_evidence is True


@pytest.mark.parametrize('how', ['gpus', 'ranks'])
def test_the_sharded_paths_refuse_the_flag_before_anything_is_opened(tmp_path, monkeypatch, how):
    home = str(tmp_path / 'never_made')
    gpus = 2 if how == 'gpus' else 1
    if how == 'ranks':
        monkeypatch.setenv('DUET_FORCE_RANKS', '1')
    else:
        monkeypatch.delenv('DUET_FORCE_RANKS', raising=False)
    with pytest.raises(ValueError, match='evidence: single-GPU path only'):
        sv_phasing.sv_phasing(home, 50, 2, 4, False, 0, gpus, evidence=True)
    with pytest.raises(ValueError, match='evidence: single-GPU path only'):
        svim_mode.sv_phasing_from_bams(home, 50, 2, 4, False, 0.9, 0, gpus, evidence=True)
    # the command: refused before the inputs are looked at and before the output directory is made
    for caller in ([], ['-b', 'svim-gpu']):
        monkeypatch.setattr(sys, 'argv', ['duet', str(tmp_path / 'no.bam'), str(tmp_path / 'no.fa'), home, '--write_evidence',
                                          '--gpus', str(gpus)] + caller)
        with pytest.raises(SystemExit) as e:
            cli.main(None)
        assert '--write_evidence' in str(e.value) and 'single-GPU' in str(e.value)
    assert not os.path.exists(home)


def test_an_input_the_native_ingest_declines_is_refused_before_anything_is_written(tmp_path, monkeypatch):
    home = str(tmp_path / 'w')
    os.makedirs(home)
    monkeypatch.delenv('DUET_FORCE_RANKS', raising=False)
    monkeypatch.setattr(sv_phasing.engine, 'default_context', lambda device=0: None)
    monkeypatch.setattr(sv_phasing, 'load_native', lambda *a, **k: (None, []))
    with pytest.raises(RuntimeError, match='--write_evidence need the native ingest'):
        sv_phasing.sv_phasing(home, 50, 2, 4, False, evidence=True)
    assert os.listdir(home) == []


def test_an_input_without_a_string_pool_is_refused_before_the_output_file_is_created(tmp_path, monkeypatch):
    import types
    home = str(tmp_path / 'w')
    os.makedirs(home)
    closed = []
    ing = types.SimpleNamespace(soa=types.SimpleNamespace(n_cands=3), rows=lambda: None, close=lambda: closed.append(1))
    monkeypatch.delenv('DUET_FORCE_RANKS', raising=False)
    monkeypatch.setattr(sv_phasing.engine, 'default_context', lambda device=0: None)
    monkeypatch.setattr(sv_phasing, 'load_native', lambda *a, **k: (ing, []))
    with pytest.raises(RuntimeError, match='--write_evidence: the native ingest has no string pool'):
        sv_phasing.sv_phasing(home, 50, 2, 4, False, evidence=True)
    assert os.listdir(home) == [] and closed == [1]


def test_the_flag_takes_the_thresholds_route_with_the_default_vector(tmp_path, monkeypatch):
    """cli.main up to the last stage, which is replaced: what it is called with."""
    from duet_amd import stages
    seen = []
    for name in ('snp_calling', 'sv_calling', 'snp_phasing'):
        monkeypatch.setattr(stages, name, lambda *a: None)
    monkeypatch.setattr(cli, 'check_envs', lambda *a: None)
    monkeypatch.setattr(cli, 'set_logging', lambda *a: None)
    monkeypatch.setattr(cli.engine, 'default_context', lambda device=0: None)
    monkeypatch.setattr(cli, 'sv_phasing', lambda *a: seen.append(a))
    monkeypatch.delenv('DUET_FORCE_RANKS', raising=False)
    home = str(tmp_path / 'out')
    for extra, want_cap, want_flag in ((['--write_evidence'], None, True), (['--write_evidence', '--pc_cap', '2400'], 2400, True),
                                       ([], None, False)):
        monkeypatch.setattr(sys, 'argv', ['duet', 'in.bam', 'ref.fa', home] + extra)
        cli.main(None)
        args = seen.pop()
        assert args[-1] is want_flag and args[-2] == want_cap
        if want_flag:
            assert np.array_equal(args[-3], tune.vector())
        else:
            assert args[-3] is None
