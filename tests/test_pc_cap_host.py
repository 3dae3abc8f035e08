# coding=utf-8
"""The PC cap as a run parameter, without a GPU: the parameterised reference (tests/pc_cap_ref.py) tied to the unpatched oracle
through demoted PC tags, the command lines and their refusals, load_vector's optional 15th key, the row and column shape of
sweep_settings with a stub in place of the device, and the resources of the new kernels."""
import functools
import json
import os
import re
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

from duet_amd import _lib, cli, devmem, engine, sv_phasing, svim_mode, tune, utils
from tests import pc_cap_ref, soa_fuzz, tune_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
CAP_MAX = (1 << 30) - 3


# ---- the reference ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fuzz(seed):
    soa = soa_fuzz.random_soa(seed, n_contigs=4)
    return soa, tune_ref.oracle_features(soa, 0, 0)


@pytest.mark.parametrize('cap', [0, 300, 972, 2400, 8099])
@pytest.mark.parametrize('seed', range(6))
def test_a_cap_is_the_oracle_on_demoted_tags(seed, cap):
    """features(soa, cap) == the unpatched oracle on the problem whose pc values in (cap, 8100] read 8101, record for record;
    and the cap changes records, so a reference that ignored it would fail here."""
    soa, at_8100 = fuzz(seed)
    got = pc_cap_ref.features(soa, 0, 0, cap)
    from oracle import ef_oracle
    assert ef_oracle.PC_MAX == 8100                                       # (restored)
    want = tune_ref.oracle_features(pc_cap_ref.demote(soa, cap), 0, 0)
    assert got == want
    differ = sum(1 for a, b in zip(got, at_8100) if a != b)
    print('seed %d cap %d: %d of %d records differ from cap 8100' % (seed, cap, differ, len(got)))
    assert differ > 0
    assert pc_cap_ref.features(soa, 0, 0, 8100) == at_8100


def test_the_reference_restores_the_constant_when_the_oracle_raises():
    from oracle import ef_oracle
    with pytest.raises(AttributeError):
        pc_cap_ref.features(None, 0, 0, 5)
    assert ef_oracle.PC_MAX == 8100


# ---- arguments --------------------------------------------------------------------------------------------------------------------

def test_the_new_symbols_are_bound():
    for sym in ('duet_ef_features_cap_device', 'duet_ef_features_cap_host', 'duet_svim_features_cap_device', 'duet_svim_features_cap_host'):
        assert sym in _lib.EXPORTS
    assert (_lib.PC_MAX, _lib.PC_CAP_MAX) == (8100, CAP_MAX)


def test_command_line_arguments():
    base = ['w', 't.vcf', '--grid', 'g.json']
    assert tune.parse_args(base).pc_cap is None
    assert tune.parse_args(base + ['--pc_cap', '4000,8100,12000']).pc_cap == [4000, 8100, 12000]
    assert tune.parse_args(base + ['--pc_cap', '0,%d' % CAP_MAX]).pc_cap == [0, CAP_MAX]
    assert tune.parse_args(['w', 't.vcf', '--fit', 'hp_f1', '--pc_cap', '2400']).pc_cap == [2400]
    duet = ['in.bam', 'ref.fa', 'out']
    assert utils.build_parser().parse_args(duet).pc_cap is None
    assert utils.build_parser().parse_args(duet + ['--pc_cap', '2400']).pc_cap == 2400
    assert utils.build_parser().parse_args(duet + ['--pc_cap', str(CAP_MAX), '-b', 'svim-gpu']).pc_cap == CAP_MAX
    for bad in ('-1', str(CAP_MAX + 1), '8100.5', 'x', ''):
        with pytest.raises(SystemExit):
            tune.parse_args(base + ['--pc_cap', bad])
        with pytest.raises(SystemExit):
            utils.build_parser().parse_args(duet + ['--pc_cap', bad])
    for bad in ('8100,', '8100,-1', '1,%d' % (CAP_MAX + 1), '1,2.0'):
        with pytest.raises(SystemExit):
            tune.parse_args(base + ['--pc_cap', bad])


def test_python_arguments():
    assert [_lib.check_pc_cap(v) for v in (None, 0, 8100, np.uint32(7), CAP_MAX)] == [None, 0, 8100, 7, CAP_MAX]
    for bad in (-1, CAP_MAX + 1, 1 << 32, 8100.0, '8100', True, [8100]):
        with pytest.raises(ValueError):
            _lib.check_pc_cap(bad)
    v = tune.vector()[None, :]
    for bad in ((), (-1,), (8100, CAP_MAX + 1), (8100.0,), (None,)):
        with pytest.raises(ValueError):
            tune.sweep_settings('no_such_dir', 'no_such.vcf', v, pc_cap=bad)
        with pytest.raises(ValueError):
            tune.fit('no_such_dir', 'no_such.vcf', pc_cap=bad)


def test_features_path_carries_the_cap():
    assert tune.features_path('d/f.tsv', dict(pc_cap=2400, svlen_thres=30, suppread_thres=2)) == 'd/f.s30.r2.p2400.tsv'
    assert tune.features_path('f', dict(cluster_max_distance=0.5, svlen_thres=30, suppread_thres=2, pc_cap=0)) == 'f.c0.5.s30.r2.p0'
    assert tune.features_path('d/f.tsv', dict(svlen_thres=30, suppread_thres=2)) == 'd/f.s30.r2.tsv'


def test_load_vector_with_and_without_the_cap(tmp_path):
    path = str(tmp_path / 'v.json')

    def put(obj):
        with open(path, 'w') as f:
            json.dump(obj, f)

    put({'c1_max_ref_num': 3})
    want = tune.vector({'c1_max_ref_num': 3})
    got = tune.load_vector(path)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    vec, cap = tune.load_vector(path, with_cap=True)
    assert np.array_equal(vec, want) and cap is None
    put({'c1_max_ref_num': 3, 'pc_cap': 2400})
    assert np.array_equal(tune.load_vector(path), want)                    # every caller of before: the 14 values
    vec, cap = tune.load_vector(path, with_cap=True)
    assert np.array_equal(vec, want) and cap == 2400
    put(dict(zip(tune.NAMES, _lib.TUNE_DEFAULTS), pc_cap=0))
    assert tune.load_vector(path, with_cap=True)[1] == 0
    for bad in (-1, CAP_MAX + 1, 2400.5, '2400', True):
        put({'pc_cap': bad})
        with pytest.raises(ValueError, match='pc_cap'):
            tune.load_vector(path)
    put({'pc_cap': 2400, 'no_such_threshold': 1})
    with pytest.raises(ValueError, match='unknown'):
        tune.load_vector(path, with_cap=True)


@pytest.mark.parametrize('how', ['gpus', 'ranks'])
def test_the_sharded_paths_refuse_the_cap_before_anything_is_opened(tmp_path, monkeypatch, how):
    home = str(tmp_path / 'never_made')
    gpus = 2 if how == 'gpus' else 1
    if how == 'ranks':
        monkeypatch.setenv('DUET_FORCE_RANKS', '1')
    else:
        monkeypatch.delenv('DUET_FORCE_RANKS', raising=False)
    with pytest.raises(ValueError, match='pc_cap: single-GPU path only'):
        sv_phasing.sv_phasing(home, 50, 2, 4, False, 0, gpus, None, 2400)
    with pytest.raises(ValueError, match='pc_cap: single-GPU path only'):
        svim_mode.sv_phasing_from_bams(home, 50, 2, 4, False, 0.9, 0, gpus, True, None, 2400)
    for bad in (-1, CAP_MAX + 1, 2400.0):
        with pytest.raises(ValueError, match='pc_cap'):
            sv_phasing.sv_phasing(home, 50, 2, 4, False, 0, 1, None, bad)
        with pytest.raises(ValueError, match='pc_cap'):
            svim_mode.sv_phasing_from_bams(home, 50, 2, 4, False, 0.9, 0, 1, False, None, bad)
    # the command: refused before the inputs are looked at and before the output directory is made
    for caller in ([], ['-b', 'svim-gpu']):
        monkeypatch.setattr(sys, 'argv', ['duet', str(tmp_path / 'no.bam'), str(tmp_path / 'no.fa'), home, '--pc_cap', '2400',
                                          '--gpus', str(gpus)] + caller)
        with pytest.raises(SystemExit) as e:
            cli.main(None)
        assert '--pc_cap' in str(e.value) and 'single-GPU' in str(e.value)
    assert not os.path.exists(home)


# ---- rows and columns, with a stub in place of the device ----------------------------------------------------------------------

class StubTune(object):
    def __init__(self, n_max, base, refdist, ratio, vectors, device='cuda:0'):
        self.K = len(vectors)
        self.feat = types.SimpleNamespace(data_ptr=lambda: 0)

    def set_candidates(self, *a):
        pass

    def stream(self):
        return 0

    def build(self, ctx, n_cands, result=None, truth=None):
        pass

    def sweep(self, ctx, n_cands):
        return np.zeros(self.K, dtype=_lib.COUNTS_DTYPE)

    def features_host(self, n_cands):
        return np.zeros(n_cands, dtype=_lib.FEATURE_DTYPE)

    # (the fit: a line of one vector; the counts say that the features of cap 8100 phase more calls rightly than any other's)
    def line(self, ctx, n_cands, base, axis, max_values=0):
        return 1, 0

    def line_value(self, i, axis):
        return 0.0

    def sweep_line(self, ctx, n_cands, first, K):
        rec = np.zeros(K, dtype=_lib.COUNTS_DTYPE)
        for n in ('n_calls', 'n_groups', 'call_tp', 'base_tp', 'call_gt', 'base_gt', 'call_hp', 'base_hp'):
            rec[n] = 2
        rec['n_groups'] = 1
        if ctx.calls[-1][2] != 8100:
            rec['call_hp'] = rec['base_hp'] = 1
        return rec


class StubProblem(object):
    def __init__(self, soa, svlen_thres, suppread_thres, device='cuda:0'):
        self.problem = types.SimpleNamespace(svlen_thres=svlen_thres, suppread_thres=suppread_thres)


class StubCtx(object):
    device_id = 0

    def __init__(self):
        self.calls = []

    def features_device(self, prob, out_ptr, stream=0, pc_cap=None):
        self.calls.append((prob.svlen_thres, prob.suppread_thres, pc_cap))


@pytest.fixture
def stubbed(monkeypatch):
    soa = soa_fuzz.random_soa(0, n_contigs=1, cands_per_contig=(5, 5), empty_contig_rate=0)
    txt = dict(chrom=['chr1'] * 5, ref=['N'] * 5, alt=['<DEL>'] * 5, svtype=['DEL'] * 5)
    monkeypatch.setattr(tune, '_candidates', lambda *a: (soa, txt))
    monkeypatch.setattr(tune, 'candidate_keys', lambda *a: (np.zeros(5, dtype=np.uint32), np.zeros(5, dtype=np.uint32), 1))
    monkeypatch.setattr(tune, 'truth_side', lambda *a, **k: dict(n_base=3))
    monkeypatch.setattr(devmem, 'DeviceTune', StubTune)
    monkeypatch.setattr(devmem, 'DeviceProblem', StubProblem)
    ctx = StubCtx()
    monkeypatch.setattr(engine, 'default_context', lambda *a: ctx)
    return ctx


def test_rows_gain_a_leading_column_only_with_the_argument(stubbed):
    vecs = np.stack([tune.vector(), tune.vector({'c1_max_ref_num': 3})])
    rows = tune.sweep_settings('w', 't.vcf', vecs, (30, 50), (2, 3), ctx=stubbed)
    assert all('pc_cap' not in r for r in rows) and list(rows[0])[:2] == ['svlen_thres', 'suppread_thres']
    assert stubbed.calls == [(s, r, None) for s in (30, 50) for r in (2, 3)]
    del stubbed.calls[:]
    seen = []
    rows = tune.sweep_settings('w', 't.vcf', vecs, (30, 50), (2, 3), ctx=stubbed, pc_cap=(9720, 2400, 8100),
                               on_features=lambda setting, cands: seen.append(dict(setting)))
    # the cap is the innermost setting; its column leads
    order = [(s, r, p) for s in (30, 50) for r in (2, 3) for p in (9720, 2400, 8100)]
    assert stubbed.calls == order
    assert [(r['svlen_thres'], r['suppread_thres'], r['pc_cap']) for r in rows] == [o for o in order for _ in vecs]
    assert all(list(r)[:3] == ['pc_cap', 'svlen_thres', 'suppread_thres'] for r in rows)
    assert list(rows[0])[3:3 + len(tune.NAMES)] == list(tune.NAMES)
    assert seen == [dict(pc_cap=p, svlen_thres=s, suppread_thres=r) for s, r, p in order]
    # one cap is a list of one
    del stubbed.calls[:]
    rows = tune.sweep_settings('w', 't.vcf', vecs, ctx=stubbed, pc_cap=8100)
    assert stubbed.calls == [(50, 2, 8100)] and [r['pc_cap'] for r in rows] == [8100, 8100]


def test_the_command_writes_the_column_only_with_the_flag(stubbed, tmp_path, capsys):
    grid = str(tmp_path / 'g.json')
    with open(grid, 'w') as f:
        json.dump([{}, {'c1_max_ref_num': 3}], f)
    out = lambda name: str(tmp_path / name)
    tune.main(['w', 't.vcf', '--grid', grid, '--out', out('a.tsv')])
    tune.main(['w', 't.vcf', '--grid', grid, '--out', out('b.tsv'), '--pc_cap', '2400,8100', '--features', out('f.tsv')])
    tune.main(['w', 't.vcf', '--grid', grid, '--out', out('c.tsv'), '--pc_cap', '8100', '-s', '30,50'])
    capsys.readouterr()
    table = {}
    for name in 'abc':
        with open(out(name + '.tsv')) as f:
            table[name] = [ln.split('\t') for ln in f.read().splitlines()]
    assert table['a'][0] == list(tune.NAMES + tune.SCORES) and len(table['a']) == 3
    assert table['b'][0] == ['pc_cap'] + list(tune.NAMES + tune.SCORES)
    assert [r[0] for r in table['b'][1:]] == ['2400', '2400', '8100', '8100']
    assert table['c'][0] == ['pc_cap', 'svlen_thres', 'suppread_thres'] + list(tune.NAMES + tune.SCORES)
    assert [tuple(r[:3]) for r in table['c'][1:]] == [('8100', '30', '2')] * 2 + [('8100', '50', '2')] * 2
    assert os.path.exists(out('f.s50.r2.p2400.tsv')) and os.path.exists(out('f.s50.r2.p8100.tsv')) and not os.path.exists(out('f.tsv'))


def test_fit_takes_the_cap_as_a_setting_and_writes_the_best_one(stubbed, tmp_path, capsys):
    got = tune.fit('w', 't.vcf', 'hp_f1', axes=['c1_max_ref_num'], rounds=1, ctx=stubbed, pc_cap=(2400, 8100, 9720))
    assert [f['setting'] for f in got['fits']] == [dict(pc_cap=p, svlen_thres=50, suppread_thres=2) for p in (2400, 8100, 9720)]
    assert got['best']['setting']['pc_cap'] == 8100 and list(got['trace'][0])[0] == 'pc_cap'
    assert 'pc_cap' not in tune.fit('w', 't.vcf', 'hp_f1', axes=['c1_max_ref_num'], rounds=1, ctx=stubbed)['fits'][0]['setting']
    out, trace = str(tmp_path / 'best.json'), str(tmp_path / 'fit.tsv')
    tune.main(['w', 't.vcf', '--fit', 'hp_f1', '--axes', 'c1_max_ref_num', '--rounds', '1', '--pc_cap', '2400,8100,9720',
               '--out_vector', out, '--trace', trace])
    assert 'pc_cap=8100' in capsys.readouterr().out
    with open(out) as f:
        obj = json.load(f)
    assert list(obj) == list(tune.NAMES) + ['pc_cap'] and obj['pc_cap'] == 8100
    vec, cap = tune.load_vector(out, with_cap=True)                        # what duet --thresholds reads
    assert cap == 8100 and len(vec) == len(tune.NAMES)
    with open(trace) as f:
        rows = [ln.split('\t') for ln in f.read().splitlines()]
    assert rows[0][:3] == ['pc_cap', 'svlen_thres', 'suppread_thres'] and [r[0] for r in rows[1:]] == ['2400', '8100', '9720']
    # without the flag: the 14 keys of before
    tune.main(['w', 't.vcf', '--fit', 'hp_f1', '--axes', 'c1_max_ref_num', '--rounds', '1', '--out_vector', out])
    capsys.readouterr()
    with open(out) as f:
        assert list(json.load(f)) == list(tune.NAMES)


# ---- the kernels --------------------------------------------------------------------------------------------------------------------

def test_cap_kernels_use_no_scratch(tmp_path):
    csrc = os.path.join(REPO, 'duet_amd', 'csrc')
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fvisibility=hidden',
           '-Wno-unused-function', '-I' + os.path.join(REPO, 'include'), '--cuda-device-only', '-S',
           '-Rpass-analysis=kernel-resource-usage', os.path.join(csrc, 'duet_tune_cap.hip'), '-o', str(tmp_path / 'duet_tune_cap.s')]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    found = re.findall(r'Function Name: (\S+) \[.*?\n(?:.*\n){0,8}?.*ScratchSize \[bytes/lane\]: (\d+)', r.stderr)
    # its own (tc_*) and the scan it instantiates from duet_prims.hip.h with its head-flag functor
    kernels = {n: int(v) for n, v in found if 'tc_' in n or 'SeedHead' in n}
    assert len(kernels) == 3 + 3, found
    assert all(v == 0 for v in kernels.values()), kernels
