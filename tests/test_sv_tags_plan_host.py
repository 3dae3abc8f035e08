# coding=utf-8
"""The planned tags from other SVs and `tune --vote_sv_tags` without a GPU: the header against the bindings and the library's
symbols, the new unit's compile remarks, the flags and their refusals, and the CPU condition -- by the references alone, the tests
of tests/test_gpu_sv_tags_plan.py and tests/test_gpu_tune_sv_tags.py can tell per-vector tags from one vector's tags reused, and a
voted run from a plain one.  Every pinned number is recomputed here."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from duet_amd import _lib, tune
from tests import helpers as H
from tests import pc_cap_ref
from tests import sv_tags_cases as K
from tests import sv_tags_ref as S
from tests import tune_sv_tags_ref as T
from tests.test_gpu_fit_cap import pooled_workdir

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('duet_sv_tags_plan_device', 'duet_sv_tags_plan_host', 'duet_sv_tags_apply_device', 'duet_sv_tags_apply_host')


# ---- header, bindings, symbols -------------------------------------------------------------------------------------------------------

def test_header_declares_the_four_entries_under_one_section():
    with open(os.path.join(REPO, 'include', 'duet_ef.h')) as f:
        text = f.read()
    at = text.index('Tags from other SVs, planned (duet_svtags_plan.hip')
    end = text.index('Diagnostics: the shared device primitives')
    for name in ENTRIES:
        assert at < text.index(name + '(') < end and name in _lib.EXPORTS
    assert '#define DUET_ABI_VERSION 1\n' in text
    proto = lambda name: re.search(name + r'\((.*?)\);', text, flags=re.S).group(1).split(',')
    assert [len(proto(n)) for n in ENTRIES] == [8, 7, 7, 6]
    assert 'STRICTER' in text[at:end]                                          # the contradiction over the masked candidates is stated


def test_library_exports_the_four_entries():
    import __graft_entry__
    __graft_entry__.build()
    out = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    names = set(l.split()[-1] for l in out.splitlines() if l.split())
    assert set(ENTRIES) <= names
    assert not any('svtags_plan' in n or n.startswith('sp_') or n.startswith('sa_') for n in names)    # nothing else of the unit is visible
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'duet_sv_tags_apply_host')
    lib = _lib.load()
    assert [len(getattr(lib, n).argtypes) for n in ENTRIES] == [8, 7, 7, 6]


# ---- the unit's compile remarks ------------------------------------------------------------------------------------------------------

HIPCC = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)
OWN = ('sp_count', 'sp_owner', 'sp_owner_check', 'sp_keys', 'sp_runs', 'sp_records', 'sp_marks', 'sp_iota', 'sa_records', 'sa_marks')


@pytest.mark.skipif(HIPCC is None, reason='hipcc not found')
def test_plan_kernels_are_integer_only_without_scratch_or_calls(tmp_path):
    csrc = os.path.join(REPO, 'duet_amd', 'csrc')
    asm = str(tmp_path / 'duet_svtags_plan.s')
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fvisibility=hidden',
           '-Wno-unused-function', '-I' + os.path.join(REPO, 'include'), '--cuda-device-only', '-S',
           '-Rpass-analysis=kernel-resource-usage', os.path.join(csrc, 'duet_svtags_plan.hip'), '-o', asm]
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


# ---- flags ---------------------------------------------------------------------------------------------------------------------------

def test_flag_refusals_come_before_anything_is_read(tmp_path, capsys):
    never = str(tmp_path / 'never')                                            # (no such work directory, truth set or grid)
    base = [never, never + '.vcf']
    cases = ((['--grid', never, '--sv_tag_min', '2'], '--sv_tag_min and --sv_tag_pc need --vote_sv_tags'),
             (['--grid', never, '--sv_tag_pc', '5'], '--sv_tag_min and --sv_tag_pc need --vote_sv_tags'),
             (['--fit', 'hp_f1', '--vote_sv_tags'], "the second run's records move with the first run's calls"),
             (['--grid', never, '--vote_sv_tags', '--join_ps'], '--vote_sv_tags and --join_ps do not work together'),
             (['--grid', never, '--vote_sv_tags', '--sv_tag_min', '-1'], 'sv_tag_min'),
             (['--grid', never, '--vote_sv_tags', '--sv_tag_pc', str((1 << 30) - 2)], 'sv_tag_pc'))
    for argv, text in cases:
        with pytest.raises(SystemExit):
            tune.main(base + argv)
        assert text in capsys.readouterr().err
    grid = str(tmp_path / 'grid.json')
    with open(grid, 'w') as f:
        json.dump(T.GRID[:2], f)
    with pytest.raises(SystemExit, match='--features with --vote_sv_tags needs a grid of exactly one vector'):
        tune.main(base + ['--grid', grid, '--vote_sv_tags', '--features', never + '.tsv'])
    assert not os.path.exists(never) and not os.path.exists(never + '.tsv')
    a = tune.parse_args(base + ['--grid', grid, '--vote_sv_tags'])
    assert a.vote_sv_tags and a.sv_tag_min is None and a.sv_tag_pc is None
    assert tune._sv_tag_lists(True, None, None) == ([1], [0])                  # the product's defaults
    a = tune.parse_args(base + ['--grid', grid, '--vote_sv_tags', '--sv_tag_min', '0,1,2', '--sv_tag_pc', '0,4000'])
    assert (a.sv_tag_min, a.sv_tag_pc) == ([0, 1, 2], [0, 4000])
    # from Python
    for kw, text in ((dict(sv_tag_min=[1]), 'need vote_sv_tags'), (dict(sv_tag_pc=[0]), 'need vote_sv_tags'),
                     (dict(vote_sv_tags=True, join_min_sv=[2]), 'not together with join_ps'),
                     (dict(vote_sv_tags=True, sv_tag_min=[-1]), 'sv_tag_min'),
                     (dict(vote_sv_tags=True, sv_tag_pc=[(1 << 30) - 2]), 'sv_tag_pc'),
                     (dict(vote_sv_tags=True, on_features=lambda *a: None), 'exactly one vector')):
        with pytest.raises(ValueError, match=text):
            tune.sweep_settings(never, never + '.vcf', tune.expand_grid(T.GRID[:2]), **kw)
    assert tune.features_path('f.tsv', tune._lead(None, 50, 2, 8100, None, 1, 0)) == 'f.s50.r2.p8100.v1.q0.tsv'
    assert tune.features_path('f.tsv', tune._lead(None, 50, 2, None, 2)) == 'f.s50.r2.j2.tsv'   # without the flag: what it was


def test_a_setting_without_candidates_gets_the_plain_rows():
    """No candidate: nothing can be tagged and the second run is the first -- every sv_tag_min, 0 or not, gets the plain sweep's
    records with marks of 0, never nan rows; no plan is made (the stand-in source has none to give)."""
    K, seen = 2, []

    class Dt(object):
        K, VEC_BYTES, torch = 2, 8 * len(_lib.TUNE_NAMES), None

        def sweep(self, ctx, n):
            return np.zeros(K, dtype=_lib.COUNTS_DTYPE)

        def sweep_strata(self, ctx, n, p):
            return np.zeros((K, 2), dtype=_lib.COUNTS_DTYPE)

        def leaf_census(self, ctx, n, vectors=None, strata=None):
            return np.zeros((K, 1 if strata is None else 2, _lib.N_LEAVES), dtype=_lib.LEAF_COUNTS_DTYPE)

    class Src(object):
        ctx = None

        def host(self, dt):
            return dict(feat=np.zeros(0, dtype=_lib.FEATURE_DTYPE))
    vecs = tune.expand_grid(T.GRID[:2])
    for mins in ([0, 1, 2], [1]):
        del seen[:]
        runs = tune._sv_tag_runs(Src(), Dt(), 0, dict(svlen_thres=50), None, dict(holdout=dict()), vecs, (mins, [0, 5]), True,
                                 lambda lead, cands: seen.append((lead['sv_tag_min'], lead['sv_tag_pc'], len(cands['feat']))))
        assert sorted(runs) == [(m, q) for m in mins for q in (0, 5)] and sorted(seen) == [(m, q, 0) for m in mins for q in (0, 5)]
        for run in runs.values():
            assert not run['bad'].any() and not run['marks'].any() and run['marks'].shape == (K, 3)
            assert run['counts'].shape == (K,) and run['strata']['holdout'].shape == (K, 2)
            assert [names for _, names in run['leaf']] == [('all',), ('train', 'test')] and all(len(per) == K for per, _ in run['leaf'])


# ---- the condition, by the references alone --------------------------------------------------------------------------------------------

VEC_A = {'c1_twohap_sv_ratio_2': 0.7, 'c1_max_ref_num': 1000}


def calls_of(soa, vec, cap=8100):
    feat = pc_cap_ref.features(K.oracle_form(soa), 50, 2, cap)
    return T.calls(feat, vec)


@pytest.mark.parametrize('seed, n_cands', zip(range(1, 9), (22, 19, 20, 21, 28, 31, 7, 21)))
def test_per_vector_tags_differ_from_reused_tags_on_the_fuzz_seeds(seed, n_cands):
    """The second-run calls of VEC_A on its own tags differ from those made on the default vector's tags, on every seed, in
    n_cands candidates; no run divides by zero."""
    soa = K.untagged_soa(seed)
    a, d = tune.vector(VEC_A), tune.vector()
    second = {}
    for name, v in (('own', a), ('reused', d)):
        pred, ps = calls_of(soa, v)
        tags, _, _ = S.sv_tags(K.problem_of(soa, pred, ps))
        second[name], _ = calls_of(K.expanded_soa(soa, tags), a)
    assert sum(1 for x, y in zip(second['own'], second['reused']) if x != y) == n_cands


@pytest.fixture(scope='module')
def golden(tmp_path_factory):
    from tests.test_c_oracle import materialise_bams
    d = tmp_path_factory.mktemp('sv_tags_plan_golden')
    home = str(d / 'w')
    shutil.copytree(os.path.join(H.GOLDEN, 'cases', 'fuzz_cutesv_s2'), home)
    materialise_bams(home)
    w = T.world_of(home)
    w.write_truth2(str(d / 'truth.vcf'))
    return w


@pytest.fixture(scope='module')
def pooled(tmp_path_factory):
    d = tmp_path_factory.mktemp('sv_tags_plan_pooled')
    w = T.world_of(pooled_workdir(str(d / 'w'), 3, lone=(0, 2)))
    w.write_truth2(str(d / 'truth.vcf'))
    return w


MARKS = {'golden': {1: (747, 86, 30), 2: (747, 34, 15)}, 'pooled': {1: (488, 124, 30), 2: (488, 59, 23)}}
# (work dir, vector, sv_tag_min) -> the leading counts on its own tags, on the default vector's tags
OWN_AGAINST_REUSED = (('golden', {'c1_max_ref_num': 3, 'c0_min_sv_num': 2}, 1, (63,), (62,)),
                      ('golden', VEC_A, 2, (73,), (72,)),
                      ('pooled', {'c1_onehap_sv_ratio_hi': 0.6}, 1, (76,), (73,)),
                      ('pooled', VEC_A, 1, (74, 9, 55, 55, 45), (75, 9, 59, 59, 49)))


@pytest.mark.parametrize('which', ['golden', 'pooled'])
def test_a_voted_run_differs_from_a_plain_one_for_every_vector(which, request):
    w = request.getfixturevalue(which)
    for m, want in MARKS[which].items():
        assert w.tags(8100, tune.vector(), m)[1] == want
    for v in tune.expand_grid(T.GRID):
        plain, voted = w.counts(w.second(8100, v, 0)[0], v), w.counts(w.second(8100, v, 1)[0], v)
        assert plain is not None and voted is not None and plain.tobytes() != voted.tobytes()


@pytest.mark.parametrize('which, vec, m, own, reused', OWN_AGAINST_REUSED)
def test_own_tags_against_the_default_vectors_tags(which, vec, m, own, reused, request):
    w = request.getfixturevalue(which)
    v = tune.vector(vec)
    assert any(np.array_equal(v, g) for g in tune.expand_grid(T.GRID))          # the GPU tests' grid holds the vector
    got_own = w.counts(w.second(8100, v, m)[0], v)
    got_reused = w.counts(w.on_tags(8100, w.tags(8100, tune.vector(), m)[0]), v)
    names = _lib.COUNTS_NAMES[:len(own)]
    assert tuple(int(got_own[n]) for n in names) == own and tuple(int(got_reused[n]) for n in names) == reused
