# coding=utf-8
"""No GPU: the claim behind the line of the PC cap (include/duet_ef.h: duet_tune_cap_line_device; tests/cap_line_ref.py), on the
parameterised reference of tests/pc_cap_ref.py.  With x_1 < .. < x_D the distinct pc values of the marks that can vote (kept
candidate, tagged read, pc <= 2^30 - 3), the feature records are the same for every cap in [x_i, x_i+1), below x_1 they are those
of cap 0 and from x_D up those of x_D -- so the line x_1 .. x_D with 0 in front holds every behaviour of the cap.  Then the pick
rule, the bindings, the command-line arguments of the cap axis, and the resources of the new kernels."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from duet_amd import _lib, engine, tune
from tests import cap_line_ref as R
from tests import pc_cap_ref, soa_fuzz

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
CAP_MAX = R.CAP_MAX
S_THRES, R_THRES = 50, 3


def pooled(seed, n_pool, zero=True):
    """A fuzz problem of at most 200 candidates whose pc values come from a pool of n_pool <= 40 values that holds 0, 8100, 8101
    and 2^30 - 3; every third read of the one-PS candidates carries hap 3, some marks have no tag (soa_fuzz's absent marks), candidates fall to each of
    the three filters (svlen 45 .. 55 against 50, svread against 3, a sixth with './.') and a few carry two phase sets.
    zero=False: pc 0 stays in the pool but only on reads that mark no kept candidate, so x_1 > 0 and the line gets its 0 in front."""
    soa = soa_fuzz.random_soa(seed, n_contigs=3, cands_per_contig=(20, 60), reads_per_contig=(10, 80), empty_contig_rate=0,
                              no_seed_contig_rate=0)
    assert 0 < soa.n_cands <= 200
    rng = np.random.default_rng(seed)
    pool = np.unique(np.concatenate([[0, 8100, 8101, CAP_MAX], rng.integers(1, 20000, n_pool - 4)])).astype(np.uint64)
    assert len(pool) <= 40
    tag = soa.read_tag.copy()
    pc = pool[rng.integers(0, len(pool), len(tag))]
    if not zero:
        kept = (soa.cand_svlen >= S_THRES) & (soa.cand_svread >= R_THRES) & (soa.cand_gt_ok != 0)
        marks = np.concatenate([soa.mark_read[soa.cand_off[c]:soa.cand_off[c + 1]] for c in np.nonzero(kept)[0]])
        voting = np.unique(marks[marks != engine.MARK_ABSENT]).astype(np.int64)
        hit = voting[pc[voting] == 0]
        pc[hit] = pool[1 + hit % (len(pool) - 1)]
        pc[np.setdiff1d(np.arange(len(tag)), voting)[::2]] = 0
    hap = tag >> np.uint64(62)
    # (hap 3 on reads of one-PS candidates only: the oracle's multi-PS vote indexes its sums by a hap of 1 or 2)
    multi = set()
    for c in range(soa.n_cands):
        rs = [int(r) for r in soa.mark_read[soa.cand_off[c]:soa.cand_off[c + 1]] if r != engine.MARK_ABSENT]
        if len(set(int(tag[r]) & 0xFFFFFFFF for r in rs)) > 1:
            multi.update(rs)
    hap[[r for r in range(0, len(tag), 3) if r not in multi]] = 3
    soa.read_tag[:] = (hap << np.uint64(62)) | (pc << np.uint64(32)) | (tag & np.uint64(0xFFFFFFFF))
    return soa


class Under(object):
    """The reference's records of one problem, per cap."""

    def __init__(self, soa, s=S_THRES, r=R_THRES):
        self.soa, self.s, self.r, self.memo = soa, s, r, {}

    def __call__(self, cap):
        if cap not in self.memo:
            self.memo[cap] = pc_cap_ref.features(self.soa, self.s, self.r, cap)
        return self.memo[cap]


@pytest.mark.parametrize('seed,n_pool,zero', [(1, 40, True), (2, 12, True), (3, 25, True), (4, 20, False), (5, 40, False)])
def test_records_change_only_at_line_values(seed, n_pool, zero):
    soa = pooled(seed, n_pool, zero)
    under = Under(soa)
    full, D = R.line(R.participants(soa, S_THRES, R_THRES))
    xs = full[1:] if len(full) == D + 1 else full
    assert 3 <= D <= 40 and xs == sorted(set(xs))
    # the mixes are there: marks without a tag, hap 3 reads, each filter on its own, class 2
    kept = (soa.cand_svlen >= S_THRES, soa.cand_svread >= R_THRES, soa.cand_gt_ok != 0)
    for i in range(3):
        others = np.logical_and(kept[(i + 1) % 3], kept[(i + 2) % 3])
        assert np.any(~kept[i] & others), i
    assert np.any(soa.mark_read == engine.MARK_ABSENT) and np.any(soa.read_tag >> np.uint64(62) == 3)
    assert any(f['cls'] == 2 for f in under(CAP_MAX))
    for i, x in enumerate(xs):
        nxt = xs[i + 1] if i + 1 < len(xs) else None
        if nxt is None:
            assert under(CAP_MAX) == under(x)                # from x_D up
            if x < CAP_MAX:
                assert under(x + 1) == under(x)
            continue
        if x + 1 < nxt:
            assert under(x + 1) == under(x), (x, nxt)
        assert under(nxt - 1) == under(x), (x, nxt)
    assert (xs[0] > 0) == (not zero)                          # (both branches below are taken by some problem)
    if xs[0] > 0:                                             # below x_1: cap 0, which is why the line gets a 0 in front
        assert full[0] == 0 and full[1:] == xs and xs[0] >= 2
        for c in (1, xs[0] // 2, xs[0] - 1):
            assert under(c) == under(0), (c, xs[0])
        assert under(xs[0]) != under(0)                       # ... and x_1 itself is another problem
    else:
        assert full == xs
    # and the line is not idle: neighbours on it differ somewhere, hap 3 and all
    assert sum(1 for a, b in zip(full, full[1:]) if under(a) != under(b)) >= 2


def test_a_value_outside_the_kept_candidates_is_not_on_the_line():
    from tests.test_gpu_pc_cap import build, cand
    SAT = CAP_MAX + 1
    soa = build([[cand(10, [(1, 100, 7), (2, 300, 7), None]),
                  cand(20, [(1, 4000, 7)], svlen=49),               # dropped by -s
                  cand(30, [(2, 5000, 7)], svread=2),               # ... by -r
                  cand(40, [(1, 6000, 7)], gt=0),                   # ... by the genotype
                  cand(50, [(3, 700, 9), (1, SAT, 9), (2, CAP_MAX, 8)])]])
    assert R.soa_line(soa, 50, 3) == ([0, 100, 300, 700, CAP_MAX], 4, 5)
    assert R.soa_line(soa, 49, 3)[0] == [0, 100, 300, 700, 4000, CAP_MAX]
    assert R.soa_line(soa, 50, 2)[0] == [0, 100, 300, 700, 5000, CAP_MAX]
    soa.cand_gt_ok[3] = 1
    assert R.soa_line(soa, 50, 3)[0] == [0, 100, 300, 700, 6000, CAP_MAX]
    # the raw form takes every tagged mark
    assert R.raw_line(soa.mark_read, soa.read_tag)[0] == [0, 100, 300, 700, 4000, 5000, 6000, CAP_MAX]
    # ... and a value nobody kept votes under scores like its lower neighbour: the records do not move
    soa.cand_gt_ok[3] = 0
    under = Under(soa)
    assert under(3999) == under(4000) == under(6000) == under(CAP_MAX - 1) != under(CAP_MAX)
    assert under(1) == under(50) == under(99) == under(0) != under(100)    # x_1 = 100: below it, cap 0
    # no participant at all: the single value 0; pc 0 present: no second 0
    none = build([[cand(10, [None, (1, SAT, 7)])]])
    assert R.soa_line(none, 0, 0) == ([0], 0, 1)
    zero = build([[cand(10, [(1, 0, 7), (2, 5, 7)])]])
    assert R.soa_line(zero, 0, 0) == ([0, 5], 2, 2)


def test_pick_rule():
    full = [0] + [3 * i + 1 for i in range(11)]              # L = 12
    n = len(full)
    assert R.pick(full, 0) == full and R.pick(full, n) == full and R.pick(full, n + 1) == full
    assert R.pick(full, 2) == [full[0], full[-1]]
    assert R.pick(full, 3) == [full[0], full[5], full[-1]]    # floor(1 * 11 / 2) = 5
    got = R.pick(full, n - 1)
    assert len(got) == n - 1 and got[0] == full[0] and got[-1] == full[-1] and got == sorted(set(got))
    assert got == [full[i * (n - 1) // (n - 2)] for i in range(n - 1)]
    # the product needs 64 bits at 2^30 values: i * (L - 1) passes 2^32
    assert (3 << 29) * ((1 << 30) - 2) >= 1 << 32


def test_bindings_and_arguments():
    for sym in ('duet_tune_cap_line_device', 'duet_tune_cap_line_host', 'duet_svim_cap_line_device', 'duet_svim_cap_line_host'):
        assert sym in _lib.EXPORTS
    assert _lib.cap_line_room(0) == 1 and _lib.cap_line_room(10) == 11 and _lib.cap_line_room(10, 4) == 4
    assert _lib.cap_line_room(1 << 31) == (1 << 30) - 1 and _lib.cap_line_room(3, 100) == 4
    base = ['w', 't.vcf', '--fit', 'hp_f1']
    assert tune.parse_args(base).fit_cap is False and tune.parse_args(base + ['--fit_cap']).fit_cap is True
    assert tune.parse_args(base + ['--axes', 'pc_cap,c1_hapread_ratio']).axes == ['pc_cap', 'c1_hapread_ratio']
    assert tune._axes(['pc_cap', 'c1_hapread_ratio']) == ['pc_cap', tune.NAMES.index('c1_hapread_ratio')]
    assert tune._axes(None) == list(range(14))                # the default stays the 14 fields
    assert tune._axes(None, True) == list(range(14)) + ['pc_cap']
    assert tune._axes(['c0_min_sv_num'], True) == [0, 'pc_cap'] and tune._axes(['pc_cap', 'c0_min_sv_num'], True) == ['pc_cap', 0]
    with pytest.raises(ValueError):
        tune._axes(['pc_caps'])
    with pytest.raises(SystemExit):
        tune.parse_args(['w', 't.vcf', '--grid', 'g.json', '--fit_cap'])


def test_cap_line_kernels_use_no_scratch_and_make_no_call(tmp_path):
    csrc = os.path.join(REPO, 'duet_amd', 'csrc')
    asm = str(tmp_path / 'duet_tune_capline.s')
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fvisibility=hidden',
           '-Wno-unused-function', '-I' + os.path.join(REPO, 'include'), '--cuda-device-only', '-S',
           '-Rpass-analysis=kernel-resource-usage', os.path.join(csrc, 'duet_tune_capline.hip'), '-o', asm]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    found = re.findall(r'Function Name: (\S+) \[.*?\n(?:.*\n){0,8}?.*ScratchSize \[bytes/lane\]: (\d+)', r.stderr)
    # its own (cl_*) and the scan it instantiates from duet_prims.hip.h with its head-flag functor
    own = {n: int(v) for n, v in found if 'cl_' in n or 'LoadHead' in n}
    assert len(own) == 3 + 3, found
    assert all(int(v) == 0 for _, v in found), found
    with open(asm) as f:
        assert 's_swappc' not in f.read()


# ---- the cap axis of the fit, with a stub in place of the device -------------------------------------------------------------------

def stub_world(monkeypatch, line, hp_of, div_zero=()):
    """tune.fit over tests/test_pc_cap_host.py's stubs: the cap line is `line`, the features under a cap in div_zero report a
    division by zero, and the one vector scores call_hp = base_hp = hp_of(cap) of 8 calls."""
    from duet_amd import devmem
    from tests import test_pc_cap_host as T

    class Tune(T.StubTune):
        def cap_line(self, ctx, prob, max_values=0):
            vals = R.pick(line, max_values)
            return np.array(vals, dtype=np.uint32), len(line) - 1, len(vals) == len(line)      # (0 in front: D = L - 1)

        def set_line_vector(self, base):
            pass

        def sweep_line(self, ctx, n_cands, first, K):
            rec = np.zeros(K, dtype=_lib.COUNTS_DTYPE)
            for n in ('n_calls', 'call_tp', 'base_tp', 'call_gt', 'base_gt'):
                rec[n] = 8
            rec['n_groups'] = 1
            cap = ctx.calls[-1][2]
            rec['call_hp'] = rec['base_hp'] = hp_of(8100 if cap is None else cap)
            return rec

    class Ctx(T.StubCtx):
        def features_device(self, prob, out_ptr, stream=0, pc_cap=None):
            T.StubCtx.features_device(self, prob, out_ptr, stream, pc_cap)
            if pc_cap in div_zero:
                raise ZeroDivisionError('division by zero')

    soa = soa_fuzz.random_soa(0, n_contigs=1, cands_per_contig=(5, 5), empty_contig_rate=0)
    txt = dict(chrom=['chr1'] * 5, ref=['N'] * 5, alt=['<DEL>'] * 5, svtype=['DEL'] * 5)
    monkeypatch.setattr(tune, '_candidates', lambda *a: (soa, txt))
    monkeypatch.setattr(tune, 'candidate_keys', lambda *a: (np.zeros(5, dtype=np.uint32), np.zeros(5, dtype=np.uint32), 1))
    monkeypatch.setattr(tune, 'truth_side', lambda *a, **k: dict(n_base=8))
    monkeypatch.setattr(devmem, 'DeviceTune', Tune)
    monkeypatch.setattr(devmem, 'DeviceProblem', T.StubProblem)
    ctx = Ctx()
    monkeypatch.setattr(engine, 'default_context', lambda *a: ctx)
    return ctx


def hp(table):
    return lambda cap: table.get(cap, 1)


def test_the_cap_axis_moves_to_the_lowest_best_value_and_skips_a_division_by_zero(monkeypatch, tmp_path, capsys):
    line = [0, 100, 200, 300, 9000]
    ctx = stub_world(monkeypatch, line, hp({100: 5, 200: 5, 8100: 3, 300: 7}), div_zero=(300,))
    got = tune.fit('w', 't.vcf', 'hp_f1', axes=['pc_cap'], rounds=4, ctx=ctx)
    fit = got['fits'][0]
    assert fit['pc_cap'] == 100 and got['best'] is fit and 'pc_cap' not in fit['setting']
    rows = got['trace']
    assert [(r['round'], r['axis'], r['old'], r['new'], r['n_vec'], r['n_distinct'], r['exact']) for r in rows] == \
        [(1, 'pc_cap', 8100, 100, 5, 4, 1), (2, 'pc_cap', 100, 100, 5, 4, 1)]    # two values attain the best: the lower; then no move
    assert rows[0]['objective_before'] == 3 / 8 and rows[0]['objective_after'] == 5 / 8 == rows[0]['hp_f1'] == fit['objective']
    assert isinstance(rows[0]['old'], int) and isinstance(rows[0]['new'], int)
    # every value ascending, last the current cap, then once more for the cap it moved to; 300 divides by zero and never wins
    caps = [c[2] for c in ctx.calls]
    assert caps == [None] + line + [8100, 100] + line + [100]
    # a start from --pc_cap and from the start dict; the setting keeps the start
    del ctx.calls[:]
    got = tune.fit('w', 't.vcf', 'hp_f1', axes=['c1_max_ref_num'], fit_cap=True, rounds=1, ctx=ctx, pc_cap=(200, 9000))
    assert [(f['setting']['pc_cap'], f['pc_cap']) for f in got['fits']] == [(200, 200), (9000, 100)]
    assert [r['axis'] for r in got['fits'][1]['trace']] == ['c1_max_ref_num', 'pc_cap']
    del ctx.calls[:]
    got = tune.fit('w', 't.vcf', 'hp_f1', start={'c1_max_ref_num': 3, 'pc_cap': 9000}, axes=['pc_cap'], rounds=1, ctx=ctx, max_values=3)
    assert [c[2] for c in ctx.calls] == [None, 9000, 0, 200, 9000, 9000, 200]     # the start's features first; line entries 0, 2, 4
    assert got['best']['pc_cap'] == 200 and got['trace'][0]['exact'] == 0 and got['trace'][0]['n_vec'] == 3
    # without the axis nothing carries the key
    plain = tune.fit('w', 't.vcf', 'hp_f1', axes=['c1_max_ref_num'], rounds=1, ctx=ctx)
    assert 'pc_cap' not in plain['fits'][0] and all(r['axis'] != 'pc_cap' for r in plain['trace'])
    # the command line
    out, trace = str(tmp_path / 'best.json'), str(tmp_path / 'fit.tsv')
    tune.main(['w', 't.vcf', '--fit', 'hp_f1', '--axes', 'c1_max_ref_num', '--fit_cap', '--rounds', '2', '--out_vector', out, '--trace', trace])
    assert 'fitted pc_cap=100' in capsys.readouterr().out
    with open(out) as f:
        obj = json.load(f)
    assert list(obj) == list(tune.NAMES) + ['pc_cap'] and obj['pc_cap'] == 100
    assert tune.load_vector(out, with_cap=True)[1] == 100
    with open(trace) as f:
        cells = [ln.split('\t') for ln in f.read().splitlines()]
    at = cells[0].index('axis')
    cap_rows = [r for r in cells[1:] if r[at] == 'pc_cap']
    assert cap_rows and cap_rows[0][cells[0].index('old')] == '8100' and cap_rows[0][cells[0].index('new')] == '100'
    # a file with the key starts the next fit there
    tune.main(['w', 't.vcf', '--fit', 'hp_f1', '--axes', 'pc_cap', '--start', out, '--rounds', '1', '--out_vector', out])
    assert 'fitted pc_cap=100' in capsys.readouterr().out


def test_a_start_cap_whose_features_divide_by_zero_has_no_fit(monkeypatch):
    ctx = stub_world(monkeypatch, [0, 100], hp({100: 5}), div_zero=(700,))
    got = tune.fit('w', 't.vcf', 'hp_f1', axes=['pc_cap'], rounds=2, ctx=ctx, pc_cap=(700, 100))
    assert got['fits'][0]['vector'] is None and 'pc_cap' not in got['fits'][0] and got['best'] is got['fits'][1]
    got = tune.fit('w', 't.vcf', 'hp_f1', start={'pc_cap': 700}, axes=['pc_cap'], rounds=2, ctx=ctx)
    assert got['best'] is None and got['fits'][0]['vector'] is None
