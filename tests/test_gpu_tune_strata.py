# coding=utf-8
"""-m gpu: the stratified sweep (duet_tune_sweep_strata_*, duet_tune_strata_build_*; tune_decide_strata, tune_groups_strata,
tune_popcount_strata and tune_strata_of of duet_amd/csrc/duet_tune.hip): every word of every (vector, stratum)
record against tests/tune_strata_ref.py -- the masked re-run, which tests/test_tune_strata_host.py holds to the evaluator on
restricted files -- on feature records and truth arrays made by hand as in tests/test_gpu_tune_score_edges.py, then the command
line end to end.  Integer equality throughout."""
import json
import math

import numpy as np
import pytest

from duet_amd import _lib, synth, tune
from tests import helpers as H
from tests import tune_score_ref, tune_strata_ref
from tests.test_gpu_tune_grid import scoring_workdir, write_truth
from tests.test_gpu_tune_score_edges import (FLIP, IN, MATCHED, RAISES, SAME, WS_BUDGET, control, cycle, level_features, per_vec_words,
                                             random_features, random_truth, random_vectors, truth_arrays)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def strata_case(flags, group, local_uid, group_stratum, ids):
    """Truth arrays and strata from per-candidate (flags, group, local truth id) and per-group strata: stratum s owns ids[s] truth
    ids, numbered stratum-major from a multiple of 32; a MATCHED candidate of a stratum without ids loses the flag."""
    gs, ids = np.asarray(group_stratum, dtype=np.uint8), np.asarray(ids, dtype=np.int64)
    group = np.asarray(group, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum((ids + 31) // 32 * 32)])
    cs = gs[group] if len(group) else np.zeros(0, dtype=np.uint8)
    flags = np.asarray(flags, dtype=np.uint16).copy()
    flags[(ids[cs] == 0) & ((flags & MATCHED) != 0)] &= np.uint16(IN | RAISES)
    uid = off[cs] + np.asarray(local_uid, dtype=np.int64) % np.maximum(ids[cs], 1)
    truth = truth_arrays(flags, group, uid, len(gs), int(off[-1]))
    return truth, dict(n_strata=len(ids), cand_stratum=cs, group_stratum=gs, uid_off=off.astype(np.uint32))


def random_case(seed, C, S, n_groups=None, ids=None):
    rng = np.random.default_rng(seed)
    n_groups = n_groups or max(S, C // 7, 1)
    t = random_truth(seed + 1, C, n_groups, 1 << 20)
    ids = ids if ids is not None else rng.integers(0, 70, S)
    gs = rng.integers(0, S, n_groups)
    gs[:min(S, n_groups)] = rng.permutation(S)[:min(S, n_groups)]       # (every stratum owns a group when there are enough)
    return strata_case(t['cand_flags'], t['cand_group'], t['cand_uid'], gs, ids)


def check(ctx, feat, vecs, truth, strata, want=None):
    S = strata['n_strata']
    want = want if want is not None else tune_strata_ref.counts(feat, vecs, truth, strata['cand_stratum'], S)
    got = ctx.sweep_strata_host(feat, vecs, truth, strata)
    assert got.dtype == _lib.COUNTS_DTYPE and got.shape == (len(vecs), S) == want.shape
    for name in _lib.COUNTS_NAMES:
        bad = np.argwhere(got[name] != want[name])
        assert bad.size == 0, '%s differs at (vector, stratum) %s: %s, expected %s' % (
            name, bad[:5].tolist(), [int(got[name][tuple(b)]) for b in bad[:5]], [int(want[name][tuple(b)]) for b in bad[:5]])
    return want


# ---- shapes -----------------------------------------------------------------------------------------------------------------

def test_one_stratum_is_the_plain_sweep(ctx):
    C = 513
    feat = random_features(1, C)
    truth, strata = random_case(2, C, 1, ids=[200])
    assert truth['n_uid'] == 224 and strata['uid_off'].tolist() == [0, 224]
    vecs = random_vectors(3, 33)
    plain, _, _ = ctx.sweep_host(feat, vecs, truth)
    got = ctx.sweep_strata_host(feat, vecs, truth, strata)
    assert got.shape == (33, 1) and got[:, 0].tobytes() == plain.tobytes()              # all ten words of every record
    assert all(int(plain[n].max()) > 0 for n in _lib.COUNTS_NAMES if n != 'reserved')
    check(ctx, feat, vecs, truth, strata)


@pytest.mark.parametrize('C', [0, 1, 255, 256, 257, 513])
@pytest.mark.parametrize('S', [2, 3, 25, 64])
def test_shapes(ctx, S, C):
    feat = random_features(10 + C, C)
    truth, strata = random_case(100 * S + C, C, S)
    vecs = random_vectors(C + 2, 65)
    want = tune_strata_ref.counts(feat, vecs, truth, strata['cand_stratum'], S)
    if C >= 255:
        assert all(int(want[n].max()) > 0 for n in _lib.COUNTS_NAMES if n != 'reserved')
        assert int((want['n_calls'].max(axis=0) > 0).sum()) >= min(S, 20)              # the calls are spread over the strata
    for K in (0, 1, 31, 32, 33, 65):
        check(ctx, feat, vecs[:K], truth, strata, want[:K])


# ---- waves ------------------------------------------------------------------------------------------------------------------

def wave_mix(cand_stratum, S, levels=None, eligible=None, seed=4):
    """320 candidates (five waves), candidate c in stratum cand_stratum[c]; group = 4 * stratum + c % 4, every candidate matched."""
    cs = np.asarray(cand_stratum, dtype=np.int64)
    C = len(cs)
    rng = np.random.default_rng(seed)
    feat = level_features(np.full(C, 10) if levels is None else levels, 1 + np.arange(C) % 3, eligible)
    flags = (IN | MATCHED | rng.integers(0, 512, C)).astype(np.uint16)
    flags[rng.random(C) < 0.1] = IN | RAISES
    truth, strata = strata_case(flags, 4 * cs + np.arange(C) % 4, rng.integers(0, 40, C), np.repeat(np.arange(S), 4), np.full(S, 40))
    assert np.array_equal(strata['cand_stratum'], cs)
    return feat, truth, strata


MIXES = {
    'change_at_lane_1': (np.where(np.arange(320) % 64 < 1, 0, 1), 2),
    'change_at_lane_63': (np.where(np.arange(320) % 64 < 63, 0, 1), 2),
    'every_lane': (np.arange(320) % 7, 7),
    'three_strata_in_one_wave': (np.where(np.arange(320) < 64, 0, np.where(np.arange(320) < 100, 1, np.where(np.arange(320) < 120, 2, 3))), 4),
    'a_stratum_with_no_candidate': (np.where(np.arange(320) % 2, 3, 1), 5),
}


@pytest.mark.parametrize('name', sorted(MIXES))
def test_wave_mixes(ctx, name):
    cs, S = MIXES[name]
    feat, truth, strata = wave_mix(cs, S)
    want = check(ctx, feat, np.stack([control(0), control(100), tune.vector()]), truth, strata)
    assert want['n_calls'][0].sum() == 320 and not want['n_calls'][1].any()
    assert [int(x) for x in want['n_calls'][0]] == np.bincount(cs, minlength=S).tolist()


@pytest.mark.parametrize('t,lanes', [(60, [127]), (50, [127, 128])])
def test_a_wave_whose_only_call_is_in_lane_63_or_lane_0(ctx, t, lanes):
    L = np.full(320, 10)
    L[127], L[128] = 60, 50
    cs = np.arange(320) // 50                                            # strata change inside waves; 127 and 128 in stratum 2
    feat, truth, strata = wave_mix(cs, 7, levels=L)
    want = check(ctx, feat, np.stack([control(t), control(10)]), truth, strata)
    assert [int(x) for x in want['n_calls'][0]] == [0, 0, len(lanes), 0, 0, 0, 0] and int(want['n_calls'][1].sum()) == 320


def test_a_stratum_without_a_call_and_one_whose_candidates_are_not_eligible(ctx):
    cs = np.arange(320) % 4
    L = np.where(cs == 1, 5, 10)                                         # control(10) emits nothing of stratum 1
    elig = (cs != 2).astype(np.uint8)                                    # stratum 2: flagged IN | MATCHED, never eligible
    feat, truth, strata = wave_mix(cs, 4, levels=L, eligible=elig)
    want = check(ctx, feat, np.stack([control(10), control(0)]), truth, strata)
    assert [int(x) for x in want['n_calls'][0]] == [80, 0, 0, 80] and [int(x) for x in want['n_calls'][1]] == [80, 80, 0, 80]
    assert not any(want[n][:, 2].any() for n in _lib.COUNTS_NAMES) and not any(want[n][0, 1] for n in _lib.COUNTS_NAMES)


# ---- flags ------------------------------------------------------------------------------------------------------------------

def test_every_value_of_the_three_bits_for_every_pred_in_two_strata_at_once(ctx):
    """tests/test_gpu_tune_score_edges.py's 24 candidates (pred p, bits b, the other preds' fields ~b) twice, interleaved: stratum
    c % 2; then two more per stratum that raise."""
    kinds = np.repeat(np.repeat((1, 2, 3), 8), 2)
    bits = np.repeat(np.tile(np.arange(8), 3), 2)
    flags = np.zeros(52, dtype=np.uint16)
    for c in range(48):
        p, b = int(kinds[c]), int(bits[c])
        flags[c] = IN | MATCHED | sum((b if q == p else ~b & 7) << (3 * (q - 1)) for q in (1, 2, 3))
    flags[48:] = IN | RAISES
    kinds = np.concatenate([kinds, [1, 2, 3, 1]])
    feat = level_features(np.full(52, 10), kinds)
    cs = np.arange(52) % 2
    truth, strata = strata_case(flags, np.arange(52), np.arange(52) // 2, cs, [26, 26])      # a group and a truth id per candidate
    want = check(ctx, feat, control(0)[None, :], truth, strata)
    assert want[0, 0].tolist() == want[0, 1].tolist() == (26, 26, 24, 24, 12, 12, 18, 18, 2, 0)
    truth, strata = strata_case(flags, cs + 2 * (np.arange(52) % 3), np.arange(52) % 5, np.tile([0, 1], 3), [5, 5])
    check(ctx, feat, control(0)[None, :], truth, strata)


# ---- truth ids --------------------------------------------------------------------------------------------------------------

def test_strata_with_0_1_31_32_33_truth_ids(ctx):
    ids = [0, 1, 31, 32, 33, 0, 64]
    C = 400
    feat = random_features(40, C, eligible=0.95)
    truth, strata = random_case(41, C, 7, n_groups=28, ids=ids)
    assert strata['uid_off'].tolist() == [0, 0, 32, 64, 96, 160, 160, 224]
    want = check(ctx, feat, np.concatenate([random_vectors(42, 3), control(0)[None, :]]), truth, strata)
    assert not want['base_tp'][:, [0, 5]].any() and want['n_calls'][:, [0, 5]].any() and (want['base_tp'].max(axis=0)[[1, 2, 3, 4, 6]] > 0).all()
    assert int(want['base_tp'].max(axis=0)[1]) == 1


def test_ids_in_the_last_word_before_a_boundary_and_the_first_after_it(ctx):
    """Two strata of 64 ids each (two words each); three candidates per stratum: stratum 0 is matched at its ids 32, 63, 63 alone
    (the last word before the boundary), stratum 1 at 0, 0, 31 (the first word after it)."""
    feat = level_features(np.full(6, 10), [3, 1, 2, 3, 1, 2])
    flags = np.full(6, IN | MATCHED | 0x1FF, dtype=np.uint16)
    truth, strata = strata_case(flags, [0, 0, 1, 2, 3, 3], [32, 63, 63, 0, 0, 31], [0, 0, 1, 1], [64, 64])
    assert sorted(set(truth['cand_uid'].tolist())) == [32, 63, 64, 95]
    want = check(ctx, feat, control(0)[None, :], truth, strata)
    assert want[0, 0].tolist() == want[0, 1].tolist() == (3, 2, 3, 2, 3, 2, 3, 2, 0, 0)
    # 512 words: both words of the boundary lie inside one wave of tune_popcount_strata
    truth, strata = strata_case(flags, [0, 0, 1, 2, 3, 3], [8160, 8191, 8191, 0, 0, 31], [0, 0, 1, 1], [8192, 8192])
    want = check(ctx, feat, control(0)[None, :], truth, strata)
    assert want[0, 0].tolist() == want[0, 1].tolist() == (3, 2, 3, 2, 3, 2, 3, 2, 0, 0)


# ---- groups -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_groups', [255, 256, 257])
def test_groups_whose_stratum_changes_inside_a_wave_of_groups(ctx, n_groups):
    C = 700
    feat = random_features(20 + n_groups, C, eligible=0.95)
    t = random_truth(21 + n_groups, C, n_groups, 1 << 20)
    gs = (np.arange(n_groups) // 37) % 3                                 # runs of 37 groups: every wave of groups holds two or three strata
    gs[-1] = 3                                                           # the last group is a stratum of its own
    group = t['cand_group'].astype(np.int64)
    group[:8] = n_groups - 1
    flags = t['cand_flags'].copy()
    flags[:8] = IN | MATCHED | 0x1FF
    feat[:8] = level_features(np.full(8, 10), [3, 1, 2, 3, 1, 2, 3, 1])
    truth, strata = strata_case(flags, group, t['cand_uid'], gs, [50, 50, 50, 5])
    want = check(ctx, feat, np.concatenate([random_vectors(22, 3), control(0)[None, :]]), truth, strata)
    assert int(want['n_groups'][3].sum()) >= 100 and want['n_groups'][3, 3] == 1 and (want['call_hp'].max(axis=0) > 0).all()


def test_a_group_without_a_pair_in_each_stratum(ctx):
    feat = level_features(np.full(12, 10), [3] * 12)
    one = [IN | MATCHED | 0x1FF, IN, IN, IN | MATCHED | 0x1FF, IN, IN | RAISES]
    # per stratum: groups with, without, with, without a pair (and a fifth group without a call)
    truth, strata = strata_case(one + one, [0, 1, 1, 2, 3, 3, 5, 6, 6, 7, 8, 8], [0, 0, 0, 1, 0, 0] * 2, [0] * 5 + [1] * 5, [2, 2])
    want = check(ctx, feat, control(0)[None, :], truth, strata)
    assert want[0, 0].tolist() == want[0, 1].tolist() == (6, 4, 2, 2, 2, 2, 2, 2, 1, 0)


def test_the_same_flip_tie_in_two_strata_with_opposite_outcomes(ctx):
    """Stratum 0: same 2 calls + 2 ids against flip 3 calls + 1 id, a tie that goes to flip (3, 1); stratum 1: same 2 + 2 against
    flip 2 + 1, which same wins (2, 2)."""
    cands = [(0, 0, SAME), (0, 1, SAME), (0, 2, FLIP), (0, 2, FLIP), (0, 2, FLIP),
             (1, 0, SAME), (1, 1, SAME), (1, 2, FLIP), (1, 2, FLIP)]
    feat = level_features(np.full(len(cands), 10), [1 + i % 3 for i in range(len(cands))])
    truth, strata = strata_case([IN | MATCHED | b for _, _, b in cands], [g for g, _, _ in cands], [u for _, u, _ in cands], [0, 1], [5, 5])
    want = check(ctx, feat, control(0)[None, :], truth, strata)
    assert (int(want['call_hp'][0, 0]), int(want['base_hp'][0, 0])) == (3, 1) and (int(want['call_hp'][0, 1]), int(want['base_hp'][0, 1])) == (2, 2)
    assert want['n_groups'][0].tolist() == [1, 1]


# ---- batches ----------------------------------------------------------------------------------------------------------------

def test_several_batches(ctx):
    """tests/test_gpu_tune_score_edges.py's three-batch case with three strata: 640,000 truth ids in three word-aligned ranges,
    2,300 vectors cycling through 17 distinct ones (a period coprime to the batch size)."""
    C, K = 300, 2300
    ids = [213344, 213344, 213312]
    rng = np.random.default_rng(50)
    feat = level_features(rng.integers(1, 100, C), rng.integers(1, 4, C), rng.random(C) < 0.9)
    pairs = [(0, 0), (0, ids[0] - 1), (1, 5), (1, ids[1] - 1), (2, 100000), (2, ids[2] - 1)]      # (group = stratum, local id)
    which = rng.integers(0, 6, C)
    flags = (IN | MATCHED | rng.integers(0, 512, C)).astype(np.uint16)
    flags[rng.random(C) < 0.15] = IN
    truth, strata = strata_case(flags, [pairs[i][0] for i in which], [pairs[i][1] for i in which], [0, 1, 2], ids)
    assert truth['n_uid'] == 640000 and truth['n_pairs'] == 6 and 639999 in truth['cand_uid']
    per_vec = per_vec_words(truth)
    fit = WS_BUDGET // (per_vec * 4)
    assert per_vec == 60012 and K * per_vec * 4 > WS_BUDGET and -(-K // fit) == 3 and fit % 17 != 0
    distinct = np.stack([control(t) for t in (0, 100, 7, 13, 21, 29, 36, 42, 50, 58, 63, 71, 77, 84, 90, 95, 99)])
    at = cycle(distinct, K)
    want = tune_strata_ref.counts(feat, distinct, truth, strata['cand_stratum'], 3)
    assert len(set(want['n_calls'].sum(axis=1).tolist())) == 17 and (want['base_hp'].max(axis=0) > 0).all()
    check(ctx, feat, distinct[at], truth, strata, want[at])


# ---- refusals, sums ---------------------------------------------------------------------------------------------------------

def test_refusals(ctx):
    feat = random_features(70, 100)
    truth, strata = random_case(71, 100, 3)
    vecs = random_vectors(72, 2)
    check(ctx, feat, vecs, truth, strata)
    for S in (0, 65):
        bad = dict(strata, n_strata=S, uid_off=np.concatenate([np.zeros(max(S - 3, 0), dtype=np.uint32), strata['uid_off']])[:S + 1])
        with pytest.raises(_lib.DuetLibraryError):
            ctx.sweep_strata_host(feat, vecs, truth, bad)
    for off in ([0, 32, 64, 128], [0, 16, truth['n_uid'], truth['n_uid']], [32, 32, 32, truth['n_uid']]):
        with pytest.raises(_lib.DuetLibraryError):                      # not n_uid at the end; not a multiple of 32; not 0 first
            ctx.sweep_strata_host(feat, vecs, truth, dict(strata, uid_off=np.array(off, dtype=np.uint32)))
    wrong = strata['cand_stratum'].copy()
    wrong[np.nonzero(truth['cand_flags'] & IN)[0][0]] = 3
    with pytest.raises(_lib.DuetLibraryError):
        ctx.sweep_strata_host(feat, vecs, truth, dict(strata, cand_stratum=wrong))
    # the build
    arrays = dict(cand_chrom=np.arange(100) % 5, n_chrom=5)
    ctx.strata_build_host(arrays, truth, [0, 1, 2, 1, 0], 3)
    for S in (0, 65):
        with pytest.raises(_lib.DuetLibraryError):
            ctx.strata_build_host(arrays, truth, [0, 0, 0, 0, 0], S)
    with pytest.raises(_lib.DuetLibraryError):
        ctx.strata_build_host(arrays, truth, [0, 1, 3, 1, 0], 3)          # a chrom_stratum entry that is not below n_strata
    check(ctx, feat, vecs, truth, strata)                                # (the context goes on working)


@pytest.mark.parametrize('seed,S', [(80, 2), (81, 25)])
def test_the_sum_over_the_strata_is_the_plain_sweep(ctx, seed, S):
    C = 1025
    feat = random_features(seed, C)
    truth, strata = random_case(seed + 1, C, S)                          # (a truth id belongs to one stratum: no shared ids)
    vecs = random_vectors(seed + 2, 9)
    got = ctx.sweep_strata_host(feat, vecs, truth, strata)
    plain, _, _ = ctx.sweep_host(feat, vecs, truth)
    for name in _lib.COUNTS_NAMES:
        assert np.array_equal(got[name].sum(axis=1), plain[name]), name
    assert int(plain['base_hp'].max()) > 20


# ---- the build --------------------------------------------------------------------------------------------------------------

def test_build_from_both_forms(ctx):
    """Six CHROM ids over four strata; per-candidate CHROM ids, then the same ids through 11 contigs (two contigs share a CHROM
    id); every fifth candidate is not a call: it gets its stratum all the same, its group entry is not written through it."""
    C, S = 700, 4
    rng = np.random.default_rng(90)
    chrom_id = np.array([0, 1, 2, 2, 3, 4, 5, 5, 1, 0, 3], dtype=np.uint32)
    contig = np.sort(rng.integers(0, 11, C)).astype(np.uint16)
    chrom = chrom_id[contig]
    chrom_stratum = np.array([3, 0, 2, 2, 1, 0], dtype=np.uint8)
    ps = rng.integers(0, 9, C)
    flags = np.where(np.arange(C) % 5 == 0, 0, IN).astype(np.uint16)
    _, group = np.unique(chrom.astype(np.int64)[flags != 0] * 100 + ps[flags != 0], return_inverse=True)
    cand_group = np.zeros(C, dtype=np.uint32)
    cand_group[flags != 0] = group
    truth = dict(cand_flags=flags, cand_group=cand_group, n_groups=int(group.max()) + 1)
    want_group = np.zeros(truth['n_groups'], dtype=np.uint8)
    want_group[group] = chrom_stratum[chrom[flags != 0]]
    for arrays in (dict(cand_chrom=chrom, n_chrom=6), dict(cand_contig=contig, chrom_id=chrom_id, n_chrom=6)):
        cand, grp = ctx.strata_build_host(arrays, truth, chrom_stratum, S)
        assert np.array_equal(cand, chrom_stratum[chrom]) and np.array_equal(grp, want_group)
    assert len(set(want_group.tolist())) == 4 and truth['n_groups'] > 30
    empty = dict(cand_flags=np.zeros(0, dtype=np.uint16), cand_group=np.zeros(0, dtype=np.uint32), n_groups=0)
    cand, grp = ctx.strata_build_host(dict(cand_chrom=np.zeros(0, dtype=np.uint32), n_chrom=1), empty, [0], 1)
    assert len(cand) == 0 and len(grp) == 0


# ---- end to end -------------------------------------------------------------------------------------------------------------

def reference_rows(cands, truth_vcf, vecs, strata):
    """-> ([K][S] ten numbers, [K][S] counts record, n_base per stratum) from the host's truth match and the masked re-run."""
    arrays = tune.prepare_truth(cands, truth_vcf)
    S = len(strata['names'])
    cs = np.array([tune.stratum_of(strata, t) for t in cands['chrom']], dtype=np.uint8)
    counts = tune_strata_ref.counts(cands['feat'], vecs, arrays, cs, S)
    n_base = tune.truth_side(truth_vcf, strata=strata)['n_base_strata']
    return [[tune.scores(counts[k, s], n_base[s]) for s in range(S)] for k in range(len(vecs))], counts, n_base


def read_tsv(path):
    with open(path) as f:
        return [ln.split('\t') for ln in f.read().splitlines()]


def check_files(out_rows, contig_rows, plain_rows, lead, cands, truth, vecs, held):
    """The rows of --out (with --holdout) and of --by_contig for ONE setting against the plain rows and the reference."""
    n = len(lead) + 24
    assert [r[:n] for r in out_rows] == plain_rows                        # the old columns, text for text
    assert out_rows[0][n:] == ['%s_%s' % (p, s) for p in ('train', 'test') for s in tune.SCORES]
    ten, _, _ = reference_rows(cands, truth, vecs, tune.strata_holdout(held))
    for k, row in enumerate(out_rows[1:]):
        assert row[n:] == [repr(float(x)) for part in (0, 1) for x in ten[k][part]], (k, row[n:], ten[k])
    assert any(not math.isnan(x) for k in range(len(vecs)) for x in ten[k][1])
    by = tune.strata_by_contig()
    ten, counts, n_base = reference_rows(cands, truth, vecs, by)
    assert contig_rows[0] == list(lead) + ['vector', 'contig'] + list(tune.COUNTS) + ['n_base'] + list(tune.SCORES)
    want = []
    for k in range(len(vecs)):
        for s, name in enumerate(by['names']):
            if int(counts['n_calls'][k, s]) or n_base[s]:
                want.append(plain_rows[1][:len(lead)] + [str(k), name] + [str(int(counts[c][k, s])) for c in tune.COUNTS] + [str(n_base[s])] +
                            [repr(float(x)) for x in ten[k][s]])
    assert contig_rows[1:] == want and len(set(r[len(lead) + 1] for r in want)) >= 3


def test_command_line_with_holdout_and_by_contig(ctx, tmp_path):
    home = str(tmp_path / 'w')
    scoring_workdir(home, 3)
    cands = tune.features(home, 50, 2, ctx=ctx)
    texts = list(dict.fromkeys(cands['chrom']))
    assert len(texts) >= 3
    truth = str(tmp_path / 'truth.vcf')
    write_truth(cands, truth, 3)
    grid = str(tmp_path / 'g.json')
    with open(grid, 'w') as f:
        json.dump([{}, {'c1_max_ref_num': 3}, {'c2_min_sv_ratio': 0.5, 'c0_min_sv_num': 2}], f)
    vecs = tune.load_grid(grid)
    out = lambda name: str(tmp_path / name)
    held = texts[:2]
    tune.main([home, truth, '--grid', grid, '--out', out('plain.tsv')])
    tune.main([home, truth, '--grid', grid, '--out', out('both.tsv'), '--holdout', ','.join(held), '--by_contig', out('contigs.tsv')])
    check_files(read_tsv(out('both.tsv')), read_tsv(out('contigs.tsv')), read_tsv(out('plain.tsv')), (), cands, truth, vecs, held)
    # each flag alone: the same columns; the plain file does not change with --by_contig
    tune.main([home, truth, '--grid', grid, '--out', out('h.tsv'), '--holdout', ','.join(held)])
    tune.main([home, truth, '--grid', grid, '--out', out('c.tsv'), '--by_contig', out('contigs2.tsv')])
    with open(out('c.tsv'), 'rb') as a, open(out('plain.tsv'), 'rb') as b:
        assert a.read() == b.read()
    assert read_tsv(out('h.tsv')) == read_tsv(out('both.tsv')) and read_tsv(out('contigs2.tsv')) == read_tsv(out('contigs.tsv'))
    with pytest.raises(SystemExit):
        tune.main([home, truth, '--grid', grid, '--out', out('x.tsv'), '--holdout', ''])


def test_command_line_from_bams_with_holdout_and_by_contig(ctx, tmp_path):
    home = str(tmp_path / 'w')
    synth.write_svim_workdir(home, H.case_contigs('genome_small', 5), 5)
    vecs = np.stack([tune.vector(), tune.vector({'c1_max_ref_num': 3})])
    # the candidates of the fused pipeline, for a truth set and for the reference (ref / alt as tune.contig_tables writes them)
    seen = []
    empty = str(tmp_path / 'one.vcf')
    with open(empty, 'w') as f:
        f.write('#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n')
        f.write('chr1\t100\tx\tN\t<DEL>\t.\tPASS\tSVTYPE=DEL;SVLEN=-60\tGT:PS\t1|0:1\n')
    tune.sweep_settings(home, empty, vecs[:1], (50,), (2,), (0.9,), from_bams=True, ctx=ctx, on_features=lambda setting, c: seen.append(c))
    cands = dict(seen[0], ref=['N'] * len(seen[0]['pos']), alt=['<%s>' % t for t in seen[0]['svtype']])
    texts = list(dict.fromkeys(cands['chrom']))
    assert len(texts) >= 3 and int(cands['feat']['eligible'].sum()) > 50
    truth = str(tmp_path / 'truth.vcf')
    write_truth(cands, truth, 5)
    grid = str(tmp_path / 'g.json')
    with open(grid, 'w') as f:
        json.dump([{}, {'c1_max_ref_num': 3}], f)
    out = lambda name: str(tmp_path / name)
    held = [texts[1], texts[-1]]
    tune.main([home, truth, '--grid', grid, '--from_bams', '--out', out('plain.tsv')])
    tune.main([home, truth, '--grid', grid, '--from_bams', '--out', out('both.tsv'), '--holdout', ','.join(held), '--by_contig', out('contigs.tsv')])
    lead = ('svlen_thres', 'suppread_thres', 'cluster_max_distance')
    assert read_tsv(out('plain.tsv'))[0][:3] == list(lead)
    check_files(read_tsv(out('both.tsv')), read_tsv(out('contigs.tsv')), read_tsv(out('plain.tsv')), lead, cands, truth, vecs, held)
