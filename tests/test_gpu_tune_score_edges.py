# coding=utf-8
"""-m gpu: the scoring half of the threshold sweep (tune_decide with a truth set, tune_groups, tune_popcount and the batching loop
of duet_tune_sweep_device, duet_amd/csrc/duet_tune.hip) through Context.sweep_host at its edge shapes: the whole COUNTS_DTYPE
record of every vector against tests/tune_score_ref.py (pinned to evaluation.evaluation by tests/test_score_refs_host.py), and
pred / ps where they are asked for.  Feature records and truth arrays are made by hand -- no work directory, no VCF.

Two kinds of feature records:
  random_features   all three classes, deg >= 1, svread + refread >= 1, a share of records that are not eligible (their other
                    fields stay filled in: the kernel has to ignore them), scored with vectors near the defaults;
  level_features    candidate c has a level L[c] in 1 .. 99 and a kind (the pred it gets when emitted: 1, 2 or 3); the vector
                    control(t) emits exactly the candidates with L >= t, so a case says which lanes of which wave emit.
Truth arrays come from chosen (flags, group, uid) through truth_arrays, which numbers the pairs group-major as
include/duet_ef.h defines them."""
import numpy as np
import pytest

from duet_amd import _lib, tune
from tests import tune_score_ref

pytestmark = pytest.mark.gpu

IN, RAISES, MATCHED = _lib.TUNE_IN_CALLS, _lib.TUNE_RAISES, _lib.TUNE_MATCHED
NAMES = _lib.TUNE_NAMES
WS_BUDGET = 256 << 20                # kWsBudget of duet_tune.hip: the sweep's workspace per batch of vectors
VEC_PER_BLOCK = 32                   # kVecPerBlock


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def random_features(seed, C, eligible=0.8):
    rng = np.random.default_rng(seed)
    f = np.zeros(C, dtype=_lib.FEATURE_DTYPE)
    f['cls'] = rng.integers(0, 3, C)
    f['deg'] = rng.integers(1, 40, C)
    f['allhap'] = rng.integers(0, f['deg'] + 1)
    f['hap1'] = rng.integers(0, f['allhap'] + 1)
    f['hap2'] = np.where(rng.random(C) < 0.3, 0, rng.integers(0, f['allhap'] - f['hap1'] + 1))      # a share of one-haplotype votes
    f['hap0'] = f['allhap'] - f['hap1'] - f['hap2']
    f['t1'] = f['hap1'].astype(np.uint64) * rng.integers(1, 8101, C).astype(np.uint64)
    f['t2'] = f['hap2'].astype(np.uint64) * rng.integers(1, 8101, C).astype(np.uint64)
    f['svread'] = rng.integers(0, 25, C)
    f['refread'] = np.where((f['cls'] == 0) & (rng.random(C) < 0.6), 0, rng.integers(0, 25, C))    # class 0 emits only at sv_ratio == 1
    f['svread'] = np.where(f['svread'] + f['refread'] == 0, 1, f['svread'])
    f['ps'] = rng.integers(1, 2 ** 32, C)
    f['kept'] = 1
    f['eligible'] = rng.random(C) < eligible
    return f


def random_vectors(seed, K):
    """Near the defaults, with the ratio thresholds moved so that every pred occurs, and a few nan / inf."""
    rng = np.random.default_rng(seed)
    out = np.tile(tune.vector(), (K, 1))
    for k in range(K):
        for j in range(14):
            u = rng.random()
            if u < 0.5:
                out[k, j] *= rng.uniform(0.4, 1.6)
            elif u < 0.53:
                out[k, j] = (np.nan, np.inf, -np.inf)[int(rng.integers(3))]
    return out


def level_features(levels, kinds, eligible=None):
    C = len(levels)
    L, kinds = np.asarray(levels, dtype=np.int64), np.asarray(kinds, dtype=np.int64)
    assert C == 0 or (L.min() >= 1 and L.max() <= 99 and set(kinds.tolist()) <= {1, 2, 3})
    f = np.zeros(C, dtype=_lib.FEATURE_DTYPE)
    three = kinds == 3
    f['cls'] = np.where(three, 0, 1)
    f['deg'] = np.where(three, 1, 2)
    f['svread'] = np.where(three, L, 1)
    f['refread'] = np.where(three, 0, 100 - L)
    f['hap1'] = f['hap2'] = np.where(three, 0, 1)
    f['allhap'] = np.where(three, 0, 2)
    f['t1'] = np.where(three, 0, np.where(kinds == 1, 200, 100))
    f['t2'] = np.where(three, 0, np.where(kinds == 1, 100, 200))
    f['ps'] = np.arange(C) * 7 + 1
    f['kept'] = 1
    f['eligible'] = 1 if eligible is None else eligible
    return f


def control(t):
    """Emits exactly the level-L candidates with L >= t: class 0 by svread >= c0_min_sv_num, class 1 (both haplotypes voted, sv_ratio
    in (0, 1]) by refread = 100 - L <= c1_max_ref_num."""
    return tune.vector({'c0_min_sv_num': t, 'c1_twohap_sv_ratio_1': 0.0, 'c1_twohap_sv_ratio_2': 1.0, 'c1_max_ref_num': 100 - t})


def truth_arrays(flags, group, uid, n_groups=None, n_uid=None):
    """cand_pair, group_pair_off and pair_uid from (flags, group, uid): the distinct (group, uid) among the MATCHED candidates,
    numbered group-major.  cand_group of a candidate outside the call list, cand_uid / cand_pair of an unmatched one are 0."""
    flags = np.asarray(flags, dtype=np.uint16)
    C = len(flags)
    assert not ((flags & MATCHED) != 0)[(flags & IN) == 0].any() and not ((flags & RAISES) != 0)[(flags & IN) == 0].any()
    group = np.where(flags & IN, np.asarray(group, dtype=np.int64), 0)
    uid = np.where(flags & MATCHED, np.asarray(uid, dtype=np.int64), 0)
    n_groups = n_groups if n_groups is not None else int(group.max(initial=-1)) + 1
    n_uid = n_uid if n_uid is not None else int(uid.max(initial=-1)) + 1
    hit = np.nonzero(flags & MATCHED)[0]
    pairs = sorted(set((int(group[c]), int(uid[c])) for c in hit))
    number = {p: i for i, p in enumerate(pairs)}
    pair = np.zeros(C, dtype=np.uint32)
    for c in hit:
        pair[c] = number[(int(group[c]), int(uid[c]))]
    off = np.zeros(n_groups + 1, dtype=np.uint32)
    for g, _ in pairs:
        off[g + 1] += 1
    off = np.cumsum(off).astype(np.uint32)
    assert C == 0 or (group.max() < max(n_groups, 1) and uid.max() < max(n_uid, 1))
    return dict(cand_flags=flags, cand_group=group.astype(np.uint32), cand_uid=uid.astype(np.uint32), cand_pair=pair, group_pair_off=off,
                pair_uid=np.array([u for _, u in pairs], dtype=np.uint32), n_uid=n_uid, n_groups=n_groups, n_pairs=len(pairs))


def random_truth(seed, C, n_groups, n_uid, fixed_uids=()):
    rng = np.random.default_rng(seed)
    r = rng.random(C)
    flags = np.where(r < 0.1, 0, IN).astype(np.uint16)
    flags |= np.where((r >= 0.1) & (r < 0.17), RAISES, 0).astype(np.uint16)
    hit = r >= 0.3
    flags |= np.where(hit, MATCHED | rng.integers(0, 512, C), 0).astype(np.uint16)          # all eight values of every pred's three bits
    uid = rng.integers(0, n_uid, C)
    at = np.nonzero(hit)[0]
    for i, u in enumerate(fixed_uids):
        if i < len(at):
            uid[at[i]] = u
    return truth_arrays(flags, rng.integers(0, n_groups, C), uid, n_groups, n_uid)


def per_vec_words(truth):
    """duet_tune_sweep_device's workspace of one vector, in 32-bit words."""
    return 3 * truth['n_groups'] + 3 * ((truth['n_uid'] + 31) // 32) + 2 * ((truth['n_pairs'] + 31) // 32) + 1


def check(ctx, feat, vecs, truth, ref=None, outputs=(True, False)):
    """-> the reference (pred [K, C], counts [K])"""
    pred, want = ref if ref is not None else tune_score_ref.preds_and_counts(feat, vecs, truth)
    for on in outputs:
        counts, got_pred, got_ps = ctx.sweep_host(feat, vecs, truth, want_pred=on, want_ps=on)
        assert counts.dtype == _lib.COUNTS_DTYPE and len(counts) == len(vecs)
        for name in _lib.COUNTS_NAMES:
            bad = np.nonzero(counts[name] != want[name])[0]
            assert bad.size == 0, '%s differs at vectors %s: %s, expected %s' % (name, bad[:5], counts[name][bad[:5]], want[name][bad[:5]])
        if on:
            assert got_pred.shape == pred.shape and np.array_equal(got_pred, pred)
            assert np.array_equal(got_ps, np.where(feat['eligible'] != 0, feat['ps'], 0))
        else:
            assert got_pred is None and got_ps is None
    return pred, want


def sl(ref, k):
    return ref[0][:k], ref[1][:k]


# ---- shapes -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C', [0, 1, 63, 64, 65, 255, 256, 257, 513])
def test_shapes(ctx, C):
    feat = random_features(C, C)
    truth = random_truth(C + 1, C, n_groups=max(1, C // 9), n_uid=max(1, C // 2), fixed_uids=(0, max(1, C // 2) - 1))
    vecs = random_vectors(C + 2, 65)
    ref = tune_score_ref.preds_and_counts(feat, vecs, truth)
    plain = np.zeros(65, dtype=_lib.COUNTS_DTYPE)                      # without a truth set: every emitted candidate, nothing else
    plain['n_calls'] = (ref[0] != 0).sum(axis=1)
    plain = (ref[0], plain)
    if C >= 255:
        assert set(np.unique(ref[0]).tolist()) == {0, 1, 2, 3} and all(ref[1][n].max() > 0 for n in _lib.COUNTS_NAMES if n != 'reserved')
        assert len(set(ref[1]['call_hp'].tolist())) > 5 and len(set(ref[1]['base_hp'].tolist())) > 5
    for K in (0, 1, 31, 32, 33, 64, 65):                              # the last block of vectors holds K % 32 of them
        check(ctx, feat, vecs[:K], truth, sl(ref, K))
        check(ctx, feat, vecs[:K], None, sl(plain, K))


# ---- waves ------------------------------------------------------------------------------------------------------------------

def wave_case():
    """320 candidates, five waves: wave 1 lane 63 at level 60, wave 2 lane 0 at level 50, wave 3 at level 5, the rest at level 10;
    three candidates of wave 4 are not eligible."""
    L = np.full(320, 10)
    L[127], L[128], L[192:256] = 60, 50, 5
    elig = np.ones(320, dtype=np.uint8)
    elig[[256, 300, 319]] = 0
    feat = level_features(L, 1 + np.arange(320) % 3, elig)
    rng = np.random.default_rng(4)
    flags = (IN | MATCHED | rng.integers(0, 512, 320)).astype(np.uint16)
    return feat, truth_arrays(flags, np.arange(320) % 6, rng.integers(0, 40, 320), 6, 40)


@pytest.mark.parametrize('t,emitted', [(100, 0), (61, 0), (60, 1), (50, 2), (10, 253), (6, 253), (5, 317), (0, 317)])
def test_waves(ctx, t, emitted):
    """t = 60: one call in all, lane 63 of wave 1; t = 50: wave 2 has exactly one, in lane 0; t = 10: wave 3 has none while every
    other wave has; t = 100: the vector emits nothing; t = 0: everything that is eligible."""
    feat, truth = wave_case()
    pred, want = check(ctx, feat, control(t)[None, :], truth)
    assert int((pred != 0).sum()) == emitted == int(want['n_calls'][0])
    if t == 60:
        assert np.nonzero(pred[0])[0].tolist() == [127]
    if t == 50:
        assert np.nonzero(pred[0])[0].tolist() == [127, 128]
    if t == 10:
        assert not pred[0, 192:256].any() and pred[0, :192].all()


def test_waves_with_several_vectors_at_once(ctx):
    feat, truth = wave_case()
    vecs = np.stack([control(t) for t in (100, 60, 50, 10, 0, 61, 5, 6, 100, 0)])
    check(ctx, feat, vecs, truth)


# ---- flags ------------------------------------------------------------------------------------------------------------------

def test_in_calls_alone_and_raises(ctx):
    C = 200
    feat = level_features(np.full(C, 10), 1 + np.arange(C) % 3)
    for extra in (0, RAISES):
        flags = np.full(C, IN | extra, dtype=np.uint16)
        flags[::5] = 0                                                 # emitted, but not in the evaluator's call list
        flags[64:128] = 0                                              # a wave that emits without any call
        truth = truth_arrays(flags, np.arange(C) % 7, np.zeros(C), 7, 1)
        _, want = check(ctx, feat, np.stack([control(0), control(100)]), truth)
        n = int((flags != 0).sum())
        assert want[0].tolist() == (n, 7, 0, 0, 0, 0, 0, 0, n if extra else 0, 0)
        assert want[1].tolist() == (0,) * 10


def test_every_value_of_the_three_bits_for_every_pred(ctx):
    """Candidate (p, b): emitted with pred p, matched, its three bits for p are b and those of the other two preds are ~b -- reading
    the wrong pred's field changes the counts.  Once every candidate a group and a truth id of its own, once all in two groups."""
    kinds = np.repeat((1, 2, 3), 8)
    bits = np.tile(np.arange(8), 3)
    flags = np.zeros(24, dtype=np.uint16)
    for c in range(24):
        p, b = int(kinds[c]), int(bits[c])
        flags[c] = IN | MATCHED | sum((b if q == p else ~b & 7) << (3 * (q - 1)) for q in (1, 2, 3))
    feat = level_features(np.full(24, 10), kinds)
    _, want = check(ctx, feat, control(0)[None, :], truth_arrays(flags, np.arange(24), np.arange(24), 24, 24))
    # gt: bit 0 (4 values of 8); a candidate alone in its group is phased when "same" or "flip" is set at all (6 of 8)
    assert want[0].tolist() == (24, 24, 24, 24, 12, 12, 18, 18, 0, 0)
    check(ctx, feat, control(0)[None, :], truth_arrays(flags, np.arange(24) % 2, np.arange(24) % 5, 2, 5))


def test_candidates_that_are_not_eligible_count_for_nothing(ctx):
    C = 300
    feat = random_features(11, C, eligible=0.0)
    feat['svread'], feat['refread'], feat['cls'] = 9, 0, 0             # (would be emitted by every sensible vector)
    flags = np.full(C, IN | RAISES | MATCHED | 0x1FF, dtype=np.uint16)
    truth = truth_arrays(flags, np.arange(C) % 4, np.arange(C) % 50, 4, 50)
    vecs = random_vectors(12, 5)
    pred, want = check(ctx, feat, vecs, truth)
    assert not pred.any() and not any(want[n].any() for n in _lib.COUNTS_NAMES)
    feat['eligible'][[0, 63, 64, 299]] = 1                             # four of them are: only they count
    truth['cand_flags'] = np.full(C, IN | MATCHED | 0x1FF, dtype=np.uint16)
    _, want = check(ctx, feat, tune.vector()[None, :], truth)
    assert want[0].tolist() == (4, 2, 4, 4, 4, 4, 4, 4, 0, 0)             # candidates 0 and 64 share group 0, 63 and 299 group 3
    _, want = check(ctx, feat, tune.vector()[None, :], None)
    assert want[0].tolist() == (4,) + (0,) * 9


# ---- groups -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_groups', [1, 255, 256, 257])
def test_group_counts_around_one_block_of_tune_groups(ctx, n_groups):
    C = 600
    feat = random_features(20 + n_groups, C, eligible=0.95)
    truth = random_truth(21 + n_groups, C, n_groups, 90)
    at = [0, 1, 255, 256, 513]                                         # control(0) emits these: the last group has a call whatever n_groups is
    feat[at] = level_features(np.full(5, 10), [3, 1, 2, 3, 1])
    flags = truth['cand_flags'].copy()
    flags[at] = IN | MATCHED | 0x1FF
    uid = np.where(flags & MATCHED, truth['cand_uid'], 0)
    uid[at] = (0, 89, 5, 89, 0)
    truth = truth_arrays(flags, (np.arange(C) + n_groups - 1 - 513 % n_groups) % n_groups, uid, n_groups, 90)
    assert truth['cand_group'][513] == n_groups - 1
    _, want = check(ctx, feat, np.concatenate([random_vectors(22, 4), control(0)[None, :]]), truth)
    assert int(want['n_groups'].max()) >= min(n_groups, 100) and int(want['call_hp'].max()) > 20


def test_a_group_without_a_pair(ctx):
    feat = level_features(np.full(6, 10), [3] * 6)
    flags = np.array([IN | MATCHED | 0x1FF, IN, IN, IN | MATCHED | 0x1FF, IN, IN | RAISES], dtype=np.uint16)
    truth = truth_arrays(flags, [0, 1, 1, 2, 3, 3], [0, 0, 0, 1, 0, 0], 5, 2)            # groups 1 and 3: calls, no pair; group 4: no call
    assert truth['group_pair_off'].tolist() == [0, 1, 1, 2, 2, 2]
    _, want = check(ctx, feat, control(0)[None, :], truth)
    assert want[0].tolist() == (6, 4, 2, 2, 2, 2, 2, 2, 1, 0)


def test_a_group_that_owns_5000_pairs(ctx):
    C = 5200
    rng = np.random.default_rng(31)
    feat = level_features(rng.integers(1, 100, C), rng.integers(1, 4, C))
    flags = (IN | MATCHED | rng.integers(0, 512, C)).astype(np.uint16)
    group = np.where(np.arange(C) < 5000, 1, rng.integers(0, 3, C))
    uid = np.where(np.arange(C) < 5000, np.arange(C), rng.integers(0, 6000, C))
    truth = truth_arrays(flags, group, uid, 3, 6000)
    assert truth['group_pair_off'][2] - truth['group_pair_off'][1] >= 5000
    _, want = check(ctx, feat, np.stack([control(t) for t in (0, 30, 70)]), truth, outputs=(True,))
    assert int(want['base_hp'][0]) > 1000


SAME, FLIP = 0b010010010, 0b100100100                                  # "same" / "flip" for every pred (no gt)


@pytest.mark.parametrize('sames,flips,want_hp', [
    ([(2, 0), (2, 1)], [(2, 2), (2, 2), (2, 2)], (3, 1)),             # same 2 + 2, flip 3 + 1: the tie goes to flip
    ([(2, 0), (2, 1)], [(2, 2), (2, 2)], (2, 2)),                     # calls 2 : 2, pairs 2 : 1: same, by the pair bits
    ([(2, 0), (2, 0)], [(2, 2), (2, 3)], (2, 2)),                     # calls 2 : 2, pairs 1 : 2: flip, by the pair bits
    ([(2, 0), (2, 1)], [(2, 2), (2, 3), (2, 4)], (3, 3))],            # same 2 + 2, flip 3 + 3
    ids=['tie_goes_to_flip', 'call_tie_broken_by_the_pairs_for_same', 'call_tie_broken_by_the_pairs_for_flip', 'flip_wins'])
def test_same_against_flip(ctx, sames, flips, want_hp):
    # group 2 of 3; (group, uid) of the "same" calls, then of the "flip" calls; the other labelling would give other sizes
    cands = [(g, u, SAME) for g, u in sames] + [(g, u, FLIP) for g, u in flips]
    feat = level_features(np.full(len(cands), 10), [1 + i % 3 for i in range(len(cands))])
    truth = truth_arrays([IN | MATCHED | b for _, _, b in cands], [g for g, _, _ in cands], [u for _, u, _ in cands], 3, 5)
    _, want = check(ctx, feat, control(0)[None, :], truth)
    assert (int(want['call_hp'][0]), int(want['base_hp'][0])) == want_hp and int(want['n_groups'][0]) == 1
    other = (len(flips), len(set(flips))) if want_hp == (len(sames), len(set(sames))) else (len(sames), len(set(sames)))
    assert other != want_hp


def test_one_truth_id_chosen_through_two_groups_counts_once(ctx):
    cands = [(0, 7, SAME), (1, 7, FLIP), (2, 7, SAME), (2, 3, SAME)]
    feat = level_features(np.full(4, 10), [1, 2, 3, 1])
    truth = truth_arrays([IN | MATCHED | b for _, _, b in cands], [g for g, _, _ in cands], [u for _, u, _ in cands], 3, 8)
    assert truth['n_pairs'] == 4
    _, want = check(ctx, feat, control(0)[None, :], truth)
    assert want[0].tolist() == (4, 3, 4, 2, 0, 0, 4, 2, 0, 0)


# ---- truth ids --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_uid', [1, 31, 32, 33, 8192, 8193])
def test_truth_id_counts_around_one_word_and_one_block_of_tune_popcount(ctx, n_uid):
    C = 300
    feat = random_features(40 + n_uid, C, eligible=0.95)
    feat[:4] = level_features(np.full(4, 10), [3, 1, 2, 3])
    truth = random_truth(41 + n_uid, C, 5, n_uid)
    flags, uid = truth['cand_flags'].copy(), truth['cand_uid'].copy()
    flags[:4] = IN | MATCHED | 0x1FF                                   # ids 0 and n_uid - 1 are matched, by candidates control(0) emits
    uid[:4] = (0, n_uid - 1, n_uid - 1, 0)
    truth = truth_arrays(flags, truth['cand_group'], uid, 5, n_uid)
    _, want = check(ctx, feat, np.concatenate([random_vectors(42, 3), control(0)[None, :]]), truth)
    assert int(want['base_tp'][3]) >= min(n_uid, 2) and int(want['base_hp'][3]) >= min(n_uid, 2)


# ---- batches ----------------------------------------------------------------------------------------------------------------

def cycle(distinct, K):
    return np.arange(K) % len(distinct)


def test_several_batches(ctx):
    """The workspace of K vectors exceeds kWsBudget (256 MiB): duet_tune_sweep_device runs three batches (v0 > 0, the workspace
    zeroed again, counts / vectors / pred offset by v0, ps from the first batch).  The vectors cycle through 17 distinct ones: a
    period coprime to the batch size, so a wrong offset lands on a different vector."""
    C, K, n_uid = 300, 2300, 640000
    rng = np.random.default_rng(50)
    feat = level_features(rng.integers(1, 100, C), rng.integers(1, 4, C), rng.random(C) < 0.9)
    pairs = [(0, 0), (0, n_uid - 1), (1, 5), (1, n_uid - 1), (2, 320000)]
    which = rng.integers(0, 5, C)
    flags = (IN | MATCHED | rng.integers(0, 512, C)).astype(np.uint16)
    flags[rng.random(C) < 0.15] = IN
    truth = truth_arrays(flags, [pairs[i][0] for i in which], [pairs[i][1] for i in which], 3, n_uid)
    assert truth['n_pairs'] == 5
    per_vec = per_vec_words(truth)
    fit = WS_BUDGET // (per_vec * 4)
    assert per_vec == 60012 and K * per_vec * 4 > WS_BUDGET and -(-K // fit) == 3 and fit % 17 != 0
    distinct = np.stack([control(t) for t in (0, 100, 7, 13, 21, 29, 36, 42, 50, 58, 63, 71, 77, 84, 90, 95, 99)])
    at = cycle(distinct, K)
    pred, want = tune_score_ref.preds_and_counts(feat, distinct, truth)
    assert len(set(want['call_hp'].tolist())) > 10 and len(set(want['n_calls'].tolist())) == 17
    check(ctx, feat, distinct[at], truth, (pred[at], want[at]))


def many_vectors_case():
    C, K = 70, 65537
    rng = np.random.default_rng(60)
    feat = level_features(rng.integers(1, 100, C), rng.integers(1, 4, C), rng.random(C) < 0.9)
    pairs = [(0, 0), (0, 39), (1, 17)]
    which = rng.integers(0, 3, C)
    flags = (IN | MATCHED | rng.integers(0, 512, C)).astype(np.uint16)
    flags[rng.random(C) < 0.15] = IN
    truth = truth_arrays(flags, [pairs[i][0] for i in which], [pairs[i][1] for i in which], 2, 40)
    distinct = np.stack([control(t) for t in (0, 100, 7, 13, 21, 29, 36, 42, 50, 58, 63, 71, 77, 84, 90, 99)])
    return feat, truth, distinct, cycle(distinct, K)


def test_65537_vectors_with_a_truth_set(ctx):
    """More vectors than the 65,535 rows of workgroups gridDim.y is documented to take.  tune_groups and tune_popcount run one row
    per vector, and the workspace budget does not cut a batch with so small a truth set: duet_tune_sweep_device caps a batch with
    a truth set at 65,535 vectors, which makes this a two-batch run (v0 = 65,535).  The counts of every vector must be right."""
    feat, truth, distinct, at = many_vectors_case()
    assert truth['n_pairs'] == 3 and len(at) * per_vec_words(truth) * 4 < WS_BUDGET      # the workspace budget does not cut the batch
    pred, want = tune_score_ref.preds_and_counts(feat, distinct, truth)
    assert len(set(want['n_calls'].tolist())) == 16 and len(set(want['call_hp'].tolist())) > 8
    check(ctx, feat, distinct[at], truth, (pred[at], want[at]), outputs=(False,))


def test_65537_vectors_without_a_truth_set(ctx):
    feat, _, distinct, at = many_vectors_case()
    pred, want = tune_score_ref.preds_and_counts(feat, distinct, None)
    assert len(set(want['n_calls'].tolist())) == 16
    check(ctx, feat, distinct[at], None, (pred[at], want[at]), outputs=(False, True))
