# coding=utf-8
"""-m gpu: the evaluator's kernels (eval_match, eval_group_sets, eval_group_choose, eval_count of duet_amd/csrc/duet_eval.hip)
through Context.eval_counts at their edge shapes, all six integers against tests/eval_ref.py (pinned to evaluation.evaluation
by tests/test_score_refs_host.py).  Flat arrays made by hand or by a small seeded generator; only set SIZES come back, so every
hand-made case is built so that the wrong choice changes a count -- the wrong neighbour has a length that fails the ratio, or a
haplotype that changes `gt` -- and states the six numbers it expects, which the reference has to give as well.

In the hand-made cases a "good" record has length 1000 and a "bad" one length 100: with calls of length 1000 and ratio 0.5
only a good record is accepted."""
import numpy as np
import pytest

from duet_amd import _lib
from duet_amd import evaluation as E
from tests import eval_ref
from tests.test_gpu_eval import synthetic_records

pytestmark = pytest.mark.gpu

U32 = 0xFFFFFFFF
GOOD, BAD = 1000, 100


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def problem(lists, calls, n_keys=None, n_groups=None, n_base_uid=None, n_call_uid=None):
    """lists: {list key: [(pos, len, uid, hp), ...] in position order}; calls: [(key, pos, len, uid, group, hp), ...]
    -> the flat arrays of evaluation.flatten.  The id and group counts default to the largest one used plus 1."""
    n_keys = n_keys if n_keys is not None else max(lists) + 1
    off, rows = [0], []
    for k in range(n_keys):
        rows.extend(lists.get(k, []))
        off.append(len(rows))
    col = lambda src, i, dt: np.array([r[i] for r in src], dtype=dt)
    return dict(base_off=np.array(off, dtype=np.uint32), base_pos=col(rows, 0, np.uint32), base_len=col(rows, 1, np.uint32),
                base_uid=col(rows, 2, np.uint32), base_hp=col(rows, 3, np.uint8),
                call_key=col(calls, 0, np.uint32), call_pos=col(calls, 1, np.uint32), call_len=col(calls, 2, np.uint32),
                call_uid=col(calls, 3, np.uint32), call_group=col(calls, 4, np.uint32), call_hp=col(calls, 5, np.uint8),
                n_groups=n_groups if n_groups is not None else max([c[4] for c in calls] + [0]) + 1,
                n_base_uid=n_base_uid if n_base_uid is not None else max([r[2] for r in rows] + [0]) + 1,
                n_call_uid=n_call_uid if n_call_uid is not None else max([c[3] for c in calls] + [0]) + 1)


def check(ctx, a, refdist, ratio, want=None):
    ref = eval_ref.counts(a, refdist, ratio)
    if want is not None:
        assert ref == tuple(want), 'the case does not hold what it is about: %s' % (ref,)
    n = ctx.eval_counts(a, refdist, ratio)
    got = tuple(int(getattr(n, f)) for f in eval_ref.NAMES)
    assert got == ref, (got, ref)
    return got


LENS = (300, 700, 1000, 4900, 7000, 1000)
RATIOS = (0.0, 0.3, 0.7, 0.1 + 0.2, 1.0)


def random_problem(seed, n_calls, n_keys=6, per_list=(1, 40), n_groups=None, n_call_uid=None, n_base_uid=None, hp_codes=5, only_key=None):
    """Truth positions on a grid of 50 and call positions on a grid of 25 (exact ties and equal positions are common), lengths whose
    quotients sit on the ratios of RATIOS, haplotype codes 0 .. hp_codes - 1, ids drawn with repeats.  only_key: every other
    list is empty."""
    rng = np.random.default_rng(seed)
    size = [int(rng.integers(per_list[0], per_list[1] + 1)) if only_key in (None, k) else 0 for k in range(n_keys)]
    off = np.concatenate([[0], np.cumsum(size)]).astype(np.uint32)
    nb = int(off[-1])
    pos = np.concatenate([np.sort(rng.integers(0, 40, s)) * 50 for s in size]).astype(np.uint32)
    n_base_uid = n_base_uid or max(1, nb * 2 // 3)
    n_call_uid = n_call_uid or max(1, n_calls * 2 // 3)
    n_groups = n_groups or max(1, n_calls // 5)
    keys = np.array([k for k in range(n_keys) if size[k]], dtype=np.uint32)
    pick = lambda hi, n: rng.integers(0, hi, n).astype(np.uint32)
    return dict(base_off=off, base_pos=pos, base_len=np.array(LENS, dtype=np.uint32)[rng.integers(0, len(LENS), nb)],
                base_uid=pick(n_base_uid, nb), base_hp=pick(hp_codes, nb).astype(np.uint8),
                call_key=keys[rng.integers(0, len(keys), n_calls)], call_pos=pick(84, n_calls) * np.uint32(25),
                call_len=np.array(LENS, dtype=np.uint32)[rng.integers(0, len(LENS), n_calls)], call_uid=pick(n_call_uid, n_calls),
                call_group=pick(n_groups, n_calls), call_hp=pick(hp_codes, n_calls).astype(np.uint8),
                n_groups=n_groups, n_base_uid=n_base_uid, n_call_uid=n_call_uid)


# ---- sizes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_calls', [0, 1, 63, 64, 65, 255, 256, 257, 513])
def test_n_calls(ctx, n_calls):
    for seed, (refdist, ratio) in enumerate(((50, 0.7), (25, 0.0), (1000, 0.3))):
        got = check(ctx, random_problem(1000 * n_calls + seed, n_calls), refdist, ratio)
        assert got[0] <= n_calls and (n_calls < 63 or got[4] > 0)
    if n_calls == 1:
        check(ctx, problem({0: [(1000, GOOD, 0, 2)]}, [(0, 1001, GOOD, 0, 0, 2)]), 1, 0.5, (1,) * 6)


def test_one_truth_record_in_all(ctx):
    a = problem({0: [(1000, GOOD, 0, 0)]}, [(0, p, GOOD, i, i % 2, i % 3) for i, p in enumerate((900, 1000, 1100, 1101, 899, 0, U32))])
    assert len(a['base_pos']) == 1
    # calls 0 .. 2 match (hp 0, 1, 2 against 0): all tp, two gt; group 0 has calls 0 (same) and 2 (nothing), group 1 call 1 (flip)
    check(ctx, a, 100, 0.5, (3, 1, 2, 1, 2, 1))


def test_one_record_list_left_on_right(ctx):
    lists = {0: [(5000, GOOD, 0, 2)], 1: [(100, BAD, 1, 2), (5000, BAD, 2, 2), (9000, BAD, 3, 2)]}
    calls = [(0, p, GOOD, i, 0, 2) for i, p in enumerate((4000, 4999, 5000, 5001, 6000, 6001, 3999))]
    check(ctx, problem(lists, calls), 1000, 0.5, (5, 1, 5, 1, 5, 1))


@pytest.mark.parametrize('key', [0, 47])
def test_48_keys_and_one_list(ctx, key):
    a = random_problem(7 + key, 200, n_keys=48, per_list=(30, 30), only_key=key)
    assert len(a['base_off']) == 49 and len(a['base_pos']) == 30 and set(a['call_key'].tolist()) == {key}
    assert check(ctx, a, 50, 0.3)[0] > 20


# ---- the nearest record ---------------------------------------------------------------------------------------------------

def test_tie_between_left_and_right_goes_right(ctx):
    lists = {0: [(1000, BAD, 0, 2), (1200, GOOD, 1, 2)], 1: [(1000, GOOD, 2, 2), (1200, BAD, 3, 2)]}
    calls = [(0, 1100, GOOD, 0, 0, 2), (1, 1100, GOOD, 1, 0, 2),        # the tie: right -- good in list 0, bad in list 1
             (0, 1099, GOOD, 2, 0, 2), (0, 1101, GOOD, 3, 0, 2),        # one nearer to the left (bad), one nearer to the right (good)
             (1, 1099, GOOD, 4, 0, 2), (1, 1101, GOOD, 5, 0, 2)]
    check(ctx, problem(lists, calls), 1000, 0.5, (3, 2, 3, 2, 3, 2))
    # each list alone: taken together, a tie that went left would lose one match in list 0 and gain one in list 1
    check(ctx, problem({0: lists[0]}, [c for c in calls if c[0] == 0]), 1000, 0.5, (2, 1, 2, 1, 2, 1))
    check(ctx, problem({0: lists[1]}, [(0,) + c[1:] for c in calls if c[0] == 1]), 1000, 0.5, (1, 1, 1, 1, 1, 1))


def test_among_equal_positions_the_first_and_at_the_end_the_last(ctx):
    lists = {0: [(3000, GOOD, 0, 2), (3000, BAD, 1, 2), (3000, BAD, 2, 2)], 1: [(3000, BAD, 3, 2), (3000, BAD, 4, 2), (3000, GOOD, 5, 2)]}
    calls = [(k, p, GOOD, 3 * k + i, 0, 2) for k in (0, 1) for i, p in enumerate((2990, 3000, 3010))]
    # list 0: 2990 and 3000 take the first record (good), 3010 has its insertion point at the end and takes the last (bad);
    # list 1: the other way round
    check(ctx, problem(lists, calls), 1000, 0.5, (3, 2, 3, 2, 3, 2))


def test_insertion_point_at_the_end_takes_the_last_record(ctx):
    lists = {0: [(100, BAD, 0, 2), (200, GOOD, 1, 2)], 1: [(100, GOOD, 2, 2), (200, BAD, 3, 2)], 2: [(100, BAD, 4, 2), (200, BAD, 5, 2), (300, GOOD, 6, 2)]}
    calls = [(0, 5000, GOOD, 0, 0, 2), (1, 5000, GOOD, 1, 0, 2), (2, 301, GOOD, 2, 0, 2), (2, U32, GOOD, 3, 0, 2)]
    check(ctx, problem(lists, calls), U32, 0.5, (3, 2, 3, 2, 3, 2))


def test_a_call_below_the_first_record(ctx):
    lists = {0: [(100, GOOD, 0, 2), (200, BAD, 1, 2)], 1: [(100, BAD, 2, 2), (200, GOOD, 3, 2)]}
    calls = [(0, 5, GOOD, 0, 0, 2), (1, 5, GOOD, 1, 0, 2), (0, 0, GOOD, 2, 0, 2), (0, 99, GOOD, 3, 0, 2)]
    check(ctx, problem(lists, calls), 1000, 0.5, (3, 1, 3, 1, 3, 1))


def test_positions_0_and_the_largest(ctx):
    lists = {0: [(0, GOOD, 0, 2), (U32, GOOD, 1, 0)]}
    # 0x7FFFFFFF is nearer to 0 by one, 0x80000000 nearer to the right end by one; only the left record's haplotype gives gt
    calls = [(0, p, GOOD, i, i, 2) for i, p in enumerate((0, U32, 0x7FFFFFFF, 0x80000000))]
    check(ctx, problem(lists, calls), U32, 0.0, (4, 2, 2, 1, 2, 1))


# ---- refdist ----------------------------------------------------------------------------------------------------------------

def test_refdist_itself_is_accepted_and_one_more_is_not(ctx):
    a = problem({0: [(50000, GOOD, 0, 2)]}, [(0, 50000 + d, GOOD, i, 0, 2) for i, d in enumerate((-300, 300, -301, 301))])
    check(ctx, a, 300, 0.0, (2, 1, 2, 1, 2, 1))
    check(ctx, a, 301, 0.0, (4, 1, 4, 1, 4, 1))
    check(ctx, a, 299, 0.0, (0, 0, 0, 0, 0, 0))


def test_refdist_0(ctx):
    a = problem({0: [(50000, GOOD, 0, 2)]}, [(0, 50000 + d, GOOD, i, 0, 2) for i, d in enumerate((0, -1, 1))])
    check(ctx, a, 0, 0.0, (1, 1, 1, 1, 1, 1))


def test_refdist_of_the_whole_range(ctx):
    a = problem({0: [(U32, GOOD, 0, 2)], 1: [(0, GOOD, 1, 2)]}, [(0, 0, GOOD, 0, 0, 2), (1, U32, GOOD, 1, 0, 2)])
    check(ctx, a, U32, 0.0, (2, 2, 2, 2, 2, 2))
    check(ctx, a, U32 - 1, 0.0, (0, 0, 0, 0, 0, 0))


# ---- the length quotient in binary64 ----------------------------------------------------------------------------------------

PAIRS = ((700, 1000), (4900, 7000), (300, 1000))


def quotient_case(pairs):
    """One truth record and two calls per pair (the lengths either way round), every call its own id; -> arrays"""
    lists = {0: [(1000 * (i + 1), b, i, 2) for i, (_, b) in enumerate(pairs)] + [(1000 * (len(pairs) + i + 1), a, len(pairs) + i, 2) for i, (a, _) in enumerate(pairs)]}
    calls = [(0, 1000 * (i + 1), a, i, 0, 2) for i, (a, _) in enumerate(pairs)] + \
            [(0, 1000 * (len(pairs) + i + 1), b, len(pairs) + i, 0, 2) for i, (_, b) in enumerate(pairs)]
    return problem(lists, calls)


@pytest.mark.parametrize('ratio,n_ok', [(0.7, 2), (0.3, 3), (0.1 + 0.2, 2)], ids=['0.7', '0.3', '0.1+0.2'])
def test_length_quotient_in_binary64(ctx, ratio, n_ok):
    # 7 / 10 == 49 / 70 == 0.7 in binary64; 3 / 10 == 0.3 < 0.1 + 0.2
    want = (2 * n_ok,) * 6
    check(ctx, quotient_case(PAIRS), 0, ratio, want)


@pytest.mark.parametrize('ratio,want', [(1.0, 2), (float('nan'), 0), (float('inf'), 0), (-1.0, 10), (0.0, 10), (0.5, 4)],
                         ids=['1.0', 'nan', 'inf', '-1.0', '0.0', '0.5'])
def test_length_quotient_at_its_ends(ctx, ratio, want):
    # (0, 0): 0 / 0 is nan, refused by every ratio; (0, 500) and (500, 0): quotient 0; (123, 123): quotient 1
    pairs = ((123, 123), (0, 0), (0, 500), (500, 0), (999, 1000), (1, U32))
    check(ctx, quotient_case(pairs), 0, ratio, (want,) * 6)


def test_both_lengths_0_are_refused_by_ratio_0(ctx):
    a = problem({0: [(1000, 0, 0, 2)], 1: [(1000, 0, 1, 2)]}, [(0, 1000, 0, 0, 0, 2), (1, 1000, 1, 1, 0, 2)])
    check(ctx, a, 10, 0.0, (1, 1, 1, 1, 1, 1))


# ---- haplotype codes --------------------------------------------------------------------------------------------------------

def hp_case(pairs):
    """Per (call code, truth code): one call, one truth record, one group of its own."""
    return problem({0: [(1000 * (i + 1), GOOD, i, bh) for i, (_, bh) in enumerate(pairs)]},
                   [(0, 1000 * (i + 1), GOOD, i, i, ch) for i, (ch, _) in enumerate(pairs)])


def test_all_nine_pairs_of_the_fixed_codes(ctx):
    # gt: both het (4) or both '1|1' (1); phased: the same code (3, '1|1' among them through the tie to flip) or mirrored hets (2)
    check(ctx, hp_case([(c, b) for c in range(3) for b in range(3)]), 10, 0.5, (9, 9, 5, 5, 5, 5))
    for c in range(3):
        for b in range(3):
            gt = int((c < 2 and b < 2) or c == b == 2)
            hp = int(c == b or {c, b} == {0, 1})
            check(ctx, hp_case([(c, b)]), 10, 0.5, (1, 1, gt, gt, hp, hp))


@pytest.mark.parametrize('pairs,want', [([(3, 3)], (1, 1, 0, 0, 1, 1)), ([(7, 7), (200, 200)], (2, 2, 0, 0, 2, 2)),
                                         ([(3, 4)], (1, 1, 0, 0, 0, 0)), ([(4, 3), (3, 2), (2, 3), (0, 3), (3, 1)], (5, 5, 0, 0, 0, 0)),
                                         ([(255, 255)], (1, 1, 0, 0, 1, 1)), ([(255, 2), (2, 255), (255, 254), (255, 0)], (4, 4, 0, 0, 0, 0))],
                         ids=['3_3', '7_7_and_200_200', '3_4', 'different_codes', '255_255', '255_and_others'])
def test_codes_of_3_and_more(ctx, pairs, want):
    # equal codes of 3 or more: "same", not gt, not "flip"; different ones: nothing
    check(ctx, hp_case(pairs), 10, 0.5, want)


# ---- id sets ----------------------------------------------------------------------------------------------------------------

def test_many_calls_share_one_id(ctx):
    lists = {0: [(1000 * (i + 1), GOOD, i, 2) for i in range(300)]}
    calls = [(0, 1000 * (i + 1), GOOD, 3 if i % 2 else 1, i % 7, 2) for i in range(300)]
    check(ctx, problem(lists, calls, n_call_uid=5), 10, 0.5, (2, 300, 2, 300, 2, 300))


def test_many_calls_match_one_truth_record(ctx):
    lists = {0: [(500000, GOOD, 1, 2)], 1: [(500000, BAD, 0, 2)]}
    calls = [(0, 500000 + i - 150, GOOD, i, i % 11, 2) for i in range(300)] + [(1, 500000, GOOD, 300 + i, 0, 2) for i in range(20)]
    check(ctx, problem(lists, calls), 1000, 0.5, (300, 1, 300, 1, 300, 1))


def test_one_truth_id_on_several_records(ctx):
    # id 4: twice in list 0, once in list 3; id 2: in lists 0 and 1
    lists = {0: [(1000, GOOD, 4, 2), (2000, GOOD, 4, 0), (3000, GOOD, 2, 2)], 1: [(1000, GOOD, 2, 1)], 3: [(1000, GOOD, 4, 2), (2000, GOOD, 0, 2)]}
    calls = [(0, 1000, GOOD, 0, 0, 2), (0, 2000, GOOD, 1, 0, 0), (0, 3000, GOOD, 2, 1, 2), (1, 1000, GOOD, 3, 1, 0), (3, 1000, GOOD, 4, 2, 2)]
    # all five match, ids {4, 2}; gt everywhere; group 0: same 2 + 1 against flip 1 + 1: same; group 1: same 1 + 1 against flip 2 + 1: flip
    check(ctx, problem(lists, calls), 10, 0.5, (5, 2, 5, 2, 5, 2))


def test_ids_that_nothing_touches_at_either_end(ctx):
    lists = {0: [(1000 * (i + 1), GOOD, 1 + i, 2) for i in range(6)]}
    calls = [(0, 1000 * (i + 1), GOOD, 1 + i, 0, 2) for i in range(6)] + [(0, 900000, GOOD, 0, 0, 2), (0, 900001, GOOD, 7, 0, 2)]
    # ids 0 and the last one exist on both sides (the unmatched calls carry them; no truth record has them) and are counted nowhere
    check(ctx, problem(lists, calls, n_base_uid=8, n_call_uid=8), 10, 0.5, (6, 6, 6, 6, 6, 6))


# ---- groups -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('own', [True, False], ids=['every_call_its_own_group', 'all_calls_in_one_group'])
def test_group_extremes(ctx, own):
    a = random_problem(77, 300, hp_codes=3)
    a['call_group'] = np.arange(300, dtype=np.uint32) if own else np.zeros(300, dtype=np.uint32)
    a['n_groups'] = 300 if own else 1
    assert check(ctx, a, 50, 0.3)[4] > 10


def test_same_equal_to_flip_goes_to_flip(ctx):
    # same: one call id (three calls share it) + truth ids {0, 1, 2} = 4; flip: call ids {1, 2, 3} + one truth id = 4
    lists = {0: [(1000, GOOD, 0, 0), (2000, GOOD, 1, 0), (3000, GOOD, 2, 0), (4000, GOOD, 3, 1)]}
    calls = [(0, 1000, GOOD, 0, 0, 0), (0, 2000, GOOD, 0, 0, 0), (0, 3000, GOOD, 0, 0, 0)] + [(0, 4000 + i, GOOD, 1 + i, 0, 0) for i in range(3)]
    check(ctx, problem(lists, calls), 10, 0.5, (4, 4, 4, 4, 3, 1))


def test_same_wins_by_one_truth_id(ctx):
    # call ids tie 2 : 2, truth ids 2 : 1
    lists = {0: [(1000, GOOD, 0, 0), (2000, GOOD, 1, 0), (4000, GOOD, 3, 1)]}
    calls = [(0, 1000, GOOD, 0, 0, 0), (0, 2000, GOOD, 1, 0, 0), (0, 4000, GOOD, 2, 0, 0), (0, 4001, GOOD, 3, 0, 0)]
    check(ctx, problem(lists, calls), 10, 0.5, (4, 3, 4, 3, 2, 2))


def test_one_truth_id_chosen_in_two_groups_counts_once(ctx):
    lists = {0: [(1000, GOOD, 0, 0)], 1: [(1000, GOOD, 0, 1)]}
    calls = [(0, 1000, GOOD, 0, 0, 0), (0, 1001, GOOD, 1, 1, 1), (1, 1000, GOOD, 2, 2, 1)]        # same, flip, same: three groups
    check(ctx, problem(lists, calls), 10, 0.5, (3, 1, 3, 1, 3, 1))


def test_one_call_id_in_two_groups_with_different_winners(ctx):
    lists = {0: [(1000, GOOD, 0, 0), (2000, GOOD, 1, 1)]}
    calls = [(0, 1000, GOOD, 5, 0, 0), (0, 2000, GOOD, 5, 1, 0),       # id 5: "same" in group 0, "flip" in group 1
             (0, 1001, GOOD, 6, 1, 0)]                                 # id 6: "same" in group 1, where flip wins the tie
    check(ctx, problem(lists, calls), 10, 0.5, (2, 2, 2, 2, 1, 2))


def test_70000_groups(ctx):
    a = random_problem(70, 300, n_groups=70000, hp_codes=3)
    a['call_group'][:4] = (0, 69999, 65535, 65536)
    assert check(ctx, a, 50, 0.3)[4] > 10


def test_too_many_groups_is_an_invalid_argument(ctx):
    a = problem({0: [(1000, GOOD, 0, 2)]}, [(0, 1000, GOOD, 0, 0, 2)], n_groups=1 << 30)
    with pytest.raises(_lib.DuetLibraryError, match=r'\(%d\).*too many phase sets' % _lib.DUET_ERR_INVALID):        # refused before any allocation
        ctx.eval_counts(a, 10, 0.5)
    a['n_groups'] = 1
    check(ctx, a, 10, 0.5, (1, 1, 1, 1, 1, 1))                         # the context is usable afterwards


# ---- the hash set -----------------------------------------------------------------------------------------------------------

def slot(labelling, group, side, ident, mask=63):
    """set_key and the multiplicative hash of set_insert (duet_eval.hip), as documented there."""
    key = labelling << 63 | group << 33 | side << 32 | ident
    return ((key * 0x9E3779B97F4A7C15 & 0xFFFFFFFFFFFFFFFF) >> 32) & mask


def ids_on_slot(labelling, group, side, want, n):
    out = [i for i in range(200000) if slot(labelling, group, side, i) == want][:n]
    assert len(out) == n
    return out


@pytest.mark.parametrize('same_wins', [False, True], ids=['tie_to_flip', 'same_by_one'])
def test_hash_probe_wraps_past_the_last_slot(ctx, same_wins):
    """8 calls: a table of 64 slots.  Brute force picks the ids so that five or six keys of the "same" labelling land on slot 63
    and the probe wraps to slots 0, 1, ..., where keys of the "flip" labelling were sent as well; every "same" key arrives more than
    once, so finding it again behind the wrap decides the count: same is 4 (5 with same_wins) against flip 4.  Counting a key twice
    makes "same" win the tie, losing one makes it lose by one.  (If the hash is ever changed these cases stay valid and only stop
    being adversarial.)"""
    u1 = ids_on_slot(0, 0, 0, 63, 1)[0]
    b = ids_on_slot(0, 0, 1, 63, 4)
    f = [ids_on_slot(1, 0, 0, s, 1)[0] for s in (0, 1, 2)]
    c1 = ids_on_slot(1, 0, 1, 0, 1)[0]
    assert sum(slot(0, 0, side, i) == 63 for side, i in [(0, u1)] + [(1, x) for x in b[:3]]) >= 3
    truth = [(b[0], 0), (b[1], 0), (b[2], 0), (b[3], 0), (c1, 1)]
    lists = {0: [(1000 * (i + 1), GOOD, u, hp) for i, (u, hp) in enumerate(truth)]}
    same_at = (1000, 2000, 3000, 1000, 4000 if same_wins else 2000)
    calls = [(0, p, GOOD, u1, 0, 0) for p in same_at] + [(0, 5000 + i, GOOD, f[i], 0, 0) for i in range(3)]
    a = problem(lists, calls)
    assert len(calls) == 8
    check(ctx, a, 10, 0.5, (4, 5, 4, 5, 1, 4) if same_wins else (4, 4, 4, 4, 3, 1))


def test_the_fullest_table_the_sizing_allows(ctx):
    # 8 calls, '1|1' against '1|1', all ids distinct: four keys per call, 32 keys in 64 slots
    a = problem({0: [(1000 * (i + 1), GOOD, i, 2) for i in range(8)]}, [(0, 1000 * (i + 1), GOOD, i, 0, 2) for i in range(8)])
    check(ctx, a, 10, 0.5, (8,) * 6)
    a = problem({0: [(1000 * (i + 1), GOOD, i, 2) for i in range(8)]}, [(0, 1000 * (i + 1), GOOD, i, i % 3, 2) for i in range(8)])
    check(ctx, a, 10, 0.5, (8,) * 6)


# ---- eval_count -------------------------------------------------------------------------------------------------------------

def spread_case(n_uid, n_calls, seed, marks=()):
    """n_calls calls, each on a truth record of its own, '1|1' on both sides (every match sets all six flags); the ids are spread
    over 0 .. n_uid - 1 on both sides, with 0, n_uid - 1 and `marks` among them."""
    rng = np.random.default_rng(seed)
    fixed = [m for m in (0, n_uid - 1) + tuple(marks) if 0 <= m < n_uid]
    ids = lambda: (fixed + rng.integers(0, n_uid, n_calls).tolist())[:n_calls]
    cu, bu = ids(), ids()[::-1]
    a = problem({0: [(1000 * (i + 1), GOOD, bu[i], 2) for i in range(n_calls)]}, [(0, 1000 * (i + 1), GOOD, cu[i], i % 5, 2) for i in range(n_calls)],
                n_base_uid=n_uid, n_call_uid=n_uid)
    return a, (len(set(cu)), len(set(bu))) * 3


@pytest.mark.parametrize('n_uid', [1, 2047, 2048, 2049])
def test_id_counts_around_one_block_of_eval_count(ctx, n_uid):
    a, want = spread_case(n_uid, 200, n_uid)
    check(ctx, a, 10, 0.5, want)


BIG = 1024 * 2048


def big_case():
    return spread_case(BIG + 5, 300, 9, marks=(BIG - 1, BIG))


def test_eval_count_grid_stride(ctx):
    # more ids than 1024 blocks of 2048 cover in one step: set flags at 0, at the last index of the first step, at the first of the
    # second and at the very end
    a, want = big_case()
    for side in ('call_uid', 'base_uid'):
        assert {0, BIG - 1, BIG, BIG + 4} <= set(a[side].tolist())
    check(ctx, a, 10, 0.5, want)


def test_workspace_re_use(ctx):
    """One context: the largest case, a 3-call case, the large one again -- stale flags, counters or table slots must not leak."""
    big, want = big_case()
    small = problem({0: [(1000, GOOD, 0, 0), (2000, GOOD, 1, 1)]}, [(0, 1000, GOOD, 0, 0, 0), (0, 2000, GOOD, 1, 0, 0), (0, 90000, GOOD, 2, 0, 2)])
    for _ in range(2):
        check(ctx, big, 10, 0.5, want)
        check(ctx, small, 10, 0.5, (2, 2, 2, 2, 1, 1))
    check(ctx, random_problem(5, 300), 50, 0.3)
    check(ctx, small, 10, 0.5, (2, 2, 2, 2, 1, 1))


# ---- evaluation_gpu -----------------------------------------------------------------------------------------------------------

def outcome(fn, *args, **kw):
    try:
        return [float(x) for x in fn(*args, **kw)]
    except (ZeroDivisionError, IndexError) as e:
        return type(e)


def test_a_negative_refdist_is_what_evaluation_makes_of_it(ctx):
    truth, calls = synthetic_records(1, 300, 400)
    assert outcome(E.evaluation_gpu, truth, calls, 1000, 0.0, ctx=ctx) == outcome(E.evaluation, truth, calls, 1000, 0.0) != ZeroDivisionError
    # abs(...) <= -1 never holds: nothing matches, precision + recall is 0 and upstream's F1 divides by it
    assert outcome(E.evaluation_gpu, truth, calls, -1, 0.0, ctx=ctx) == outcome(E.evaluation, truth, calls, -1, 0.0) == ZeroDivisionError


# ---- breadth ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('part', range(4))
def test_random_small_problems(ctx, part):
    rng = np.random.default_rng(900 + part)
    matched = 0
    for i in range(80):
        n_calls = int(rng.integers(1, 301))
        a = random_problem(100000 * part + i, n_calls, n_keys=int(rng.integers(1, 7)), per_list=(1, int(rng.integers(1, 41))))
        refdist = int(rng.choice((0, 24, 25, 26, 50, 75, 1000)))
        matched += check(ctx, a, refdist, float(rng.choice(RATIOS)))[0]
    assert matched > 1000
