# coding=utf-8
"""-m gpu: the leaf census (duet_tune_leaf_census_host / _device; tune_leaf_labels and tune_leaf_census of
duet_amd/csrc/duet_tune_leaf.hip): every word of every (vector, stratum, leaf) record against tests/tune_leaf_ref.py -- which
tests/test_tune_leaf_host.py ties to the recorded preds and to tune_score_ref -- on feature records and truth arrays made by hand
as in tests/test_gpu_tune_score_edges.py, then DeviceTune.leaf_census and the command line.  Integer equality throughout."""
import json

import numpy as np
import pytest

from duet_amd import _lib, tune
from tests import tune_leaf_ref
from tests.test_gpu_tune_grid import scoring_workdir, write_truth
from tests.test_gpu_tune_score_edges import (FLIP, IN, MATCHED, RAISES, SAME, WS_BUDGET, control, cycle, level_features, per_vec_words,
                                             random_features, random_truth, random_vectors, truth_arrays)
from tests.test_gpu_tune_strata import random_case, read_tsv

pytestmark = pytest.mark.gpu

SUMMED = ('n_calls', 'call_tp', 'call_gt', 'call_hp', 'n_raise')       # the fields a sweep record shares with a leaf record
LEAF = {n: i for i, n in enumerate(_lib.LEAF_NAMES)}


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def device_census(ctx, feat, vecs, truth=None, cs=None, S=1):
    """duet_tune_leaf_census_device on arrays uploaded here -> LEAF_COUNTS_DTYPE[K, S, 18]"""
    import torch
    dev = torch.device('cuda:%d' % ctx.device_id)
    keep = []

    def up(a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        t = torch.zeros(a.nbytes + 64, dtype=torch.uint8, device=dev)
        if a.nbytes:
            t[:a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev)
        keep.append(t)
        return t.data_ptr()

    vecs = np.ascontiguousarray(vecs, dtype=np.float64).reshape(-1, 14)
    K, C = len(vecs), len(feat)
    t = None
    if truth is not None:
        t = _lib.TuneTruth()
        t.n_uid, t.n_groups, t.n_pairs = truth['n_uid'], truth['n_groups'], truth['n_pairs']
        for name, dt in _lib.TRUTH_ARRAYS:
            setattr(t, name, up(truth[name], dt))
    st = None
    if cs is not None:
        st = _lib.TuneStrata()
        st.n_strata, st.cand_stratum = S, up(cs, np.uint8)
    rec = _lib.LEAF_COUNTS_DTYPE.itemsize * _lib.N_LEAVES
    out = torch.full((max(K * S, 1) * rec,), 0xA5, dtype=torch.uint8, device=dev)     # (the entry zeroes the records itself)
    ctx.leaf_census_device(up(feat, _lib.FEATURE_DTYPE), C, up(vecs, np.float64), K, t, st, out.data_ptr(),
                           torch.cuda.current_stream(dev).cuda_stream)
    return out[:K * S * rec].cpu().numpy().view(_lib.LEAF_COUNTS_DTYPE).reshape(K, S, _lib.N_LEAVES).copy()


def same_records(got, want, what):
    assert got.dtype == _lib.LEAF_COUNTS_DTYPE and got.shape == want.shape, (what, got.shape, want.shape)
    for name in _lib.LEAF_COUNTS_NAMES:
        bad = np.argwhere(got[name] != want[name])
        assert bad.size == 0, '%s: %s differs at (vector, stratum, leaf) %s: %s, expected %s' % (
            what, name, bad[:5].tolist(), [int(got[name][tuple(b)]) for b in bad[:5]], [int(want[name][tuple(b)]) for b in bad[:5]])


def check(ctx, feat, vecs, truth=None, cs=None, S=1, want=None):
    """Both entries against the reference -> the reference"""
    want = want if want is not None else tune_leaf_ref.census(feat, vecs, truth, cs, S)
    strata = dict(n_strata=S, cand_stratum=cs) if cs is not None else None
    same_records(ctx.leaf_census_host(feat, vecs, truth, strata), want, 'host')
    same_records(device_census(ctx, feat, vecs, truth, cs, S), want, 'device')
    return want


def edge_vectors(seed, K):
    """random_vectors with an all-nan, an all-+inf and an all--inf vector among the first."""
    vecs = random_vectors(seed, K)
    vecs[1 % K], vecs[min(2, K - 1)], vecs[min(3, K - 1)] = np.nan, np.inf, -np.inf
    return vecs


def strata_of_groups(truth, S, seed):
    """cand_stratum: a function of the group for the candidates in the call list (a group lies inside one stratum), anything
    for the others."""
    rng = np.random.default_rng(seed)
    listed = (truth['cand_flags'] & IN) != 0
    return np.where(listed, truth['cand_group'] % S, rng.integers(0, S, len(listed))).astype(np.uint8)


# ---- shapes -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C', [0, 1, 63, 64, 65, 255, 256, 257, 513])
def test_shapes(ctx, C):
    feat = random_features(C, C)
    truth = random_truth(C + 1, C, n_groups=max(1, C // 9), n_uid=max(1, C // 2), fixed_uids=(0, max(1, C // 2) - 1))
    vecs = edge_vectors(C + 2, 65)
    want = tune_leaf_ref.census(feat, vecs, truth)
    bare = tune_leaf_ref.census(feat, vecs)
    if C >= 255:
        assert all(int(want[n].max()) > 0 for n in _lib.LEAF_COUNTS_NAMES)
        assert int((want['n_cands'].sum(axis=(0, 1)) > 0).sum()) == 18                    # every leaf is reached
    zeros = np.zeros(C, dtype=np.uint8)
    for K in (0, 1, 31, 32, 33, 65):                                                      # the last block of vectors holds K % 32
        check(ctx, feat, vecs[:K], truth, want=want[:K])
        check(ctx, feat, vecs[:K], None, want=bare[:K])                                   # truth == NULL: n_cands and n_calls only
        check(ctx, feat, vecs[:K], truth, zeros, 1, want=want[:K])                        # strata == NULL is S = 1


# ---- waves ------------------------------------------------------------------------------------------------------------------

def pool_by_leaf(seed=70, n=6000):
    """Eligible random records sorted by the leaf the default vector sends them to -> {leaf: records}.  The last 400 are made
    class 2 with one or two supporting reads and none for the reference: c2_near_few and c2_far_*, which are rare otherwise."""
    feat = random_features(seed, n, eligible=1.0)
    feat['cls'][-400:], feat['refread'][-400:] = 2, 0
    feat['svread'][-400:] = 1 + np.arange(400) % 2
    leaf, _ = tune_leaf_ref.leaves_from_features(feat, tune.vector())
    by = {l: feat[leaf == l] for l in range(18)}
    need = {l: 7 for l in range(18)}
    need.update({LEAF['c0_call']: 64, LEAF['c1_two_hom']: 64, LEAF['c1_two_mid_hom']: 64, LEAF['c2_near_call']: 64, LEAF['c2_low_ratio']: 64})
    assert all(len(by[l]) >= need[l] for l in range(18)), {l: len(by[l]) for l in range(18)}
    return by


@pytest.fixture(scope='module')
def pool():
    return pool_by_leaf()


def test_waves_of_all_leaves_of_one_leaf_and_without_a_listed_candidate(ctx, pool):
    """Wave 0 holds all 18 leaves (lane l in leaf l % 18), wave 1 a single leaf, wave 2 no listed candidate, wave 3 candidates
    that are flagged but not eligible among eligible ones of two leaves; wave 4 is cut by C."""
    one = lambda leaf, i: pool[leaf][i:i + 1]
    parts = [one(l % 18, l // 18) for l in range(64)] + [pool[LEAF['c1_two_mid_hom']][:64], pool[LEAF['c2_near_call']][:64]] + \
        [one((0, 17)[l % 2], 10 + l // 2) for l in range(64)] + [pool[LEAF['c0_call']][20:37]]
    feat = np.concatenate(parts)
    C = len(feat)
    assert C == 273
    rng = np.random.default_rng(71)
    flags = (IN | MATCHED | rng.integers(0, 512, C)).astype(np.uint16)
    flags[rng.random(C) < 0.15] = IN | RAISES
    flags[128:192] = 0
    feat['eligible'][192:256:3] = 0                                                      # flagged, grouped, matched -- and never decided
    truth = truth_arrays(flags, np.arange(C) % 11, rng.integers(0, 60, C), 11, 60)
    vecs = np.concatenate([tune.vector()[None, :], edge_vectors(72, 8)])
    want = check(ctx, feat, vecs, truth)
    d = want[0, 0]
    assert all(d['n_cands'][l] == 3 + (l < 10) for l in range(1, 17) if l not in (3, 15))  # wave 0: 64 lanes over 18 leaves
    assert d['n_cands'][LEAF['c1_two_mid_hom']] == 64 + 3 and d['n_cands'][LEAF['c2_near_call']] == 64 + 4
    assert d['n_listed'][LEAF['c2_near_call']] == 4 and int(d['n_cands'].sum()) == C - 22
    assert d['n_cands'][0] + d['n_cands'][17] == 7 + 42 + 17
    # the same candidates, no truth set
    check(ctx, feat, vecs, None)
    # and all of them not eligible: nothing anywhere
    feat['eligible'] = 0
    assert not any(check(ctx, feat, vecs, truth)[n].any() for n in _lib.LEAF_COUNTS_NAMES)


def test_a_group_over_three_leaves_and_two_tiles_with_a_tie(ctx, pool):
    """Group 1's calls: "same" in c0_call (tile 0) and c1_two_hom (tile 1), two truth ids: 2 + 2; "flip" in c0_call (tile 1),
    c1_two_het (tile 0) and c1_two_hom (tile 0), one truth id: 3 + 1.  The tie goes to flip, in every leaf."""
    C = 300
    filler = pool[LEAF['c2_low_ratio']]
    feat = np.array([filler[c % len(filler)] for c in range(C)])
    place = {10: ('c0_call', SAME, 0), 290: ('c1_two_hom', SAME, 1), 270: ('c0_call', FLIP, 2), 20: ('c1_two_het', FLIP, 2),
             200: ('c1_two_hom', FLIP, 2)}
    flags = np.full(C, IN, dtype=np.uint16)
    group, uid = np.zeros(C, dtype=np.int64), np.zeros(C, dtype=np.int64)
    for c, (leaf, bits, u) in place.items():
        feat[c] = pool[LEAF[leaf]][5]
        flags[c], group[c], uid[c] = IN | MATCHED | bits, 1, u
    # group 2: the same calls one "flip" short -- "same" wins there
    for c, (leaf, bits, u) in {30: ('c0_call', SAME, 3), 280: ('c1_two_hom', SAME, 4), 40: ('c1_two_het', FLIP, 5), 260: ('c0_call', FLIP, 5)}.items():
        feat[c] = pool[LEAF[leaf]][6]
        flags[c], group[c], uid[c] = IN | MATCHED | bits, 2, u
    truth = truth_arrays(flags, group, uid, 3, 6)
    want = check(ctx, feat, tune.vector()[None, :], truth)
    hp = want['call_hp'][0, 0]
    assert hp[LEAF['c0_call']] == 1 + 1 and hp[LEAF['c1_two_het']] == 1 and hp[LEAF['c1_two_hom']] == 1 + 1 and int(hp.sum()) == 5
    plain, _, _ = ctx.sweep_host(feat, tune.vector()[None, :], truth)
    assert int(plain['call_hp'][0]) == 5 and int(plain['n_groups'][0]) == 2


# ---- strata -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('S', [2, 64])
def test_strata_mixed_inside_waves(ctx, S):
    C = 513
    feat = random_features(80 + S, C, eligible=0.9)
    truth = random_truth(81 + S, C, n_groups=150, n_uid=200)
    cs = strata_of_groups(truth, S, 82)
    vecs = edge_vectors(83, 33)
    want = check(ctx, feat, vecs, truth, cs, S)
    assert int((want['n_calls'].sum(axis=(0, 2)) > 0).sum()) > S // 2 and int((want['n_cands'].sum(axis=(0, 2)) > 0).sum()) == S
    # identity 2: the strata sum to the S = 1 records
    same_records(tune_leaf_ref.summed(ctx.leaf_census_host(feat, vecs, truth, dict(n_strata=S, cand_stratum=cs)), 1),
                 ctx.leaf_census_host(feat, vecs, truth)[:, 0], 'sum over strata')
    check(ctx, feat, vecs[:3], None, cs, S)                                               # strata without a truth set


def test_identities_against_the_sweeps(ctx):
    """Summed over the leaves, the five shared fields are duet_tune_sweep_*'s and, per stratum, duet_tune_sweep_strata_*'s."""
    C, S = 700, 5
    feat = random_features(90, C)
    truth, strata = random_case(91, C, S)
    vecs = edge_vectors(92, 40)
    plain, _, _ = ctx.sweep_host(feat, vecs, truth)
    per = ctx.sweep_strata_host(feat, vecs, truth, strata)
    one = ctx.leaf_census_host(feat, vecs, truth)
    by = ctx.leaf_census_host(feat, vecs, truth, strata)
    for n in SUMMED:
        assert np.array_equal(one[n].sum(axis=2)[:, 0], plain[n]), n
        assert np.array_equal(by[n].sum(axis=2), per[n]), n
        assert np.array_equal(by[n].sum(axis=1), one[n][:, 0]), n
    assert int(plain['call_hp'].max()) > 20 and len(set(plain['call_hp'].tolist())) > 5
    same_records(device_census(ctx, feat, vecs, truth, strata['cand_stratum'], S), by, 'device')


def test_a_census_changes_no_later_sweep(ctx):
    C = 400
    feat = random_features(95, C)
    truth = random_truth(96, C, 40, 120)
    vecs = random_vectors(97, 70)
    before = ctx.sweep_host(feat, vecs, truth, want_pred=True, want_ps=True)
    check(ctx, feat, vecs[:40], truth, strata_of_groups(truth, 3, 98), 3)
    after = ctx.sweep_host(feat, vecs, truth, want_pred=True, want_ps=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))


# ---- batches ----------------------------------------------------------------------------------------------------------------

def test_several_batches(ctx):
    """The shape of test_gpu_tune_score_edges.test_several_batches: the sweep's workspace of K vectors exceeds its budget, so the
    census runs three batches (scratch sweep, labels and records offset by v0)."""
    C, K, n_uid = 300, 2300, 640000
    rng = np.random.default_rng(50)
    feat = level_features(rng.integers(1, 100, C), rng.integers(1, 4, C), rng.random(C) < 0.9)
    pairs = [(0, 0), (0, n_uid - 1), (1, 5), (1, n_uid - 1), (2, 320000)]
    which = rng.integers(0, 5, C)
    flags = (IN | MATCHED | rng.integers(0, 512, C)).astype(np.uint16)
    flags[rng.random(C) < 0.15] = IN
    truth = truth_arrays(flags, [pairs[i][0] for i in which], [pairs[i][1] for i in which], 3, n_uid)
    fit = WS_BUDGET // (per_vec_words(truth) * 4)
    assert -(-K // fit) == 3 and fit % 17 != 0
    distinct = np.stack([control(t) for t in (0, 100, 7, 13, 21, 29, 36, 42, 50, 58, 63, 71, 77, 84, 90, 95, 99)])
    at = cycle(distinct, K)
    want = tune_leaf_ref.census(feat, distinct, truth)
    assert len(set(want['call_hp'].sum(axis=(1, 2)).tolist())) > 10
    same_records(ctx.leaf_census_host(feat, distinct[at], truth), want[at], 'host')
    cs = strata_of_groups(truth, 2, 51)
    same_records(ctx.leaf_census_host(feat, distinct[at], truth, dict(n_strata=2, cand_stratum=cs)),
                 tune_leaf_ref.census(feat, distinct, truth, cs, 2)[at], 'host, two strata')


# ---- refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals(ctx):
    C = 100
    feat = random_features(60, C)
    truth = random_truth(61, C, 9, 30)
    vecs = random_vectors(62, 3)
    cs = strata_of_groups(truth, 3, 63)
    for S in (0, 65, 1 << 20):
        with pytest.raises(_lib.DuetLibraryError):
            ctx.leaf_census_host(feat, vecs, truth, dict(n_strata=S, cand_stratum=cs))
    with pytest.raises(_lib.DuetLibraryError):                                           # a stratum entry that is not below S
        ctx.leaf_census_host(feat, vecs, truth, dict(n_strata=2, cand_stratum=cs))
    wrong = dict(truth, cand_group=np.where(truth['cand_flags'] & IN, 9, 0))
    with pytest.raises(_lib.DuetLibraryError):                                           # a call's group that is not below n_groups
        ctx.leaf_census_host(feat, vecs, wrong)
    with pytest.raises(_lib.DuetLibraryError):                                           # a truth array that is needed and NULL
        ctx.leaf_census_host(feat, vecs, dict(truth, cand_flags=np.zeros(0, dtype=np.uint16)))
    import ctypes
    rc = ctx.lib.duet_tune_leaf_census_host(ctx.handle, feat.ctypes.data, C, vecs.ctypes.data, 3, None, None, None)
    assert rc != 0 and 'leaf record' in ctx.last_error()
    rc = ctx.lib.duet_tune_leaf_census_device(ctx.handle, None, C, None, 3, None, None, ctypes.c_void_p(16), None)
    assert rc != 0
    # nothing to do is no refusal: zeroed records
    assert ctx.leaf_census_host(feat, vecs[:0], truth).shape == (0, 1, 18)
    none = ctx.leaf_census_host(feat[:0], vecs, dict(truth, **{n: truth[n][:0] for n in ('cand_flags', 'cand_group', 'cand_uid', 'cand_pair')}))
    assert none.shape == (3, 1, 18) and not any(none[n].any() for n in _lib.LEAF_COUNTS_NAMES)
    check(ctx, feat, vecs, truth, cs, 3)                                                 # (the context goes on working)


# ---- DeviceTune and the command line ----------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def work(ctx, tmp_path_factory):
    d = tmp_path_factory.mktemp('leaf')
    home = str(d / 'w')
    scoring_workdir(home, 3)
    cands = tune.features(home, 50, 2, ctx=ctx)
    truth = str(d / 'truth.vcf')
    write_truth(cands, truth, 3)
    grid = str(d / 'g.json')
    with open(grid, 'w') as f:
        json.dump([{}, {'c1_max_ref_num': 3}, {'c2_min_sv_ratio': 0.5, 'c0_min_sv_num': 2, 'c1_twohap_sv_ratio_2': 'nan'}], f)
    texts = list(dict.fromkeys(cands['chrom']))
    assert len(texts) >= 3
    return dict(dir=d, home=home, cands=cands, truth=truth, grid=grid, vecs=tune.load_grid(grid), held=texts[:2])


def want_rows(lead, labels, feat, vecs, arrays, cands=None, held=None):
    """The data rows of --by_leaf for one setting, as text: stratum `all`, then train / test."""
    rows = tune.leaf_rows(lead, labels, tune_leaf_ref.census(feat, vecs, arrays))
    if held is not None:
        st = tune.strata_holdout(held)
        cs = np.array([tune.stratum_of(st, t) for t in cands['chrom']], dtype=np.uint8)
        rows += tune.leaf_rows(lead, labels, tune_leaf_ref.census(feat, vecs, arrays, cs, 2), ('train', 'test'))
    cols = tuple(lead) + tune.LEAF_COLS
    return [[repr(r[n]) if isinstance(r[n], float) else str(r[n]) for n in cols] for r in rows]


def test_device_tune_leaf_census(ctx, work):
    from duet_amd.devmem import DeviceTune
    cands, vecs = work['cands'], work['vecs']
    arrays = tune.prepare_truth(cands, work['truth'])
    C = len(cands['feat'])
    key, chrom, n_chrom = tune.candidate_keys(cands)
    dt = DeviceTune(C, tune.truth_side(work['truth']), 1000, 0.0, vectors=vecs)
    dt.set_candidates(cands['pos'], cands['svlen'], key, chrom, n_chrom)
    import torch
    dt.feat[:cands['feat'].nbytes] = torch.from_numpy(cands['feat'].view(np.uint8).copy()).to(dt.device)
    dt.build(ctx, C)
    plain = dt.sweep(ctx, C)
    got = dt.leaf_census(ctx, C)
    same_records(got, tune_leaf_ref.census(cands['feat'], vecs, arrays), 'the resident grid')
    for n in SUMMED:
        assert np.array_equal(got[n].sum(axis=2)[:, 0], plain[n]), n
    assert int(plain['call_hp'].max()) > 0
    other = edge_vectors(5, 7)
    same_records(dt.leaf_census(ctx, C, other), tune_leaf_ref.census(cands['feat'], other, arrays), 'vectors of its own')
    st = tune.strata_holdout(work['held'])
    b = tune.truth_side(work['truth'], strata=st)
    p = dt.set_strata(tune.chrom_strata(cands['chrom'], st), b['uid_off'], b['base_uid'])
    dt.build_strata(ctx, C, strata=p)
    cs = np.array([tune.stratum_of(st, t) for t in cands['chrom']], dtype=np.uint8)
    same_records(dt.leaf_census(ctx, C, strata=p), tune_leaf_ref.census(cands['feat'], vecs, arrays, cs, 2), 'the holdout pass')


def test_command_line_with_a_grid_and_holdout(ctx, work):
    out = lambda name: str(work['dir'] / name)
    home, truth, grid, cands, vecs = work['home'], work['truth'], work['grid'], work['cands'], work['vecs']
    arrays = tune.prepare_truth(cands, truth)
    tune.main([home, truth, '--grid', grid, '--out', out('plain.tsv')])
    tune.main([home, truth, '--grid', grid, '--out', out('leaf_out.tsv'), '--by_leaf', out('leaf.tsv')])
    with open(out('plain.tsv'), 'rb') as a, open(out('leaf_out.tsv'), 'rb') as b:
        assert a.read() == b.read()                                                       # --out does not change with --by_leaf
    rows = read_tsv(out('leaf.tsv'))
    assert rows[0] == list(tune.LEAF_COLS) and len(rows) == 1 + 3 * 18
    assert rows[1:] == want_rows({}, range(3), cands['feat'], vecs, arrays)
    assert sum(int(r[7]) for r in rows[1:19]) > 20 and any(r[-1] not in ('nan', '0.0', '1.0') for r in rows[1:])
    held = work['held']
    tune.main([home, truth, '--grid', grid, '--out', out('h.tsv'), '--holdout', ','.join(held)])
    tune.main([home, truth, '--grid', grid, '--out', out('h_leaf.tsv'), '--holdout', ','.join(held), '--by_leaf', out('leaf_h.tsv'),
               '--by_contig', out('contigs.tsv')])
    with open(out('h.tsv'), 'rb') as a, open(out('h_leaf.tsv'), 'rb') as b:
        assert a.read() == b.read()
    rows = read_tsv(out('leaf_h.tsv'))
    assert len(rows) == 1 + 3 * 18 * 3 and [r[1] for r in rows[1::18]][:5] == ['all', 'all', 'all', 'train', 'test']
    assert rows[1:] == want_rows({}, range(3), cands['feat'], vecs, arrays, cands, held)
    assert sum(int(r[7]) for r in rows[1:] if r[1] == 'test') > 0 and sum(int(r[7]) for r in rows[1:] if r[1] == 'train') > 0


def test_command_line_with_caps_and_settings(ctx, work):
    out = lambda name: str(work['dir'] / name)
    home, truth, grid, cands, vecs = work['home'], work['truth'], work['grid'], work['cands'], work['vecs']
    tune.main([home, truth, '--grid', grid, '--out', out('caps.tsv'), '--pc_cap', '2400,8100', '-r', '2,3', '--by_leaf', out('leaf_caps.tsv')])
    rows = read_tsv(out('leaf_caps.tsv'))
    lead = ('pc_cap', 'svlen_thres', 'suppread_thres')
    assert rows[0] == list(lead) + list(tune.LEAF_COLS) and len(rows) == 1 + 4 * 3 * 18
    want, differ = [], []
    for r_ in (2, 3):
        for cap in (2400, 8100):
            feat = ctx.features_host(cands['soa'], 50, r_, pc_cap=cap)
            arrays = tune.prepare_truth(dict(cands, feat=feat), truth)
            want += want_rows(dict(pc_cap=cap, svlen_thres=50, suppread_thres=r_), range(3), feat, vecs, arrays)
            differ.append(feat.tobytes())
    assert rows[1:] == want and len(set(differ)) >= 2


def test_command_line_with_fit(ctx, work):
    out = lambda name: str(work['dir'] / name)
    home, truth, cands, held = work['home'], work['truth'], work['cands'], work['held']
    arrays = tune.prepare_truth(cands, truth)
    args = [home, truth, '--fit', 'hp_f1', '--rounds', '2', '--axes', 'c1_max_ref_num,c2_min_sv_ratio,c1_twohap_sv_ratio_2']
    tune.main(args + ['--out_vector', out('best.json'), '--trace', out('fit.tsv'), '--by_leaf', out('leaf_fit.tsv'), '--holdout', ','.join(held)])
    tune.main(args + ['--out_vector', out('best1.json'), '--trace', out('fit1.tsv'), '--holdout', ','.join(held)])
    for a, b in (('best.json', 'best1.json'), ('fit.tsv', 'fit1.tsv')):
        with open(out(a), 'rb') as fa, open(out(b), 'rb') as fb:
            assert fa.read() == fb.read()                                                 # the fit's own files do not change
    fitted = tune.load_vector(out('best.json'))
    rows = read_tsv(out('leaf_fit.tsv'))
    lead = dict(svlen_thres=50, suppread_thres=2)
    assert rows[0] == list(lead) + list(tune.LEAF_COLS) and len(rows) == 1 + 2 * 3 * 18
    want = want_rows(lead, ('start',), cands['feat'], tune.vector()[None, :], arrays, cands, held) + \
        want_rows(lead, ('fitted',), cands['feat'], fitted[None, :], arrays, cands, held)
    assert rows[1:] == want
    start, end = ([r for r in rows[1:] if r[2] == v and r[3] == 'all'] for v in ('start', 'fitted'))
    if not np.array_equal(fitted, tune.vector()):                                         # the fit moved candidates between leaves
        assert [r[4:] for r in start] != [r[4:] for r in end]
    assert sum(int(r[7]) for r in end) > 0
