# coding=utf-8
"""-m gpu: the sweep's truth arrays built on the device (duet_tune_truth_build_host / _device, duet_amd/csrc/duet_tune_truth.hip)
against tune.prepare_truth, the normative text, on hand-made inputs: every case states its candidates and truth records once;
prepare_truth reads them as text (rows and a truth VCF), the device gets them as the SoA arrays this file derives by hand
(hand_key, hand_base -- not through tune.candidate_keys / tune.truth_side).

Flags, truth ids and the two counts must agree exactly; groups and pairs up to renumbering (same_partition, the offsets' rules).
Each case also asserts that the reference side holds what the case is about.

The length-ratio cases: a candidate or truth record shorter than 50 never reaches the match (the parser drops it), so the pairs
(7, 10), (49, 70) and (3, 10) are stated a hundredfold -- (700, 1000), (4900, 7000), (300, 1000): the same rationals, hence the
same binary64 quotients, which is what the cases are about (7 / 10 == 49 / 70 in binary64 although 7 * 70 == 49 * 10 only in
exact arithmetic would say so; 3 / 10 < 0.1 + 0.2)."""
import numpy as np
import pytest

from duet_amd import _lib, evaluation, tune

pytestmark = pytest.mark.gpu

IN, RAISES, MATCHED = _lib.TUNE_IN_CALLS, _lib.TUNE_RAISES, _lib.TUNE_MATCHED
NONE, SKIP = _lib.TUNE_KEY_NONE, _lib.TUNE_KEY_SKIP
TYPES = ('DEL', 'INS', 'INV', 'DUP')


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def cand(chrom, pos, ln, svtype, ps, elig=1, alt=None):
    return dict(chrom=chrom, pos=pos, len=ln, type=svtype, ps=ps, elig=elig, alt=alt or '<%s>' % svtype)


def hand_key(chrom, svtype, alt):
    """What evaluation.parse_vcf makes of the row 'chrom ... N alt ... SVLEN=..;SVTYPE=<svtype>': list key, NONE or SKIP."""
    if chrom[3:] not in evaluation.LABELS:
        return SKIP
    if not any(k in svtype or k in alt for k in ('INS', 'DEL', 'DUP')):
        return SKIP
    t = alt[1:-1] if alt in ('<INS>', '<DEL>', '<DUP:TANDEM>', '<DUP:INT>', '<DUP>') else '<%s>' % svtype
    if 'DUP' in t:
        t = 'INS'
    if chrom in evaluation.CHROMS and t in ('INS', 'DEL'):
        return 2 * evaluation.CHROMS.index(chrom) + ('INS', 'DEL').index(t)
    return NONE


def hand_base(truth):
    """truth: (chrom, pos, len, type, id, hp), every one kept by the parser -> the truth side's arrays."""
    uid, lists = {}, [[] for _ in range(2 * len(evaluation.CHROMS))]
    for chrom, pos, ln, t, name, hp in truth:
        u = uid.setdefault(name + chrom + str(pos), len(uid))
        if chrom in evaluation.CHROMS:
            lists[2 * evaluation.CHROMS.index(chrom) + ('INS', 'DEL').index(t)].append((pos, ln, u, {'1|0': 0, '0|1': 1, '1|1': 2}.get(hp, 3)))
    off, rows = [0], []
    for lst in lists:
        rows.extend(sorted(lst, key=lambda r: r[0]))
        off.append(len(rows))
    col = lambda i, dt: np.array([r[i] for r in rows], dtype=dt)
    return dict(base_off=np.array(off, dtype=np.uint32), base_pos=col(0, np.uint32), base_len=col(1, np.uint32),
                base_uid=col(2, np.uint32), base_hp=col(3, np.uint8), n_base_uid=len(uid))


def features_of(cands):
    feat = np.zeros(len(cands), dtype=_lib.FEATURE_DTYPE)
    feat['eligible'] = [c['elig'] for c in cands]
    feat['kept'] = feat['eligible']
    feat['ps'] = [c['ps'] for c in cands]
    return feat


def reference(tmp_path, cands, truth, refdist, ratio, bed=''):
    path = str(tmp_path / 'truth.vcf')
    with open(path, 'w') as f:
        f.write('##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n')
        for chrom, pos, ln, t, name, hp in truth:
            f.write('%s\t%d\t%s\tN\t<%s>\t.\tPASS\tSVTYPE=%s;SVLEN=%d\tGT:PS\t%s:1\n' % (chrom, pos, name, t, t, ln if t == 'INS' else -ln, hp))
    d = dict(feat=features_of(cands), chrom=[c['chrom'] for c in cands], pos=np.array([c['pos'] for c in cands], dtype=np.uint32),
             svlen=np.array([c['len'] for c in cands], dtype=np.uint32), ref=['N'] * len(cands), alt=[c['alt'] for c in cands],
             svtype=[c['type'] for c in cands])
    ref = tune.prepare_truth(d, path, refdist, ratio, bed)
    assert ref['n_base'] == len(truth)                    # (the hand-made truth side holds what the parser keeps)
    return ref


def same_partition(a, b):
    """Two labellings put the same elements together."""
    fwd, back = {}, {}
    return all(fwd.setdefault(x, y) == y and back.setdefault(y, x) == x for x, y in zip(a.tolist(), b.tolist()))


def compare(ref, got):
    C = len(ref['cand_flags'])
    assert np.array_equal(got['cand_flags'][:C], ref['cand_flags']), (got['cand_flags'][:C], ref['cand_flags'])
    assert np.array_equal(got['cand_uid'][:C], ref['cand_uid'])
    assert (got['n_groups'], got['n_pairs'], got['n_uid']) == (ref['n_groups'], ref['n_pairs'], ref['n_uid'])
    G, P = got['n_groups'], got['n_pairs']
    fl = ref['cand_flags']
    calls, hits = np.nonzero(fl & IN)[0], np.nonzero(fl & MATCHED)[0]
    g, p, off, pu = got['cand_group'], got['cand_pair'], got['group_pair_off'].astype(np.int64), got['pair_uid']
    # every output of a candidate that is not a call is 0; so is the pair of one that is not matched
    assert not g[(fl & IN) == 0].any() and not p[(fl & MATCHED) == 0].any()
    assert len(off) == G + 1 and len(pu) == P
    # two candidates share a device group iff they share a reference group; the ids are dense
    assert same_partition(g[calls], ref['cand_group'][calls]) and sorted(set(g[calls].tolist())) == list(range(G))
    assert off[0] == 0 and off[G] == P and (np.diff(off) >= 0).all()
    ref_off = ref['group_pair_off']
    for c in calls:                                        # also for a group without any pair
        rg = int(ref['cand_group'][c])
        assert off[g[c] + 1] - off[g[c]] == ref_off[rg + 1] - ref_off[rg]
    for c in hits:
        assert pu[p[c]] == got['cand_uid'][c]
        assert off[g[c]] <= p[c] < off[g[c] + 1]
    assert same_partition(p[hits], ref['cand_pair'][hits]) and sorted(set(p[hits].tolist())) == list(range(P))


def device_build(ctx, feat, arrays, refdist, ratio):
    """duet_tune_truth_build_device on resident copies (devmem.DeviceTune) -> the same dict truth_build_host returns."""
    from duet_amd.devmem import DeviceTune
    C = len(feat)
    dt = DeviceTune(C, arrays, refdist, ratio, tune.vector()[None, :])
    if C:
        dt.feat[:feat.nbytes] = dt.torch.from_numpy(feat.view(np.uint8).copy()).to(dt.device)
    result = None
    if 'key_table' not in arrays:
        dt.set_candidates(arrays['cand_pos'], arrays['cand_len'], arrays['cand_key'], arrays['cand_chrom'], arrays['n_chrom'])
    else:
        bed = tuple(arrays[k] for k in ('bed_off', 'bed_lo', 'bed_hi')) if 'bed_off' in arrays else None
        dt.set_tables(arrays['key_table'], arrays['chrom_id'], arrays['n_chrom'], bed)
        result = _lib.ClusterResult()
        result.cand_contig, result.cand_type = dt._up('cc', arrays['cand_contig'], np.uint16), dt._up('ct', arrays['cand_type'], np.uint8)
        result.cand_pos, result.cand_span = dt._up('cp', arrays['cand_pos'], np.uint32), dt._up('cs', arrays['cand_len'], np.uint32)
    dt.build(ctx, C, result)
    t = dt.truth
    size = dict(group_pair_off=t.n_groups + 1, pair_uid=t.n_pairs)
    out = {name: dt.keep[name][:size.get(name, C) * np.dtype(d).itemsize].cpu().numpy().view(d).copy() for name, d in _lib.TRUTH_ARRAYS}
    out.update(n_uid=t.n_uid, n_groups=t.n_groups, n_pairs=t.n_pairs)
    return out


def run_case(ctx, tmp_path, cands, truth, refdist=1000, ratio=0.0):
    """Per-candidate form through both entries -> the reference arrays (for the case's own assertions)."""
    ref = reference(tmp_path, cands, truth, refdist, ratio)
    ids = {}
    arrays = dict(hand_base(truth), cand_pos=np.array([c['pos'] for c in cands], dtype=np.uint32),
                  cand_len=np.array([c['len'] for c in cands], dtype=np.uint32),
                  cand_key=np.array([hand_key(c['chrom'], c['type'], c['alt']) for c in cands], dtype=np.uint32),
                  cand_chrom=np.array([ids.setdefault(c['chrom'], len(ids)) for c in cands], dtype=np.uint32), n_chrom=max(len(ids), 1))
    feat = features_of(cands)
    assert ref['n_uid'] == arrays['n_base_uid']
    compare(ref, ctx.truth_build_host(feat, arrays, refdist, ratio))
    compare(ref, device_build(ctx, feat, arrays, refdist, ratio))
    return ref


def some_truth(n=40, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        out.append(('chr%d' % (1 + i % 2), int(rng.integers(1000, 200000)), int(rng.integers(50, 900)), ('INS', 'DEL')[int(rng.integers(2))],
                    't%d' % i, ('1|0', '0|1', '1|1', '1|2')[int(rng.integers(4))]))
    return out


@pytest.mark.parametrize('C', [0, 1, 63, 64, 65, 257])
def test_sizes(ctx, tmp_path, C):
    truth = some_truth()
    rng = np.random.default_rng(C)
    cands = []
    for i in range(C):
        t = truth[int(rng.integers(len(truth)))]
        near = i % 3 != 2
        cands.append(cand(t[0], t[1] + (int(rng.integers(-300, 300)) if i else 0) if near else int(rng.integers(1000, 200000)),
                          int(t[2] * rng.uniform(0.7, 1.3)) + 1, t[3], int(rng.integers(1, 9)), elig=int(i % 7 != 3)))
    ref = run_case(ctx, tmp_path, cands, truth, 200, 0.5)
    assert ref['n_base'] == len(truth)
    if C:
        assert (ref['cand_flags'] & MATCHED).any()
    if C >= 63:
        assert ref['n_pairs'] > 8 and ref['n_groups'] > 8 and ((ref['cand_flags'] & (IN | MATCHED)) == IN).any()


def test_no_eligible_candidate(ctx, tmp_path):
    truth = some_truth()
    ref = run_case(ctx, tmp_path, [cand(t[0], t[1], t[2], t[3], 5, elig=0) for t in truth[:30]], truth)
    assert len(ref['cand_flags']) == 30 and not ref['cand_flags'].any() and ref['n_groups'] == 0 and ref['n_pairs'] == 0


def test_one_record_list_left_on_right(ctx, tmp_path):
    truth = [('chr1', 5000, 100, 'INS', 'a', '1|0')]
    ref = run_case(ctx, tmp_path, [cand('chr1', p, 100, 'INS', 3) for p in (4000, 4999, 5000, 5001, 6000, 6001, 3999)], truth)
    assert [bool(f & MATCHED) for f in ref['cand_flags']] == [True, True, True, True, True, False, False]


def test_tie_goes_right_and_equal_positions_take_the_first(ctx, tmp_path):
    truth = [('chr1', 1000, 100, 'DEL', 'left', '1|0'), ('chr1', 1200, 100, 'DEL', 'right', '0|1'),
             ('chr1', 3000, 100, 'DEL', 'x1', '1|0'), ('chr1', 3000, 100, 'DEL', 'x2', '0|1'), ('chr1', 3000, 100, 'DEL', 'x3', '1|1')]
    cands = [cand('chr1', 1100, 100, 'DEL', 1), cand('chr1', 1099, 100, 'DEL', 1), cand('chr1', 1101, 100, 'DEL', 1),
             cand('chr1', 2990, 100, 'DEL', 1), cand('chr1', 3000, 100, 'DEL', 1), cand('chr1', 3010, 100, 'DEL', 1)]
    ref = run_case(ctx, tmp_path, cands, truth)
    # ids number the records in file order: left 0, right 1, x1 2, x3 4
    assert ref['cand_uid'].tolist() == [1, 0, 1, 2, 2, 4]                  # (behind the last record the insertion point is the end: its left neighbour)


def test_refdist_edge(ctx, tmp_path):
    truth = [('chr2', 50000, 100, 'INS', 'a', '1|1')]
    ref = run_case(ctx, tmp_path, [cand('chr2', 50000 + d, 100, 'INS', 1) for d in (-300, 300, -301, 301)], truth, refdist=300)
    assert [bool(f & MATCHED) for f in ref['cand_flags']] == [True, True, False, False]


@pytest.mark.parametrize('ratio', [0.7, 0.3, 0.1 + 0.2])
def test_length_ratio_in_binary64(ctx, tmp_path, ratio):
    truth = [('chr1', 1000, 1000, 'INS', 'a', '1|0'), ('chr1', 5000, 7000, 'INS', 'b', '1|0'), ('chr1', 9000, 1000, 'INS', 'c', '1|0'),
             ('chr1', 13000, 700, 'INS', 'd', '1|0')]
    cands = [cand('chr1', 1000, 700, 'INS', 1), cand('chr1', 5000, 4900, 'INS', 1), cand('chr1', 9000, 300, 'INS', 1),
             cand('chr1', 13000, 1000, 'INS', 1)]
    ref = run_case(ctx, tmp_path, cands, truth, ratio=ratio)
    want = {0.7: [True, True, False, True], 0.3: [True, True, True, True], 0.1 + 0.2: [True, True, False, True]}[ratio]
    assert [bool(f & MATCHED) for f in ref['cand_flags']] == want


def test_empty_list_raises_and_keys_without_a_list(ctx, tmp_path):
    truth = [('chr1', 1000, 100, 'INS', 'a', '1|0')]
    cands = [cand('chr1', 1000, 100, 'INS', 1),                       # matched
             cand('chr1', 1000, 100, 'DEL', 1),                       # chr1 DEL: an empty list
             cand('chr2', 1000, 100, 'INS', 1),                       # chr2: an empty list
             cand('chr1', 1000, 100, 'INS', 1, alt='ACGT'),           # type '<INS>': kept, no list
             cand('abc1', 1000, 100, 'INS', 1),                       # label 1, not chr1: kept, no list
             cand('chr1', 1000, 100, 'INV', 1),                       # dropped
             cand('chrUn', 1000, 100, 'INS', 1),                      # dropped
             cand('chr1', 1000, 100, 'DUP', 1)]                       # DUP counts as INS
    ref = run_case(ctx, tmp_path, cands, truth)
    assert ref['cand_flags'].tolist()[1:3] == [IN | RAISES, IN | RAISES]
    assert ref['cand_flags'].tolist()[3:7] == [IN, IN, 0, 0]
    assert ref['cand_flags'][0] & MATCHED and ref['cand_flags'][7] & MATCHED
    assert ref['n_groups'] == 3                                        # chr1_:1, chr2_:1, abc1_:1


def test_length_49_and_50(ctx, tmp_path):
    truth = [('chr1', 1000, 60, 'INS', 'a', '1|0')]
    ref = run_case(ctx, tmp_path, [cand('chr1', 1000, 49, 'INS', 1), cand('chr1', 1000, 50, 'INS', 1), cand('chr1', 1000, 49, 'INS', 2)], truth)
    assert ref['cand_flags'][0] == 0 and ref['cand_flags'][1] & MATCHED and ref['n_groups'] == 1


def test_key_bits_above_32(ctx, tmp_path):
    big = 2 ** 32 - 2
    truth = [('chr1', 1000, 100, 'INS', 'a', '1|0'), ('chr2', 1000, 100, 'INS', 'b', '1|0')]
    cands = [cand('chr1', 1000, 100, 'INS', 7), cand('chr2', 1000, 100, 'INS', big), cand('chr2', 1100, 100, 'INS', big),
             cand('chr2', 1000, 100, 'INS', 7), cand('chr1', 1200, 100, 'INS', big), cand('chr2', 1300, 100, 'INS', big - 1)]
    ref = run_case(ctx, tmp_path, cands, truth)
    # one ps under two CHROM ids: two groups
    assert ref['n_groups'] == 5 and ref['cand_group'][1] == ref['cand_group'][2] != ref['cand_group'][4]
    assert ref['cand_group'][0] != ref['cand_group'][3]


@pytest.mark.parametrize('own', [True, False])
def test_every_candidate_its_own_group_or_all_in_one(ctx, tmp_path, own):
    truth = some_truth(30, 5)
    cands = [cand(t[0] if own else 'chr1', t[1] + 5, t[2], t[3], 100 + i if own else 9) for i, t in enumerate(truth * 5)]
    ref = run_case(ctx, tmp_path, cands, truth)
    assert ref['n_groups'] == (len(cands) if own else 1) and ref['n_pairs'] > 10


def test_one_uid_from_one_group_and_from_two(ctx, tmp_path):
    # two truth records share the id string (ID + CHROM + POS) and differ in type: one uid in two lists
    truth = [('chr1', 1000, 100, 'INS', 'a', '1|0'), ('chr1', 1000, 100, 'DEL', 'a', '0|1'), ('chr1', 9000, 100, 'INS', 'b', '1|1')]
    cands = [cand('chr1', 1000, 100, 'INS', 1), cand('chr1', 1001, 100, 'DEL', 1),            # same group: one pair
             cand('chr1', 1002, 100, 'INS', 2), cand('chr1', 1003, 100, 'DEL', 3),            # two groups: two pairs
             cand('chr1', 50000, 100, 'INS', 4), cand('chr1', 50001, 100, 'DEL', 4)]          # a group without a match
    ref = run_case(ctx, tmp_path, cands, truth)
    assert ref['n_uid'] == 2 and ref['cand_uid'].tolist()[:4] == [0, 0, 0, 0]
    assert ref['n_groups'] == 4 and ref['n_pairs'] == 3 and ref['cand_pair'][0] == ref['cand_pair'][1]
    g = int(ref['cand_group'][4])
    assert ref['group_pair_off'][g] == ref['group_pair_off'][g + 1]


def test_haplotype_codes(ctx, tmp_path):
    truth = [('chr1', 1000 * (i + 1), 100, 'INS', 'h%d' % i, hp) for i, hp in enumerate(('1|0', '0|1', '1|1', '1|2'))]
    ref = run_case(ctx, tmp_path, [cand('chr1', 1000 * (i + 1), 100, 'INS', 1) for i in range(4)], truth)
    low = [int(f) & 0x1FF for f in ref['cand_flags']]
    #           p = 1: gt same | p = 2: gt flip     p = 1: gt flip | p = 2: gt same     p = 3: all three
    assert low == [0b000101011, 0b000011101, 0b111000000, 0] and all(f & MATCHED for f in ref['cand_flags'])


def test_table_and_bed_form(ctx, tmp_path):
    """The table form (cluster result columns, key_table, chrom_id, BED ranges) through both entries: the four type codes, two
    contigs sharing a CHROM text (one group), a contig without ranges, positions on a range's closed ends and one past them."""
    texts = ['chr1', 'chr1', 'chr2', 'chr3', '4']
    ranges = {0: [(900, 1100), (5000, 5000)], 1: [(900, 1100), (5000, 5000)], 2: [(0, 100000)], 3: []}       # merged, sorted, closed
    truth = [('chr1', 1000, 100, 'INS', 'a', '1|0'), ('chr1', 1000, 100, 'DEL', 'b', '0|1'), ('chr2', 2000, 100, 'INS', 'c', '1|1'),
             ('chr1', 5000, 100, 'INS', 'd', '1|0')]
    rows = [(0, 1, 1000, 100, 7), (1, 1, 1001, 100, 7),                # contigs 0 and 1 are both chr1: one group, one pair
            (0, 0, 1000, 100, 8), (0, 2, 1000, 100, 8), (0, 3, 1002, 100, 8),      # DEL, INV (dropped), DUP (counts as INS)
            (0, 1, 899, 100, 9), (0, 1, 900, 100, 9), (0, 1, 1100, 100, 9), (0, 1, 1101, 100, 9), (1, 1, 5000, 100, 9), (1, 1, 5001, 100, 9),
            (2, 1, 2000, 100, 7), (2, 0, 2000, 100, 7),                # chr2 DEL: an empty list
            (3, 1, 1000, 100, 7),                                      # chr3 has no range: dropped
            (4, 1, 1000, 100, 7)]                                      # '4': dropped by the label test
    cands = [cand(texts[k], pos, ln, TYPES[t], ps) for k, t, pos, ln, ps in rows]
    bed = str(tmp_path / 'r.bed')
    with open(bed, 'w') as f:
        for k in (0, 2):
            for a, b in ranges[k]:
                f.write('%s\t%d\t%d\n' % (texts[k], a, b))
    ref = reference(tmp_path, cands, truth, 1000, 0.0, bed)
    fl = ref['cand_flags'].tolist()
    assert [bool(x & IN) for x in fl] == [True, True, True, False, True, False, True, True, False, True, False, True, True, False, False]
    assert fl[12] == IN | RAISES and ref['cand_group'][0] == ref['cand_group'][1] and ref['cand_pair'][0] == ref['cand_pair'][1]
    ids = {}
    chrom_id = np.array([ids.setdefault(t, len(ids)) for t in texts], dtype=np.uint32)
    key_table = np.array([hand_key(text, t, '<%s>' % t) for text in texts for t in TYPES], dtype=np.uint32)
    bed_off = np.cumsum([0] + [len(ranges.get(k, [])) for k in range(len(texts))]).astype(np.uint32)
    flat = [r for k in range(len(texts)) for r in ranges.get(k, [])]
    table = (bed_off, np.array([a for a, _ in flat], dtype=np.uint32), np.array([b for _, b in flat], dtype=np.uint32))
    arrays = dict(hand_base(truth), cand_pos=np.array([r[2] for r in rows], dtype=np.uint32), cand_len=np.array([r[3] for r in rows], dtype=np.uint32),
                  cand_contig=np.array([r[0] for r in rows], dtype=np.uint16), cand_type=np.array([r[1] for r in rows], dtype=np.uint8),
                  key_table=key_table, chrom_id=chrom_id, n_chrom=len(ids), bed_off=table[0], bed_lo=table[1], bed_hi=table[2])
    feat = features_of(cands)
    compare(ref, ctx.truth_build_host(feat, arrays, 1000, 0.0))
    compare(ref, device_build(ctx, feat, arrays, 1000, 0.0))
    # without the BED ranges nothing is dropped for its position
    ref = reference(tmp_path, cands, truth, 1000, 0.0)
    assert bool(ref['cand_flags'][5] & IN) and bool(ref['cand_flags'][13] & IN)
    for k in ('bed_off', 'bed_lo', 'bed_hi'):
        del arrays[k]
    compare(ref, ctx.truth_build_host(feat, arrays, 1000, 0.0))
    compare(ref, device_build(ctx, feat, arrays, 1000, 0.0))
