# coding=utf-8
"""No GPU: the meaning of the stratified sweep.  tests/tune_strata_ref.py (the masked re-run on tests/tune_score_ref.py) equals
evaluation.evaluation on the callset and the truth set restricted to a stratum's CHROM texts -- on synthetic work directories of
three contigs and on hand-written rows: an id text that two contigs share, strata where the restricted evaluator raises -- and
tune.truth_side(strata=..) numbers the truth ids as include/duet_ef.h's duet_tune_strata asks."""
import math

import numpy as np
import pytest

from duet_amd import _lib, tune
from duet_amd import evaluation as E
from tests import tune_ref, tune_score_ref, tune_strata_ref
from tests.test_gpu_tune import random_vectors, scoring_workdir, write_truth
from tests.test_gpu_tune_score_edges import control, level_features, random_features, random_truth
from tests.test_gpu_tune_score_edges import random_vectors as vectors_near_defaults
from tests.test_score_refs_host import host_candidates

NAN10 = (math.nan,) * 10
HEAD = '##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n'


def restricted(truth_recs, call_recs, strata, s, refdist, pctsim):
    """The unmodified evaluator on the records whose CHROM text is in stratum s; nan where it raises."""
    keep = lambda recs: [r for r in recs if tune.stratum_of(strata, r['chr']) == s]
    try:
        return tuple(float(x) for x in E.evaluation(keep(truth_recs), keep(call_recs), refdist, pctsim))
    except (ZeroDivisionError, IndexError):
        return NAN10


def cand_strata(cands, strata):
    return np.array([tune.stratum_of(strata, t) for t in cands['chrom']], dtype=np.uint8)


def check_against_evaluator(tmp_path, cands, truth_vcf, called_text, vecs, strata, refdist=1000, pctsim=0.0, skip=False):
    """-> [K][S] the reference's ten numbers, each compared with the restricted evaluator's."""
    arrays = tune.prepare_truth(cands, truth_vcf, refdist, pctsim, '', skip)
    S = len(strata['names'])
    counts = tune_strata_ref.counts(cands['feat'], vecs, arrays, cand_strata(cands, strata), S)
    truth_recs = E.parse_vcf(truth_vcf, skip, '')
    n_base = [sum(1 for r in truth_recs if tune.stratum_of(strata, r['chr']) == s) for s in range(S)]
    out = []
    for k, v in enumerate(vecs):
        called = str(tmp_path / 'called.vcf')
        with open(called, 'w') as f:
            f.write(called_text(v))
        call_recs = E.parse_vcf(called, skip, '')
        row = []
        for s in range(S):
            got = tune.scores(counts[k, s], n_base[s])
            want = restricted(truth_recs, call_recs, strata, s, refdist, pctsim)
            assert tune_ref.same_floats(got, want), (k, strata['names'][s], counts[k, s], got, want)
            row.append(got)
        out.append(row)
    return out


@pytest.mark.parametrize('seed,kind,refdist,pctsim,skip', [(3, 'by_contig', 1000, 0.0, False), (3, 'holdout', 1000, 0.0, False),
                                                           (6, 'by_contig', 300, 0.7, False), (3, 'holdout', 1000, 0.0, True)],
                         ids=['by_contig', 'holdout_of_two_contigs', 'pctsim_0.7', 'skip_phasing'])
def test_reference_equals_the_restricted_evaluator(tmp_path, seed, kind, refdist, pctsim, skip):
    home = str(tmp_path / 'w')
    scoring_workdir(home, seed)
    cands = host_candidates(home)
    texts = list(dict.fromkeys(cands['chrom']))
    assert len(texts) >= 3 and int(cands['feat']['eligible'].sum()) > 20
    truth = str(tmp_path / 'truth.vcf')
    write_truth(home, cands, truth, seed)
    strata = tune.strata_by_contig() if kind == 'by_contig' else tune.strata_holdout(texts[:2])
    vecs = np.concatenate([tune.vector()[None, :], random_vectors(cands['feat'], 3, seed)])
    rows = check_against_evaluator(tmp_path, cands, truth, lambda v: tune_ref.phased_text(home, 50, 2, v), vecs, strata, refdist, pctsim,
                                   skip)
    scored = [s for s in range(len(strata['names'])) if not math.isnan(rows[0][s][1])]
    assert len(scored) >= (3 if kind == 'by_contig' else 2)               # (several strata have numbers, and they differ)
    assert len(set(rows[0][s] for s in scored)) == len(scored)


# ---- hand-written rows ------------------------------------------------------------------------------------------------------

def hand_cands(rows):
    """rows: (chrom, pos, svtype, svlen, ps) -> cands as tune.features returns them, every candidate emitted by control(0)."""
    feat = level_features(np.full(len(rows), 10), [1 + i % 3 for i in range(len(rows))])
    feat['ps'] = [r[4] for r in rows]
    return dict(feat=feat, chrom=[r[0] for r in rows], pos=np.array([r[1] for r in rows], dtype=np.uint32),
                svtype=[r[2] for r in rows], svlen=np.array([r[3] for r in rows], dtype=np.uint32), ref=['N'] * len(rows),
                alt=['<%s>' % r[2] for r in rows])


def hand_called(cands):
    def text(v):
        pred = tune_ref.preds_from_features(cands['feat'], v)
        return HEAD + ''.join(tune.row_text(cands['chrom'][c], int(cands['pos'][c]), c + 1, 'N', cands['alt'][c], int(cands['svlen'][c]),
                                            cands['svtype'][c], tune.HP_TEXT[p], int(cands['feat']['ps'][c]))
                              for c, p in enumerate(pred) if p)
    return text


def write_truth_rows(path, rows):
    """rows: (chrom, pos, id, svtype, svlen, hp)"""
    with open(path, 'w') as f:
        f.write(HEAD)
        for ch, pos, rid, t, ln, hp in rows:
            f.write('%s\t%d\t%s\tN\t<%s>\t.\tPASS\tSVTYPE=%s;SVLEN=%d\tGT:PS\t%s:1\n' % (ch, pos, rid, t, t, ln if t == 'INS' else -ln, hp))


SHARED = [('chr1', 2345678, '.', 'INS', 100, '1|0'), ('chr12', 345678, '.', 'INS', 100, '0|1'), ('chr3', 500, 't3', 'DEL', 80, '1|1')]


@pytest.mark.parametrize('held,n_ids', [(['chr1', 'chr12'], (1, 1)), (['chr12'], (2, 1))], ids=['one_stratum', 'two_strata'])
def test_an_id_text_that_two_contigs_share(tmp_path, held, n_ids):
    """'.' + 'chr1' + '2345678' == '.' + 'chr12' + '345678': matched on both contigs, the id counts once in a stratum that holds
    both contigs and once in each stratum when they are apart."""
    truth = str(tmp_path / 'truth.vcf')
    write_truth_rows(truth, SHARED)
    recs = E.parse_vcf(truth, False, '')
    assert recs[0]['id'] == recs[1]['id'] == '.chr12345678'
    cands = hand_cands([('chr1', 2345700, 'INS', 100, 5), ('chr12', 345600, 'INS', 100, 5), ('chr3', 520, 'DEL', 80, 9)])
    strata = tune.strata_holdout(held)
    rows = check_against_evaluator(tmp_path, cands, truth, hand_called(cands), control(0)[None, :], strata)
    arrays = tune.prepare_truth(cands, truth)
    counts = tune_strata_ref.counts(cands['feat'], control(0)[None, :], arrays, cand_strata(cands, strata), 2)
    assert counts['call_tp'][0].tolist() == ([1, 2] if len(held) == 2 else [2, 1])
    assert counts['base_tp'][0].tolist() == ([1, 1] if len(held) == 2 else [2, 1])
    assert not any(math.isnan(x) for row in rows[0] for x in row)
    side = tune.truth_side(truth, strata=strata)
    assert np.diff(side['uid_off'].astype(np.int64)).tolist() == [32, 32] and side['n_base_strata'] == ([1, 2] if len(held) == 2 else [2, 1])
    used = [set(int(u) for u in side['base_uid'] if side['uid_off'][s] <= u < side['uid_off'][s + 1]) for s in range(2)]
    assert tuple(len(u) for u in used) == n_ids                         # the truth ids per (stratum, id text)
    assert tune.truth_side(truth)['n_base_uid'] == 2                      # ... and per id text, as the whole file is scored


def test_strata_where_the_restricted_evaluator_raises(tmp_path):
    """chr1: a matched call; chr2: an INS call whose contig has DEL truth records only (IndexError upstream); chr4: calls and no
    truth record at all; chr5: a truth record and no call (ZeroDivisionError upstream): nan there, numbers on chr1."""
    truth = str(tmp_path / 'truth.vcf')
    write_truth_rows(truth, [('chr1', 1000, 'a', 'INS', 100, '1|0'), ('chr2', 1000, 'b', 'DEL', 100, '1|0'), ('chr5', 1000, 'c', 'INS', 100, '1|1')])
    cands = hand_cands([('chr1', 1010, 'INS', 100, 5), ('chr2', 1010, 'INS', 100, 5), ('chr2', 1020, 'DEL', 100, 5), ('chr4', 10, 'DEL', 100, 7)])
    strata = tune.strata_by_contig()
    rows = check_against_evaluator(tmp_path, cands, truth, hand_called(cands), control(0)[None, :], strata)[0]
    nan = [name for name, row in zip(strata['names'], rows) if math.isnan(row[0])]
    assert sorted(set(strata['names']) - set(nan)) == ['chr1'] and rows[0][1:4] == (1.0, 1.0, 1.0)
    arrays = tune.prepare_truth(cands, truth)
    counts = tune_strata_ref.counts(cands['feat'], control(0)[None, :], arrays, cand_strata(cands, strata), 25)[0]
    assert counts['n_raise'].tolist() == [0, 1, 0, 1] + [0] * 21 and counts['n_calls'].tolist() == [1, 2, 0, 1] + [0] * 21
    # two strata: the one with chr2 and chr4 raises, the other (chr1, chr5) is scored
    rows = check_against_evaluator(tmp_path, cands, truth, hand_called(cands), control(0)[None, :], tune.strata_holdout(['chr2', 'chr4']))[0]
    assert not math.isnan(rows[0][0]) and math.isnan(rows[1][0])


def test_truth_side_numbers_the_ids_per_stratum(tmp_path):
    truth = str(tmp_path / 'truth.vcf')
    rows = [('chr%d' % (1 + i % 3), 1000 + 10 * i, 't%d' % (i % 40), 'INS' if i % 2 else 'DEL', 60 + i, '1|0') for i in range(100)]
    rows += [('abc1', 77, 'odd', 'INS', 90, '0|1'), ('chrX', 5, 'x', 'DEL', 70, '1|1'), ('chr1', 1000, 't0', 'DEL', 60, '1|0')]
    write_truth_rows(truth, rows)
    recs = E.parse_vcf(truth, False, '')
    assert len(recs) == len(rows)                                         # ('abc1' is kept: its text from the fourth character on is a label)
    plain = tune.truth_side(truth)
    for strata in (tune.strata_by_contig(), tune.strata_holdout(['chr2', 'chrX'])):
        S = len(strata['names'])
        side = tune.truth_side(truth, strata=strata)
        off = side['uid_off'].astype(np.int64)
        assert len(off) == S + 1 and off[0] == 0 and (off % 32 == 0).all() and (np.diff(off) >= 0).all() and off[-1] == side['n_base_uid']
        assert sum(side['n_base_strata']) == len(recs) == side['n_base']
        for name in ('base_off', 'base_pos', 'base_len', 'base_hp'):
            assert np.array_equal(side[name], plain[name])
        # a record's id lies in its stratum's range, and two records share an id iff they share stratum and id text
        listed = [r for k in range(len(plain['base_off']) - 1)
                  for r in sorted((r for r in recs if tune._LIST_KEY.get((r['chr'], r['type'])) == k), key=lambda r: r['pos'])]
        assert len(listed) == len(side['base_uid']) == len(recs) - 1      # (all but the 'abc1' record are in a list)
        key_of = {}
        for r, u in zip(listed, side['base_uid'].tolist()):
            s = tune.stratum_of(strata, r['chr'])
            assert off[s] <= u < off[s + 1]
            assert key_of.setdefault(u, (s, r['id'])) == (s, r['id'])
        assert len(set(key_of.values())) == len(key_of)
        other = tune.stratum_of(strata, 'abc1')
        assert strata['names'][other] == ('other' if S == 25 else 'train')
        by_text = {}
        for r in recs:
            by_text[tune.stratum_of(strata, r['chr'])] = by_text.get(tune.stratum_of(strata, r['chr']), 0) + 1
        assert side['n_base_strata'] == [by_text.get(s, 0) for s in range(S)] and side['n_base_strata'][other] >= 1
    assert tune.strata_by_contig()['names'] == tuple(E.CHROMS) + ('other',)
    with pytest.raises(ValueError):
        tune.strata_holdout([])


def test_the_two_forms_of_the_reference_agree():
    C, S = 400, 5
    feat = random_features(7, C)
    truth = random_truth(8, C, n_groups=30, n_uid=64)
    rng = np.random.default_rng(9)
    cand_stratum = rng.integers(0, S - 1, 30)[truth['cand_group']]        # (a group lies in one stratum; stratum 4 has no candidate)
    vecs = vectors_near_defaults(10, 6)
    a = tune_strata_ref.counts_masked(feat, vecs, truth, cand_stratum, S)
    b = tune_strata_ref.counts(feat, vecs, truth, cand_stratum, S)
    assert a.shape == (6, S) and np.array_equal(a, b)
    assert all(int(a[n][:, :4].max()) > 0 for n in _lib.COUNTS_NAMES if n != 'reserved') and not any(a[n][:, 4].any() for n in _lib.COUNTS_NAMES)
    # one stratum is the plain sweep
    one = tune_strata_ref.counts(feat, vecs, truth, np.zeros(C, dtype=np.uint8), 1)
    assert np.array_equal(one[:, 0], tune_score_ref.counts(feat, vecs, truth))
