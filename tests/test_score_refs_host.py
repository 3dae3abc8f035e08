# coding=utf-8
"""No GPU: the two plain references the device scoring is tested against (tests/eval_ref.py, tests/tune_score_ref.py) pinned to
evaluation.evaluation -- on the numbers recorded from the reference's own evaluator, on the synthetic callsets of
tests/test_gpu_eval.py and on the text tune_ref.phased_text writes -- so that a wrong reference cannot make the GPU tests pass."""
import json
import os

import numpy as np
import pytest

from duet_amd import _lib, tune
from duet_amd import evaluation as E
from tests import eval_ref, tune_ref, tune_score_ref
from tests import helpers as H
from tests.test_gpu_eval import synthetic_records
from tests.test_gpu_tune import evaluate, random_vectors, scoring_workdir, write_truth


def ten_numbers(truth, calls, refdist, ratio):
    """evaluation's ten numbers from eval_ref's six counts: the same binary64 quotients."""
    n = dict(zip(eval_ref.NAMES, eval_ref.counts(E.flatten(truth, calls), refdist, ratio)))

    def prf(tp_c, tp_b):
        p, r = tp_c / len(calls), tp_b / len(truth)
        return p, r, 2 * p * r / (p + r)

    return (len(calls) / len(set(s['ps'] for s in calls)),) + prf(n['call_tp'], n['base_tp']) + prf(n['call_gt'], n['base_gt']) + \
        prf(n['call_hp'], n['base_hp'])


def test_eval_ref_on_the_recorded_reference_numbers():
    d = os.path.join(H.GOLDEN, 'eval')
    with open(os.path.join(d, 'expected.json')) as f:
        cases = json.load(f)
    assert len(cases) == 24
    for c in cases:
        pair = os.path.join(d, 'pair%d' % c['pair'])
        bed = os.path.join(pair, 'regions.bed') if c['bed'] else ''
        truth = E.parse_vcf(os.path.join(pair, 'truth.vcf'), c['skip_phasing'], bed)
        calls = E.parse_vcf(os.path.join(pair, 'call.vcf'), c['skip_phasing'], bed)
        got = [float(x) for x in ten_numbers(truth, calls, c['refdist'], c['pctsim'])]
        assert tune_ref.same_floats(got, [float(x) for x in E.evaluation(truth, calls, c['refdist'], c['pctsim'])]), c
        assert got == c['result'], c


@pytest.mark.parametrize('seed,n_truth,n_calls,refdist,ratio', [(1, 300, 400, 1000, 0.0), (2, 3000, 5000, 100, 0.7), (4, 2000, 2500, 3, 0.9)])
def test_eval_ref_on_synthetic_callsets(seed, n_truth, n_calls, refdist, ratio):
    truth, calls = synthetic_records(seed, n_truth, n_calls)
    want = [float(x) for x in E.evaluation(truth, calls, refdist, ratio)]
    assert tune_ref.same_floats([float(x) for x in ten_numbers(truth, calls, refdist, ratio)], want)
    assert want[1] > 0 and want[7] > 0                                 # (something matched, something phased)


def host_candidates(home, s=50, r=2):
    """tune.features without the device: the same candidates, the features from the oracle's filter, class, seeds and vote."""
    soa, txt = tune._candidates(home, s, r, False, 2)
    want = tune_ref.oracle_features(soa, s, r)
    feat = np.zeros(soa.n_cands, dtype=_lib.FEATURE_DTYPE)
    for name in ('kept', 'eligible', 'cls', 'hap1', 'hap2', 'hap0', 'allhap', 't1', 't2', 'ps', 'deg', 'svread', 'refread'):
        feat[name] = [w[name] for w in want]
    return dict(feat=feat, pos=soa.cand_pos.copy(), svlen=soa.cand_svlen.copy(), soa=soa, **txt)


@pytest.mark.parametrize('seed,refdist,pctsim', [(3, 1000, 0.0), (6, 300, 0.7)])
def test_tune_score_ref_equals_the_evaluator_on_the_written_text(tmp_path, seed, refdist, pctsim):
    home = str(tmp_path / 'w')
    scoring_workdir(home, seed)
    cands = host_candidates(home)
    assert int(cands['feat']['eligible'].sum()) > 20
    truth = str(tmp_path / 'truth.vcf')
    write_truth(home, cands, truth, seed)
    arrays = tune.prepare_truth(cands, truth, refdist, pctsim)
    vecs = np.concatenate([tune.vector()[None, :], random_vectors(cands['feat'], 4, seed)])
    counts = tune_score_ref.counts(cands['feat'], vecs, arrays)
    scored = 0
    for k, v in enumerate(vecs):
        called = str(tmp_path / 'called.vcf')
        with open(called, 'w') as f:
            f.write(tune_ref.phased_text(home, 50, 2, v))
        want = evaluate(truth, called, refdist, pctsim, '', False)
        got = tune.scores(counts[k], arrays['n_base'])
        assert tune_ref.same_floats(got, want), (v, counts[k], got, want)
        scored += got[7] > 0
    assert scored                                                       # (not every row is nan)
    # without a truth set: every emitted candidate, nothing else
    plain = tune_score_ref.counts(cands['feat'], vecs)
    for k, v in enumerate(vecs):
        assert int(plain['n_calls'][k]) == sum(1 for p in tune_ref.preds_from_features(cands['feat'], v) if p)
        assert not any(int(plain[n][k]) for n in _lib.COUNTS_NAMES if n != 'n_calls')
