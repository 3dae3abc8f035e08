# coding=utf-8
"""Test-side meaning of the stratified sweep (duet_tune_sweep_strata_*, include/duet_ef.h: duet_tune_strata): the record of
(vector, stratum) is the plain sweep's record after DUET_TUNE_IN_CALLS has been cleared on every candidate outside the stratum --
the masked re-run, on tests/tune_score_ref.py, which tests/test_score_refs_host.py holds to evaluation.evaluation.

    counts_masked   literally that: one tune_score_ref.counts per stratum on masked flags
    counts          the same numbers with the predictions made once and each stratum's record taken over its own candidates only
                    (tune_score_ref.counts_of_preds skips a candidate without DUET_TUNE_IN_CALLS before it reads anything else of it,
                    so leaving such a candidate out is masking it); tests/test_tune_strata_host.py holds the two to each other"""
import numpy as np

from duet_amd import _lib
from tests import tune_score_ref

IN = _lib.TUNE_IN_CALLS
CAND_ARRAYS = ('cand_flags', 'cand_group', 'cand_uid', 'cand_pair')


def counts_masked(feat, vectors, truth, cand_stratum, n_strata):
    """-> COUNTS_DTYPE[K, S]"""
    vectors = np.asarray(vectors, dtype=np.float64).reshape(-1, len(_lib.TUNE_NAMES))
    cand_stratum = np.asarray(cand_stratum)
    flags = np.asarray(truth['cand_flags'], dtype=np.uint16)
    out = np.zeros((len(vectors), n_strata), dtype=_lib.COUNTS_DTYPE)
    for s in range(n_strata):
        masked = dict(truth, cand_flags=np.where(cand_stratum == s, flags, flags & np.uint16(~IN & 0xFFFF)))
        out[:, s] = tune_score_ref.counts(feat, vectors, masked)
    return out


def counts(feat, vectors, truth, cand_stratum, n_strata):
    """-> COUNTS_DTYPE[K, S]"""
    pred = tune_score_ref.preds_and_counts(feat, vectors, None)[0]
    cand_stratum = np.asarray(cand_stratum)
    out = np.zeros((len(pred), n_strata), dtype=_lib.COUNTS_DTYPE)
    for s in range(n_strata):
        at = np.nonzero(cand_stratum == s)[0]
        sub = dict(truth, **{n: np.asarray(truth[n])[at] for n in CAND_ARRAYS})
        for k in range(len(pred)):
            rec = tune_score_ref.counts_of_preds(feat[at], pred[k, at].tolist(), sub)
            for name in _lib.COUNTS_NAMES:
                out[name][k, s] = rec[name]
    return out


def group_strata(truth, cand_stratum):
    """group_stratum u8[n_groups] from the calls (255 for a group without a call: the device never reads it)."""
    out = np.full(int(truth['n_groups']), 255, dtype=np.uint8)
    flags = np.asarray(truth['cand_flags'])
    for c in np.nonzero(flags & IN)[0]:
        g = int(truth['cand_group'][c])
        assert out[g] in (255, int(cand_stratum[c])), 'the calls of group %d are in two strata' % g
        out[g] = cand_stratum[c]
    return out
