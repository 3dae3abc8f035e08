# coding=utf-8
"""`tune --vote_sv_tags` by the references alone, shared by tests/test_sv_tags_plan_host.py and tests/test_gpu_tune_sv_tags.py: per
vector its OWN two-pass run -- the reference's features under the cap (tests/pc_cap_ref.py), the restated tree on them
(tests/tune_ref.py), the reference's tags from those calls (tests/sv_tags_ref.py), the reference's features again on the expanded
problem -- then the host truth match and the restated counts on the second run's records."""
import numpy as np

from duet_amd import tune
from tests import cap_line_ref as R
from tests import pc_cap_ref, tune_ref, tune_score_ref
from tests import sv_tags_cases as K
from tests import sv_tags_ref as S
from tests.test_gpu_fit_cap import HEAD, World

# the default vector, and four whose second run differs from one made on the default vector's tags (the condition)
GRID = [{}, {'c1_max_ref_num': 3, 'c0_min_sv_num': 2}, {'c1_twohap_sv_ratio_2': 0.7, 'c1_max_ref_num': 1000},
        {'c1_onehap_sv_ratio_hi': 0.6}, {'c1_hapread_ratio': 0.4}]


def calls(feat, vec):
    """The first run of `vec` on the records -> (pred list, ps list: the phase set of eligible candidates, else 0)."""
    return tune_ref.preds_from_features(feat, vec), [int(f['ps']) if f['eligible'] else 0 for f in feat]


class SvWorld(World):
    """World with the marks' names: second(cap, vec, m, q) is the second run's records for ONE vector."""

    def __init__(self, soa, txt, s, r, mark_name, n_names):
        World.__init__(self, K.oracle_form(soa), txt, s, r, line=([0], 0))
        self.raw, self.mark_name, self.n_names = soa, [int(x) for x in mark_name], int(n_names)
        self.smemo = {}

    def tags(self, cap, vec, m=1, q=0):
        """-> (out_tag list, (n_untagged, n_given, n_own_only)) from the first-run calls of `vec` under `cap`."""
        key = (cap, tuple(float(x) for x in vec), m, q)
        if key not in self.smemo:
            soa = self.raw
            pred, ps = calls(self.features(cap), vec)
            p = S.R.Problem([int(x) for x in soa.cand_off], [int(x) for x in soa.mark_read], self.mark_name, self.n_names, pred, ps,
                            [int(x) for x in soa.cand_pos], [int(t) for t in soa.read_tag], cand_ctg_off=[int(x) for x in soa.cand_ctg_off])
            out, _, counts = S.sv_tags(p, m, q, cap)
            self.smemo[key] = out, counts
        return self.smemo[key]

    def on_tags(self, cap, out_tag):
        """The reference's records of the run on the expanded problem with those words."""
        key = ('feat', cap, np.array(out_tag, dtype=np.uint64).tobytes())
        if key not in self.smemo:
            self.smemo[key] = R.records(pc_cap_ref.features(K.oracle_form(K.expanded_soa(self.raw, out_tag)), self.s, self.r, cap))
        return self.smemo[key]

    def second(self, cap, vec, m=1, q=0):
        """-> (records of the second run of `vec`, its mark counters); m == 0: the first run's records, counters of 0."""
        if m == 0:
            return self.features(cap), (0, 0, 0)
        out, counts = self.tags(cap, vec, m, q)
        return self.on_tags(cap, out), counts

    def write_truth2(self, path, cap=8100, vec=None, m=1, q=0):
        """World.write_truth on the second run of `vec` (default: the default vector): one record per emitted call."""
        vec = tune.vector() if vec is None else vec
        feat, _ = self.second(cap, vec, m, q)
        rows = list(HEAD)
        for c, p in enumerate(tune_ref.preds_from_features(feat, vec)):
            if p:
                t, ln = self.cands['svtype'][c], int(self.cands['svlen'][c])
                rows.append('%s\t%d\ttruth%d\tN\t<%s>\t.\tPASS\tSVTYPE=%s;SVLEN=%d\tGT:PS\t%s:%d\n' % (
                    self.cands['chrom'][c], int(self.cands['pos'][c]), c, t, t, ln if t in ('INS', 'DUP') else -ln, tune.HP_TEXT[p],
                    int(feat['ps'][c])))
        with open(path, 'w') as f:
            f.writelines(rows)
        self.truth_vcf = path
        return path

    def counts(self, feat, vec):
        """The count record of `vec` swept alone over `feat`, or None where the records divide by zero."""
        if R.div_zero(feat):
            return None
        return tune_score_ref.counts(feat, np.asarray(vec, dtype=np.float64).reshape(1, -1), self.truth(feat))[0]


def world_of(home, s=50, r=2):
    soa, txt = tune._candidates(home, s, r, False, 4)
    names, n_names = tune._mark_names(home, False, 4)
    return SvWorld(soa, txt, s, r, names, n_names)
