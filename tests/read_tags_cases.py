# coding=utf-8
"""Problems for the read tags (tests/read_tags_ref.py: Problem), shared by tests/test_read_tags_host.py and
tests/test_gpu_read_tags.py: hand-stated ones, and the five random ones with synthetic names, calls and phase sets."""
import numpy as np

from duet_amd import synth
from tests import read_tags_ref as R
from tests import soa_fuzz

ABSENT = R.ABSENT
RANDOM = (dict(seed=1), dict(seed=2, n_contigs=5), dict(seed=3, deg=(1, 70)), dict(seed=4, absent_rate=2),
          dict(seed=5, n_contigs=1, cands_per_contig=(30, 60), empty_contig_rate=0))


def tag(hap, pc, ps):
    return (hap << 62) | (pc << 32) | ps


def problem(contigs, tags=(), n_names=None, form='off', permute=0):
    """contigs: a list of candidate lists; a candidate is dict(pred=, ps=, pos=, marks=[(name, read), ...]), read an index into
    `tags` or ABSENT.  form: 'off' (cand_ctg_off) or 'contig' (cand_contig).  permute: a seed -- the raw marks are shuffled by it
    and mark_order leads each CSR slot back to its raw mark."""
    off, names, reads, pred, ps, pos, ctg_off, ctg = [0], [], [], [], [], [], [0], []
    for k, cands in enumerate(contigs):
        for c in cands:
            for name, read in c['marks']:
                names.append(name)
                reads.append(read)
            off.append(len(names))
            pred.append(c.get('pred', 1))
            ps.append(c.get('ps', 7))
            pos.append(c.get('pos', 1000))
            ctg.append(k)
        ctg_off.append(len(pred))
    order = None
    if permute:
        M = len(names)
        order = np.random.RandomState(permute).permutation(M)              # slot i is raw mark order[i]
        raw_names, raw_reads = [0] * M, [0] * M
        for slot in range(M):
            raw_names[order[slot]], raw_reads[order[slot]] = names[slot], reads[slot]
        names, reads, order = raw_names, raw_reads, order.tolist()
    n = (max(names) + 1 if names else 1) if n_names is None else n_names
    return R.Problem(off, reads, names, n, pred, ps, pos, list(tags), cand_ctg_off=ctg_off if form == 'off' else None,
                     cand_contig=ctg if form != 'off' else None, mark_order=order)


def same_in_other_forms(p, seed=11):
    """The problem of p (cand_ctg_off form, identity order) in the three other forms: cand_contig, permuted, both."""
    K = len(p.cand_ctg_off) - 1
    ctg = [k for k in range(K) for _ in range(p.cand_ctg_off[k + 1] - p.cand_ctg_off[k])]
    M = len(p.mark_read)
    order = np.random.RandomState(seed).permutation(M)
    raw_names, raw_reads = [0] * M, [0] * M
    for slot in range(M):
        raw_names[order[slot]], raw_reads[order[slot]] = p.mark_name[slot], p.mark_read[slot]
    common = (p.n_names, p.pred, p.ps, p.cand_pos, p.read_tag)
    return [R.Problem(p.cand_off, p.mark_read, p.mark_name, *common, cand_contig=ctg),
            R.Problem(p.cand_off, raw_reads, raw_names, *common, cand_ctg_off=p.cand_ctg_off, mark_order=order.tolist()),
            R.Problem(p.cand_off, raw_reads, raw_names, *common, cand_contig=ctg, mark_order=order.tolist())]


def random_problem(**kw):
    """A soa_fuzz.random_soa problem with synthetic names and calls.  A read's name is its index, a mark without a read gets a name
    of its own behind them (reads belong to one contig there, so names do too).  A candidate's phase set is the one most of its
    tagged marks carry and its call the vote of the haplotypes in it -- 1|0 or 0|1 by majority, 1|1 on a tie, dropped without a
    tagged mark --, with every seventh call turned over, so that some reads disagree with the calls and some are placed on both
    haplotypes as often."""
    soa = soa_fuzz.random_soa(**kw)
    rng = synth.SplitMix(0x7EAD0000 + kw['seed'])
    mark_read = [int(x) for x in soa.mark_read]
    tags = [int(t) for t in soa.read_tag]
    names, fresh = [], len(tags)
    for r in mark_read:
        if r == ABSENT:
            names.append(fresh)
            fresh += 1
        else:
            names.append(r)
    C = len(soa.cand_pos)
    pred, ps = [], []
    turn = rng.below(max(C, 1), 7)
    for c in range(C):
        votes = {}
        for m in range(int(soa.cand_off[c]), int(soa.cand_off[c + 1])):
            r = mark_read[m]
            if r == ABSENT or tags[r] == R.UNTAGGED or (tags[r] >> 62) not in (1, 2):
                continue
            votes.setdefault(tags[r] & 0xFFFFFFFF, [0, 0])[(tags[r] >> 62) - 1] += 1
        if not votes:
            pred.append(0)
            ps.append(0)
            continue
        best = max(sorted(votes), key=lambda q: sum(votes[q]))
        h1, h2 = votes[best]
        call = 1 if h1 > h2 else (2 if h2 > h1 else 3)
        if call != 3 and int(turn[c]) == 0:
            call = 3 - call
        pred.append(call)
        ps.append(best)
    return R.Problem([int(x) for x in soa.cand_off], mark_read, names, max(fresh, 1), pred, ps, [int(x) for x in soa.cand_pos], tags,
                     cand_ctg_off=[int(x) for x in soa.cand_ctg_off])


def default_names(n_names):
    """-> (texts, name_off, name_pool) of n_names names read_<index>."""
    texts = ['read_%d' % i for i in range(n_names)]
    return (texts,) + pool_of(texts)


def pool_of(texts):
    off = np.zeros(len(texts) + 1, dtype=np.uint64)
    np.cumsum([len(t.encode()) for t in texts], out=off[1:])
    return off, ''.join(texts).encode()
