# coding=utf-8
"""Problems for the tags from other SVs (tests/sv_tags_ref.py), shared by tests/test_sv_tags_host.py and
tests/test_gpu_sv_tags.py: the hand-stated ones come from tests/read_tags_cases.py: problem; here are the random ones, made so that
the feature matters, and the whole second run on the CPU."""
import numpy as np

from duet_amd import engine
from oracle import c_oracle
from tests import read_tags_ref as R
from tests import soa_fuzz
from tests import sv_tags_ref as S

SHARE = 3                       # every SHARE-th read of each contig loses its tag word: a third of the reads
# seeds of 1..8 for which the reference alone gives a gained candidate, a mark in n_own_only and no division by zero, with
# (n_untagged, n_given, n_own_only) and the candidates gained -- tests/test_sv_tags_host.py recomputes every number
PINNED = {1: ((2640, 886, 171), 23), 2: ((3939, 1154, 193), 35), 3: ((1933, 412, 44), 13), 4: ((3749, 438, 49), 15),
          5: ((1837, 556, 103), 13), 6: ((3494, 715, 31), 8), 7: ((2000, 865, 103), 23), 8: ((2837, 274, 73), 10)}


def untagged_soa(seed):
    """soa_fuzz.random_soa(seed) with the tag word of every SHARE-th read of each contig turned to all-ones: reads are shared
    between candidates there, as they are in a BAM, so untagged reads are too."""
    soa = soa_fuzz.random_soa(seed)
    tags = soa.read_tag.copy()
    for k in range(len(soa.read_off) - 1):
        tags[int(soa.read_off[k]):int(soa.read_off[k + 1]):SHARE] = S.UNTAGGED
    kw = {name: getattr(soa, name) for name, _ in engine.EfSoA.FIELDS}
    kw['read_tag'] = tags
    return engine.EfSoA(read_off=soa.read_off, **kw)


def mark_names(soa):
    """A read's name is its index; a mark without a read gets a name of its own behind them -> (mark_name, n_names)."""
    names, fresh = [], soa.n_reads
    for r in soa.mark_read:
        if int(r) == S.ABSENT:
            names.append(fresh)
            fresh += 1
        else:
            names.append(int(r))
    return names, max(fresh, 1)


def problem_of(soa, pred, ps, form='off', mark_order=None):
    """The entries' problem over an E/F problem and its calls.  mark_order: a permutation -- the raw marks are laid out so that
    CSR slot i is raw mark mark_order[i]."""
    names, n_names = mark_names(soa)
    reads = [int(x) for x in soa.mark_read]
    if mark_order is not None:
        raw_names, raw_reads = [0] * len(names), [0] * len(names)
        for slot, raw in enumerate(mark_order):
            raw_names[raw], raw_reads[raw] = names[slot], reads[slot]
        names, reads = raw_names, raw_reads
    off = [int(x) for x in soa.cand_ctg_off]
    ctg = [k for k in range(len(off) - 1) for _ in range(off[k + 1] - off[k])]
    return R.Problem([int(x) for x in soa.cand_off], reads, names, n_names, [int(x) for x in pred], [int(x) for x in ps],
                     [int(x) for x in soa.cand_pos], [int(t) for t in soa.read_tag], cand_ctg_off=off if form == 'off' else None,
                     cand_contig=ctg if form != 'off' else None, mark_order=None if mark_order is None else list(mark_order))


def expanded_soa(soa, out_tag):
    """The second run's E/F problem: a mark is its own read."""
    kw = {name: getattr(soa, name) for name, _ in engine.EfSoA.FIELDS}
    kw['read_tag'] = np.array(out_tag, dtype=np.uint64)
    kw['mark_read'] = np.arange(soa.n_marks, dtype=np.uint32)
    return engine.EfSoA(read_off=soa.cand_off[soa.cand_ctg_off], **kw)


def second_run(soa, calls, min_votes=1, pc_new=0):
    """The whole feature by the reference: calls(soa) -> (pred, ps) of the route.
    -> dict(p0, s0, out_tag, counts, p1, s1, codes: the change names per candidate)"""
    p0, s0 = calls(soa)
    out, _, counts = S.sv_tags(problem_of(soa, p0, s0), min_votes, pc_new)
    p1, s1 = calls(expanded_soa(soa, out))
    codes = [S.change(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(p0, s0, p1, s1)]
    return dict(p0=p0, s0=s0, out_tag=out, counts=counts, p1=p1, s1=s1, codes=codes)


class DivZero(Exception):
    pass


def oracle_form(soa):
    """The same problem as the C oracle can read it: it knows one spelling of "no tag", the absent index (an all-ones word is a
    tag with PS 2^32 - 1 to it), so every mark whose word is all-ones or whose index lies outside the table becomes absent."""
    reads = soa.mark_read.astype(np.int64)
    inside = (reads != S.ABSENT) & (reads < soa.n_reads)
    words = soa.read_tag[np.where(inside, reads, 0)] if soa.n_reads else np.zeros(len(reads), dtype=np.uint64)
    kw = {name: getattr(soa, name) for name, _ in engine.EfSoA.FIELDS}
    kw['mark_read'] = np.where(inside & (words != np.uint64(S.UNTAGGED)), reads, S.ABSENT).astype(np.uint32)
    return engine.EfSoA(read_off=soa.read_off, **kw)


def oracle_calls(soa):
    rc, p, s = c_oracle.ef(oracle_form(soa), 50, 2)
    if rc:
        raise DivZero(rc)
    return p[:soa.n_cands], s[:soa.n_cands]
