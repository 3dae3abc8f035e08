# coding=utf-8
"""Tags from other SVs (include/duet_ef.h: duet_sv_tags_device) in plain Python: loops and dicts, one step
of the rule per block.  The one reference of tests/test_sv_tags_host.py and tests/test_gpu_sv_tags.py.  Problems are
tests/read_tags_ref.py: Problem (the entries take the same arrays)."""
from tests import read_tags_ref as R

ABSENT = R.ABSENT
UNTAGGED = R.UNTAGGED
CAP_MAX = (1 << 30) - 3
Refused = R.Refused


def tag(hap, pc, ps):
    return (hap << 62) | (pc << 32) | ps


def has_tag(p, read):
    """The header's one definition of "the mark has a tag"."""
    return read != ABSENT and read < len(p.read_tag) and int(p.read_tag[read]) != UNTAGGED


def best(recs, min_votes):
    """recs: {ps: [n_h1, n_h2]} -> (hap, ps) of the phase set with the largest |n_h1 - n_h2|, ties to the smaller PS; None when that
    is below min_votes or there is no record."""
    pick = None
    for ps in sorted(recs):
        d = recs[ps][0] - recs[ps][1]
        if pick is None or abs(d) > abs(pick[0]):
            pick = (d, ps)
    if pick is None or abs(pick[0]) < min_votes:
        return None
    return (1 if pick[0] > 0 else 2, pick[1])


def sv_tags(p, min_votes=1, pc_new=0, pc_cap=R.PC_MAX):
    """-> (out_tag, out_index, (n_untagged, n_given, n_own_only)); Refused where the entries refuse."""
    if pc_cap > CAP_MAX or pc_new > CAP_MAX:
        raise Refused('pc_cap or pc_new')
    if min_votes < 1:
        raise Refused('min_votes')
    if (p.cand_ctg_off is None) == (p.cand_contig is None):
        raise Refused('both or neither contig form')
    C, M = len(p.pred), len(p.mark_read)
    if p.cand_ctg_off is not None:
        off = p.cand_ctg_off
        if off[0] != 0 or off[-1] != C or any(off[k] > off[k + 1] for k in range(len(off) - 1)):
            raise Refused('cand_ctg_off')
    if C == 0 or M == 0:
        return None, None, (0, 0, 0)
    if any(int(x) > 3 for x in p.pred):
        raise Refused('pred above 3')
    if any(int(p.cand_off[c]) > int(p.cand_off[c + 1]) or int(p.cand_off[c + 1]) > M for c in range(C)):
        raise Refused('cand_off')
    if any(int(n) >= p.n_names for n in p.mark_name):
        raise Refused('mark_name')
    if p.mark_order is not None and any(int(x) >= M for x in p.mark_order):
        raise Refused('mark_order')

    # every raw mark's candidate, through the slots
    cand_of = [None] * M
    for c in range(C):
        for slot in range(int(p.cand_off[c]), int(p.cand_off[c + 1])):
            raw = slot if p.mark_order is None else int(p.mark_order[slot])
            if cand_of[raw] is not None:
                raise Refused('a raw mark named twice')
            cand_of[raw] = c

    # section 20's records, and per (candidate, name) the candidate's own marks
    recs, own, where = {}, {}, {}
    for m in range(M):
        c = cand_of[m]
        if c is None or int(p.pred[c]) not in (1, 2):
            continue
        name = int(p.mark_name[m])
        recs.setdefault(name, {}).setdefault(int(p.ps[c]), [0, 0])[int(p.pred[c]) - 1] += 1
        own[(c, name)] = own.get((c, name), 0) + 1
        w = where.setdefault(name, (set(), set()))
        w[0].add(R.contig_of(p, c))
        w[1].add(int(p.mark_read[m]))
    for name, (contigs, reads) in where.items():
        if len(contigs) > 1:
            raise Refused('name %d on two contigs' % name)
        if len(reads) > 1:
            raise Refused('name %d with two read indices' % name)

    out, n_untagged, n_given, n_own_only = [], 0, 0, 0
    for m in range(M):
        read = int(p.mark_read[m])
        if has_tag(p, read):
            out.append(int(p.read_tag[read]))
            continue
        n_untagged += 1
        name, c = int(p.mark_name[m]), cand_of[m]
        with_own = {ps: list(v) for ps, v in recs.get(name, {}).items()}
        without = {ps: list(v) for ps, v in with_own.items()}
        if c is not None and int(p.pred[c]) in (1, 2):
            without[int(p.ps[c])][int(p.pred[c]) - 1] -= own[(c, name)]
        got = best(without, min_votes)
        if got is None:
            out.append(UNTAGGED)
            n_own_only += best(with_own, min_votes) is not None
        else:
            out.append(tag(got[0], pc_new, got[1]))
            n_given += 1
    return out, list(range(M)), (n_untagged, n_given, n_own_only)


def expanded(p, out_tag):
    """The second run's problem: read_tag = out_tag, mark_read = the identity over the raw marks."""
    return R.Problem(p.cand_off, list(range(len(p.mark_read))), p.mark_name, p.n_names, p.pred, p.ps, p.cand_pos, out_tag,
                     cand_ctg_off=p.cand_ctg_off, cand_contig=p.cand_contig, mark_order=p.mark_order)


CHANGE = ('none', 'gained', 'lost', 'same', 'relabelled', 'to_het', 'to_hom', 'other')


def change(p0, s0, p1, s1):
    """The change code of one candidate between two runs, with an empty block table (relabelled coincides with same)."""
    if p0 == 0 and p1 == 0:
        return 'none'
    if p0 == 0:
        return 'gained'
    if p1 == 0:
        return 'lost'
    if (p1, s1) == (p0, s0):
        return 'same'
    if p0 == 3 and p1 in (1, 2):
        return 'to_het'
    if p0 in (1, 2) and p1 == 3:
        return 'to_hom'
    return 'other'
