# coding=utf-8
"""Read tags from phased SVs (include/duet_ef.h: duet_read_tags_device) in plain Python: loops and dicts, one
step of the rule per block.  The one reference of tests/test_read_tags_host.py and tests/test_gpu_read_tags.py."""
import bisect

import numpy as np

ABSENT = 0xFFFFFFFF
UNTAGGED = 0xFFFFFFFFFFFFFFFF
PC_MAX = 8100
FIELDS = ('name', 'contig', 'ps', 'read', 'n_h1', 'n_h2', 'pos_min', 'pos_max', 'status', 'reserved')
COLUMNS = ('CHROM', 'READ', 'PS', 'N_SV', 'N_H1', 'N_H2', 'HP_SV', 'TAG_HP', 'TAG_PS', 'TAG_PC', 'STATUS', 'POS_MIN', 'POS_MAX')
STATUS = ('agree', 'disagree', 'tie', 'new', 'other_ps')


class Refused(ValueError):
    """What the entries answer with DUET_ERR_INVALID."""


class Problem(object):
    """The arrays of one problem, as the entries take them; exactly one of cand_ctg_off / cand_contig."""

    def __init__(self, cand_off, mark_read, mark_name, n_names, pred, ps, cand_pos, read_tag, cand_ctg_off=None, cand_contig=None,
                 mark_order=None):
        self.cand_off, self.mark_read, self.mark_name, self.n_names = list(cand_off), list(mark_read), list(mark_name), int(n_names)
        self.pred, self.ps, self.cand_pos, self.read_tag = list(pred), list(ps), list(cand_pos), list(read_tag)
        self.cand_ctg_off = None if cand_ctg_off is None else list(cand_ctg_off)
        self.cand_contig = None if cand_contig is None else list(cand_contig)
        self.mark_order = None if mark_order is None else list(mark_order)

    def arrays(self):
        """The keyword arguments of _lib.Context.read_tags_host."""
        return dict(cand_off=self.cand_off, mark_read=self.mark_read, mark_name=self.mark_name, n_names=self.n_names, pred=self.pred,
                    ps=self.ps, cand_pos=self.cand_pos, read_tag=np.array(self.read_tag, dtype=np.uint64),
                    cand_ctg_off=self.cand_ctg_off, cand_contig=self.cand_contig, mark_order=self.mark_order)


def contig_of(p, c):
    if p.cand_contig is not None:
        return int(p.cand_contig[c])
    return bisect.bisect_right(p.cand_ctg_off, c) - 1          # the k with cand_ctg_off[k] <= c < cand_ctg_off[k + 1]


def usable(p, read, pc_cap):
    """The read's own tag as (hap, pc, ps) when it is usable, else None."""
    if read == ABSENT or read >= len(p.read_tag):
        return None
    t = int(p.read_tag[read])
    if t == UNTAGGED:
        return None
    hap, pc, ps = t >> 62, (t >> 32) & 0x3FFFFFFF, t & 0xFFFFFFFF
    return (hap, pc, ps) if hap in (1, 2) and pc <= pc_cap else None


def status_of(p, rec, pc_cap):
    sv = 1 if rec['n_h1'] > rec['n_h2'] else (2 if rec['n_h2'] > rec['n_h1'] else 0)
    tag = usable(p, rec['read'], pc_cap)
    if tag is not None and tag[2] != rec['ps']:
        return 'other_ps'
    if sv == 0:
        return 'tie'
    if tag is not None:
        return 'agree' if tag[0] == sv else 'disagree'
    return 'new'


def read_tags(p, pc_cap=PC_MAX):
    """-> the records as a list of dicts (FIELDS), ascending by (name, ps); Refused where the entries refuse."""
    if pc_cap > (1 << 30) - 3:
        raise Refused('pc_cap')
    if (p.cand_ctg_off is None) == (p.cand_contig is None):
        raise Refused('both or neither contig form')
    C, M = len(p.pred), len(p.mark_read)
    if any(int(x) > 3 for x in p.pred):
        raise Refused('pred above 3')
    recs, where = {}, {}                                        # where: name -> the contigs and read indices of its marks
    for c in range(C):
        if int(p.pred[c]) not in (1, 2):
            continue
        for slot in range(int(p.cand_off[c]), int(p.cand_off[c + 1])):
            raw = slot if p.mark_order is None else int(p.mark_order[slot])
            if raw >= M:
                raise Refused('mark_order')
            name, read = int(p.mark_name[raw]), int(p.mark_read[raw])
            if name >= p.n_names:
                raise Refused('mark_name')
            pos, k = int(p.cand_pos[c]), contig_of(p, c)
            r = recs.setdefault((name, int(p.ps[c])), dict(name=name, contig=k, ps=int(p.ps[c]), read=read, n_h1=0, n_h2=0, pos_min=pos,
                                                           pos_max=pos, status=0, reserved=0))
            r['n_h1' if int(p.pred[c]) == 1 else 'n_h2'] += 1
            r['pos_min'], r['pos_max'] = min(r['pos_min'], pos), max(r['pos_max'], pos)
            w = where.setdefault(name, (set(), set()))
            w[0].add(k)
            w[1].add(read)
    for name, (contigs, reads) in where.items():
        if len(contigs) > 1:
            raise Refused('name %d on two contigs' % name)
        if len(reads) > 1:
            raise Refused('name %d with two read indices' % name)
    out = [recs[key] for key in sorted(recs)]
    for r in out:
        r['status'] = STATUS.index(status_of(p, r, pc_cap))
    return out


def records(recs, dtype):
    """The list of dicts as a structured array of `dtype` (duet_amd._lib.READ_TAG_DTYPE)."""
    out = np.zeros(len(recs), dtype=dtype)
    for i, r in enumerate(recs):
        for f in FIELDS:
            out[f][i] = r[f]
    return out


def header():
    return '\t'.join(COLUMNS) + '\n'


def rows_text(recs, names, chrom_texts, read_tag):
    """One row per record; names[i]: the text of name i (str)."""
    out = []
    for r in recs:
        n_h1, n_h2, read = int(r['n_h1']), int(r['n_h2']), int(r['read'])
        hp_sv = '1' if n_h1 > n_h2 else ('2' if n_h2 > n_h1 else '.')
        tag_hp = tag_ps = tag_pc = '.'
        if read != ABSENT and read < len(read_tag) and int(read_tag[read]) != UNTAGGED:
            t = int(read_tag[read])
            hap = t >> 62
            tag_hp = str(hap) if hap in (1, 2) else '.'
            tag_ps, tag_pc = str(t & 0xFFFFFFFF), str((t >> 32) & 0x3FFFFFFF)
        out.append('%s\t%s\t%d\t%d\t%d\t%d\t%s\t%s\t%s\t%s\t%s\t%d\t%d\n' % (
            chrom_texts[int(r['contig'])], names[int(r['name'])], r['ps'], n_h1 + n_h2, n_h1, n_h2, hp_sv, tag_hp, tag_ps, tag_pc,
            STATUS[int(r['status'])], r['pos_min'], r['pos_max']))
    return ''.join(out)


def summary(recs):
    """{status name: count} over the records."""
    return {s: sum(1 for r in recs if int(r['status']) == i) for i, s in enumerate(STATUS)}
