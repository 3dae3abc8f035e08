# coding=utf-8
"""The joined phase sets (include/duet_ef.h: duet_ps_join_tags_device, duet_ps_join_diff_device) in plain
Python: loops and dicts, one step of the rule per function.  The one reference of tests/test_ps_join_host.py and
tests/test_gpu_ps_join.py."""
import numpy as np

from duet_amd import engine
from tests import ps_links_ref as L

UNTAGGED = 0xFFFFFFFFFFFFFFFF
NAMES = ('none', 'gained', 'lost', 'same', 'relabelled', 'to_het', 'to_hom', 'other')
REPORTED = ('gained', 'lost', 'to_het', 'to_hom', 'other')
HP = {0: '.', 1: '1|0', 2: '0|1', 3: '1|1'}
COLUMNS = ('CHROM', 'POS', 'SVLEN', 'CHANGE', 'HP', 'PS', 'HP_JOINED', 'PS_JOINED')


def select(recs, min_sv):
    """The indices of the links with a verdict whose winning side counts at least min_sv candidates."""
    keep = []
    for i, r in enumerate(recs):
        v = L.verdict(r)
        if v == 'same' and int(r['n_same']) >= min_sv:
            keep.append(i)
        if v == 'flip' and int(r['n_flip']) >= min_sv:
            keep.append(i)
    return keep


def blocks_used(recs, min_sv=2):
    """-> (rows [(contig, ps, block, flip)] ascending, conflicts [indices into recs]): the spanning forest over the selected links;
    a phase set that only the other links name is a block of its own."""
    keep = select(recs, min_sv)
    rows, conflicts = L.blocks([recs[i] for i in keep])
    have = set((k, ps) for k, ps, _, _ in rows)
    for r in recs:
        for ps in (int(r['ps_a']), int(r['ps_b'])):
            if (int(r['contig']), ps) not in have:
                have.add((int(r['contig']), ps))
                rows.append((int(r['contig']), ps, ps, 0))
    return sorted(rows), [keep[i] for i in conflicts]


def as_dict(rows):
    return {(int(k), int(ps)): (int(block), int(flip)) for k, ps, block, flip in rows}


def remap(read_tag, read_off, rows):
    """-> (the remapped tag words, how many changed)."""
    tab = as_dict(rows)
    out = [int(t) for t in read_tag]
    n = 0
    for k in range(len(read_off) - 1):
        for r in range(int(read_off[k]), int(read_off[k + 1])):
            t = out[r]
            if t == UNTAGGED:
                continue
            hap, pc, ps = t >> 62, (t >> 32) & 0x3FFFFFFF, t & 0xFFFFFFFF
            if (k, ps) not in tab:
                continue
            block, flip = tab[(k, ps)]
            if flip == 1 and hap in (1, 2):
                hap = 3 - hap
            new = (hap << 62) | (pc << 32) | block
            n += new != t
            out[r] = new
    return np.array(out, dtype=np.uint64), n


def remapped_soa(soa, rows):
    kw = {name: getattr(soa, name).copy() for name, _ in engine.EfSoA.FIELDS}
    kw['read_tag'] = remap(soa.read_tag, soa.read_off, rows)[0]
    return engine.EfSoA(read_off=soa.read_off.copy(), **kw)


def change_code(k, p0, s0, p1, s1, tab):
    if p0 == 0 and p1 == 0:
        return 0
    if p0 == 0:
        return 1
    if p1 == 0:
        return 2
    if (p1, s1) == (p0, s0):
        return 3
    block, flip = tab.get((k, s0), (s0, 0))
    pe = 3 - p0 if flip == 1 and p0 in (1, 2) else p0
    if (p1, s1) == (pe, block):
        return 4
    if p0 == 3 and p1 in (1, 2):
        return 5
    if p0 in (1, 2) and p1 == 3:
        return 6
    return 7


def contig_column(cand_ctg_off):
    out = []
    for k in range(len(cand_ctg_off) - 1):
        out += [k] * (int(cand_ctg_off[k + 1]) - int(cand_ctg_off[k]))
    return out


def diff(cand_contig, pred0, ps0, pred1, ps1, rows):
    """-> (codes u8[C], counts u32[8])."""
    tab = as_dict(rows)
    codes = [change_code(int(cand_contig[c]), int(pred0[c]), int(ps0[c]), int(pred1[c]), int(ps1[c]), tab) for c in range(len(pred0))]
    counts = [0] * 8
    for x in codes:
        counts[x] += 1
    return np.array(codes, dtype=np.uint8), np.array(counts, dtype=np.uint32)


def header():
    return '\t'.join(COLUMNS) + '\n'


def report_text(chrom_texts, cand_contig, pos, svlen, codes, pred0, ps0, pred1, ps1):
    out = []
    for c in range(len(codes)):
        name = NAMES[int(codes[c])]
        if name not in REPORTED:
            continue
        before = (HP[int(pred0[c])], '%d' % ps0[c]) if int(pred0[c]) else ('.', '.')
        after = (HP[int(pred1[c])], '%d' % ps1[c]) if int(pred1[c]) else ('.', '.')
        out.append('%s\t%d\t%d\t%s\t%s\t%s\t%s\t%s\n' % ((chrom_texts[int(cand_contig[c])], pos[c], svlen[c], name) + before + after))
    return ''.join(out)
