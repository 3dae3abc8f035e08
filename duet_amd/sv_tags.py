# coding=utf-8
"""Tags from other SVs (include/duet_ef.h: duet_sv_tags_device): the host side of `duet --vote_sv_tags`.

A read WhatsHap could not tag may still support a heterozygous SV call, and that call says which haplotype the read lies on.  The
device gives every untagged mark the haplotype the OTHER het calls listing its read place it on (per mark, leave-one-out: no call
votes for itself), as one tag word per raw mark; the second run is the ordinary run over those words through an identity index.
Here: the checks of the two settings, the file names, the report of the calls that changed and the log line.  The report has one
row per candidate whose call changed -- thousands, not millions: it is formatted on the host.
"""

import numpy as np

REPORT_COLUMNS = ('CHROM', 'POS', 'SVLEN', 'CHANGE', 'HP', 'PS', 'HP_NEW', 'PS_NEW')
REPORTED = (1, 2, 5, 6, 7)              # gained, lost, to_het, to_hom, other (_lib.JOIN_CHANGE_NAMES): `none` and `same` are not listed
HP_TEXT = ('.', '1|0', '0|1', '1|1')
MIN_VOTES = 1                           # --sv_tag_min: |n_h1 - n_h2| a read's other calls must reach
PC_NEW = 0                              # --sv_tag_pc: the PC a derived tag carries
PC_LIMIT = (1 << 30) - 3
COUNT_NAMES = ('untagged', 'given', 'own_only')


def path_vcf(home):
    return home + '/phased_sv.sv_tags.vcf'


def path_report(home):
    return home + '/phased_sv.sv_tags_report.tsv'


def check_min_votes(n):
    """--sv_tag_min as an integer >= 1, or ValueError."""
    v = int(n)
    if v != n or not 1 <= v <= 0xFFFFFFFF:
        raise ValueError('sv_tag_min: an integer >= 1, not %r' % (n,))
    return v


def check_pc_new(p):
    """--sv_tag_pc as an integer in 0 .. 2^30 - 3, or ValueError."""
    v = int(p)
    if v != p or not 0 <= v <= PC_LIMIT:
        raise ValueError('sv_tag_pc: an integer in 0 .. %d, not %r' % (PC_LIMIT, p))
    return v


def check_settings(vote_sv_tags, sv_tag_min, sv_tag_pc, gpus=1, join_ps=False):
    """The keyword form of the flags -> (min_votes, pc_new), or None without the flag; ValueError where `duet` refuses."""
    import os
    if not vote_sv_tags:
        if sv_tag_min is not None or sv_tag_pc is not None:
            raise ValueError('sv_tag_min / sv_tag_pc need vote_sv_tags')
        return None
    if int(gpus) > 1 or os.environ.get('DUET_FORCE_RANKS') == '1':
        raise ValueError('vote_sv_tags: single-GPU path only')
    if join_ps:
        raise ValueError('vote_sv_tags: not together with join_ps')
    return (check_min_votes(MIN_VOTES if sv_tag_min is None else sv_tag_min), check_pc_new(PC_NEW if sv_tag_pc is None else sv_tag_pc))


def change_codes(pred0, ps0, pred1, ps1):
    """The change code of every candidate between two runs as duet_ps_join_diff_* gives it under an empty table (`relabelled`
    coincides with `same`), on the host -> (change u8[C], counts u32[8]).  For callers without a context."""
    p0, p1 = np.asarray(pred0, dtype=np.int64), np.asarray(pred1, dtype=np.int64)
    s0, s1 = np.asarray(ps0, dtype=np.int64), np.asarray(ps1, dtype=np.int64)
    het0, het1 = (p0 == 1) | (p0 == 2), (p1 == 1) | (p1 == 2)
    change = np.select([(p0 == 0) & (p1 == 0), p0 == 0, p1 == 0, (p0 == p1) & (s0 == s1), (p0 == 3) & het1, het0 & (p1 == 3)],
                       [0, 1, 2, 3, 5, 6], default=7).astype(np.uint8)
    return change, np.bincount(change, minlength=8).astype(np.uint32)


def report_header():
    return '\t'.join(REPORT_COLUMNS) + '\n'


def _hp_ps(pred, ps):
    return (HP_TEXT[pred], str(ps)) if pred else ('.', '.')


def report_text(chrom_texts, cand_contig, pos, svlen, change, pred0, ps0, pred1, ps1):
    """The data rows of phased_sv.sv_tags_report.tsv: one per candidate whose change code is in REPORTED, in candidate order.
    chrom_texts: the CHROM text per contig; cand_contig: the contig index per candidate; svlen: the candidates' abs(SVLEN)."""
    from duet_amd import _lib
    out = []
    for c in np.flatnonzero(np.isin(np.asarray(change), REPORTED)):
        t = chrom_texts[int(cand_contig[c])]
        out.append('\t'.join((t.decode() if isinstance(t, bytes) else t, str(int(pos[c])), str(int(svlen[c])),
                              _lib.JOIN_CHANGE_NAMES[int(change[c])]) + _hp_ps(int(pred0[c]), int(ps0[c])) +
                             _hp_ps(int(pred1[c]), int(ps1[c]))) + '\n')
    return ''.join(out)


def summary_text(mark_counts, change_counts):
    """The log line of the second run: the three mark counters, then the change counts by name (`relabelled` cannot occur)."""
    from duet_amd import _lib
    text = ', '.join('%d marks %s' % (int(v), n) for n, v in zip(COUNT_NAMES, mark_counts))
    return text + '; ' + ', '.join('%s %d' % (n, int(v)) for n, v in zip(_lib.JOIN_CHANGE_NAMES, change_counts) if n != 'relabelled')


def write_report(home, text):
    with open(path_report(home), 'w') as out:
        out.write(report_header())
        out.write(text)
