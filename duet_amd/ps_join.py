# coding=utf-8
"""Joined phase sets (include/duet_ef.h: duet_ps_join_tags_device, duet_ps_join_diff_device): the host side
of `duet --join_ps`.

The phase-set links (duet_amd/ps_links.py) say which phase sets the SV candidates tie into one block.  Here: which links are
trusted, the table (contig, PS) -> (BLOCK, FLIP) as the record array the device takes, and the text of the report.  The device
remaps the read tags under the table, the run is repeated on them, and the device compares the two runs candidate by candidate
(_lib.JOIN_CHANGE_NAMES).  The report has one row per candidate whose call changed -- thousands, not millions: it is formatted on
the host.
"""

import numpy as np

from duet_amd import ps_links

REPORT_COLUMNS = ('CHROM', 'POS', 'SVLEN', 'CHANGE', 'HP', 'PS', 'HP_JOINED', 'PS_JOINED')
REPORTED = (1, 2, 5, 6, 7)              # gained, lost, to_het, to_hom, other: `none`, `same` and `relabelled` are not listed
HP_TEXT = ('.', '1|0', '0|1', '1|1')
MIN_SV = 2                              # --join_min_sv: no candidate is rescued by a link that it alone observes


def path_vcf(home):
    return home + '/phased_sv.joined.vcf'


def path_report(home):
    return home + '/phased_sv.join_report.tsv'


def path_blocks(home):
    return home + '/phased_sv.join_blocks.tsv'


def check_min_sv(min_sv):
    """--join_min_sv as an integer >= 1, or ValueError."""
    n = int(min_sv)
    if n != min_sv or n < 1:
        raise ValueError('join_min_sv: an integer >= 1, not %r' % (min_sv,))
    return n


def select(records, min_sv=MIN_SV):
    """The links (PS_LINK_DTYPE) that join phase sets: verdict `same` or `flip`, the winning side seen by at least min_sv
    candidates.  ps_links.blocks(select(records, n)) joins what ps_links.blocks(records, min_sv=n) joins."""
    keep = []
    for i, r in enumerate(records):
        v = ps_links.verdict(r)
        if v != '.' and int(r['n_' + v]) >= min_sv:
            keep.append(i)
    return records[np.asarray(keep, dtype=np.int64)]


def table(rows):
    """The rows (contig, ps, block, flip) of ps_links.blocks as the record array of duet_ps_join_* (_lib.PS_BLOCK_DTYPE)."""
    from duet_amd import _lib
    out = np.zeros(len(rows), dtype=_lib.PS_BLOCK_DTYPE)
    for i, row in enumerate(rows):
        out[i] = tuple(int(x) for x in row)
    return out


def report_header():
    return '\t'.join(REPORT_COLUMNS) + '\n'


def _hp_ps(pred, ps):
    return (HP_TEXT[pred], str(ps)) if pred else ('.', '.')


def report_text(chrom_texts, cand_contig, pos, svlen, change, pred0, ps0, pred1, ps1):
    """The data rows of phased_sv.join_report.tsv: one per candidate whose change code is in REPORTED, in candidate order.
    chrom_texts: the CHROM text per contig; cand_contig: the contig index per candidate; svlen: the candidates' abs(SVLEN)."""
    from duet_amd import _lib
    out = []
    for c in np.flatnonzero(np.isin(np.asarray(change), REPORTED)):
        t = chrom_texts[int(cand_contig[c])]
        out.append('\t'.join((t.decode() if isinstance(t, bytes) else t, str(int(pos[c])), str(int(svlen[c])),
                              _lib.JOIN_CHANGE_NAMES[int(change[c])]) + _hp_ps(int(pred0[c]), int(ps0[c])) +
                             _hp_ps(int(pred1[c]), int(ps1[c]))) + '\n')
    return ''.join(out)


def summary_text(counts, n_changed=None, n_blocks=None):
    """The log line of a joined run: the eight counts by name, then the remapped reads and the table's rows where given."""
    from duet_amd import _lib
    text = ', '.join('%s %d' % (n, int(v)) for n, v in zip(_lib.JOIN_CHANGE_NAMES, counts))
    if n_changed is not None:
        text += '; %d read tags remapped' % n_changed
    if n_blocks is not None:
        text += '; %d phase sets in the table' % n_blocks
    return text


def write_blocks(home, rows, chrom_texts):
    with open(path_blocks(home), 'w') as out:
        out.write(ps_links.blocks_header())
        out.write(ps_links.blocks_text(rows, chrom_texts))


def write_report(home, text):
    with open(path_report(home), 'w') as out:
        out.write(report_header())
        out.write(text)
