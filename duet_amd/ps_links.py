# coding=utf-8
"""Phase-set links (include/duet_ef.h: duet_ps_links_device): the host side of `duet --write_ps_links`.

The device builds one record per pair of neighbouring phase sets that the SV candidates of a contig tie together
(_lib.PS_LINK_DTYPE).  Here: the verdict of a record, the two tables as text, and the blocks the links join the phase sets into.
The tables have thousands of rows, not millions: they are formatted on the host.
"""

import numpy as np

COLUMNS = ('CHROM', 'PS_A', 'PS_B', 'N_SV', 'N_SAME', 'N_FLIP', 'N_OPEN', 'W_SAME', 'W_FLIP', 'POS_MIN', 'POS_MAX', 'VERDICT')
BLOCK_COLUMNS = ('CHROM', 'PS', 'BLOCK', 'FLIP')


def links_path(home):
    return home + '/phased_sv.ps_links.tsv'


def blocks_path(home):
    return home + '/phased_sv.ps_blocks.tsv'


def header():
    """The header line of phased_sv.ps_links.tsv."""
    return '\t'.join(COLUMNS) + '\n'


def blocks_header():
    """The header line of phased_sv.ps_blocks.tsv."""
    return '\t'.join(BLOCK_COLUMNS) + '\n'


def verdict(rec):
    """(n_same, w_same) against (n_flip, w_flip), lexicographically: 'same', 'flip', or '.' when they are equal."""
    same, flip = (int(rec['n_same']), int(rec['w_same'])), (int(rec['n_flip']), int(rec['w_flip']))
    return 'same' if same > flip else ('flip' if flip > same else '.')


def _text(t):
    return t.decode() if isinstance(t, bytes) else t


def rows_text(records, chrom_texts):
    """The data rows of phased_sv.ps_links.tsv, one per record in the records' order; CHROM = chrom_texts[contig]."""
    out = []
    for r in records:
        out.append('\t'.join([_text(chrom_texts[int(r['contig'])])] +
                             [str(int(r[f])) for f in ('ps_a', 'ps_b', 'n_sv', 'n_same', 'n_flip', 'n_open', 'w_same', 'w_flip', 'pos_min',
                                                      'pos_max')] + [verdict(r)]) + '\n')
    return ''.join(out)


def blocks(records, min_sv=1):
    """A maximum spanning forest per contig over the links whose verdict is not '.' and whose winning side counts at least min_sv
    candidates (1: every verdict link; the other links still name their phase sets): the links are taken in the order
    (-n_win, -w_win, row index), win being the verdict's side; a link joins two components or agrees with the sense they already
    imply; one that contradicts it is not applied.
    -> (rows, conflicts): rows = one (contig, ps, block, flip) per phase set that occurs in any link, ascending by (contig, ps),
    block = the smallest PS of its component, flip = 0 / 1 relative to that PS; conflicts = the row indices of the contradicting
    links, in the order they were met."""
    order = []
    for i, r in enumerate(records):
        v = verdict(r)
        if v == '.':
            continue
        side = 'same' if v == 'same' else 'flip'
        if int(r['n_' + side]) < min_sv:
            continue
        order.append((-int(r['n_' + side]), -int(r['w_' + side]), i, 0 if v == 'same' else 1))
    order.sort()
    parent, parity = {}, {}                     # union-find: parity[x] = sense of x relative to parent[x]

    def find(x):
        path = []
        while parent[x] != x:
            path.append(x)
            x = parent[x]
        # compress: re-hang the path under the root, parities accumulated from the root's side
        acc = 0
        for y in reversed(path):
            acc ^= parity[y]
            parent[y], parity[y] = x, acc
        return x

    for r in records:
        for ps in (int(r['ps_a']), int(r['ps_b'])):
            node = (int(r['contig']), ps)
            if node not in parent:
                parent[node], parity[node] = node, 0
    conflicts = []
    for _, _, i, sense in order:
        r = records[i]
        a, b = (int(r['contig']), int(r['ps_a'])), (int(r['contig']), int(r['ps_b']))
        ra, rb = find(a), find(b)
        between = parity[a] ^ parity[b]         # (after find, a node hangs under its root: parity is relative to the root)
        if ra == rb:
            if between != sense:
                conflicts.append(i)
            continue
        lo, hi = (ra, rb) if ra < rb else (rb, ra)      # the smaller PS stays the root: it names the block
        parent[hi], parity[hi] = lo, between ^ sense
    rows = []
    for node in sorted(parent):
        root = find(node)
        rows.append((node[0], node[1], root[1], parity[node]))
    return rows, conflicts


def blocks_text(rows, chrom_texts):
    """The data rows of phased_sv.ps_blocks.tsv."""
    return ''.join('%s\t%d\t%d\t%d\n' % (_text(chrom_texts[k]), ps, block, flip) for k, ps, block, flip in rows)


def write(home, records, chrom_texts):
    """Both tables of `records` (PS_LINK_DTYPE, ascending) into <home>; -> (links, phase sets, conflicts)."""
    rows, conflicts = blocks(records)
    with open(links_path(home), 'w') as out:
        out.write(header())
        out.write(rows_text(records, chrom_texts))
    with open(blocks_path(home), 'w') as out:
        out.write(blocks_header())
        out.write(blocks_text(rows, chrom_texts))
    return len(records), len(rows), len(conflicts)


def empty():
    from duet_amd import _lib
    return np.zeros(0, dtype=_lib.PS_LINK_DTYPE)
