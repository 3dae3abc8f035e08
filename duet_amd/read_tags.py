# coding=utf-8
"""Read tags from phased SVs (include/duet_ef.h: duet_read_tags_device): the host side of the table
phased_sv.read_tags.tsv.

The device builds one record per (read name, phase set) over the supporting reads of the heterozygous calls
(_lib.READ_TAG_DTYPE) and formats one row per record (duet_read_tags_rows_*).  Here: the header line, the status names, the
count per status, the same rows in plain Python for a table small enough not to need the device, and the file itself.
"""

import numpy as np

from duet_amd import _lib

COLUMNS = _lib.READ_TAG_COLUMNS
STATUS_NAMES = _lib.READ_TAG_STATUS_NAMES
ABSENT = _lib.MARK_ABSENT
UNTAGGED = 0xFFFFFFFFFFFFFFFF


def path(home):
    return home + '/phased_sv.read_tags.tsv'


def header():
    """The header line of phased_sv.read_tags.tsv."""
    return '\t'.join(COLUMNS) + '\n'


def empty():
    return np.zeros(0, dtype=_lib.READ_TAG_DTYPE)


def summary(records):
    """{status name: count} over the records, every status present."""
    counts = np.bincount(np.asarray(records['status'], dtype=np.int64), minlength=len(STATUS_NAMES))
    return {s: int(counts[i]) for i, s in enumerate(STATUS_NAMES)}


def summary_text(records):
    """The log line's text: the record count and the count per status."""
    counts = summary(records)
    return '%d read tag records: %s' % (len(records), ', '.join('%s %d' % (s, counts[s]) for s in STATUS_NAMES))


def _text(t):
    return t.decode() if isinstance(t, bytes) else t


def hp_sv(rec):
    """'1', '2' or '.': the haplotype the SV calls place the read on."""
    n_h1, n_h2 = int(rec['n_h1']), int(rec['n_h2'])
    return '1' if n_h1 > n_h2 else ('2' if n_h2 > n_h1 else '.')


def own_tag(rec, read_tag):
    """(TAG_HP, TAG_PS, TAG_PC) of the record's read: its own tag word whatever the cap, '.' each when it has none."""
    read = int(rec['read'])
    if read == ABSENT or read >= len(read_tag) or int(read_tag[read]) == UNTAGGED:
        return '.', '.', '.'
    t = int(read_tag[read])
    hap = t >> 62
    return (str(hap) if hap in (1, 2) else '.'), str(t & 0xFFFFFFFF), str((t >> 32) & 0x3FFFFFFF)


def rows_text(records, names, chrom_texts, read_tag):
    """The data rows of phased_sv.read_tags.tsv, one per record in the records' order; names[i]: the text of name i."""
    out = []
    for r in records:
        n_h1, n_h2 = int(r['n_h1']), int(r['n_h2'])
        out.append('\t'.join([_text(chrom_texts[int(r['contig'])]), _text(names[int(r['name'])]), str(int(r['ps'])), str(n_h1 + n_h2),
                              str(n_h1), str(n_h2), hp_sv(r)] + list(own_tag(r, read_tag)) +
                             [STATUS_NAMES[int(r['status'])], str(int(r['pos_min'])), str(int(r['pos_max']))]) + '\n')
    return ''.join(out)


def names_of(name_off, name_pool):
    """The name texts (bytes) of a pool: name j = name_pool[name_off[j] .. name_off[j + 1])."""
    pool = bytes(name_pool) if isinstance(name_pool, (bytes, bytearray)) else np.asarray(name_pool, dtype=np.uint8).tobytes()
    return [pool[int(name_off[j]):int(name_off[j + 1])] for j in range(len(name_off) - 1)]


def write(home, rows):
    """The header line and `rows` (bytes: what duet_read_tags_rows_* wrote, or rows_text(...).encode()) into <home>."""
    with open(path(home), 'wb') as out:
        out.write(header().encode())
        out.write(rows)
