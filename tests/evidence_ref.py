# coding=utf-8
"""Test-side restatement of the evidence table (duet_amd/csrc/duet_evidence.hip; include/duet_ef.h, "Evidence table"): the two
states beside the 18 leaves on top of tune_leaf_ref.leaf_of, and the text of a row by plain % formatting."""
import numpy as np

from duet_amd import _lib
from tests import tune_leaf_ref

NO_SEED, FILTERED = 0xFD, 0xFE
COLUMNS = ('CHROM', 'POS', 'SVTYPE', 'SVLEN', 'SVREAD', 'REFREAD', 'MARKS', 'RULE', 'CLASS', 'HAP1', 'HAP2', 'HAP0', 'VOTERS', 'PCSUM1',
           'PCSUM2', 'PS', 'HP')
HP_TEXT = ('.', '1|0', '0|1', '1|1')
TYPES = ('DEL', 'INS', 'INV', 'DUP')


def leaves(feat, v):
    """feat FEATURE_DTYPE[C], one vector -> (leaf u8[C], pred u8[C]): the leaf of an eligible candidate, NO_SEED for one that is kept
    but not eligible, FILTERED for one that is not kept; pred 0 unless eligible."""
    leaf, pred = tune_leaf_ref.leaves_from_features(feat, v)
    state = np.where(feat['kept'] != 0, NO_SEED, FILTERED)
    return np.where(leaf >= 0, leaf, state).astype(np.uint8), pred.astype(np.uint8)


def rule_text(code):
    code = int(code)
    if code == FILTERED:
        return 'filtered'
    if code == NO_SEED:
        return 'no_seed'
    return _lib.LEAF_NAMES[code]                  # (IndexError: not a code)


def row_text(chrom, pos, svtype, svlen, f, leaf, pred):
    """One row; f: one FEATURE_DTYPE record (or a dict of its fields)."""
    g = lambda n: int(f[n])
    cls = '%d' % g('cls') if g('kept') else '.'
    vote = ['%d' % g(n) for n in ('hap1', 'hap2', 'hap0', 'allhap', 't1', 't2', 'ps')] if g('eligible') else ['.'] * 7
    return '%s\t%d\t%s\t%d\t%d\t%d\t%d\t%s\t%s\t%s\t%s\n' % (chrom, int(pos), svtype, int(svlen), g('svread'), g('refread'), g('deg'),
                                                             rule_text(leaf), cls, '\t'.join(vote), HP_TEXT[int(pred)])


def rows_text(chrom, pos, svtype, svlen, feat, leaf, pred):
    """The data rows, in candidate order; chrom / svtype: one str per candidate."""
    return ''.join(row_text(chrom[c], pos[c], svtype[c], svlen[c], feat[c], leaf[c], pred[c]) for c in range(len(feat)))


def table_text(cand_contig, cand_type, cand_pos, cand_span, chrom_texts, feat, leaf, pred):
    """The rows of the table form: CHROM by contig index, SVTYPE by type code 0 .. 3."""
    return rows_text([chrom_texts[int(k)] for k in cand_contig], cand_pos, [TYPES[int(t)] for t in cand_type], cand_span, feat, leaf, pred)


def header():
    return '\t'.join(COLUMNS) + '\n'


def pool_of(chrom, svtype, ref=None, alt=None):
    """Per-candidate strs -> (pool u8[], str_off u32[4 C + 1]) in duet_rows_problem's layout (CHROM, REF, ALT, SVTYPE)."""
    C = len(chrom)
    ref = ref if ref is not None else ['N'] * C
    alt = alt if alt is not None else ['<X>'] * C
    parts, off = [], [0]
    for c in range(C):
        for t in (chrom[c], ref[c], alt[c], svtype[c]):
            b = t.encode() if isinstance(t, str) else t
            parts.append(b)
            off.append(off[-1] + len(b))
    return np.frombuffer(b''.join(parts), dtype=np.uint8).copy(), np.array(off, dtype=np.uint32)
