# coding=utf-8
"""The data rows of phased_sv.vcf in the svim-gpu mode, restated in plain Python on the CHROM texts themselves (include/duet_ef.h:
duet_svim_phased_rows_*): what duet_amd/svim_mode.py rows_text writes once it has looked the texts up in a work directory."""

TYPES = ('DEL', 'INS', 'INV', 'DUP')
HP = {1: '1|0', 2: '0|1', 3: '1|1'}


def rows(texts, contig, types, pos, span, pred, ps):
    """(CHROM text per contig, per candidate: contig, type, pos, span, pred, ps) -> bytes.  Raises ValueError where the library
    refuses: a kept candidate with pred > 3 or a contig that has no text."""
    texts = [t.decode('utf-8') if isinstance(t, bytes) else t for t in texts]
    keep = [i for i in range(len(pred)) if int(pred[i]) != 0]
    for i in keep:
        if int(pred[i]) > 3 or int(contig[i]) >= len(texts):
            raise ValueError('candidate %d cannot be written' % i)
    # stable: ties on (CHROM text, POS) keep candidate order; str order is the byte order of the UTF-8 the file holds
    keep.sort(key=lambda i: (texts[int(contig[i])], int(pos[i])))
    out = []
    for n, i in enumerate(keep):
        t = TYPES[int(types[i]) & 3]
        ln = int(span[i])
        out.append('%s\t%d\tDuet.%d\tN\t<%s>\t.\tPASS\tSVLEN=%d;SVTYPE=<%s>\tHP:PS\t%s:%d\n' % (
            texts[int(contig[i])], int(pos[i]), n + 1, t, ln if t in ('INS', 'DUP') else -ln, t, HP[int(pred[i])], int(ps[i])))
    return ''.join(out).encode('utf-8')


def rows_of(texts, res):
    return rows(texts, res['cand_contig'], res['cand_type'], res['cand_pos'], res['cand_span'], res['pred'], res['ps'])
