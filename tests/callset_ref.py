# coding=utf-8
"""Plain-Python statement of the rows of sv_calling/variants.vcf in the svim-gpu mode: the tests'
reference for duet_svim_vcf_rows_device / _host, in the manner of tests/tune_ref.py."""

TYPES = ('DEL', 'INS', 'INV', 'DUP')


def genotype(n, dp):
    """1/1 if 5n >= 4 DP, else 0/1 if 5n >= DP, else 0/0 (integers)."""
    if 5 * n >= 4 * dp:
        return '1/1'
    return '0/1' if 5 * n >= dp else '0/0'


def rows(res, mark_names, depth, depth_off, depth_bin, chrom_texts):
    """res: cluster result dict(order, cand_off, cand_contig, cand_type, cand_pos, cand_span); mark_names: the read name (str)
    of every RAW mark; depth / depth_off: binned coverage per contig; chrom_texts: CHROM text per contig.  -> text of the rows."""
    out = []
    row_in_contig = {}
    order, off = [int(x) for x in res['order']], [int(x) for x in res['cand_off']]
    for c in range(len(res['cand_pos'])):
        k, t = int(res['cand_contig'][c]), int(res['cand_type'][c])
        if t > 3:
            raise ValueError('type code %d' % t)
        pos, span = int(res['cand_pos'][c]), int(res['cand_span'][c])
        members = order[off[c]:off[c + 1]]
        n = len(members)
        i = row_in_contig.get(k, 0) + 1
        row_in_contig[k] = i
        lo, hi = int(depth_off[k]), int(depth_off[k + 1])
        d = int(depth[lo + min(pos // depth_bin, hi - lo - 1)]) if hi > lo else 0
        ref = max(d - n, 0)
        dp = n + ref
        T = TYPES[t]
        end = pos if T == 'INS' else pos + span
        svlen = -span if T == 'DEL' else span
        chrom = chrom_texts[k]
        out.append('%s\t%d\tsvim_gpu.%s.%d\tN\t<%s>\t.\tPASS\tSVTYPE=%s;END=%d;SVLEN=%d;SUPPORT=%d;READS=%s\tGT:DP:AD\t%s:%d:%d,%d\n' % (
            chrom, pos, chrom, i, T, T, end, svlen, n, ','.join(mark_names[m] for m in members), genotype(n, dp), dp, ref, n))
    return ''.join(out)


def names_of(got):
    """NativeIngest.extract(..., names=True) result -> the read name of every raw mark."""
    pool, off = bytes(got['name_pool']), got['name_off']
    table = [pool[int(off[j]):int(off[j + 1])].decode() for j in range(len(off) - 1)]
    return [table[int(j)] for j in got['mark_name']]
