# coding=utf-8
"""SVIM mode without the external caller: the haplotagged BAMs of <home>/snp_phasing alone ->
raw SV marks (CIGAR insertions / deletions, native BAM pass) -> stage A0 -> adapter -> step E/F, the last three in one
device pipeline (duet_svim_phase_device).  Upstream runs `svim alignment` here (src/duet/sv_calling.py:13-15) and reads
its VCF back; the extraction and clustering rules used instead are this repository's own (oracle/svim_oracle.py,
oracle/cluster_oracle.c; parity unpinned), step E/F is the pinned one.
"""

import logging
import os
import time

import numpy as np

from duet_amd import bamio, engine
from duet_amd.native import NativeIngest
from duet_amd.read_file import init_chrom_list


def device_compute(ctx, chrom_texts=None, row_texts=None, thresholds=None, pc_cap=None, evidence_texts=None, ps_links=False,
                   read_tag_texts=None, join_min_sv=None, sv_tags=None):
    """-> compute(extracted arrays, svlen_thres, suppread_thres, max_dist, depth_bin) -> dict of result arrays, on ctx's GPU:
    stage A0 -> adapter -> step E/F in one device pipeline (duet_svim_phase_device).  chrom_texts (CHROM text per contig): the
    extracted arrays carry the marks' read names, and the result also holds `calls`, the rows of sv_calling/variants.vcf formatted
    on the same resident arrays (duet_svim_vcf_rows_device).  row_texts (CHROM text per contig): the result also holds `rows` /
    `n_rows`, the data rows of phased_sv.vcf sorted and formatted on the resident arrays (duet_svim_phased_rows_device).
    thresholds (float64[14], --thresholds): the decision is made with this vector -- the candidates' features
    (duet_svim_features_device; pc_cap: under that PC cap, duet_svim_features_cap_device) and one vector applied to them
    (duet_tune_sweep_device) in place of the fused run's E/F.  evidence_texts (CHROM text per contig; needs thresholds): the result
    also holds `evidence`, the data rows of the evidence table, one per candidate (duet_evidence_rows_device).  ps_links: the result
    also holds `ps_links`, the phase-set link records of the candidates (duet_svim_ps_links_device; the voters under pc_cap).
    read_tag_texts (CHROM text per contig; the extracted arrays carry the marks' read names): the result also holds `read_tags`,
    (records, rows) of the read tags of the calls just made (duet_read_tags_device and its rows; a tag usable under pc_cap).
    join_min_sv (--join_ps; needs row_texts): the result also holds `join`, the run over the phase sets that the links of at least
    that many candidates join (DeviceSvim.run_joined): dict(blocks, pred, ps, change, counts, n_changed, rows, n_rows), or
    dict(blocks, error) when the joined run raised ZeroDivisionError.
    sv_tags (--vote_sv_tags, (min_votes, pc_new); needs row_texts and the marks' read names): the result also holds `sv_tags`, the
    run with the untagged reads voting by the tags the other SVs give them (DeviceSvim.run_sv_tags): dict(pred, ps, change, counts,
    marks, rows, n_rows), or dict(error) when that run raised ZeroDivisionError."""
    if evidence_texts is not None and thresholds is None:
        raise ValueError('the evidence table needs a threshold vector')
    if sv_tags is not None and row_texts is None:
        raise ValueError('the run with the tags of the other SVs needs the CHROM texts of its rows')
    if join_min_sv is not None and row_texts is None:
        raise ValueError('the joined run needs the CHROM texts of its rows')

    def compute(got, svlen_thres, suppread_thres, max_dist, depth_bin):
        from duet_amd.devmem import DeviceSvim
        ds = DeviceSvim(got, got['read_tag'], got['depth'], got['depth_off'], depth_bin, svlen_thres, suppread_thres,
                        max_dist=max_dist, device='cuda:%d' % ctx.device_id)
        if thresholds is not None:
            ds.run_thresholds(ctx, thresholds, pc_cap=pc_cap, keep_features=evidence_texts is not None)
        else:
            ds.run_fused(ctx)
            ctx.check(ds.torch.cuda.current_stream(ds.device).cuda_stream)
        out = ds.fetch()
        res = dict(cand_contig=out['cand_contig'], cand_type=out['cand_type'], cand_pos=out['cand_pos'],
                   cand_span=out['cand_span'], support=np.diff(out['cand_off'].astype(np.int64)), pred=out['pred'], ps=out['ps'])
        if row_texts is not None:
            res['rows'], res['n_rows'] = ds.phased_rows(ctx, row_texts)
        if chrom_texts is not None:
            res['calls'] = ds.vcf_rows(ctx, got, chrom_texts)
        if evidence_texts is not None:
            res['evidence'] = ds.evidence_rows(ctx, evidence_texts)
        if read_tag_texts is not None:
            res['read_tags'] = ds.read_tags(ctx, got, read_tag_texts, pc_cap=pc_cap)
        links = None
        if ps_links or join_min_sv is not None:
            links = ds.ps_links(ctx, pc_cap=pc_cap)                 # (last: it clusters again, into the same result arrays)
        if ps_links:
            res['ps_links'] = links
        if join_min_sv is not None:
            from duet_amd import ps_join, ps_links as links_mod
            blocks = links_mod.blocks(links, min_sv=join_min_sv)[0]
            res['join'] = join = dict(blocks=blocks)
            try:
                join.update(ds.run_joined(ctx, ps_join.table(blocks), got['read_off'], thresholds=thresholds, pc_cap=pc_cap))
                join['rows'], join['n_rows'] = ds.phased_rows(ctx, row_texts, pred=join['pred'], ps=join['ps'])
                N = len(join['change'])
                join['pred'], join['ps'] = join['pred'][:N].cpu().numpy(), join['ps'][:N].cpu().numpy().view(np.uint32)
            except ZeroDivisionError as e:
                join['error'] = e                                   # (raised once phased_sv.vcf has been written in full)
        if sv_tags is not None:
            res['sv_tags'] = second = dict()
            try:
                second.update(ds.run_sv_tags(ctx, got, min_votes=sv_tags[0], pc_new=sv_tags[1], thresholds=thresholds, pc_cap=pc_cap))
                second['rows'], second['n_rows'] = ds.phased_rows(ctx, row_texts, pred=second['pred'], ps=second['ps'])
                N = len(second['change'])
                second['pred'], second['ps'] = second['pred'][:N].cpu().numpy(), second['ps'][:N].cpu().numpy().view(np.uint32)
            except ZeroDivisionError as e:
                second['error'] = e                                 # (raised once phased_sv.vcf has been written in full)
        return res
    return compute


def host_compute(ctx, chrom_texts=None):
    """The same through host arrays (duet_svim_phase_host, duet_svim_vcf_rows_host): what a rank of `-b svim-gpu --gpus N`
    uses -- no torch in the process."""
    def compute(got, svlen_thres, suppread_thres, max_dist, depth_bin):
        out = ctx.svim_host(got, got['read_tag'], got['depth'], got['depth_off'], depth_bin, svlen_thres, suppread_thres, max_dist=max_dist,
                            want_order=chrom_texts is not None)
        res = dict(cand_contig=out['cand_contig'], cand_type=out['cand_type'], cand_pos=out['cand_pos'], cand_span=out['cand_span'],
                   support=np.diff(out['cand_off'].astype(np.int64)), pred=out['pred'], ps=out['ps'])
        if chrom_texts is not None:
            res['calls'] = ctx.svim_vcf_rows_host(out, len(got['pos']), got['mark_name'], got['name_off'], got['name_pool'], got['depth'],
                                                  got['depth_off'], depth_bin, chrom_texts)
        return res
    return compute


class ReadNameError(ValueError):
    """A read name that READS= of sv_calling/variants.vcf cannot hold."""


def check_read_names(got):
    """A read name with ',' or ';' cannot be listed in READS= and read back: such a name fails the run (--write_sv_calls)."""
    pool = got['name_pool']
    bad = np.flatnonzero((pool == ord(',')) | (pool == ord(';')))
    if bad.size:
        j = int(np.searchsorted(got['name_off'], bad[0], side='right')) - 1
        name = pool[int(got['name_off'][j]):int(got['name_off'][j + 1])].tobytes().decode('utf-8', 'replace')
        raise ReadNameError('read name %r contains "," or ";": it cannot be listed in READS= of sv_calling/variants.vcf '
                         '(--write_sv_calls)' % name)


def phase_from_bams(home, svlen_thres=50, suppread_thres=2, thread=4, include_all_ctgs=False, max_dist=0.9,
                    min_sv_size=40, min_mapq=20, depth_bin=1000, ctx=None, only=None, compute=None, names=False, keep_names=False):
    """-> dict(chroms, cand_contig u16[N], cand_type u8[N] (1 INS / 0 DEL), cand_pos, cand_span, support, pred, ps).
    only: the contig indices to read (a rank of a sharded run; the contig numbering stays the whole list's);
    compute: what turns the extracted arrays into results (default: the GPU pipeline on ctx);
    names (--write_sv_calls): the marks' read names are extracted and checked before anything runs on the device, and the
    result also holds `calls`, the rows of sv_calling/variants.vcf (a compute made with chrom_texts).  A compute made with
    row_texts adds `rows` / `n_rows`: the data rows of phased_sv.vcf, sorted and formatted on the device.
    keep_names (--write_read_tags): the marks' read names are extracted for the compute, unchecked: no READS= lists them."""
    chroms = init_chrom_list(include_all_ctgs, home)
    ing, got = NativeIngest.extract(home + '/snp_phasing/', chroms, thread, min_sv_size, min_mapq, depth_bin, only=only,
                                    names=names or keep_names)
    if ing is None:
        raise RuntimeError('signature extraction declined the input: %s' % got)
    ing.close()
    if names:
        check_read_names(got)
    N0 = dict(chroms=chroms, cand_contig=np.zeros(0, np.uint16), cand_type=np.zeros(0, np.uint8),
              cand_pos=np.zeros(0, np.uint32), cand_span=np.zeros(0, np.uint32), support=np.zeros(0, np.int64),
              pred=np.zeros(0, np.uint8), ps=np.zeros(0, np.uint32))
    N0['n_marks'] = 0
    if names:
        N0['calls'] = np.zeros(0, np.uint8)
    if len(got['pos']) == 0:
        return N0
    if compute is None:
        compute = device_compute(ctx if ctx is not None else engine.default_context(),
                                 spelled_contigs(home, chroms) if names else None)
    out = compute(got, svlen_thres, suppread_thres, max_dist, depth_bin)
    return dict(out, chroms=chroms, n_marks=len(got['pos']))


SV_TYPE_NAMES = ('DEL', 'INS', 'INV', 'DUP')          # the extraction's type codes (oracle/svim_oracle.py)


def spelled_contigs(home, chroms):
    """CHROM text per contig: the spelling of its BAM (chr<c>.bam else <c>.bam, as sv_phasing_fn.py:19-24 looks them up)."""
    names = []
    for c in chroms:
        names.append('chr' + c if os.path.exists(os.path.join(home, 'snp_phasing', 'chr' + c + '.bam')) else c)
    return names


def rows_text(home, res):
    """Rows in phased_sv.vcf's layout (write_file.py:6-17) for the phased candidates of `res`: symbolic REF/ALT,
    sorted like sv_phasing_fn.py:229 (CHROM as text, POS), ids renumbered."""
    names = spelled_contigs(home, res['chroms'])
    hp = {1: '1|0', 2: '0|1', 3: '1|1'}
    keep = np.nonzero(res['pred'])[0]
    order = sorted(keep, key=lambda i: (names[int(res['cand_contig'][i])], int(res['cand_pos'][i])))
    out = []
    for n, i in enumerate(order):
        t = SV_TYPE_NAMES[int(res['cand_type'][i]) & 3]
        ln = int(res['cand_span'][i])
        # (the sign rule of sv_phasing_fn.py:225: positive for INS and DUP, negative for everything else)
        out.append('%s\t%d\tDuet.%d\tN\t<%s>\t.\tPASS\tSVLEN=%d;SVTYPE=<%s>\tHP:PS\t%s:%d\n' % (
            names[int(res['cand_contig'][i])], int(res['cand_pos'][i]), n + 1, t, ln if t in ('INS', 'DUP') else -ln, t,
            hp[int(res['pred'][i])], int(res['ps'][i])))
    return ''.join(out)


def contig_lines(home, chroms):
    """The ##contig lines of this mode: one per listed contig that has a BAM, from the BAM's own reference list."""
    lines = []
    for c, name in zip(chroms, spelled_contigs(home, chroms)):
        bam = os.path.join(home, 'snp_phasing', name + '.bam')
        if not os.path.exists(bam):
            continue
        for ref, length in bamio.read_refs(bam):
            if ref == name:
                lines.append('##contig=<ID=%s,length=%d>\n' % (ref, length))
                break
    return ''.join(lines)


def header_text(home, chroms):
    """phased_sv.vcf header lines (write_file.py:19-45).  Upstream copies the ##contig lines of the caller VCF; this mode
    has no caller VCF, so every listed contig that has a BAM contributes one line from the BAM's own reference list."""
    from duet_amd.write_file import _COLS, _HEAD
    return _HEAD + contig_lines(home, chroms) + _COLS


# sv_calling/variants.vcf of this mode (--write_sv_calls): the clustered candidates in the repository's own
# dialect, modelled on SVIM's -- readable by read_file.parse_vcf (READS= / GT:DP:AD) and the native VCF ingest
CALLSET_INFO = ''.join(line + '\n' for line in (
    '##ALT=<ID=DEL,Description="Deletion">',
    '##ALT=<ID=INS,Description="Insertion">',
    '##ALT=<ID=INV,Description="Inversion">',
    '##ALT=<ID=DUP,Description="Duplication">',
    '##INFO=<ID=SVTYPE,Number=1,Type=String,Description="Type of structural variant">',
    '##INFO=<ID=END,Number=1,Type=Integer,Description="End position of the variant described in this record">',
    '##INFO=<ID=SVLEN,Number=1,Type=Integer,Description="Difference in length between REF and ALT alleles">',
    '##INFO=<ID=SUPPORT,Number=1,Type=Integer,Description="Number of reads supporting this variant">',
    '##INFO=<ID=READS,Number=.,Type=String,Description="Names of the supporting reads">',
    '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
    '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Read depth">',
    '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Read depth for each allele">',
))
CALLSET_COLS = '\t'.join(('#CHROM', 'POS', 'ID', 'REF', 'ALT', 'QUAL', 'FILTER', 'INFO', 'FORMAT', 'SAMPLE')) + '\n'


def callset_header_text(home, chroms):
    return '##fileformat=VCFv4.2\n##source=duet_amd svim-gpu\n' + contig_lines(home, chroms) + CALLSET_INFO + CALLSET_COLS


def callset_path(home):
    return os.path.join(home, 'sv_calling', 'variants.vcf')


def write_callset(home, chroms, rows):
    """<home>/sv_calling/variants.vcf: header + the rows (bytes or a uint8 array), replacing any old file."""
    os.makedirs(os.path.join(home, 'sv_calling'), exist_ok=True)
    with open(callset_path(home), 'wb') as out:
        out.write(callset_header_text(home, chroms).encode())
        out.write(rows)


# ------------------------------------------------------------------------------------------------------------------
# the same over the N GPUs of one node (BASELINE configs[3]: `--sv_caller svim --cluster_max_distance 0.9`, 8 GPUs)
# ------------------------------------------------------------------------------------------------------------------
# Partitions of stage A0 never cross a contig and step E/F is per contig, so RAW MARKS shard by contig exactly like
# candidates do: a rank reads whole contigs' BAMs (marks, tag tables, depth bins), runs the device pipeline on them,
# and the candidates are reassembled by one all-gather of fixed-size records -- sized by a 16-byte exchange of the
# counts, since how many candidates a rank finds is a result, not an input.  Rank 0 writes the rows.

REC_WORDS = 5                     # u32 per candidate: contig | type << 16 | pred << 24, pos, span, support, ps


def bam_weights(home, chroms):
    """Bytes of each listed contig's BAM (0 without one): what the contig -> rank assignment balances.  Every rank
    computes the same numbers from the directory alone."""
    out = []
    for c, name in zip(chroms, spelled_contigs(home, chroms)):
        path = os.path.join(home, 'snp_phasing', name + '.bam')
        out.append(os.path.getsize(path) if os.path.exists(path) else 0)
    return out


def pack_records(res):
    n = len(res['pred'])
    rec = np.zeros((n, REC_WORDS), dtype=np.uint32)
    if n:
        rec[:, 0] = res['cand_contig'].astype(np.uint32) | (res['cand_type'].astype(np.uint32) << 16) | \
            (res['pred'].astype(np.uint32) << 24)
        rec[:, 1], rec[:, 2] = res['cand_pos'], res['cand_span']
        rec[:, 3], rec[:, 4] = res['support'], res['ps']
    return rec


def unpack_records(rec):
    rec = rec.reshape(-1, REC_WORDS)
    return dict(cand_contig=(rec[:, 0] & 0xFFFF).astype(np.uint16), cand_type=((rec[:, 0] >> 16) & 0xFF).astype(np.uint8),
                pred=(rec[:, 0] >> 24).astype(np.uint8), cand_pos=rec[:, 1].copy(), cand_span=rec[:, 2].copy(),
                support=rec[:, 3].astype(np.int64), ps=rec[:, 4].copy())


def part_path(home, rank):
    """Where a rank of a sharded --write_sv_calls run leaves its contigs' callset rows for rank 0 (removed by rank 0)."""
    return os.path.join(home, 'sv_calling', 'variants.vcf.rank%d.part' % rank)


def rank_body(home, svlen_thres, suppread_thres, thread, include_all_ctgs, max_dist, rank, world, compute, to_device=None,
              star=None, gather=None, write_sv_calls=False, format_rows=None):
    """One rank of the sharded SVIM mode.  compute as in phase_from_bams.  Rank 0 appends the rows to the file that
    already holds the header.  -> exit code (5: division by zero on some rank).
    star / gather (duet_amd/comm.py; round 4): how many candidates a rank finds is a result, not an input, so the ranks first
    tell each other their counts -- 16 bytes each, a control message over the TCP star that also carried RCCL's id -- and then
    ONE all-gather (gather.allgather: RCCL inside libduet_ef.so, or the star in the one-GPU plumbing mode) moves the fixed-size
    candidate records.  Without them: torch.distributed's default group for both (the CPU tests over gloo, DUET_COMM=torch);
    to_device: where its tensors live.
    write_sv_calls: every rank writes its contigs' callset rows (part_path) BEFORE the exchange of the counts; rank 0 then
    writes phased_sv.vcf whole (the parent wrote no header) and assembles sv_calling/variants.vcf from the parts
    (status 6: a read name that READS= cannot hold, on some rank -- nothing is written).
    format_rows: (merged result dict, CHROM text per contig) -> the bytes of phased_sv.vcf's data rows, what rank 0 writes
    (rank_main: duet_svim_phased_rows_host on the rank's context); default: rows_text."""
    from duet_amd import dist as D
    chroms = init_chrom_list(include_all_ctgs, home)
    owned = D.lpt_assign(bam_weights(home, chroms), world)
    status, res = 0, None
    try:
        res = phase_from_bams(home, svlen_thres, suppread_thres, max(1, int(thread) // world), include_all_ctgs,
                              max_dist=max_dist, min_sv_size=max(int(svlen_thres), 1), only=set(owned[rank]), compute=compute,
                              names=write_sv_calls)
    except ZeroDivisionError:
        status = 5
    except ReadNameError as e:
        logging.error(str(e))
        status, res = 6, None
    if write_sv_calls and status == 0:
        os.makedirs(os.path.join(home, 'sv_calling'), exist_ok=True)
        with open(part_path(home, rank), 'wb') as f:
            f.write(res['calls'])
    merge = lambda g, counts: _merge_and_write(home, chroms, g, counts, world, owned if write_sv_calls else None, format_rows)
    rec = pack_records(res) if res is not None else np.zeros((0, REC_WORDS), dtype=np.uint32)
    if gather is not None:
        mine = np.array([len(rec), status, res['n_marks'] if res is not None else 0, 0], dtype=np.int32)
        counts = np.frombuffer(b''.join(star.allgather(mine.tobytes())), dtype=np.int32).reshape(world, 4)
        if int(counts[:, 1].max()) != 0:
            return _failed(home, rank, world, counts, write_sv_calls)
        n_max = max(int(counts[:, 0].max()), 1)
        slot = np.zeros(n_max * REC_WORDS, dtype=np.uint32)
        slot[:rec.size] = rec.reshape(-1)
        g = gather.allgather(slot.view(np.uint8))                 # the ONE data-path collective: fixed-size candidate records
        if rank != 0:
            return 0
        g = np.ascontiguousarray(g).view(np.uint32).reshape(world, n_max, REC_WORDS)
        return merge(g, counts)
    import torch
    import torch.distributed as td
    dev = to_device if to_device is not None else torch.device('cpu')
    mine = torch.tensor([len(rec), status, res['n_marks'] if res is not None else 0, 0], dtype=torch.int32, device=dev)
    counts = torch.empty(4 * world, dtype=torch.int32, device=dev)
    td.all_gather_into_tensor(counts, mine)                       # 16 bytes per rank: how large the records' slots must be
    counts = counts.cpu().numpy().reshape(world, 4)
    if int(counts[:, 1].max()) != 0:
        return _failed(home, rank, world, counts, write_sv_calls)
    n_max = max(int(counts[:, 0].max()), 1)
    slot = torch.zeros(n_max * REC_WORDS, dtype=torch.int32, device=dev)
    if len(rec):
        slot[:rec.size] = torch.from_numpy(rec.reshape(-1).view(np.int32)).to(dev)
    gathered = torch.empty(world * n_max * REC_WORDS, dtype=torch.int32, device=dev)
    td.all_gather_into_tensor(gathered, slot)                     # the ONE data-path collective: fixed-size candidate records
    if rank != 0:
        return 0
    g = gathered.cpu().numpy().view(np.uint32).reshape(world, n_max, REC_WORDS)
    return merge(g, counts)


def _failed(home, rank, world, counts, write_sv_calls):
    """Some rank failed (status 5 or 6): rank 0 removes the callset parts every rank has written by now."""
    if write_sv_calls and rank == 0:
        for r in range(world):
            if os.path.exists(part_path(home, r)):
                os.remove(part_path(home, r))
    return int(counts[:, 1].max())


def _assemble_callset(home, chroms, owned, merged, world):
    """rank 0: sv_calling/variants.vcf from the ranks' parts.  A part holds its rank's contigs in contig-list order, and the
    first row of contig k is the one whose ID is svim_gpu.<CHROM>.1; the contigs are written in contig-list order."""
    texts = spelled_contigs(home, chroms)
    has_rows = np.bincount(merged['cand_contig'].astype(np.int64), minlength=len(chroms)) > 0
    data, block = [], {}
    for r in range(world):
        with open(part_path(home, r), 'rb') as f:
            data.append(f.read())
        starts, at = [], 0
        for k in sorted(owned[r]):
            if has_rows[k]:
                i = data[r].find(('\tsvim_gpu.%s.1\t' % texts[k]).encode(), at)
                starts.append((k, data[r].rfind(b'\n', 0, i) + 1))
                at = i + 1
        for j, (k, s0) in enumerate(starts):
            block[k] = (r, s0, starts[j + 1][1] if j + 1 < len(starts) else len(data[r]))
    os.makedirs(os.path.join(home, 'sv_calling'), exist_ok=True)
    with open(callset_path(home), 'wb') as out:
        out.write(callset_header_text(home, chroms).encode())
        for k in range(len(chroms)):
            if k in block:
                r, s0, e0 = block[k]
                out.write(memoryview(data[r])[s0:e0])
    for r in range(world):
        os.remove(part_path(home, r))


def _merge_and_write(home, chroms, g, counts, world, owned=None, format_rows=None):
    """rank 0: the gathered records [world, n_max, REC_WORDS] -> rows appended to phased_sv.vcf.  owned (--write_sv_calls): the
    contig -> rank assignment; phased_sv.vcf is then written whole and sv_calling/variants.vcf assembled from the parts.
    format_rows: see rank_body."""
    parts = [unpack_records(g[r, :int(counts[r, 0])]) for r in range(world)]
    merged = {k: np.concatenate([p_[k] for p_ in parts]) for k in parts[0]}
    # contigs are owned whole and a rank's candidates come contig-major: a stable sort by contig is the single-GPU order
    order = np.argsort(merged['cand_contig'], kind='stable')
    merged = {k: v[order] for k, v in merged.items()}
    merged['chroms'] = chroms
    logging.info('  %d SV marks clustered into %d candidates on %d GPUs, %d phased (clustering rule: parity unpinned)' % (
        int(counts[:, 2].sum()), len(merged['pred']), world, int(np.count_nonzero(merged['pred']))))
    logging.info('write phased callset into .vcf file')
    if format_rows is not None:
        rows = format_rows(merged, spelled_contigs(home, chroms))
        with open(home + '/phased_sv.vcf', 'wb' if owned is not None else 'ab') as out:
            if owned is not None:
                out.write(header_text(home, chroms).encode())
            out.write(rows)
    elif owned is not None:
        with open(home + '/phased_sv.vcf', 'w') as out:
            out.write(header_text(home, chroms) + rows_text(home, merged))
    else:
        with open(home + '/phased_sv.vcf', 'a') as out:
            out.write(rows_text(home, merged))
    if owned is not None:
        logging.info('write the clustered SV calls into sv_calling/variants.vcf')
        _assemble_callset(home, chroms, owned, merged, world)
    return 0


def device_format_rows(ctx):
    """-> rank_body's format_rows for a rank process: rank 0 sorts and formats the merged records on its GPU
    (duet_svim_phased_rows_host)."""
    return lambda merged, row_texts: ctx.svim_phased_rows_host(merged, row_texts)[0]


def rank_main(argv):
    """Entry of one rank process: python -m duet_amd.svim_mode HOME SVLEN SUPP THREAD ALL_CTGS MAX_DIST"""
    import datetime
    home, svlen_thres, suppread_thres, thread = argv[0], int(argv[1]), int(argv[2]), int(argv[3])
    all_ctgs, max_dist = argv[4] == '1', float(argv[5])
    write_sv_calls = len(argv) > 6 and argv[6] == '1'
    texts = spelled_contigs(home, init_chrom_list(all_ctgs, home)) if write_sv_calls else None
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    one_gpu = os.environ.get('DUET_ONE_GPU') == '1'
    device_id = 0 if one_gpu else int(os.environ.get('LOCAL_RANK', rank))
    if os.environ.get('DUET_COMM', '') != 'torch':
        # (no torch in this process: see duet_amd/multi.py rank_main)
        os.environ['DUET_NO_TORCH'] = '1'
        from duet_amd import _lib, comm
        if rank == 0:
            from duet_amd.utils import add_stream_logging
            add_stream_logging(home)
        ctx = _lib.Context(device_id)                    # raises when libduet_ef.so / the GPU is missing: no fallback
        star = comm.TcpStar(rank, world, timeout=float(os.environ.get('DUET_RDZV_TIMEOUT', '300')))
        gather = None
        try:
            gather = comm.HostGather(star) if one_gpu else comm.RcclGather(ctx, star)
            return rank_body(home, svlen_thres, suppread_thres, thread, all_ctgs, max_dist, rank, world, host_compute(ctx, texts),
                             star=star, gather=gather, write_sv_calls=write_sv_calls, format_rows=device_format_rows(ctx))
        finally:
            if gather is not None:
                gather.close()
            star.close()
    import torch
    import torch.distributed as td
    from duet_amd import _lib
    if rank == 0:
        from duet_amd.utils import add_stream_logging
        add_stream_logging(home)
    torch.cuda.set_device(device_id)
    limit = datetime.timedelta(seconds=float(os.environ.get('DUET_RDZV_TIMEOUT', '300')))
    if one_gpu:
        td.init_process_group('gloo', rank=rank, world_size=world, timeout=limit)
    else:
        td.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device('cuda', device_id), timeout=limit)
    try:
        ctx = _lib.Context(device_id)                    # raises when libduet_ef.so / the GPU is missing: no fallback
        return rank_body(home, svlen_thres, suppread_thres, thread, all_ctgs, max_dist, rank, world, device_compute(ctx, texts),
                         to_device=None if one_gpu else torch.device('cuda', device_id), write_sv_calls=write_sv_calls,
                         format_rows=device_format_rows(ctx))
    finally:
        td.destroy_process_group()


def sv_phasing_from_bams(home, svlen_thres, suppread_thres, thread, include_all_ctgs, cluster_max_distance=0.9, device=0,
                         gpus=1, write_sv_calls=False, thresholds=None, pc_cap=None, evidence=False, ps_links=False, read_tags=False,
                         join_ps=False, join_min_sv=2, vote_sv_tags=False, sv_tag_min=None, sv_tag_pc=None):
    """`duet ... -b svim-gpu -c <max distance>`: SV calling (signatures + clustering, what `-b svim` delegates to the
    external `svim alignment ... --cluster_max_distance c`, sv_calling.py:13-15) AND SV phasing on the GPU, from the
    haplotagged BAMs of <home>/snp_phasing -> <home>/phased_sv.vcf.  The clustering half is this repository's own rule
    (parity unpinned); step E/F is the pinned one.
    write_sv_calls (--write_sv_calls): also every clustered candidate -> <home>/sv_calling/variants.vcf;
    the marks' read names are extracted and checked first, and no file is written before they pass.
    thresholds (--thresholds): a vector of the decision's 14 constants (duet_amd/tune.py: vector) in place of the built-in ones;
    single-GPU path only.
    pc_cap (--pc_cap): the PC cap of the vote in place of 8100, on the same route (without thresholds the vector is the defaults);
    the clustered calls of --write_sv_calls do not depend on it.
    evidence (--write_evidence): also <home>/phased_sv.evidence.tsv, one row per clustered candidate with its vote, the rule of the
    tree it ended at and the call, formatted on the device; the route of thresholds (without one the vector is the defaults).
    ps_links (--write_ps_links): also <home>/phased_sv.ps_links.tsv and <home>/phased_sv.ps_blocks.tsv, how the clustered candidates
    tie neighbouring phase sets together (duet_amd/ps_links.py); single-GPU path only, whichever route the decision takes.
    read_tags (--write_read_tags): also <home>/phased_sv.read_tags.tsv, the haplotype the heterozygous calls place each supporting
    read on (duet_amd/read_tags.py), from the resident cluster result and calls; single-GPU path only.
    join_ps, join_min_sv (--join_ps [--join_min_sv N]): also the same pipeline again on the read tags remapped over the phase sets
    that the links of at least N candidates tie into one block -> <home>/phased_sv.joined.vcf, with
    <home>/phased_sv.join_blocks.tsv and <home>/phased_sv.join_report.tsv (duet_amd/ps_join.py); single-GPU path only, by the
    route the other keywords give the decision.  phased_sv.vcf is written first and in full.
    vote_sv_tags, sv_tag_min, sv_tag_pc (--vote_sv_tags [--sv_tag_min N] [--sv_tag_pc P]): also the same pipeline again with the
    untagged reads voting by the haplotype the other heterozygous calls give them -> <home>/phased_sv.sv_tags.vcf with
    <home>/phased_sv.sv_tags_report.tsv (duet_amd/sv_tags.py); single-GPU path only, not together with join_ps, by the route the
    other keywords give the decision.  phased_sv.vcf is written first and in full."""
    from duet_amd import sv_tags as sv_tags_mod
    sv_tags = sv_tags_mod.check_settings(vote_sv_tags, sv_tag_min, sv_tag_pc, gpus=gpus, join_ps=join_ps)
    if join_ps:
        from duet_amd import ps_join
        if int(gpus) > 1 or os.environ.get('DUET_FORCE_RANKS') == '1':
            raise ValueError('join_ps: single-GPU path only')
        join_min_sv = ps_join.check_min_sv(join_min_sv)
    else:
        join_min_sv = None
    if read_tags and (int(gpus) > 1 or os.environ.get('DUET_FORCE_RANKS') == '1'):
        raise ValueError('read_tags: single-GPU path only')
    if ps_links and (int(gpus) > 1 or os.environ.get('DUET_FORCE_RANKS') == '1'):
        raise ValueError('ps_links: single-GPU path only')
    if evidence:
        from duet_amd import tune
        if int(gpus) > 1 or os.environ.get('DUET_FORCE_RANKS') == '1':
            raise ValueError('evidence: single-GPU path only')
        if thresholds is None:
            thresholds = tune.vector()
    if pc_cap is not None:
        from duet_amd import _lib, tune
        pc_cap = _lib.check_pc_cap(pc_cap)
        if int(gpus) > 1 or os.environ.get('DUET_FORCE_RANKS') == '1':
            raise ValueError('pc_cap: single-GPU path only')
        if thresholds is None:
            thresholds = tune.vector()
    if thresholds is not None and (int(gpus) > 1 or os.environ.get('DUET_FORCE_RANKS') == '1'):
        raise ValueError('thresholds: single-GPU path only')
    bar = '*' * 25
    logging.info('%s SV CALLING + PHASING (GPU, svim-gpu) STARTED %s' % (bar, bar))
    t0 = time.time()
    chroms = init_chrom_list(include_all_ctgs, home)
    out_vcf = home + '/phased_sv.vcf'
    if not write_sv_calls:
        logging.info('create output .vcf file')
        with open(out_vcf, 'w') as out:
            out.write(header_text(home, chroms))
    if thresholds is not None:
        from duet_amd import tune
        logging.info('  thresholds: ' + ', '.join('%s=%r' % (n, float(v)) for n, v in zip(tune.NAMES, thresholds)))
    if pc_cap is not None:
        logging.info('  pc_cap: %d' % pc_cap)
    logging.info('extract SNP and SV signatures from the haplotagged alignments')
    if int(gpus) > 1 or os.environ.get('DUET_FORCE_RANKS') == '1':       # (see sv_phasing.py)
        from duet_amd import launch
        argv = ['-m', 'duet_amd.svim_mode', home, str(int(svlen_thres)), str(int(suppread_thres)), str(int(thread)),
                '1' if include_all_ctgs else '0', repr(float(cluster_max_distance))] + (['1'] if write_sv_calls else [])
        env = {'PYTHONPATH': os.pathsep.join([os.path.dirname(os.path.dirname(os.path.abspath(__file__)))] +
                                             ([os.environ['PYTHONPATH']] if os.environ.get('PYTHONPATH') else []))}
        for h in logging.getLogger().handlers:
            h.flush()
        if any(isinstance(h, logging.FileHandler) for h in logging.getLogger().handlers):
            env['DUET_RANK_LOG'] = '1'
        rc = launch.spawn_ranks(int(gpus), argv, extra_env=env, timeout=float(os.environ.get('DUET_RANK_TIMEOUT', '3600')))
        if rc == 5:
            raise ZeroDivisionError('division by zero')
        if rc == 6:
            raise ReadNameError('svim-gpu on %d GPUs: a read name contains "," or ";" and cannot be listed in READS= of '
                             'sv_calling/variants.vcf (the rank that found it logged its name)' % int(gpus))
        if rc == 124:
            raise RuntimeError('svim-gpu on %d GPUs: the ranks did not finish within DUET_RANK_TIMEOUT; they were killed' % int(gpus))
        if rc:
            raise RuntimeError('svim-gpu on %d GPUs failed: a rank exited with code %d' % (int(gpus), rc))
        logging.info('%s SV CALLING + PHASING COMPLETED IN %ss %s' % (bar, round(time.time() - t0, 3), bar))
        return
    # (--write_sv_calls: the names are checked inside, before the device runs and before any file is written)
    ctx = None if write_sv_calls else engine.default_context(int(device))

    def compute(*args):
        texts = spelled_contigs(home, chroms)
        return device_compute(ctx if ctx is not None else engine.default_context(int(device)), texts if write_sv_calls else None,
                              row_texts=texts, thresholds=thresholds, pc_cap=pc_cap, evidence_texts=texts if evidence else None,
                              ps_links=bool(ps_links), read_tag_texts=texts if read_tags else None, join_min_sv=join_min_sv,
                              sv_tags=sv_tags)(*args)
    res = phase_from_bams(home, svlen_thres, suppread_thres, thread, include_all_ctgs, max_dist=cluster_max_distance,
                          min_sv_size=max(int(svlen_thres), 1), names=bool(write_sv_calls), compute=compute,
                          keep_names=bool(read_tags) or sv_tags is not None)
    # the data rows come sorted and formatted from the device; without a single mark nothing ran and there are none
    if 'rows' not in res and len(res['pred']):
        raise RuntimeError('svim-gpu: the device pipeline returned candidates without the rows of phased_sv.vcf')
    rows, n_rows = res.get('rows', b''), int(res.get('n_rows', 0))
    logging.info('  %d SV marks clustered into %d candidates, %d phased (clustering rule: parity unpinned)' % (
        res['n_marks'], len(res['pred']), n_rows))
    logging.info('write phased callset into .vcf file')
    if evidence:
        from duet_amd import _lib
        from duet_amd.sv_phasing import evidence_path
        with open(evidence_path(home), 'wb') as out:       # (without a single mark nothing ran: the header line alone)
            out.write(_lib.evidence_header())
            out.write(bytes(memoryview(np.ascontiguousarray(res.get('evidence', np.zeros(0, dtype=np.uint8))))))
    if ps_links:
        from duet_amd import ps_links as links_mod
        from duet_amd.sv_phasing import write_ps_links       # (without a single mark nothing ran: the header lines alone)
        write_ps_links(home, (res.get('ps_links', links_mod.empty()), spelled_contigs(home, chroms)))
    if read_tags:
        from duet_amd import read_tags as tags_mod
        from duet_amd.sv_phasing import write_read_tags      # (without a single mark nothing ran: the header line alone)
        recs, text = res.get('read_tags', (tags_mod.empty(), np.zeros(0, dtype=np.uint8)))
        write_read_tags(home, (recs, bytes(memoryview(np.ascontiguousarray(text)))))
    if write_sv_calls:
        with open(out_vcf, 'wb') as out:
            out.write(header_text(home, chroms).encode())
            out.write(rows)
        logging.info('write the clustered SV calls into sv_calling/variants.vcf')
        write_callset(home, chroms, res['calls'])
    else:
        with open(out_vcf, 'ab') as out:
            out.write(rows)
    if join_min_sv is not None:
        write_join(home, chroms, res, join_min_sv)
    if sv_tags is not None:
        write_sv_tags(home, chroms, res, sv_tags)
    logging.info('%s SV CALLING + PHASING COMPLETED IN %ss %s' % (bar, round(time.time() - t0, 3), bar))


def write_sv_tags(home, chroms, res, settings):
    """The two files of --vote_sv_tags from the result's `sv_tags` (device_compute), after phased_sv.vcf has been written in full.
    phased_sv.sv_tags.vcf is created with its header first: where the second run raised ZeroDivisionError it stays header-only, no
    report is written and the error is raised here.  Without a single mark nothing ran: the header lines alone."""
    from duet_amd import sv_tags
    logging.info('phase the SVs again with the tags of the other SVs (--vote_sv_tags, at least %d votes, PC %d)' % settings)
    texts = spelled_contigs(home, chroms)
    second = res.get('sv_tags', dict())
    with open(sv_tags.path_vcf(home), 'w') as out:
        out.write(header_text(home, chroms))
    if 'error' in second:
        raise second['error']
    with open(sv_tags.path_vcf(home), 'ab') as out:
        out.write(bytes(memoryview(np.ascontiguousarray(second.get('rows', np.zeros(0, dtype=np.uint8))))))
    report = ''
    if 'change' in second:
        report = sv_tags.report_text(texts, res['cand_contig'], res['cand_pos'], res['cand_span'], second['change'], res['pred'],
                                     res['ps'], second['pred'], second['ps'])
    sv_tags.write_report(home, report)
    logging.info('  ' + sv_tags.summary_text(second.get('marks', (0, 0, 0)), second.get('counts', np.zeros(8, dtype=np.uint32))))


def write_join(home, chroms, res, min_sv):
    """The three files of --join_ps from the result's `join` (device_compute), after phased_sv.vcf has been written in full.
    phased_sv.joined.vcf is created with its header first: where the joined run raised ZeroDivisionError it stays header-only, no
    report is written and the error is raised here.  Without a single mark nothing ran: the header lines alone."""
    from duet_amd import ps_join
    logging.info('phase the SVs again over the joined phase sets (--join_ps, links of at least %d SVs)' % min_sv)
    texts = spelled_contigs(home, chroms)
    join = res.get('join', dict(blocks=[]))
    with open(ps_join.path_vcf(home), 'w') as out:
        out.write(header_text(home, chroms))
    ps_join.write_blocks(home, join['blocks'], texts)
    if 'error' in join:
        raise join['error']
    with open(ps_join.path_vcf(home), 'ab') as out:
        out.write(bytes(memoryview(np.ascontiguousarray(join.get('rows', np.zeros(0, dtype=np.uint8))))))
    report = ''
    if 'change' in join:
        report = ps_join.report_text(texts, res['cand_contig'], res['cand_pos'], res['cand_span'], join['change'], res['pred'],
                                     res['ps'], join['pred'], join['ps'])
    ps_join.write_report(home, report)
    logging.info('  ' + ps_join.summary_text(join.get('counts', np.zeros(8, dtype=np.uint32)), join.get('n_changed', 0),
                                             len(join['blocks'])))


if __name__ == '__main__':
    import sys
    sys.exit(rank_main(sys.argv[1:]))
