# coding=utf-8
"""Stage driver of step E/F (mirror of src/duet/sv_phasing.py:8-20): same paths, same log lines.

Two host paths feed the same HIP kernels:
  * native  -- libduet_ingest.so tokenises the VCF, reads the BAM tags and formats the rows (C++);
  * python  -- duet_amd/read_file.py + sv_phasing_fn.py + write_file.py, which mirror upstream's Python
               including its exceptions.
The native path declines anything it does not vouch for (non-ASCII bytes, malformed numbers, missing
fields ...) and the Python path then takes over, so the observable behaviour is upstream's either way.
Set DUET_NATIVE_INGEST=0 to force the Python path; DUET_DEVICE_ROWS=0 keeps the native path but formats the rows on
the host instead of on the device.

Twelve additive keyword arguments (upstream's five positionals are unchanged): `vote_sv_tags`, `sv_tag_min`, `sv_tag_pc` = also
phase the SVs again with the untagged reads voting by the haplotype the other heterozygous calls give them, into
<home>/phased_sv.sv_tags.vcf with <home>/phased_sv.sv_tags_report.tsv (duet_amd/sv_tags.py; single-GPU native path, by the route
the other keywords give the decision; not together with `join_ps`), `join_ps`, `join_min_sv` = also phase the SVs again
over the phase sets that the links of at least join_min_sv candidates tie into one block, into <home>/phased_sv.joined.vcf, with
<home>/phased_sv.join_blocks.tsv and <home>/phased_sv.join_report.tsv (duet_amd/ps_join.py; single-GPU native path, by the route
the other keywords give the decision), `read_tags` = also write
<home>/phased_sv.read_tags.tsv, the haplotype the heterozygous calls place each of their supporting reads on, per read and phase
set (duet_amd/read_tags.py; single-GPU native path, with or without `thresholds`; under `pc_cap` a read's own tag is usable under
that cap), `ps_links` = also write
<home>/phased_sv.ps_links.tsv and <home>/phased_sv.ps_blocks.tsv, how the SV candidates tie neighbouring phase sets together
(duet_amd/ps_links.py; single-GPU native path, with or without `thresholds`; under `pc_cap` the voters are that cap's),
`evidence` = also write
<home>/phased_sv.evidence.tsv, one row per candidate with its vote, the rule of the tree it ended at and the call (the route of
`thresholds`, with the default vector where none is given), `thresholds` = a vector of the decision's
T1-T5 constants (duet_amd/tune.py; native single-GPU path only), `pc_cap` = the PC cap of the vote in place of 8100 (the same
path; without `thresholds` the vector is the defaults), `device` = HIP device index of a
single-GPU run, `gpus` = N > 1 shards the contigs over N GPUs of the node, one process per GPU
(duet_amd/multi.py: longest-processing-time-first on mark counts, the three kernels per rank, ONE all-gather of the
(pred, ps) records over RCCL, rank 0 writes phased_sv.vcf).
"""

import logging
import os
import time

from duet_amd import engine
from duet_amd.read_file import init_chrom_list
from duet_amd.sv_phasing_fn import generate_phased_callset
from duet_amd.write_file import print_sv, print_sv_header

_BAR = '*' * 25


def load_native(home, thread, include_all_ctgs, caller_vcf, log=True, names=False):
    """Native ingest of <home> -> (NativeIngest, chrom_list) or (None, chrom_list) when the Python path has to take
    over (library missing, input declined, or switched off).  names: the join keeps every mark's read name (--write_read_tags)."""
    chrom_list = init_chrom_list(include_all_ctgs, home)
    if os.environ.get('DUET_NATIVE_INGEST') == '0' or os.environ.get('DUET_USE_SAMTOOLS') == '1':
        return None, chrom_list
    from duet_amd.native import NativeIngest
    ing = NativeIngest.load(caller_vcf, home + '/snp_phasing/', chrom_list, thread, names=names)
    if ing is None:
        return None, chrom_list
    if ing.handle is None:
        if log:
            logging.info('native ingest declined (%s); using the Python path' % ing.why)
        return None, chrom_list
    return ing, chrom_list


def log_ingest(ing, chrom_list):
    """Upstream's log lines for the two ingest steps (sv_phasing_fn.py:12,30-33,37,41-45)."""
    snp, sv = ing.log_lines(chrom_list)
    logging.info('extract SNP signatures')
    for line in snp:
        logging.info(line)
    logging.info('extract SV signatures')
    for line in sv:
        logging.info(line)


def write_header(ing, include_all_ctgs, out_vcf):
    """Upstream creates the output file with its header BEFORE any candidate is evaluated (sv_phasing.py:16), so a
    later exception (e.g. ZeroDivisionError, sv_phasing_fn.py:123) leaves a header-only file; so does this."""
    with open(out_vcf, 'wb') as out:
        out.write(ing.header(include_all_ctgs))


def contig_texts(ing, chrom_list, flag='--write_ps_links'):
    """The CHROM text the rows of phased_sv.vcf carry for every contig: that of the contig's first candidate in the ingest's
    string pool (a contig without candidates: its name in the chrom list -- no row carries it)."""
    texts = list(chrom_list)
    if ing.soa.n_cands:
        rows = ing.rows()
        if rows is None:
            raise RuntimeError('%s: the native ingest has no string pool for this input' % flag)
        pool, off, ctg = rows['pool'], rows['str_off'], ing.soa.cand_ctg_off
        for k in range(ing.soa.n_contigs):
            if ctg[k + 1] > ctg[k]:
                c = int(ctg[k])
                texts[k] = pool[int(off[4 * c]):int(off[4 * c + 1])].tobytes().decode('utf-8', 'replace')
    return texts


def native_ps_links(ing, chrom_list, svlen_thres, suppread_thres, ctx, pc_cap=None):
    """(records, CHROM text per contig) of the ingest's problem (duet_ps_links_host), while the ingest is still open."""
    from duet_amd import ps_links
    texts = contig_texts(ing, chrom_list)
    records = ctx.ps_links_host(ing.soa, svlen_thres, suppread_thres, pc_cap=pc_cap) if ing.soa.n_cands else ps_links.empty()
    return records, texts


def write_ps_links(home, links):
    from duet_amd import ps_links
    logging.info('write the phase-set links into phased_sv.ps_links.tsv and phased_sv.ps_blocks.tsv')
    n, n_ps, n_conflicts = ps_links.write(home, *links)
    logging.info('  %d links over %d phase sets, %d contradicted' % (n, n_ps, n_conflicts))


def native_read_tags(ing, chrom_list, pred, ps, ctx, pc_cap=None):
    """(records, data rows as bytes) of phased_sv.read_tags.tsv for the ingest's problem and its calls (duet_read_tags_host,
    duet_read_tags_rows_host), while the ingest is still open."""
    from duet_amd import read_tags
    soa = ing.soa
    if not soa.n_cands or not soa.n_marks:
        return read_tags.empty(), b''
    nm, texts = ing.mark_names(), contig_texts(ing, chrom_list, '--write_read_tags')
    records = ctx.read_tags_host(soa.cand_off, soa.mark_read, nm['mark_name'], len(nm['name_off']) - 1, pred, ps, soa.cand_pos,
                                 soa.read_tag, cand_ctg_off=soa.cand_ctg_off, pc_cap=pc_cap)
    return records, ctx.read_tags_rows_host(records, nm['name_off'], nm['name_pool'], texts, soa.read_tag)


def write_read_tags(home, tags):
    from duet_amd import read_tags
    logging.info('write the read tags into phased_sv.read_tags.tsv')
    read_tags.write(home, tags[1])
    logging.info('  ' + read_tags.summary_text(tags[0]))


def native_join(home, ing, chrom_list, include_all_ctgs, svlen_thres, suppread_thres, ctx, min_sv, run, pc_cap=None):
    """--join_ps on the ingest's problem, while the ingest is still open and after phased_sv.vcf has been written in full: the
    links' blocks (duet_amd/ps_links.py: blocks, min_sv), the read tags under them (duet_ps_join_tags_host), `run` -- soa ->
    (pred, ps), the route the first run took -- on both tag tables, the change codes (duet_ps_join_diff_host), the three files.
    phased_sv.joined.vcf is created with its header before the joined run: a ZeroDivisionError there leaves it header-only, with no
    report beside it."""
    from duet_amd import ps_join, ps_links as links_mod
    import numpy as np
    soa = ing.soa
    texts = contig_texts(ing, chrom_list, '--join_ps')
    logging.info('phase the SVs again over the joined phase sets (--join_ps, links of at least %d SVs)' % min_sv)
    with open(ps_join.path_vcf(home), 'wb') as out:
        out.write(ing.header(include_all_ctgs))
    records = ctx.ps_links_host(soa, svlen_thres, suppread_thres, pc_cap=pc_cap) if soa.n_cands else links_mod.empty()
    rows, _ = links_mod.blocks(records, min_sv=min_sv)
    ps_join.write_blocks(home, rows, texts)
    table = ps_join.table(rows)
    body, report, n_changed = b'', '', 0
    counts = np.zeros(8, dtype=np.uint32)
    if soa.n_cands:
        pred0, ps0 = run(soa)
        tags, n_changed = ctx.ps_join_tags_host(soa.read_tag, soa.read_off, table)
        kw = {name: getattr(soa, name) for name, _ in engine.EfSoA.FIELDS}
        kw['read_tag'] = tags
        pred1, ps1 = run(engine.EfSoA(read_off=soa.read_off, **kw))
        change, counts = ctx.ps_join_diff_host(pred0, ps0, pred1, ps1, table, soa.n_contigs, cand_ctg_off=soa.cand_ctg_off)
        body = ing.emit_rows(pred1, ps1)
        contig = np.repeat(np.arange(soa.n_contigs), np.diff(soa.cand_ctg_off.astype(np.int64)))
        report = ps_join.report_text(texts, contig, soa.cand_pos, soa.cand_svlen, change, pred0, ps0, pred1, ps1)
    with open(ps_join.path_vcf(home), 'ab') as out:
        out.write(body)
    ps_join.write_report(home, report)
    logging.info('  ' + ps_join.summary_text(counts, n_changed, len(rows)))


def native_sv_tags(home, ing, chrom_list, include_all_ctgs, ctx, settings, run, pc_cap=None, first=None):
    """--vote_sv_tags on the ingest's problem, while the ingest is still open and after phased_sv.vcf has been written in full:
    the first run's calls -- `first` = (pred, ps) where the caller has them, else `run`, soa -> (pred, ps), the route the first run
    took (the fused rows entry keeps its calls on the device) --, one tag word per mark from those calls
    (duet_sv_tags_host; settings = (min_votes, pc_new)), `run` again on the expanded problem (read_tag = the words, mark_read = the
    identity), the change codes (duet_ps_join_diff_host under an empty table), the two files.  phased_sv.sv_tags.vcf is created
    with its header before the second run: a ZeroDivisionError there leaves it header-only, with no report beside it."""
    from duet_amd import _lib, sv_tags
    import numpy as np
    soa = ing.soa
    texts = contig_texts(ing, chrom_list, '--vote_sv_tags')
    logging.info('phase the SVs again with the tags of the other SVs (--vote_sv_tags, at least %d votes, PC %d)' % settings)
    with open(sv_tags.path_vcf(home), 'wb') as out:
        out.write(ing.header(include_all_ctgs))
    body, report, marks = b'', '', (0, 0, 0)
    counts = np.zeros(8, dtype=np.uint32)
    if soa.n_cands:
        pred0, ps0 = first if first is not None else run(soa)
        nm = ing.mark_names()
        tags, index, marks = ctx.sv_tags_host(soa.cand_off, soa.mark_read, nm['mark_name'], len(nm['name_off']) - 1, pred0, ps0,
                                              soa.read_tag, cand_ctg_off=soa.cand_ctg_off, pc_cap=pc_cap, min_votes=settings[0],
                                              pc_new=settings[1])
        kw = {name: getattr(soa, name) for name, _ in engine.EfSoA.FIELDS}
        kw['read_tag'], kw['mark_read'] = tags, index
        # (a mark is its own read now: the "reads" of contig k are the marks of its candidates)
        pred1, ps1 = run(engine.EfSoA(read_off=soa.cand_off[soa.cand_ctg_off], **kw))
        change, counts = ctx.ps_join_diff_host(pred0, ps0, pred1, ps1, np.zeros(0, dtype=_lib.PS_BLOCK_DTYPE), soa.n_contigs,
                                               cand_ctg_off=soa.cand_ctg_off)
        body = ing.emit_rows(pred1, ps1)
        contig = np.repeat(np.arange(soa.n_contigs), np.diff(soa.cand_ctg_off.astype(np.int64)))
        report = sv_tags.report_text(texts, contig, soa.cand_pos, soa.cand_svlen, change, pred0, ps0, pred1, ps1)
    with open(sv_tags.path_vcf(home), 'ab') as out:
        out.write(body)
    sv_tags.write_report(home, report)
    logging.info('  ' + sv_tags.summary_text(marks, counts))


def _native(home, svlen_thres, suppread_thres, thread, include_all_ctgs, caller_vcf, out_vcf, ctx, ps_links=False, read_tags=False,
            join_min_sv=None, sv_tags=None):
    ing, chrom_list = load_native(home, thread, include_all_ctgs, caller_vcf, names=read_tags or sv_tags is not None)
    if ing is None:
        if sv_tags is not None:
            raise RuntimeError('--vote_sv_tags needs the native ingest, which declined this input (or DUET_NATIVE_INGEST=0)')
        if join_min_sv is not None:
            raise RuntimeError('--join_ps needs the native ingest, which declined this input (or DUET_NATIVE_INGEST=0)')
        if read_tags:
            raise RuntimeError('--write_read_tags needs the native ingest, which declined this input (or DUET_NATIVE_INGEST=0)')
        if ps_links:
            raise RuntimeError('--write_ps_links needs the native ingest, which declined this input (or DUET_NATIVE_INGEST=0)')
        return False
    links, tags = None, None
    try:
        if ps_links:
            contig_texts(ing, chrom_list)           # (before the output file is created: a refusal leaves nothing behind)
        if read_tags:
            contig_texts(ing, chrom_list, '--write_read_tags')
        if join_min_sv is not None:
            contig_texts(ing, chrom_list, '--join_ps')
        if sv_tags is not None:
            contig_texts(ing, chrom_list, '--vote_sv_tags')
        write_header(ing, include_all_ctgs, out_vcf)
        log_ingest(ing, chrom_list)
        logging.info('integrate read weight information')
        logging.info('calculate read weight statistics')
        logging.info('predict SV haplotypes in the callset')
        rows = None if os.environ.get('DUET_DEVICE_ROWS') == '0' else ing.rows()
        calls = None                                # (the first run's (pred, ps), where they came back to the host)
        if rows is not None and ing.soa.n_cands:
            # (pred, ps) stay on the device; it also orders and formats the rows (duet_ef_rows_run_host)
            body = ctx.ef_rows_host(ing.soa, rows, svlen_thres, suppread_thres)[0]
        else:
            pred, ps = calls = engine.run_ef(ing.soa, svlen_thres, suppread_thres, ctx=ctx)
            body = ing.emit_rows(pred, ps)
        if ps_links:
            links = native_ps_links(ing, chrom_list, svlen_thres, suppread_thres, ctx)
        if read_tags:
            # (the rows above keep their route, so phased_sv.vcf is what it is without the flag; the calls themselves come from
            # one more E/F run on the same problem)
            pred, ps = engine.run_ef(ing.soa, svlen_thres, suppread_thres, ctx=ctx) if ing.soa.n_cands else ((), ())
            calls = (pred, ps) if ing.soa.n_cands else calls
            tags = native_read_tags(ing, chrom_list, pred, ps, ctx)
        logging.info('write phased callset into .vcf file')
        if join_min_sv is not None:
            # (phased_sv.vcf first and in full: whatever the joined run does, it is what it is without the flag)
            with open(out_vcf, 'ab') as out:
                out.write(body)
            body = b''
            native_join(home, ing, chrom_list, include_all_ctgs, svlen_thres, suppread_thres, ctx, join_min_sv,
                        lambda soa: engine.run_ef(soa, svlen_thres, suppread_thres, ctx=ctx))
        if sv_tags is not None:
            # (phased_sv.vcf first and in full: whatever the second run does, it is what it is without the flag)
            with open(out_vcf, 'ab') as out:
                out.write(body)
            body = b''
            native_sv_tags(home, ing, chrom_list, include_all_ctgs, ctx, sv_tags,
                           lambda soa: engine.run_ef(soa, svlen_thres, suppread_thres, ctx=ctx), first=calls)
    except BaseException:
        ing.close()
        raise
    ing.close_in_background()                       # (the rows are out: freeing the ingest's memory needs nobody's attention)
    with open(out_vcf, 'ab') as out:
        out.write(body)
    if links is not None:
        write_ps_links(home, links)
    if tags is not None:
        write_read_tags(home, tags)
    return True


def evidence_path(home):
    return home + '/phased_sv.evidence.tsv'


def _native_thresholds(home, svlen_thres, suppread_thres, thread, include_all_ctgs, caller_vcf, out_vcf, ctx, vec, pc_cap=None,
                       evidence=False, ps_links=False, read_tags=False, join_min_sv=None, sv_tags=None):
    """The native path with the decision's constants taken from `vec` (duet_amd/tune.py): ingest, the feature export (pc_cap:
    under that PC cap, duet_ef_features_cap_host), a sweep of one vector that keeps its (pred, ps), the rows.
    evidence: also <home>/phased_sv.evidence.tsv, one row per candidate formatted on the device (duet_evidence_rows_host, the text
    form over the ingest's string pool).  ps_links: also the two phase-set link tables, the voters under the same PC cap.
    read_tags: also <home>/phased_sv.read_tags.tsv from this route's (pred, ps), a read's own tag usable under the same PC cap.
    join_min_sv (not None: --join_ps): also the run over the joined phase sets, by this route again (native_join).
    sv_tags (not None: --vote_sv_tags, (min_votes, pc_new)): also the run with the tags of the other SVs, by this route again
    (native_sv_tags)."""
    from duet_amd import _lib, tune
    ing, chrom_list = load_native(home, thread, include_all_ctgs, caller_vcf, names=read_tags or sv_tags is not None)
    if ing is None:
        raise RuntimeError('--thresholds / --pc_cap / --write_evidence%s need the native ingest, which declined this input '
                           '(or DUET_NATIVE_INGEST=0)' % ((' / --write_ps_links' if ps_links else '') +
                                                          (' / --write_read_tags' if read_tags else '') +
                                                          (' / --join_ps' if join_min_sv is not None else '') +
                                                          (' / --vote_sv_tags' if sv_tags is not None else '')))
    table, links, tags = None, None, None
    try:
        rows = None
        if ps_links:
            contig_texts(ing, chrom_list)           # (before the output file is created: a refusal leaves nothing behind)
        if read_tags:
            contig_texts(ing, chrom_list, '--write_read_tags')
        if join_min_sv is not None:
            contig_texts(ing, chrom_list, '--join_ps')
        if sv_tags is not None:
            contig_texts(ing, chrom_list, '--vote_sv_tags')
        if evidence and ing.soa.n_cands:
            rows = ing.rows()                       # (before the output file is created: a refusal leaves nothing behind)
            if rows is None:
                raise RuntimeError('--write_evidence: the native ingest has no string pool for this input')
        write_header(ing, include_all_ctgs, out_vcf)
        log_ingest(ing, chrom_list)
        logging.info('integrate read weight information')
        logging.info('calculate read weight statistics')
        logging.info('predict SV haplotypes in the callset')
        logging.info('  thresholds: ' + ', '.join('%s=%r' % (n, float(v)) for n, v in zip(tune.NAMES, vec)))
        if pc_cap is not None:
            logging.info('  pc_cap: %d' % pc_cap)
        body = b''
        if ing.soa.n_cands:
            feat = ctx.features_host(ing.soa, svlen_thres, suppread_thres, pc_cap=pc_cap)
            pred, ps = tune.apply(dict(feat=feat), vec, ctx=ctx)
            body = ing.emit_rows(pred, ps)
        if evidence:
            table = b''
            if ing.soa.n_cands:
                leaf, _ = tune.explain(dict(feat=feat), vec, ctx=ctx)
                table = ctx.evidence_rows_host(feat, leaf, pred, ing.soa.cand_pos, ing.soa.cand_svlen, rows=rows)
        if ps_links:
            links = native_ps_links(ing, chrom_list, svlen_thres, suppread_thres, ctx, pc_cap=pc_cap)
        if read_tags:
            tags = native_read_tags(ing, chrom_list, pred, ps, ctx, pc_cap=pc_cap) if ing.soa.n_cands else \
                native_read_tags(ing, chrom_list, (), (), ctx)
        logging.info('write phased callset into .vcf file')
        if join_min_sv is not None:
            # (phased_sv.vcf first and in full: whatever the joined run does, it is what it is without the flag)
            with open(out_vcf, 'ab') as out:
                out.write(body)
            body = b''
            native_join(home, ing, chrom_list, include_all_ctgs, svlen_thres, suppread_thres, ctx, join_min_sv,
                        lambda soa: tune.apply(dict(feat=ctx.features_host(soa, svlen_thres, suppread_thres, pc_cap=pc_cap)), vec,
                                               ctx=ctx), pc_cap=pc_cap)
        if sv_tags is not None:
            # (phased_sv.vcf first and in full: whatever the second run does, it is what it is without the flag)
            with open(out_vcf, 'ab') as out:
                out.write(body)
            body = b''
            native_sv_tags(home, ing, chrom_list, include_all_ctgs, ctx, sv_tags,
                           lambda soa: tune.apply(dict(feat=ctx.features_host(soa, svlen_thres, suppread_thres, pc_cap=pc_cap)), vec,
                                                  ctx=ctx), pc_cap=pc_cap, first=(pred, ps) if ing.soa.n_cands else None)
    finally:
        ing.close()
    with open(out_vcf, 'ab') as out:
        out.write(body)
    if table is not None:
        logging.info('write the evidence table into phased_sv.evidence.tsv')
        with open(evidence_path(home), 'wb') as out:
            out.write(_lib.evidence_header())
            out.write(table)
    if links is not None:
        write_ps_links(home, links)
    if tags is not None:
        write_read_tags(home, tags)


def sv_phasing(home, svlen_thres, suppread_thres, thread, include_all_ctgs, device=0, gpus=1, thresholds=None, pc_cap=None,
               evidence=False, ps_links=False, read_tags=False, join_ps=False, join_min_sv=2, vote_sv_tags=False, sv_tag_min=None,
               sv_tag_pc=None):
    # (additive: the second run with the tags of the other SVs -- the native single-GPU path, whichever route the decision takes;
    # refused before anything is opened)
    from duet_amd import sv_tags as sv_tags_mod
    sv_tags = sv_tags_mod.check_settings(vote_sv_tags, sv_tag_min, sv_tag_pc, gpus=gpus, join_ps=join_ps)
    if join_ps:
        # (additive: the run over the joined phase sets -- the native single-GPU path, whichever route the decision takes)
        from duet_amd import ps_join
        if int(gpus) > 1 or os.environ.get('DUET_FORCE_RANKS') == '1':
            raise ValueError('join_ps: single-GPU path only')
        join_min_sv = ps_join.check_min_sv(join_min_sv)
    else:
        join_min_sv = None
    if read_tags and (int(gpus) > 1 or os.environ.get('DUET_FORCE_RANKS') == '1'):
        # (additive: the read tags -- the native single-GPU path, whichever route the decision takes)
        raise ValueError('read_tags: single-GPU path only')
    if ps_links and (int(gpus) > 1 or os.environ.get('DUET_FORCE_RANKS') == '1'):
        # (additive: the phase-set links -- the native single-GPU path, whichever route the decision takes)
        raise ValueError('ps_links: single-GPU path only')
    if evidence:
        # (additive: the evidence table -- the route is that of `thresholds`, with the default vector where none is given)
        from duet_amd import tune
        if int(gpus) > 1 or os.environ.get('DUET_FORCE_RANKS') == '1':
            raise ValueError('evidence: single-GPU path only')
        if thresholds is None:
            thresholds = tune.vector()
    if pc_cap is not None:
        # (additive: the PC cap of the vote -- refused before anything is opened; the route is that of `thresholds`)
        from duet_amd import _lib, tune
        pc_cap = _lib.check_pc_cap(pc_cap)
        if int(gpus) > 1 or os.environ.get('DUET_FORCE_RANKS') == '1':
            raise ValueError('pc_cap: single-GPU path only')
        if thresholds is None:
            thresholds = tune.vector()
    logging.info('%s SV PHASING STARTED %s' % (_BAR, _BAR))
    t0 = time.time()
    caller_vcf = home + '/sv_calling/variants.vcf'
    out_vcf = home + '/phased_sv.vcf'
    logging.info('create output .vcf file')
    done = False
    if thresholds is not None:
        # (additive: T1-T5 constants of the caller's own, duet_amd/tune.py -- single GPU, native ingest only)
        if int(gpus) > 1 or os.environ.get('DUET_FORCE_RANKS') == '1':
            raise ValueError('thresholds: single-GPU path only')
        _native_thresholds(home, svlen_thres, suppread_thres, thread, include_all_ctgs, caller_vcf, out_vcf,
                           engine.default_context(int(device)), thresholds, pc_cap, evidence=bool(evidence), ps_links=bool(ps_links),
                           read_tags=bool(read_tags), join_min_sv=join_min_sv, sv_tags=sv_tags)
        done = True
    # (DUET_FORCE_RANKS=1: the one-process-per-GPU path even with one GPU -- rank 0 of 1 over RCCL; tests use it to take the
    # collective through the real backend on a one-GPU box)
    if not done and (int(gpus) > 1 or os.environ.get('DUET_FORCE_RANKS') == '1'):
        from duet_amd import multi
        done = multi.sv_phasing_sharded(home, svlen_thres, suppread_thres, thread, include_all_ctgs, int(gpus))
    if not done:
        ctx = engine.default_context(int(device))
        if not _native(home, svlen_thres, suppread_thres, thread, include_all_ctgs, caller_vcf, out_vcf, ctx, ps_links=bool(ps_links),
                       read_tags=bool(read_tags), join_min_sv=join_min_sv, sv_tags=sv_tags):
            print_sv_header(caller_vcf, out_vcf, include_all_ctgs)
            rows = generate_phased_callset(caller_vcf, home + '/snp_phasing/', svlen_thres, suppread_thres, thread,
                                           include_all_ctgs, ctx=ctx)
            print_sv(rows, out_vcf)
    logging.info('%s SV PHASING COMPLETED IN %ss %s' % (_BAR, round(time.time() - t0, 3), _BAR))
