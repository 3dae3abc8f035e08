# coding=utf-8
"""The `duet` command: BAM REFERENCE OUTPUT [-t -m -c -s -r -a -b] as upstream (src/duet/duet:14-28), two additive
flags (--device, --gpus).  The pipeline is a table of stages; B, C, D shell out to external tools (duet_amd/stages.py),
the last one -- SV phasing, steps E/F -- runs on the MI355X."""

import logging
import os
import time

from duet_amd import engine, stages
from duet_amd.sv_phasing import sv_phasing
from duet_amd.utils import check_envs, parse_args, set_logging

_BAR = '*' * 25


def pipeline(a):
    """(callable, arguments) per stage, in upstream's fixed order: SNP call, SV call, SNP phase, SV phase.
    `-b svim-gpu` (additive): no external SV caller -- signatures, `--cluster_max_distance` clustering and phasing all run on
    the GPU from the haplotagged BAMs (duet_amd/svim_mode.py)."""
    # (--write_ps_links travels as a keyword: the positional arguments of the last stage stay what they were)
    extra = {'ps_links': True} if getattr(a, 'write_ps_links', False) else {}
    if getattr(a, 'write_read_tags', False):
        extra['read_tags'] = True                           # (--write_read_tags: a keyword too)
    if getattr(a, 'join_ps', False):
        extra['join_ps'] = True                             # (--join_ps [--join_min_sv N]: two keywords)
        extra['join_min_sv'] = 2 if getattr(a, 'join_min_sv', None) is None else a.join_min_sv
    if getattr(a, 'vote_sv_tags', False):
        extra['vote_sv_tags'] = True                        # (--vote_sv_tags [--sv_tag_min N] [--sv_tag_pc P]: three keywords)
        extra['sv_tag_min'], extra['sv_tag_pc'] = getattr(a, 'sv_tag_min', None), getattr(a, 'sv_tag_pc', None)
    if a.sv_caller == 'svim-gpu':
        from duet_amd.svim_mode import sv_phasing_from_bams
        last = (lambda *args: sv_phasing_from_bams(*args, **extra)) if extra else sv_phasing_from_bams
        return (
            (stages.snp_calling, (a.OUTPUT, a.REFERENCE, a.BAM, a.min_allele_frequency, a.thread, a.include_all_ctgs)),
            (stages.snp_phasing, (a.OUTPUT, a.REFERENCE, a.BAM, a.thread)),
            (last, (a.OUTPUT, a.sv_min_size, a.min_support_read, a.thread, a.include_all_ctgs,
                    a.cluster_max_distance, a.device, a.gpus, a.write_sv_calls,
                    getattr(a, 'threshold_vector', None), getattr(a, 'pc_cap_value', None),
                    bool(getattr(a, 'write_evidence', False)))),
        )
    last = (lambda *args: sv_phasing(*args, **extra)) if extra else sv_phasing
    return (
        (stages.snp_calling, (a.OUTPUT, a.REFERENCE, a.BAM, a.min_allele_frequency, a.thread, a.include_all_ctgs)),
        (stages.sv_calling, (a.OUTPUT, a.REFERENCE, a.BAM, a.cluster_max_distance, a.sv_min_size, a.thread, a.sv_caller,
                             a.min_support_read)),
        (stages.snp_phasing, (a.OUTPUT, a.REFERENCE, a.BAM, a.thread)),
        (last, (a.OUTPUT, a.sv_min_size, a.min_support_read, a.thread, a.include_all_ctgs, a.device, a.gpus,
                a.threshold_vector, a.pc_cap_value, bool(getattr(a, 'write_evidence', False)))),
    )


def main(argv):
    a = parse_args(argv)
    a.threshold_vector, a.pc_cap_value, a.join_min_sv_file = None, None, None
    if a.write_sv_calls and a.sv_caller != 'svim-gpu':
        # (additive: the clustered calls exist only in the svim-gpu mode; every other caller writes sv_calling/variants.vcf itself)
        raise SystemExit('duet: --write_sv_calls works with -b svim-gpu only')
    if a.thresholds is not None:
        # (additive: the decision's constants from a file -- checked before any stage runs)
        # (-b svim-gpu on one GPU takes a vector too: one fitted on the BAM path, `tune --from_bams --fit`, is usable on it)
        if a.gpus > 1 or os.environ.get('DUET_FORCE_RANKS') == '1':
            raise SystemExit('duet: --thresholds works on the single-GPU path with an external SV caller only '
                             '(not with --gpus > 1 or -b svim-gpu)')
        from duet_amd import tune
        a.threshold_vector, a.pc_cap_value, a.join_min_sv_file = tune.load_vector(a.thresholds, with_cap=True, with_join=True)
    if a.pc_cap is not None:
        # (additive: the PC cap of the vote, sv_phasing_fn.py:76,88,201 -- the flag wins over a pc_cap key of the thresholds file;
        # without --thresholds the vector is the defaults)
        if a.gpus > 1 or os.environ.get('DUET_FORCE_RANKS') == '1':
            raise SystemExit('duet: --pc_cap works on the single-GPU path only (not with --gpus > 1)')
        a.pc_cap_value = a.pc_cap
    if a.write_evidence:
        # (additive: the evidence table, OUTPUT/phased_sv.evidence.tsv -- it takes the route of --thresholds, with the default
        # vector where none is given, so it is refused where that route is)
        if a.gpus > 1 or os.environ.get('DUET_FORCE_RANKS') == '1':
            raise SystemExit('duet: --write_evidence works on the single-GPU path only (not with --gpus > 1)')
        if a.threshold_vector is None:
            from duet_amd import tune
            a.threshold_vector = tune.vector()
    if a.write_ps_links:
        # (additive: the phase-set link tables, OUTPUT/phased_sv.ps_links.tsv and OUTPUT/phased_sv.ps_blocks.tsv -- built from the
        # problem one GPU holds; the decision keeps whatever route the other flags give it)
        if a.gpus > 1 or os.environ.get('DUET_FORCE_RANKS') == '1':
            raise SystemExit('duet: --write_ps_links works on the single-GPU path only (not with --gpus > 1)')
    if a.write_read_tags:
        # (additive: the per-read table, OUTPUT/phased_sv.read_tags.tsv -- built from the calls and the marks one GPU holds; the
        # decision keeps whatever route the other flags give it)
        if a.gpus > 1 or os.environ.get('DUET_FORCE_RANKS') == '1':
            raise SystemExit('duet: --write_read_tags works on the single-GPU path only (not with --gpus > 1)')
    if a.join_min_sv is not None and not a.join_ps:
        raise SystemExit('duet: --join_min_sv needs --join_ps')
    if a.join_ps:
        # (additive: the second run over the joined phase sets, OUTPUT/phased_sv.joined.vcf with its two tables -- built from the
        # problem one GPU holds; both runs keep whatever route the other flags give the decision)
        if a.gpus > 1 or os.environ.get('DUET_FORCE_RANKS') == '1':
            raise SystemExit('duet: --join_ps works on the single-GPU path only (not with --gpus > 1)')
        if a.join_min_sv is not None and a.join_min_sv < 1:
            raise SystemExit('duet: --join_min_sv takes an integer >= 1')
        if a.join_min_sv is None:
            a.join_min_sv = a.join_min_sv_file              # (a join_min_sv key of the thresholds file, what `tune --fit --join_ps` writes; the flag wins)
    if (a.sv_tag_min is not None or a.sv_tag_pc is not None) and not a.vote_sv_tags:
        raise SystemExit('duet: --sv_tag_min and --sv_tag_pc need --vote_sv_tags')
    if a.vote_sv_tags:
        # (additive: the second run with the tags of the other SVs, OUTPUT/phased_sv.sv_tags.vcf with its report -- built from the
        # problem one GPU holds; both runs keep whatever route the other flags give the decision)
        from duet_amd import sv_tags
        if a.gpus > 1 or os.environ.get('DUET_FORCE_RANKS') == '1':
            raise SystemExit('duet: --vote_sv_tags works on the single-GPU path only (not with --gpus > 1)')
        if a.join_ps:
            raise SystemExit('duet: --vote_sv_tags and --join_ps do not work together')
        if a.sv_tag_min is not None and a.sv_tag_min < 1:
            raise SystemExit('duet: --sv_tag_min takes an integer >= 1')
        if a.sv_tag_pc is not None and not 0 <= a.sv_tag_pc <= sv_tags.PC_LIMIT:
            raise SystemExit('duet: --sv_tag_pc takes an integer in 0 .. %d' % sv_tags.PC_LIMIT)
    check_envs(a.REFERENCE, a.BAM)
    os.makedirs(a.OUTPUT, exist_ok=True)
    set_logging(a.OUTPUT)
    began = time.time()
    logging.info(_BAR + ' DUET STARTED ' + _BAR)
    todo = pipeline(a)
    if a.gpus > 1:
        # N devices and the library, checked in a child BEFORE the external stages run (hours of Clair3 / WhatsHap should
        # not end in "no GPU"); this process stays GPU-free -- it starts the ranks later (duet_amd/launch.py)
        from duet_amd import launch
        launch.probe_devices(1 if os.environ.get('DUET_ONE_GPU') == '1' else a.gpus)
    for fn, args in todo[:-1]:
        fn(*args)
    if a.gpus <= 1 and os.environ.get('DUET_FORCE_RANKS') != '1':
        engine.default_context(a.device)      # fail before the last stage if there is no MI355X / no library
    elif a.gpus <= 1:
        # (DUET_FORCE_RANKS=1: the last stage starts a rank process even for one GPU -- this process must stay GPU-free,
        # so the device is probed in a child)
        from duet_amd import launch
        launch.probe_devices(1)
    fn, args = todo[-1]
    fn(*args)
    logging.info('%s DUET FINISHED IN %ss %s' % (_BAR, round(time.time() - began, 3), _BAR))
    logging.info('OUTPUT .VCF FILE AT ' + a.OUTPUT + '/phased_sv.vcf')
