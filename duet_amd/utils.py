# coding=utf-8
"""Flags, logging and input checks of the `duet` command (mirror of src/duet/utils.py:8-50).

Flag names, defaults, help texts and the positional order are upstream's (utils.py:19-44), so an
existing command line works unchanged.  Two additive options select the device (--device) or shard the contigs
over several GPUs (--gpus); --thresholds and --pc_cap replace the decision's constants on the single-GPU path,
--write_evidence adds the per-candidate evidence table there, --write_ps_links the phase-set link tables, --write_read_tags the
per-read table of the haplotypes the phased SVs place their supporting reads on, --join_ps [--join_min_sv N] a second run over the
phase sets that the SVs tie into one block, --vote_sv_tags [--sv_tag_min N] [--sv_tag_pc P] a second run in which the untagged
reads vote with the haplotype the other SV calls give them.
"""

import argparse
import logging
import os
import sys

_OPTIONS = (
    # short, long, type, default, help
    ('-t', '--thread', int, 4, 'number of threads to use [%(default)s] (SV phasing: while the caller VCF is first read beside the '
                               'BAM loop both use this many workers -- up to twice the number for a few milliseconds; '
                               'DUET_INGEST_STRICT_THREADS=1 splits the budget instead and keeps it a hard bound)'),
    ('-m', '--min_allele_frequency', float, 0.25,
     'minimum allele frequency required to call a candidate SNP [%(default)s]'),
    ('-c', '--cluster_max_distance', float, 0.9,
     'maximum span-position distance between SV marks in a cluster to call a SV candidates, '
     'when the base SV caller is SVIM [%(default)s]'),
    ('-s', '--sv_min_size', int, 50, 'minimum SV size to be reported [%(default)s]'),
    ('-r', '--min_support_read', int, 2,
     'minimum number of reads that support a SV to be reported [%(default)s]'),
)
_POSITIONALS = (
    ('BAM', 'sorted alignment file in .bam format (along with .bai file in the same directory)'),
    ('REFERENCE', 'indexed reference genome in .fasta format (along with .fai file in the same directory)'),
    ('OUTPUT', 'working and output directory (existing files in the directory will be overwritten)'),
)


def pc_cap_arg(text):
    """--pc_cap: an integer in 0 .. 2^30 - 3 (the read tag word saturates PC at 2^30 - 2, and a saturated value never votes)."""
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError('--pc_cap: %r is not an integer' % (text,))
    if not 0 <= v <= (1 << 30) - 3:
        raise argparse.ArgumentTypeError('--pc_cap: %d is not in 0 .. 2^30 - 3' % v)
    return v


def build_parser():
    ap = argparse.ArgumentParser(
        description='SNP-Assisted Structural Variant Calling and Phasing Using Oxford Nanopore Sequencing')
    for short, long_, typ, default, text in _OPTIONS:
        ap.add_argument(short, long_, type=typ, default=default, help=text)
    ap.add_argument('-a', '--include_all_ctgs', action='store_true',
                    help='call variants on all contigs, otherwise call chr{1..22,X,Y} [%(default)s]')
    ap.add_argument('-b', '--sv_caller', type=str, default='cutesv',
                    help='choose the base SV caller from cuteSV ("cutesv"), Sniffles (sniffles), or SVIM ("svim") '
                         '[%(default)s]; "svim-gpu" clusters the SV marks with --cluster_max_distance on the GPU instead of '
                         'running svim')
    ap.add_argument('--device', type=int, default=0, help='HIP device index for SV phasing [%(default)s]')
    ap.add_argument('--gpus', type=int, default=1,
                    help='number of GPUs for SV phasing: contigs are sharded over them, one process per GPU [%(default)s]')
    ap.add_argument('--thresholds', type=str, default=None,
                    help='JSON object of T1-T5 threshold values (duet_amd/tune.py names; the others keep their defaults) for the '
                         'SV phasing decision; one GPU only (the native path, or -b svim-gpu)')
    ap.add_argument('--pc_cap', type=pc_cap_arg, default=None,
                    help='reads with a PC tag above this never vote in the SV phasing decision [8100, or the pc_cap of '
                         '--thresholds]; one GPU only (the native path, or -b svim-gpu)')
    ap.add_argument('--write_evidence', action='store_true',
                    help='also write OUTPUT/phased_sv.evidence.tsv: one row per SV candidate, phased or not, with its vote, the rule '
                         'of the decision tree it ended at and the call; one GPU only (the native path, or -b svim-gpu)')
    ap.add_argument('--write_ps_links', action='store_true',
                    help='also write OUTPUT/phased_sv.ps_links.tsv and OUTPUT/phased_sv.ps_blocks.tsv: which WhatsHap phase sets the SV '
                         'candidates tie together, in which sense and how strongly, and the blocks they join into; one GPU only (the '
                         'native path, or -b svim-gpu)')
    ap.add_argument('--write_read_tags', action='store_true',
                    help='also write OUTPUT/phased_sv.read_tags.tsv: one row per supporting read and phase set of the heterozygous '
                         'calls, with the haplotype the calls place the read on, its own tag, and whether they agree; one GPU only '
                         '(the native path, or -b svim-gpu)')
    ap.add_argument('--join_ps', action='store_true',
                    help='also phase the SVs again over the phase sets that the SV candidates themselves tie into one block: writes '
                         'OUTPUT/phased_sv.joined.vcf, OUTPUT/phased_sv.join_blocks.tsv (the blocks used) and '
                         'OUTPUT/phased_sv.join_report.tsv (the calls that changed); phased_sv.vcf stays what it is; one GPU only (the '
                         'native path, or -b svim-gpu)')
    ap.add_argument('--join_min_sv', type=int, default=None,
                    help='with --join_ps: a link joins two phase sets only when at least this many SV candidates agree on it '
                         '[the join_min_sv key of the --thresholds file, else 2]')
    ap.add_argument('--vote_sv_tags', action='store_true',
                    help='also phase the SVs again with the untagged reads voting: a read without a WhatsHap tag gets the haplotype '
                         'that the OTHER heterozygous SV calls listing it place it on; writes OUTPUT/phased_sv.sv_tags.vcf and '
                         'OUTPUT/phased_sv.sv_tags_report.tsv (the calls that changed); phased_sv.vcf stays what it is; one GPU only '
                         '(the native path, or -b svim-gpu); not together with --join_ps')
    ap.add_argument('--sv_tag_min', type=int, default=None,
                    help='with --vote_sv_tags: a read gets a tag only when the other calls favour one haplotype by at least this many '
                         'marks [1]')
    ap.add_argument('--sv_tag_pc', type=int, default=None,
                    help='with --vote_sv_tags: the PC the derived tags carry, 0 .. 2^30 - 3 [0]')
    ap.add_argument('--write_sv_calls', action='store_true',
                    help='with -b svim-gpu, also write the clustered SV calls to OUTPUT/sv_calling/variants.vcf')
    for name, text in _POSITIONALS:
        ap.add_argument(name, type=str, help=text)
    return ap


def parse_args(argv):
    # upstream ignores `argv` and reads sys.argv (utils.py:43); so does this
    return build_parser().parse_args()


def set_logging(home):
    fmt = logging.Formatter('%(asctime)s [%(levelname)s] %(message)s', datefmt='%H:%M:%S')
    root = logging.getLogger()
    root.setLevel(logging.INFO)
    for handler in (logging.FileHandler(home + '/run_duet.log', mode='w'), logging.StreamHandler()):
        handler.setFormatter(fmt)
        root.addHandler(handler)


def add_stream_logging(home):
    """Logging of a rank process started by duet_amd/multi.py: the same line format on stderr, appended to
    <home>/run_duet.log when the parent logs there (DUET_RANK_LOG=1)."""
    fmt = logging.Formatter('%(asctime)s [%(levelname)s] %(message)s', datefmt='%H:%M:%S')
    root = logging.getLogger()
    root.setLevel(logging.INFO)
    handlers = [logging.StreamHandler()]
    if os.environ.get('DUET_RANK_LOG') == '1':
        handlers.append(logging.FileHandler(home + '/run_duet.log', mode='a'))
    for handler in handlers:
        handler.setFormatter(fmt)
        root.addHandler(handler)


def check_envs(ref_path, aln_path):
    if not os.path.exists(aln_path + '.bai'):
        sys.exit("[ERROR] Alignment index .bai file not found, please run 'samtools index " + aln_path + "' first")
    if not os.path.exists(ref_path + '.fai'):
        sys.exit("[ERROR] Reference index .fai file not found, please run 'samtools faidx " + ref_path + "' first")
