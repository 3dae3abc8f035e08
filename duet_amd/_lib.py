# coding=utf-8
"""ctypes binding of include/duet_ef.h (libduet_ef.so, hand-written HIP for gfx950).

There is deliberately NO CPU fallback: if the shared library is missing or no MI355X is visible,
every entry point raises.  Build the library with `python -c "import __graft_entry__ as g; g.build()"`
(or `make -C duet_amd/csrc`).
"""

import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'lib', 'libduet_ef.so')

DUET_OK = 0
DUET_ERR_INVALID = -1
DUET_ERR_DIV_ZERO = -5
DUET_ERR_TIMEOUT = -6
MARK_ABSENT = 0xFFFFFFFF
PC_MAX = 8100                   # DUET_PC_MAX: the reference's PC cap (sv_phasing_fn.py:76,88,201)
PC_CAP_MAX = (1 << 30) - 3      # the largest cap the *_cap entries take: the tag word saturates pc at 2^30 - 2
N_KERNELS = 3
KERNEL_NAMES = ('ef_classify', 'ef_seed_sort', 'ef_finalize')

# every symbol include/duet_ef.h declares (checked by tests/test_abi.py)
EXPORTS = ('duet_abi_version', 'duet_ctx_create', 'duet_ctx_destroy', 'duet_last_error',
           'duet_ctx_set_profiling', 'duet_ctx_set_debug', 'duet_ef_run_device', 'duet_ef_check', 'duet_ef_run_host',
           'duet_ef_profile_collect', 'duet_ef_get_seed_ps', 'duet_cluster_run_device', 'duet_cluster_run_host', 'duet_svim_phase_device', 'duet_svim_phase_host', 'duet_rows_run_device',
           'duet_ef_rows_run_host', 'duet_eval_run_host', 'duet_eval_details_host', 'duet_comm_unique_id', 'duet_comm_create', 'duet_comm_allgather_device',
           'duet_comm_allgather_host', 'duet_comm_destroy', 'duet_comm_set_timeout', 'duet_comm_block_bytes',
           'duet_comm_ef_allgather', 'duet_comm_rccl_version', 'duet_comm_info', 'duet_comm_selftest',
           'duet_ef_features_device', 'duet_ef_features_host', 'duet_tune_sweep_device', 'duet_tune_sweep_host',
           'duet_svim_vcf_rows_device', 'duet_svim_vcf_rows_host', 'duet_svim_phased_rows_device', 'duet_svim_phased_rows_host',
           'duet_svim_features_device', 'duet_svim_features_host', 'duet_tune_truth_build_device', 'duet_tune_truth_build_host',
           'duet_tune_strata_build_device', 'duet_tune_strata_build_host', 'duet_tune_sweep_strata_device',
           'duet_tune_sweep_strata_host', 'duet_tune_line_device', 'duet_tune_line_host',
           'duet_ef_features_cap_device', 'duet_ef_features_cap_host', 'duet_svim_features_cap_device', 'duet_svim_features_cap_host',
           'duet_tune_cap_line_device', 'duet_tune_cap_line_host', 'duet_svim_cap_line_device', 'duet_svim_cap_line_host',
           'duet_tune_leaf_census_device', 'duet_tune_leaf_census_host', 'duet_tune_leaves_device', 'duet_tune_leaves_host',
           'duet_evidence_rows_device', 'duet_evidence_rows_host',
           'duet_ps_links_device', 'duet_ps_links_host', 'duet_svim_ps_links_device', 'duet_svim_ps_links_host',
           'duet_read_tags_device', 'duet_read_tags_host', 'duet_read_tags_rows_device', 'duet_read_tags_rows_host',
           'duet_ps_join_tags_device', 'duet_ps_join_tags_host', 'duet_ps_join_diff_device', 'duet_ps_join_diff_host',
           'duet_ps_blocks_device', 'duet_ps_blocks_host', 'duet_ps_join_links_device',
           'duet_sv_tags_device', 'duet_sv_tags_host',
           'duet_sv_tags_plan_device', 'duet_sv_tags_plan_host', 'duet_sv_tags_apply_device', 'duet_sv_tags_apply_host',
           'duet_prims_sort_host', 'duet_prims_scan_host', 'duet_prims_local_sort_host')


class EfProblem(ctypes.Structure):
    _fields_ = [('n_contigs', ctypes.c_uint32), ('n_cands', ctypes.c_uint32), ('n_marks', ctypes.c_uint32),
                ('n_reads', ctypes.c_uint32),
                ('cand_ctg_off', ctypes.c_void_p), ('read_tag', ctypes.c_void_p), ('cand_pos', ctypes.c_void_p),
                ('cand_svlen', ctypes.c_void_p), ('cand_svread', ctypes.c_void_p), ('cand_refread', ctypes.c_void_p),
                ('cand_gt_ok', ctypes.c_void_p), ('cand_off', ctypes.c_void_p), ('mark_read', ctypes.c_void_p),
                ('svlen_thres', ctypes.c_uint32), ('suppread_thres', ctypes.c_uint32)]


class EfStats(ctypes.Structure):
    _fields_ = [('algorithmic_bytes', ctypes.c_uint64), ('n_seed_ps', ctypes.c_uint32),
                ('n_profiled_runs', ctypes.c_uint32), ('kernel_ms', ctypes.c_float * N_KERNELS),
                ('total_ms', ctypes.c_float)]


class ClusterProblem(ctypes.Structure):
    _fields_ = [('n_marks', ctypes.c_uint32), ('part_gap', ctypes.c_uint32), ('part_max', ctypes.c_uint32),
                ('n_contigs_hint', ctypes.c_uint32), ('n_types_hint', ctypes.c_uint32), ('max_pos_hint', ctypes.c_uint32),
                ('max_span_hint', ctypes.c_uint32), ('reserved', ctypes.c_uint32),
                ('max_dist', ctypes.c_double), ('normalizer', ctypes.c_double),
                ('mark_contig', ctypes.c_void_p), ('mark_type', ctypes.c_void_p), ('mark_pos', ctypes.c_void_p),
                ('mark_span', ctypes.c_void_p)]


class ClusterResult(ctypes.Structure):
    _fields_ = [('order', ctypes.c_void_p), ('cand_off', ctypes.c_void_p), ('cand_contig', ctypes.c_void_p),
                ('cand_type', ctypes.c_void_p), ('cand_pos', ctypes.c_void_p), ('cand_span', ctypes.c_void_p),
                ('n_cands', ctypes.c_void_p)]


class SvimProblem(ctypes.Structure):
    _fields_ = [('marks', ClusterProblem), ('mark_read', ctypes.c_void_p), ('read_tag', ctypes.c_void_p),
                ('n_reads', ctypes.c_uint32), ('n_contigs', ctypes.c_uint32), ('depth', ctypes.c_void_p),
                ('depth_off', ctypes.c_void_p), ('depth_bin', ctypes.c_uint32), ('svlen_thres', ctypes.c_uint32),
                ('suppread_thres', ctypes.c_uint32), ('reserved', ctypes.c_uint32)]


class CallsetNames(ctypes.Structure):
    _fields_ = [('mark_name', ctypes.c_void_p), ('name_off', ctypes.c_void_p), ('name_pool', ctypes.c_void_p),
                ('n_names', ctypes.c_uint32), ('n_contigs', ctypes.c_uint32), ('chrom', ctypes.POINTER(ctypes.c_char_p))]


def callset_bound(n_cands, n_marks, name_off, chrom_texts):
    """The size duet_svim_vcf_rows_* can need at most (include/duet_ef.h): what the caller allocates for one call."""
    longest = int(np.max(np.diff(np.asarray(name_off, dtype=np.int64)))) if len(name_off) > 1 else 0
    chrom = max([len(c.encode()) for c in chrom_texts] + [0])
    return int(n_cands) * (2 * chrom + 168) + int(n_marks) * (longest + 1) + 64


def chrom_bytes(chrom_texts):
    """CHROM texts as the bytes the library compares and writes (str: UTF-8, whose byte order is Python's str order)."""
    return [c if isinstance(c, bytes) else c.encode() for c in chrom_texts]


def phased_rows_bound(n_rows, chrom_texts):
    """The size duet_svim_phased_rows_* can need at most for n_rows rows (include/duet_ef.h): a row without CHROM is at most
    95 bytes."""
    return int(n_rows) * (max([len(c) for c in chrom_bytes(chrom_texts)] + [0]) + 96)


def callset_names(mark_name, name_off, name_pool, chrom_texts, keep):
    """-> CallsetNames over the given arrays (host or device pointers: ints are taken as device pointers); `keep` collects what
    must outlive the call."""
    n = CallsetNames()
    for field, a in (('mark_name', mark_name), ('name_off', name_off), ('name_pool', name_pool)):
        if isinstance(a, int):
            setattr(n, field, a)
        else:
            keep.append(a)
            setattr(n, field, a.ctypes.data if a.size else None)
    n.n_names = int(len(name_off) if not isinstance(name_off, int) else 0)
    texts = (ctypes.c_char_p * max(len(chrom_texts), 1))(*[c.encode() for c in chrom_texts])
    keep.append(texts)
    n.n_contigs = len(chrom_texts)
    n.chrom = texts
    return n


class RowsProblem(ctypes.Structure):
    _fields_ = [('n_contigs', ctypes.c_uint32), ('n_cands', ctypes.c_uint32), ('cand_ctg_off', ctypes.c_void_p),
                ('pred', ctypes.c_void_p), ('ps', ctypes.c_void_p), ('cand_pos', ctypes.c_void_p),
                ('cand_svlen', ctypes.c_void_p), ('cand_plus', ctypes.c_void_p), ('cand_chrom_rank', ctypes.c_void_p),
                ('n_chrom_texts', ctypes.c_uint32), ('max_pos', ctypes.c_uint32), ('pool', ctypes.c_void_p),
                ('pool_bytes', ctypes.c_uint64), ('str_off', ctypes.c_void_p), ('cand_off', ctypes.c_void_p),
                ('mark_read', ctypes.c_void_p), ('read_tag', ctypes.c_void_p)]


class EvalProblem(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ('n_base', 'n_calls', 'n_groups', 'n_keys', 'n_base_uid', 'n_call_uid', 'refdist',
                                               'reserved')] + [('ratio', ctypes.c_double)] + \
               [(n, ctypes.c_void_p) for n in ('base_off', 'base_pos', 'base_len', 'base_uid', 'base_hp', 'call_key', 'call_pos',
                                               'call_len', 'call_uid', 'call_group', 'call_hp')]


class EvalCounts(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ('call_tp', 'base_tp', 'call_gt', 'base_gt', 'call_hp', 'base_hp')]


# the evaluator's per-record outcome (include/duet_ef.h: duet_eval_call_rec, 12 bytes; duet_eval_base_rec, 24 bytes)
EVAL_CALL_DTYPE = np.dtype([('base', '<u4'), ('dist', '<u4'), ('bits', '<u4')])
EVAL_BASE_DTYPE = np.dtype([('n_calls', '<u4'), ('n_gt', '<u4'), ('n_hp', '<u4'), ('nearest', '<u4'), ('nearest_dist', '<u4'),
                            ('reason', 'u1'), ('reserved', 'u1', (3,))])
EVAL_NEAR, EVAL_SIZE, EVAL_MATCHED, EVAL_GT, EVAL_SAME, EVAL_FLIP, EVAL_LABEL, EVAL_HP = (1 << i for i in range(8))   # DUET_EVAL_NEAR ..
EVAL_REASON_NAMES = ('no_call', 'far', 'size', 'elsewhere')                        # DUET_EVAL_NO_CALL .. DUET_EVAL_ELSEWHERE
EVAL_HIT = 255                                                                     # DUET_EVAL_HIT
EVAL_NONE = 0xFFFFFFFF

# threshold sweep (include/duet_ef.h, "Threshold sweep"; duet_amd/tune.py)
TUNE_NAMES = ('c0_min_sv_num', 'c2_min_sv_ratio', 'c2_max_avgsc_diff', 'c2_min_sv_num', 'c2_min_hap0', 'c1_onehap_sv_ratio_lo',
              'c1_onehap_sv_ratio_hi', 'c1_hapread_ratio', 'c1_max_avgsc_diff', 'c1_twohap_sv_ratio_1', 'c1_twohap_sv_ratio_2',
              'c1_max_ref_num', 'c1_twohap_sv_ratio_3', 'c1_max_totsc_ratio')
TUNE_DEFAULTS = (4.0, 0.72, 1369.5, 3.0, 6.0, 0.24, 0.9, 0.75, 2400.0, 0.3, 0.45, 10.0, 0.75, 9.72)
FEATURE_DTYPE = np.dtype([('t1', '<u8'), ('t2', '<u8'), ('hap1', '<u4'), ('hap2', '<u4'), ('hap0', '<u4'), ('allhap', '<u4'),
                          ('deg', '<u4'), ('svread', '<u4'), ('refread', '<u4'), ('ps', '<u4'), ('eligible', 'u1'), ('kept', 'u1'),
                          ('cls', 'u1'), ('reserved0', 'u1'), ('reserved1', '<u4')])
COUNTS_NAMES = ('n_calls', 'n_groups', 'call_tp', 'base_tp', 'call_gt', 'base_gt', 'call_hp', 'base_hp', 'n_raise', 'reserved')
COUNTS_DTYPE = np.dtype([(n, '<u4') for n in COUNTS_NAMES])
TUNE_IN_CALLS, TUNE_RAISES, TUNE_MATCHED = 0x1000, 0x2000, 0x4000
# the leaf census (include/duet_ef.h, "Leaf census"): the 18 exits of the tree, their nominal pred (1: 1 or 2), the record
LEAF_NAMES = ('c0_call', 'c0_drop', 'c2_low_ratio', 'c2_near_call', 'c2_near_few', 'c2_far_call', 'c2_far_few', 'c1_one_low',
              'c1_one_het', 'c1_one_het_gated', 'c1_one_hom', 'c1_one_hom_gated', 'c1_two_low', 'c1_two_het_ref', 'c1_two_het',
              'c1_two_mid_hom', 'c1_two_mid_het', 'c1_two_hom')
LEAF_PRED = (3, 0, 0, 3, 0, 3, 0, 0, 1, 0, 3, 0, 0, 0, 1, 3, 1, 3)
N_LEAVES = len(LEAF_NAMES)
# the evidence table (include/duet_ef.h, "Evidence table"): the two states beside the 18 leaves, the columns of a row
LEAF_NO_SEED, LEAF_FILTERED = 0xFD, 0xFE
EVIDENCE_COLUMNS = ('CHROM', 'POS', 'SVTYPE', 'SVLEN', 'SVREAD', 'REFREAD', 'MARKS', 'RULE', 'CLASS', 'HAP1', 'HAP2', 'HAP0', 'VOTERS',
                    'PCSUM1', 'PCSUM2', 'PS', 'HP')
EVIDENCE_ROW_MAX = 180          # a row's bytes at most, without its CHROM and SVTYPE pieces
LEAF_COUNTS_NAMES = ('n_cands', 'n_listed', 'n_matched', 'n_calls', 'call_tp', 'call_gt', 'call_hp', 'n_raise')
LEAF_COUNTS_DTYPE = np.dtype([(n, '<u4') for n in LEAF_COUNTS_NAMES])


class EvidenceProblem(ctypes.Structure):
    """duet_evidence_problem; chrom is host memory in both forms."""
    _fields_ = [('n_cands', ctypes.c_uint32), ('n_contigs', ctypes.c_uint32)] + \
               [(n, ctypes.c_void_p) for n in ('feat', 'leaf', 'pred', 'cand_pos', 'cand_svlen', 'pool')] + \
               [('pool_bytes', ctypes.c_uint64)] + [(n, ctypes.c_void_p) for n in ('str_off', 'cand_contig', 'cand_type')] + \
               [('chrom', ctypes.POINTER(ctypes.c_char_p))]


def evidence_bound(n_cands, longest_chrom, longest_svtype=3):
    """The size duet_evidence_rows_* can need at most (include/duet_ef.h): what the caller allocates for one call."""
    return int(n_cands) * (int(longest_chrom) + int(longest_svtype) + EVIDENCE_ROW_MAX)


def evidence_header():
    """The header line of phased_sv.evidence.tsv."""
    return ('\t'.join(EVIDENCE_COLUMNS) + '\n').encode()


# phase-set links (include/duet_ef.h, "Phase-set links"; duet_amd/ps_links.py): one record per (contig, ps_a, ps_b)
class PsLink(ctypes.Structure):
    """duet_ps_link (56 bytes)."""
    _fields_ = [('w_same', ctypes.c_uint64), ('w_flip', ctypes.c_uint64)] + \
               [(n, ctypes.c_uint32) for n in ('contig', 'ps_a', 'ps_b', 'n_sv', 'n_same', 'n_flip', 'n_open', 'pos_min', 'pos_max',
                                               'reserved')]


PS_LINK_DTYPE = np.dtype([('w_same', '<u8'), ('w_flip', '<u8')] +
                         [(n, '<u4') for n in ('contig', 'ps_a', 'ps_b', 'n_sv', 'n_same', 'n_flip', 'n_open', 'pos_min', 'pos_max',
                                               'reserved')])


def ps_links_room(n_marks):
    """The records duet_ps_links_* can write at most (include/duet_ef.h): what the caller allocates for one call."""
    return max(int(n_marks), 1) - 1


# read tags from phased SVs (include/duet_ef.h, "Read tags from phased SVs"; duet_amd/read_tags.py): one record per (name, ps)
READ_TAG_FIELDS = ('name', 'contig', 'ps', 'read', 'n_h1', 'n_h2', 'pos_min', 'pos_max', 'status', 'reserved')
READ_TAG_DTYPE = np.dtype([(n, '<u4') for n in READ_TAG_FIELDS])                     # duet_read_tag_rec (40 bytes)
READ_TAG_STATUS_NAMES = ('agree', 'disagree', 'tie', 'new', 'other_ps')            # DUET_READ_TAG_AGREE .. DUET_READ_TAG_OTHER_PS
READ_TAG_COLUMNS = ('CHROM', 'READ', 'PS', 'N_SV', 'N_H1', 'N_H2', 'HP_SV', 'TAG_HP', 'TAG_PS', 'TAG_PC', 'STATUS', 'POS_MIN', 'POS_MAX')
READ_TAG_ROW_MAX = 104          # a row's bytes at most, without its CHROM and READ pieces


class ReadTagsProblem(ctypes.Structure):
    """duet_read_tags_problem; cand_ctg_off is host memory in both forms."""
    _fields_ = [(n, ctypes.c_uint32) for n in ('n_cands', 'n_marks', 'n_reads', 'n_names', 'n_contigs', 'reserved')] + \
               [(n, ctypes.c_void_p) for n in ('cand_off', 'mark_order', 'mark_read', 'mark_name', 'pred', 'ps', 'cand_pos',
                                               'cand_ctg_off', 'cand_contig', 'read_tag')]


def read_tags_bound(n_recs, name_off, chrom_texts):
    """The size duet_read_tags_rows_* can need at most (include/duet_ef.h): what the caller allocates for one call."""
    longest = int(np.max(np.diff(np.asarray(name_off, dtype=np.int64)))) if len(name_off) > 1 else 0
    chrom = max([len(c) for c in chrom_bytes(chrom_texts)] + [0])
    return int(n_recs) * (chrom + longest + READ_TAG_ROW_MAX)


# joined phase sets (include/duet_ef.h, "Joined phase sets"; duet_amd/ps_join.py): the table's rows, the change codes
PS_BLOCK_DTYPE = np.dtype([(n, '<u4') for n in ('contig', 'ps', 'block', 'flip')])      # duet_ps_block (16 bytes)
JOIN_CHANGE_NAMES = ('none', 'gained', 'lost', 'same', 'relabelled', 'to_het', 'to_hom', 'other')   # DUET_PS_JOIN_NONE .. _OTHER


class PsBlocksCounts(ctypes.Structure):     # duet_ps_blocks_counts
    _fields_ = [(n, ctypes.c_uint32) for n in ('n_rows', 'n_trusted', 'n_conflicts', 'n_components')]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class SvTagsPlanInfo(ctypes.Structure):     # duet_sv_tags_plan_info
    _fields_ = [(n, ctypes.c_uint32) for n in ('n_untagged', 'n_records', 'n_runs', 'n_contributing')]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class TuneTruth(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ('n_uid', 'n_groups', 'n_pairs', 'reserved')] + \
               [(n, ctypes.c_void_p) for n in ('cand_flags', 'cand_group', 'cand_uid', 'cand_pair', 'group_pair_off', 'pair_uid')]


TUNE_KEY_NONE, TUNE_KEY_SKIP = 0xFFFFFFFE, 0xFFFFFFFF
TUNE_MAX_STRATA = 64


class TuneStrata(ctypes.Structure):
    """duet_tune_strata; uid_off is host memory in both forms."""
    _fields_ = [('n_strata', ctypes.c_uint32), ('reserved', ctypes.c_uint32)] + \
               [(n, ctypes.c_void_p) for n in ('cand_stratum', 'group_stratum', 'uid_off')]


class TuneTruthProblem(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ('n_cands', 'n_keys', 'n_base', 'n_base_uid', 'n_chrom', 'n_contigs', 'refdist',
                                               'reserved')] + [('ratio', ctypes.c_double)] + \
               [(n, ctypes.c_void_p) for n in ('feat', 'cand_pos', 'cand_len', 'cand_key', 'cand_chrom', 'cand_contig', 'cand_type',
                                               'key_table', 'chrom_id', 'bed_off', 'bed_lo', 'bed_hi', 'base_off', 'base_pos',
                                               'base_len', 'base_uid', 'base_hp')]


# the arrays of a TuneTruthProblem and their element types: per candidate (either form), the tables, the truth side
TRUTH_PROBLEM_ARRAYS = (('cand_pos', np.uint32), ('cand_len', np.uint32), ('cand_key', np.uint32), ('cand_chrom', np.uint32),
                        ('cand_contig', np.uint16), ('cand_type', np.uint8), ('key_table', np.uint32), ('chrom_id', np.uint32),
                        ('bed_off', np.uint32), ('bed_lo', np.uint32), ('bed_hi', np.uint32), ('base_off', np.uint32),
                        ('base_pos', np.uint32), ('base_len', np.uint32), ('base_uid', np.uint32), ('base_hp', np.uint8))
TRUTH_ARRAYS = (('cand_flags', np.uint16), ('cand_group', np.uint32), ('cand_uid', np.uint32), ('cand_pair', np.uint32),
                ('group_pair_off', np.uint32), ('pair_uid', np.uint32))


def eval_problem(arrays, refdist, ratio):
    """The flat host arrays of duet_amd/evaluation.py's flatten -> (EvalProblem, what must outlive the call)."""
    p = EvalProblem()
    keep = {}
    for name, dt in (('base_off', np.uint32), ('base_pos', np.uint32), ('base_len', np.uint32), ('base_uid', np.uint32),
                     ('base_hp', np.uint8), ('call_key', np.uint32), ('call_pos', np.uint32), ('call_len', np.uint32),
                     ('call_uid', np.uint32), ('call_group', np.uint32), ('call_hp', np.uint8)):
        keep[name] = np.ascontiguousarray(arrays[name], dtype=dt)
        setattr(p, name, keep[name].ctypes.data if keep[name].size else None)
    p.n_base, p.n_calls = len(keep['base_pos']), len(keep['call_pos'])
    p.n_keys, p.n_groups = len(keep['base_off']) - 1, int(arrays['n_groups'])
    p.n_base_uid, p.n_call_uid = int(arrays['n_base_uid']), int(arrays['n_call_uid'])
    p.refdist, p.ratio = clamp_u32(refdist), float(ratio)
    return p, keep


class DuetLibraryError(RuntimeError):
    pass


_lib = None


def load():
    """Load libduet_ef.so (once). Raises DuetLibraryError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DuetLibraryError('%s is missing: the HIP extension has not been built '
                               '(run __graft_entry__.build()); there is no CPU fallback' % LIB_PATH)
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64/libhsa-runtime64 and loads
    # them by unversioned name, so if this library pulled in /opt/rocm's copy first, torch would load a
    # second runtime and find no GPU.  Importing torch first makes the loader bind our DT_NEEDED
    # libamdhip64.so.7 to the copy torch already mapped (same SONAME).
    # (DUET_NO_TORCH=1: a process that will never import torch -- the rank processes of `duet --gpus N`, duet_amd/multi.py --
    # skips this: the library then binds /opt/rocm's runtime, as RCCL does)
    if os.environ.get('DUET_NO_TORCH') != '1':
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = ctypes.CDLL(LIB_PATH)
    lib.duet_abi_version.restype = ctypes.c_int
    lib.duet_ctx_create.restype = ctypes.c_void_p
    lib.duet_ctx_create.argtypes = [ctypes.c_int]
    lib.duet_ctx_destroy.restype = None
    lib.duet_ctx_destroy.argtypes = [ctypes.c_void_p]
    lib.duet_last_error.restype = ctypes.c_char_p
    lib.duet_last_error.argtypes = [ctypes.c_void_p]
    lib.duet_ctx_set_profiling.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.duet_ctx_set_debug.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    lib.duet_ef_run_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(EfProblem), ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p]
    lib.duet_ef_check.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.duet_ef_run_host.argtypes = [ctypes.c_void_p, ctypes.POINTER(EfProblem), ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.POINTER(EfStats)]
    lib.duet_ef_profile_collect.argtypes = [ctypes.c_void_p, ctypes.POINTER(EfStats)]
    lib.duet_ef_get_seed_ps.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]
    lib.duet_cluster_run_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(ClusterProblem),
                                            ctypes.POINTER(ClusterResult), ctypes.c_void_p]
    lib.duet_cluster_run_host.argtypes = [ctypes.c_void_p, ctypes.POINTER(ClusterProblem), ctypes.POINTER(ClusterResult)]
    lib.duet_rows_run_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(RowsProblem), ctypes.c_void_p, ctypes.c_uint64,
                                         ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p]
    lib.duet_ef_rows_run_host.argtypes = [ctypes.c_void_p, ctypes.POINTER(EfProblem), ctypes.POINTER(RowsProblem), ctypes.c_void_p,
                                          ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)]
    lib.duet_eval_run_host.argtypes = [ctypes.c_void_p, ctypes.POINTER(EvalProblem), ctypes.POINTER(EvalCounts)]
    lib.duet_eval_details_host.argtypes = [ctypes.c_void_p, ctypes.POINTER(EvalProblem), ctypes.POINTER(EvalCounts), ctypes.c_void_p,
                                           ctypes.c_void_p]
    lib.duet_svim_phase_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(SvimProblem), ctypes.POINTER(ClusterResult),
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p]
    lib.duet_svim_phase_host.argtypes = [ctypes.c_void_p, ctypes.POINTER(SvimProblem), ctypes.POINTER(ClusterResult),
                                         ctypes.c_void_p, ctypes.c_void_p]
    lib.duet_comm_unique_id.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.duet_comm_create.restype = ctypes.c_void_p
    lib.duet_comm_create.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.duet_comm_allgather_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    lib.duet_comm_allgather_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    lib.duet_comm_rccl_version.argtypes = [ctypes.c_void_p]
    lib.duet_comm_set_timeout.argtypes = [ctypes.c_void_p, ctypes.c_double]
    lib.duet_comm_block_bytes.restype = ctypes.c_uint64
    lib.duet_comm_block_bytes.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    lib.duet_comm_ef_allgather.argtypes = [ctypes.c_void_p, ctypes.POINTER(EfProblem), ctypes.c_void_p, ctypes.c_uint32,
                                           ctypes.c_uint32, ctypes.c_void_p]
    lib.duet_comm_info.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_int)] * 5
    lib.duet_comm_selftest.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    lib.duet_ef_features_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(EfProblem), ctypes.c_void_p, ctypes.c_void_p]
    lib.duet_ef_features_host.argtypes = [ctypes.c_void_p, ctypes.POINTER(EfProblem), ctypes.c_void_p]
    lib.duet_tune_sweep_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32,
                                           ctypes.POINTER(TuneTruth), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.duet_tune_sweep_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32,
                                         ctypes.POINTER(TuneTruth), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.duet_comm_destroy.restype = None
    lib.duet_comm_destroy.argtypes = [ctypes.c_void_p]
    for fn in (lib.duet_svim_vcf_rows_device, lib.duet_svim_vcf_rows_host):
        fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(SvimProblem), ctypes.POINTER(ClusterResult), ctypes.c_uint32,
                       ctypes.POINTER(CallsetNames), ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)] + \
                      ([ctypes.c_void_p] if fn is lib.duet_svim_vcf_rows_device else [])
    for fn in (lib.duet_svim_phased_rows_device, lib.duet_svim_phased_rows_host):
        fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ClusterResult), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                       ctypes.c_uint32, ctypes.POINTER(ctypes.c_char_p), ctypes.c_void_p, ctypes.c_uint64,
                       ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)] + \
                      ([ctypes.c_void_p] if fn is lib.duet_svim_phased_rows_device else [])
    lib.duet_svim_features_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(SvimProblem), ctypes.POINTER(ClusterResult),
                                              ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p]
    lib.duet_svim_features_host.argtypes = [ctypes.c_void_p, ctypes.POINTER(SvimProblem), ctypes.POINTER(ClusterResult), ctypes.c_void_p]
    lib.duet_tune_truth_build_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(TuneTruthProblem), ctypes.POINTER(TuneTruth),
                                                 ctypes.c_void_p]
    lib.duet_tune_truth_build_host.argtypes = [ctypes.c_void_p, ctypes.POINTER(TuneTruthProblem), ctypes.POINTER(TuneTruth)]
    lib.duet_tune_strata_build_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(TuneTruthProblem), ctypes.POINTER(TuneTruth),
                                                  ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.duet_tune_strata_build_host.argtypes = lib.duet_tune_strata_build_device.argtypes[:-1]
    lib.duet_tune_sweep_strata_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32,
                                                  ctypes.POINTER(TuneTruth), ctypes.POINTER(TuneStrata), ctypes.c_void_p, ctypes.c_void_p]
    lib.duet_tune_sweep_strata_host.argtypes = lib.duet_tune_sweep_strata_device.argtypes[:-1]
    lib.duet_tune_leaf_census_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32,
                                                 ctypes.POINTER(TuneTruth), ctypes.POINTER(TuneStrata), ctypes.c_void_p, ctypes.c_void_p]
    lib.duet_tune_leaf_census_host.argtypes = lib.duet_tune_leaf_census_device.argtypes[:-1]
    lib.duet_tune_leaves_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p]
    lib.duet_tune_leaves_host.argtypes = lib.duet_tune_leaves_device.argtypes[:-1]
    lib.duet_evidence_rows_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(EvidenceProblem), ctypes.c_void_p, ctypes.c_uint64,
                                              ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
    lib.duet_evidence_rows_host.argtypes = lib.duet_evidence_rows_device.argtypes[:-1]
    lib.duet_ps_links_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(EfProblem), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32,
                                         ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p]
    lib.duet_ps_links_host.argtypes = lib.duet_ps_links_device.argtypes[:-1]
    lib.duet_svim_ps_links_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(SvimProblem), ctypes.POINTER(ClusterResult), ctypes.c_uint32,
                                              ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                              ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p]
    lib.duet_svim_ps_links_host.argtypes = [ctypes.c_void_p, ctypes.POINTER(SvimProblem), ctypes.POINTER(ClusterResult), ctypes.c_uint32,
                                            ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    lib.duet_read_tags_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(ReadTagsProblem), ctypes.c_uint32, ctypes.c_void_p,
                                          ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p]
    lib.duet_read_tags_host.argtypes = lib.duet_read_tags_device.argtypes[:-1]
    lib.duet_read_tags_rows_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(CallsetNames),
                                               ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                                               ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
    lib.duet_read_tags_rows_host.argtypes = lib.duet_read_tags_rows_device.argtypes[:-1]
    lib.duet_ps_join_tags_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                             ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32),
                                             ctypes.c_void_p]
    lib.duet_ps_join_tags_host.argtypes = lib.duet_ps_join_tags_device.argtypes[:-1]
    lib.duet_ps_join_diff_device.argtypes = [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 6 + \
                                            [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p]
    lib.duet_ps_join_diff_host.argtypes = lib.duet_ps_join_diff_device.argtypes[:-1]
    lib.duet_ps_blocks_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                          ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32,
                                          ctypes.POINTER(PsBlocksCounts), ctypes.c_void_p]
    lib.duet_ps_blocks_host.argtypes = lib.duet_ps_blocks_device.argtypes[:-1]
    lib.duet_ps_join_links_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                              ctypes.POINTER(PsBlocksCounts), ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p]
    lib.duet_sv_tags_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(ReadTagsProblem)] + [ctypes.c_uint32] * 3 + [ctypes.c_void_p] * 4
    lib.duet_sv_tags_host.argtypes = lib.duet_sv_tags_device.argtypes[:-1]
    lib.duet_sv_tags_plan_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(ReadTagsProblem), ctypes.c_void_p, ctypes.c_uint32,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(SvTagsPlanInfo), ctypes.c_void_p]
    lib.duet_sv_tags_plan_host.argtypes = lib.duet_sv_tags_plan_device.argtypes[:-1]
    lib.duet_sv_tags_apply_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 3
    lib.duet_sv_tags_apply_host.argtypes = lib.duet_sv_tags_apply_device.argtypes[:-1]
    lib.duet_tune_line_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32,
                                          ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32),
                                          ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p]
    lib.duet_tune_line_host.argtypes = lib.duet_tune_line_device.argtypes[:-1]
    lib.duet_ef_features_cap_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(EfProblem), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    lib.duet_ef_features_cap_host.argtypes = lib.duet_ef_features_cap_device.argtypes[:-1]
    lib.duet_svim_features_cap_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(SvimProblem), ctypes.POINTER(ClusterResult),
                                                  ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p]
    lib.duet_svim_features_cap_host.argtypes = [ctypes.c_void_p, ctypes.POINTER(SvimProblem), ctypes.POINTER(ClusterResult),
                                                ctypes.c_uint32, ctypes.c_void_p]
    for fn, prob in ((lib.duet_tune_cap_line_device, EfProblem), (lib.duet_svim_cap_line_device, SvimProblem)):
        fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(prob), ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32),
                       ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p]
    lib.duet_tune_cap_line_host.argtypes = lib.duet_tune_cap_line_device.argtypes[:-1]
    lib.duet_svim_cap_line_host.argtypes = lib.duet_svim_cap_line_device.argtypes[:-1]
    lib.duet_prims_sort_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                         ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.duet_prims_scan_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_int,
                                         ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p]
    lib.duet_prims_local_sort_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                               ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    _lib = lib
    return lib


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else ctypes.c_void_p(0)


def fill_cluster_problem(p, contig, mtype, pos, span, max_dist, part_gap, part_max, normalizer, hints=True):
    """The scalar fields of ClusterProblem p and, with hints, the four sizes the sort key is packed by, from the mark arrays
    (the array pointers are the caller's: host or device)."""
    M = len(pos)
    p.n_marks, p.part_gap, p.part_max = M, int(part_gap), int(part_max)
    p.max_dist, p.normalizer = float(max_dist), float(normalizer)
    if hints and M:
        p.n_contigs_hint = int(np.max(contig)) + 1
        p.n_types_hint = int(np.max(mtype)) + 1
        p.max_pos_hint = int(np.max(pos))
        p.max_span_hint = max(int(np.max(span)), 1)
    return M


def bind_cluster_result(arrays, n_cands=None):
    """-> a ClusterResult over the host arrays of dict `arrays` (a field without an array, or with an empty one, stays null);
    n_cands: the c_uint32 the entry writes the count to."""
    res = ClusterResult()
    for k, a in arrays.items():
        setattr(res, k, a.ctypes.data if a is not None and a.size else None)
    if n_cands is not None:
        res.n_cands = ctypes.addressof(n_cands)
    return res


CONTEXTS_CREATED = 0            # > 0: this process has initialised HIP (duet_amd/launch.py refuses to start ranks from it)


class Context(object):
    """One duet_ctx on one HIP device."""

    def __init__(self, device_id=0):
        global CONTEXTS_CREATED
        self.lib = load()
        self.handle = self.lib.duet_ctx_create(int(device_id))
        if not self.handle:
            raise DuetLibraryError('duet_ctx_create(%d) failed: %s' % (
                device_id, self.lib.duet_last_error(None).decode('utf-8', 'replace')))
        self.device_id = int(device_id)
        CONTEXTS_CREATED += 1

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.duet_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return self.lib.duet_last_error(self.handle).decode('utf-8', 'replace')

    def _raise(self, rc):
        msg = self.lib.duet_last_error(self.handle).decode('utf-8', 'replace')
        if rc == DUET_ERR_DIV_ZERO:
            raise ZeroDivisionError('division by zero')        # what upstream raises (sv_phasing_fn.py:123)
        raise DuetLibraryError('duet_ef call failed (%d): %s' % (rc, msg))

    def set_profiling(self, mode):
        """0 off, 1 (or True) events around ef_classify only, 2 around every kernel."""
        rc = self.lib.duet_ctx_set_profiling(self.handle, int(mode))
        if rc:
            self._raise(rc)

    def set_debug(self, flags):
        rc = self.lib.duet_ctx_set_debug(self.handle, int(flags))
        if rc:
            self._raise(rc)

    # -- host arrays ---------------------------------------------------------------------------
    def run_host(self, soa, svlen_thres, suppread_thres, want_stats=False):
        """soa: engine.EfSoA with numpy arrays. Returns (pred u8[C], ps u32[C][, stats])."""
        prob, keep = problem_from_arrays(soa, svlen_thres, suppread_thres)
        C = soa.n_cands
        pred = np.zeros(C, dtype=np.uint8)
        ps = np.zeros(C, dtype=np.uint32)
        stats = EfStats()
        # (statistics only when asked for: the seed count behind a two-launch run costs an ef_seed_sort launch of its own)
        rc = self.lib.duet_ef_run_host(self.handle, ctypes.byref(prob), _ptr(pred), _ptr(ps), ctypes.byref(stats) if want_stats else None)
        del keep
        if rc:
            self._raise(rc)
        return (pred, ps, stats) if want_stats else (pred, ps)

    # -- device pointers (torch tensors' data_ptr()) -----------------------------------------------
    def run_device(self, prob, out_pred_ptr, out_ps_ptr, stream=0):
        rc = self.lib.duet_ef_run_device(self.handle, ctypes.byref(prob), ctypes.c_void_p(out_pred_ptr),
                                         ctypes.c_void_p(out_ps_ptr), ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)

    def check(self, stream=0):
        rc = self.lib.duet_ef_check(self.handle, ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)

    def profile_collect(self):
        st = EfStats()
        rc = self.lib.duet_ef_profile_collect(self.handle, ctypes.byref(st))
        if rc:
            self._raise(rc)
        return st

    # -- stage A0: span-position clustering ---------------------------------------------------------
    def ef_rows_host(self, soa, rows, svlen_thres, suppread_thres):
        """duet_ef_rows_run_host: host arrays in (an EfSoA and NativeIngest.rows()), the text of the data rows out.
        -> (bytes, number of rows)"""
        p, keep = problem_from_arrays(soa, svlen_thres, suppread_thres)
        pool = np.ascontiguousarray(rows['pool'], dtype=np.uint8)
        str_off = np.ascontiguousarray(rows['str_off'], dtype=np.uint32)
        rank = np.ascontiguousarray(rows['chrom_rank'], dtype=np.uint16)
        plus = np.ascontiguousarray(rows['plus'], dtype=np.uint8)
        r = RowsProblem()
        r.n_contigs, r.n_cands = soa.n_contigs, soa.n_cands
        r.n_chrom_texts, r.max_pos = int(rows['n_chrom_texts']), int(rows['max_pos'])
        r.pool, r.pool_bytes, r.str_off = pool.ctypes.data, int(rows['pool_bytes']), str_off.ctypes.data
        r.cand_chrom_rank, r.cand_plus = rank.ctypes.data, plus.ctypes.data
        cap = int(rows['pool_bytes']) + 96 * soa.n_cands + 64
        out = np.empty(cap, dtype=np.uint8)
        n = ctypes.c_uint64(0)
        n_rows = ctypes.c_uint32(0)
        rc = self.lib.duet_ef_rows_run_host(self.handle, ctypes.byref(p), ctypes.byref(r), out.ctypes.data, ctypes.c_uint64(cap),
                                            ctypes.byref(n), ctypes.byref(n_rows))
        del keep
        if rc:
            self._raise(rc)
        return out[:n.value].tobytes(), n_rows.value

    def rows_device(self, prob, out_ptr, cap, stream):
        """duet_rows_run_device: -> (bytes written, rows)."""
        n = ctypes.c_uint64(0)
        rows = ctypes.c_uint32(0)
        rc = self.lib.duet_rows_run_device(self.handle, ctypes.byref(prob), ctypes.c_void_p(out_ptr), ctypes.c_uint64(cap),
                                           ctypes.byref(n), ctypes.byref(rows), ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)
        return n.value, rows.value

    def cluster_host(self, contig, mtype, pos, span, max_dist=0.9, part_gap=1000, part_max=100, normalizer=900.0,
                     hints=True):
        """Cluster SV marks (host numpy arrays) into candidates on the GPU.
        -> dict(order, cand_off, cand_contig, cand_type, cand_pos, cand_span) trimmed to the candidate count."""
        contig = np.ascontiguousarray(contig, dtype=np.uint16)
        mtype = np.ascontiguousarray(mtype, dtype=np.uint8)
        pos = np.ascontiguousarray(pos, dtype=np.uint32)
        span = np.ascontiguousarray(span, dtype=np.uint32)
        prob = ClusterProblem()
        M = fill_cluster_problem(prob, contig, mtype, pos, span, max_dist, part_gap, part_max, normalizer, hints)
        prob.mark_contig, prob.mark_type, prob.mark_pos, prob.mark_span = [
            a.ctypes.data if a.size else None for a in (contig, mtype, pos, span)]
        out = dict(order=np.zeros(max(M, 1), dtype=np.uint32), cand_off=np.zeros(M + 1, dtype=np.uint32),
                   cand_contig=np.zeros(max(M, 1), dtype=np.uint16), cand_type=np.zeros(max(M, 1), dtype=np.uint8),
                   cand_pos=np.zeros(max(M, 1), dtype=np.uint32), cand_span=np.zeros(max(M, 1), dtype=np.uint32))
        n = ctypes.c_uint32(0)
        res = bind_cluster_result(out, n)
        rc = self.lib.duet_cluster_run_host(self.handle, ctypes.byref(prob), ctypes.byref(res))
        if rc:
            self._raise(rc)
        N = n.value
        return dict(order=out['order'][:M], cand_off=out['cand_off'][:N + 1], cand_contig=out['cand_contig'][:N],
                    cand_type=out['cand_type'][:N], cand_pos=out['cand_pos'][:N], cand_span=out['cand_span'][:N])

    def _svim_host_problem(self, marks, read_tag, depth, depth_off, depth_bin, svlen_thres, suppread_thres, max_dist, part_gap,
                           part_max, normalizer, want_order):
        """-> (SvimProblem, ClusterResult, result arrays, order or None, n_cands word, keepalive) over host arrays."""
        arr = {k: np.ascontiguousarray(marks[k], dtype=dt) for k, dt in (('contig', np.uint16), ('type', np.uint8), ('pos', np.uint32),
                                                                        ('span', np.uint32), ('read', np.uint32))}
        read_tag = np.ascontiguousarray(read_tag, dtype=np.uint64)
        depth = np.ascontiguousarray(depth, dtype=np.uint32)
        depth_off = np.ascontiguousarray(depth_off, dtype=np.uint32)
        p = SvimProblem()
        M = fill_cluster_problem(p.marks, arr['contig'], arr['type'], arr['pos'], arr['span'], max_dist, part_gap, part_max, normalizer)
        p.marks.mark_contig, p.marks.mark_type = arr['contig'].ctypes.data, arr['type'].ctypes.data
        p.marks.mark_pos, p.marks.mark_span = arr['pos'].ctypes.data, arr['span'].ctypes.data
        p.mark_read = arr['read'].ctypes.data
        p.read_tag = read_tag.ctypes.data if read_tag.size else None
        p.n_reads, p.n_contigs = len(read_tag), len(depth_off) - 1
        p.depth = depth.ctypes.data if depth.size else None
        p.depth_off = depth_off.ctypes.data
        p.depth_bin, p.svlen_thres, p.suppread_thres = int(depth_bin), int(svlen_thres), int(suppread_thres)
        out = dict(cand_off=np.zeros(M + 1, dtype=np.uint32), cand_contig=np.zeros(max(M, 1), dtype=np.uint16),
                   cand_type=np.zeros(max(M, 1), dtype=np.uint8), cand_pos=np.zeros(max(M, 1), dtype=np.uint32),
                   cand_span=np.zeros(max(M, 1), dtype=np.uint32))
        n = ctypes.c_uint32(0)
        order = np.zeros(max(M, 1), dtype=np.uint32) if want_order else None
        res = bind_cluster_result(dict(out, order=order), n)
        return p, res, out, order, n, (arr, read_tag, depth, depth_off)

    @staticmethod
    def _svim_trim(out, N):
        return dict(cand_off=out['cand_off'][:N + 1], cand_contig=out['cand_contig'][:N], cand_type=out['cand_type'][:N],
                    cand_pos=out['cand_pos'][:N], cand_span=out['cand_span'][:N])

    def svim_host(self, marks, read_tag, depth, depth_off, depth_bin, svlen_thres, suppread_thres, max_dist=0.9, part_gap=1000,
                  part_max=100, normalizer=900.0, want_order=False):
        """The fused SVIM-mode pipeline on host arrays (duet_svim_phase_host): raw marks dict(contig, type, pos, span, read) ->
        dict(cand_off, cand_contig, cand_type, cand_pos, cand_span, pred, ps) trimmed to the candidate count (want_order: and
        the cluster order, order u32[M])."""
        p, res, out, order, n, keep = self._svim_host_problem(marks, read_tag, depth, depth_off, depth_bin, svlen_thres, suppread_thres,
                                                              max_dist, part_gap, part_max, normalizer, want_order)
        M = p.marks.n_marks
        pred, ps = np.zeros(max(M, 1), dtype=np.uint8), np.zeros(max(M, 1), dtype=np.uint32)
        rc = self.lib.duet_svim_phase_host(self.handle, ctypes.byref(p), ctypes.byref(res), _ptr(pred), _ptr(ps))
        del keep
        if rc:
            self._raise(rc)
        N = n.value
        got = dict(self._svim_trim(out, N), pred=pred[:N], ps=ps[:N])
        if want_order:
            got['order'] = order[:M]
        return got

    def svim_features_host(self, marks, read_tag, depth, depth_off, depth_bin, svlen_thres, suppread_thres, max_dist=0.9,
                           part_gap=1000, part_max=100, normalizer=900.0, pc_cap=None):
        """duet_svim_features_host: like svim_host, with the candidates' features (FEATURE_DTYPE[N]) in place of pred / ps.
        pc_cap: duet_svim_features_cap_host with that PC cap."""
        cap = check_pc_cap(pc_cap)
        p, res, out, _, n, keep = self._svim_host_problem(marks, read_tag, depth, depth_off, depth_bin, svlen_thres, suppread_thres,
                                                          max_dist, part_gap, part_max, normalizer, False)
        feat = np.zeros(max(p.marks.n_marks, 1), dtype=FEATURE_DTYPE)
        if cap is None:
            rc = self.lib.duet_svim_features_host(self.handle, ctypes.byref(p), ctypes.byref(res), _ptr(feat))
        else:
            rc = self.lib.duet_svim_features_cap_host(self.handle, ctypes.byref(p), ctypes.byref(res), cap, _ptr(feat))
        del keep
        if rc:
            self._raise(rc)
        return dict(self._svim_trim(out, n.value), feat=feat[:n.value])

    def svim_vcf_rows_device(self, sv_problem, result, n_cands, names, out_ptr, cap, stream):
        """duet_svim_vcf_rows_device on resident arrays (DeviceSvim.vcf_rows) -> bytes written."""
        n = ctypes.c_uint64(0)
        rc = self.lib.duet_svim_vcf_rows_device(self.handle, ctypes.byref(sv_problem), ctypes.byref(result), int(n_cands),
                                                ctypes.byref(names), ctypes.c_void_p(out_ptr), ctypes.c_uint64(cap), ctypes.byref(n),
                                                ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)
        return n.value

    def svim_vcf_rows_host(self, res, n_marks, mark_name, name_off, name_pool, depth, depth_off, depth_bin, chrom_texts):
        """duet_svim_vcf_rows_host: the rows of sv_calling/variants.vcf for a cluster result (host arrays: order, cand_off,
        cand_contig, cand_type, cand_pos, cand_span), the raw marks' names and the binned depth -> bytes."""
        N = len(res['cand_pos'])
        if N == 0:
            return b''
        arr = {k: np.ascontiguousarray(res[k], dtype=dt) for k, dt in (
            ('order', np.uint32), ('cand_off', np.uint32), ('cand_contig', np.uint16), ('cand_type', np.uint8),
            ('cand_pos', np.uint32), ('cand_span', np.uint32))}
        r = bind_cluster_result(arr)
        depth = np.ascontiguousarray(depth, dtype=np.uint32)
        depth_off = np.ascontiguousarray(depth_off, dtype=np.uint32)
        p = SvimProblem()
        p.marks.n_marks = int(n_marks)
        p.n_contigs = len(depth_off) - 1
        p.depth = depth.ctypes.data if depth.size else None
        p.depth_off = depth_off.ctypes.data
        p.depth_bin = int(depth_bin)
        keep = []
        name_off = np.ascontiguousarray(name_off, dtype=np.uint64)
        nm = callset_names(np.ascontiguousarray(mark_name, dtype=np.uint32), name_off,
                           np.ascontiguousarray(name_pool, dtype=np.uint8), chrom_texts, keep)
        nm.n_names = len(name_off) - 1
        cap = callset_bound(N, n_marks, name_off, chrom_texts)
        out = np.empty(cap, dtype=np.uint8)
        n = ctypes.c_uint64(0)
        rc = self.lib.duet_svim_vcf_rows_host(self.handle, ctypes.byref(p), ctypes.byref(r), N, ctypes.byref(nm), out.ctypes.data,
                                              ctypes.c_uint64(cap), ctypes.byref(n))
        if rc:
            self._raise(rc)
        return out[:n.value].tobytes()

    def svim_phased_rows_device(self, result, n_cands, pred_ptr, ps_ptr, chrom_texts, out_ptr, cap, stream):
        """duet_svim_phased_rows_device on resident arrays (DeviceSvim.phased_rows) -> (bytes written, rows)."""
        texts = chrom_bytes(chrom_texts)
        arr = (ctypes.c_char_p * max(len(texts), 1))(*texts)
        n, rows = ctypes.c_uint64(0), ctypes.c_uint32(0)
        rc = self.lib.duet_svim_phased_rows_device(self.handle, ctypes.byref(result), int(n_cands), ctypes.c_void_p(pred_ptr),
                                                   ctypes.c_void_p(ps_ptr), len(texts), arr, ctypes.c_void_p(out_ptr),
                                                   ctypes.c_uint64(cap), ctypes.byref(n), ctypes.byref(rows), ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)
        return n.value, rows.value

    def svim_phased_rows_host(self, res, chrom_texts):
        """duet_svim_phased_rows_host: the rows of phased_sv.vcf for host arrays (dict: cand_contig, cand_type, cand_pos, cand_span,
        pred, ps -- e.g. the merged records of a sharded run) -> (bytes, rows)."""
        arr = {k: np.ascontiguousarray(res[k], dtype=dt) for k, dt in (
            ('cand_contig', np.uint16), ('cand_type', np.uint8), ('cand_pos', np.uint32), ('cand_span', np.uint32),
            ('pred', np.uint8), ('ps', np.uint32))}
        N = len(arr['pred'])
        r = bind_cluster_result({k: arr[k] for k in ('cand_contig', 'cand_type', 'cand_pos', 'cand_span')})
        texts = chrom_bytes(chrom_texts)
        chrom = (ctypes.c_char_p * max(len(texts), 1))(*texts)
        cap = phased_rows_bound(int(np.count_nonzero(arr['pred'])), texts)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        n, rows = ctypes.c_uint64(0), ctypes.c_uint32(0)
        rc = self.lib.duet_svim_phased_rows_host(self.handle, ctypes.byref(r), N, _ptr(arr['pred']), _ptr(arr['ps']), len(texts), chrom,
                                                 out.ctypes.data, ctypes.c_uint64(cap), ctypes.byref(n), ctypes.byref(rows))
        if rc:
            self._raise(rc)
        return out[:n.value].tobytes(), rows.value

    def eval_counts(self, arrays, refdist, ratio):
        """duet_eval_run_host: `arrays` = dict of the flat host arrays (duet_amd/evaluation.py: flatten) -> EvalCounts."""
        p, keep = eval_problem(arrays, refdist, ratio)
        out = EvalCounts()
        rc = self.lib.duet_eval_run_host(self.handle, ctypes.byref(p), ctypes.byref(out))
        del keep
        if rc:
            self._raise(rc)
        return out

    def eval_details_host(self, problem):
        """duet_eval_details_host: `problem` = the flat host arrays of evaluation.flatten with 'refdist' and 'ratio' beside them
        -> (EvalCounts, calls EVAL_CALL_DTYPE[n_calls], base EVAL_BASE_DTYPE[n_base])."""
        p, keep = eval_problem(problem, problem['refdist'], problem['ratio'])
        counts = EvalCounts()
        calls = np.zeros(p.n_calls, dtype=EVAL_CALL_DTYPE)
        base = np.zeros(p.n_base, dtype=EVAL_BASE_DTYPE)
        rc = self.lib.duet_eval_details_host(self.handle, ctypes.byref(p), ctypes.byref(counts), calls.ctypes.data if p.n_calls else None,
                                             base.ctypes.data if p.n_base else None)
        del keep
        if rc:
            self._raise(rc)
        return counts, calls, base

    def features_host(self, soa, svlen_thres, suppread_thres, pc_cap=None):
        """duet_ef_features_host -> structured array of FEATURE_DTYPE[C].  Raises ZeroDivisionError where E/F would.
        pc_cap: duet_ef_features_cap_host with that PC cap (None: the reference's 8100 through the entry above)."""
        cap = check_pc_cap(pc_cap)
        prob, keep = problem_from_arrays(soa, svlen_thres, suppread_thres)
        out = np.zeros(soa.n_cands, dtype=FEATURE_DTYPE)
        if cap is None:
            rc = self.lib.duet_ef_features_host(self.handle, ctypes.byref(prob), _ptr(out))
        else:
            rc = self.lib.duet_ef_features_cap_host(self.handle, ctypes.byref(prob), cap, _ptr(out))
        del keep
        if rc:
            self._raise(rc)
        return out

    def sweep_host(self, feat, vectors, truth=None, want_pred=False, want_ps=False):
        """duet_tune_sweep_host: feat FEATURE_DTYPE[C], vectors float64[K, 14], truth = dict of the prepared arrays
        (duet_amd/tune.py: prepare_truth) or None -> (counts COUNTS_DTYPE[K], pred u8[K, C] or None, ps u32[C] or None)"""
        feat = np.ascontiguousarray(feat, dtype=FEATURE_DTYPE)
        vec = np.ascontiguousarray(vectors, dtype=np.float64).reshape(-1, len(TUNE_NAMES))
        C, K = len(feat), len(vec)
        counts = np.zeros(K, dtype=COUNTS_DTYPE)
        pred = np.zeros((K, C), dtype=np.uint8) if want_pred else None
        ps = np.zeros(C, dtype=np.uint32) if want_ps else None
        t, keep = None, []
        if truth is not None:
            t = TuneTruth()
            t.n_uid, t.n_groups, t.n_pairs = int(truth['n_uid']), int(truth['n_groups']), int(truth['n_pairs'])
            for name, dt in (('cand_flags', np.uint16), ('cand_group', np.uint32), ('cand_uid', np.uint32), ('cand_pair', np.uint32),
                             ('group_pair_off', np.uint32), ('pair_uid', np.uint32)):
                a = np.ascontiguousarray(truth[name], dtype=dt)
                keep.append(a)
                setattr(t, name, a.ctypes.data if a.size else None)
        rc = self.lib.duet_tune_sweep_host(self.handle, _ptr(feat), C, _ptr(vec), K, ctypes.byref(t) if t is not None else None,
                                           _ptr(counts), _ptr(pred), _ptr(ps))
        del keep
        if rc:
            self._raise(rc)
        return counts, pred, ps

    def truth_build_host(self, feat, arrays, refdist, ratio):
        """duet_tune_truth_build_host: feat FEATURE_DTYPE[C]; arrays = dict of the host arrays of a TuneTruthProblem (cand_pos,
        cand_len, then cand_key + cand_chrom or cand_contig + cand_type + key_table + chrom_id [+ bed_off, bed_lo, bed_hi]; the truth
        side base_off, base_pos, base_len, base_uid, base_hp) and the words n_base_uid, n_chrom
        -> dict of the six truth arrays trimmed to their sizes, n_uid, n_groups, n_pairs (what tune.prepare_truth returns)."""
        feat = np.ascontiguousarray(feat, dtype=FEATURE_DTYPE)
        C = len(feat)
        p, keep = TuneTruthProblem(), [feat]
        p.feat = feat.ctypes.data if C else None
        for name, dt in TRUTH_PROBLEM_ARRAYS:
            if arrays.get(name) is None:
                continue
            a = np.ascontiguousarray(arrays[name], dtype=dt)
            keep.append(a)
            setattr(p, name, a.ctypes.data if a.size else None)
        p.n_cands, p.n_keys, p.n_base = C, len(arrays['base_off']) - 1, len(arrays['base_pos'])
        p.n_base_uid, p.n_chrom = int(arrays['n_base_uid']), int(arrays['n_chrom'])
        p.n_contigs = len(arrays['chrom_id']) if arrays.get('chrom_id') is not None else 0
        p.refdist, p.ratio = clamp_u32(refdist), float(ratio)
        out = {name: np.zeros(C + (1 if name == 'group_pair_off' else 0), dtype=dt) for name, dt in TRUTH_ARRAYS}
        t = TuneTruth()
        for name, _ in TRUTH_ARRAYS:
            setattr(t, name, out[name].ctypes.data if out[name].size else None)
        rc = self.lib.duet_tune_truth_build_host(self.handle, ctypes.byref(p), ctypes.byref(t))
        del keep
        if rc:
            self._raise(rc)
        out['group_pair_off'] = out['group_pair_off'][:t.n_groups + 1]
        out['pair_uid'] = out['pair_uid'][:t.n_pairs]
        out.update(n_uid=t.n_uid, n_groups=t.n_groups, n_pairs=t.n_pairs)
        return out

    def strata_build_host(self, arrays, truth, chrom_stratum, n_strata):
        """duet_tune_strata_build_host: arrays = the CHROM ids of a TuneTruthProblem's candidates (cand_chrom, or cand_contig +
        chrom_id) and n_chrom; truth = the truth arrays of the same candidates (cand_flags, cand_group, n_groups); chrom_stratum
        u8[n_chrom] -> (cand_stratum u8[C], group_stratum u8[n_groups])"""
        flags = np.ascontiguousarray(truth['cand_flags'], dtype=np.uint16)
        group = np.ascontiguousarray(truth['cand_group'], dtype=np.uint32)
        C = len(flags)
        p, keep = TuneTruthProblem(), []
        for name, dt in (('cand_chrom', np.uint32), ('cand_contig', np.uint16), ('chrom_id', np.uint32)):
            if arrays.get(name) is None:
                continue
            a = np.ascontiguousarray(arrays[name], dtype=dt)
            keep.append(a)
            setattr(p, name, a.ctypes.data if a.size else None)
        p.n_cands, p.n_chrom = C, int(arrays['n_chrom'])
        p.n_contigs = len(arrays['chrom_id']) if arrays.get('chrom_id') is not None else 0
        t = TuneTruth()
        t.n_groups = int(truth['n_groups'])
        t.cand_flags, t.cand_group = (a.ctypes.data if C else None for a in (flags, group))
        cs = np.ascontiguousarray(chrom_stratum, dtype=np.uint8)
        assert len(cs) >= p.n_chrom or C == 0, 'chrom_stratum holds one entry per CHROM id'
        cand, grp = np.zeros(C, dtype=np.uint8), np.zeros(C, dtype=np.uint8)
        rc = self.lib.duet_tune_strata_build_host(self.handle, ctypes.byref(p), ctypes.byref(t), _ptr(cs), int(n_strata), _ptr(cand),
                                                  _ptr(grp))
        del keep
        if rc:
            self._raise(rc)
        return cand, grp[:t.n_groups].copy()

    def sweep_strata_host(self, feat, vectors, truth, strata):
        """duet_tune_sweep_strata_host: feat, vectors, truth as for sweep_host; strata = dict(n_strata, cand_stratum u8[C],
        group_stratum u8[n_groups], uid_off u32[S + 1]) -> counts COUNTS_DTYPE[K, S]"""
        feat = np.ascontiguousarray(feat, dtype=FEATURE_DTYPE)
        vec = np.ascontiguousarray(vectors, dtype=np.float64).reshape(-1, len(TUNE_NAMES))
        C, K, S = len(feat), len(vec), int(strata['n_strata'])
        t, keep = TuneTruth(), []
        t.n_uid, t.n_groups, t.n_pairs = int(truth['n_uid']), int(truth['n_groups']), int(truth['n_pairs'])
        for name, dt in TRUTH_ARRAYS:
            a = np.ascontiguousarray(truth[name], dtype=dt)
            keep.append(a)
            setattr(t, name, a.ctypes.data if a.size else None)
        st = TuneStrata()
        st.n_strata = S if 0 <= S <= 0xFFFFFFFF else 0xFFFFFFFF
        for name, dt in (('cand_stratum', np.uint8), ('group_stratum', np.uint8), ('uid_off', np.uint32)):
            a = np.ascontiguousarray(strata[name], dtype=dt)
            keep.append(a)
            setattr(st, name, a.ctypes.data if a.size else None)
        assert not 1 <= S <= TUNE_MAX_STRATA or len(keep[-1]) == S + 1, 'uid_off holds n_strata + 1 entries'
        counts = np.zeros((K, S if 1 <= S <= TUNE_MAX_STRATA else 1), dtype=COUNTS_DTYPE)
        rc = self.lib.duet_tune_sweep_strata_host(self.handle, _ptr(feat), C, _ptr(vec), K, ctypes.byref(t), ctypes.byref(st),
                                                  _ptr(counts))
        del keep
        if rc:
            self._raise(rc)
        return counts

    def leaf_census_host(self, feat, vectors, truth=None, strata=None):
        """duet_tune_leaf_census_host: feat, vectors, truth (or None) as for sweep_host; strata = dict(n_strata, cand_stratum
        u8[C]) or None (S = 1) -> LEAF_COUNTS_DTYPE[K, S, N_LEAVES]"""
        feat = np.ascontiguousarray(feat, dtype=FEATURE_DTYPE)
        vec = np.ascontiguousarray(vectors, dtype=np.float64).reshape(-1, len(TUNE_NAMES))
        C, K = len(feat), len(vec)
        t, st, keep = None, None, []
        if truth is not None:
            t = TuneTruth()
            t.n_uid, t.n_groups, t.n_pairs = int(truth['n_uid']), int(truth['n_groups']), int(truth['n_pairs'])
            for name, dt in TRUTH_ARRAYS:
                a = np.ascontiguousarray(truth[name], dtype=dt)
                keep.append(a)
                setattr(t, name, a.ctypes.data if a.size else None)
        S = 1
        if strata is not None:
            S = int(strata['n_strata'])
            st = TuneStrata()
            st.n_strata = S if 0 <= S <= 0xFFFFFFFF else 0xFFFFFFFF
            a = np.ascontiguousarray(strata['cand_stratum'], dtype=np.uint8)
            assert len(a) == C, 'cand_stratum holds one entry per candidate'
            keep.append(a)
            st.cand_stratum = a.ctypes.data if a.size else None
        out = np.zeros((K, S if 1 <= S <= TUNE_MAX_STRATA else 1, N_LEAVES), dtype=LEAF_COUNTS_DTYPE)
        rc = self.lib.duet_tune_leaf_census_host(self.handle, _ptr(feat), C, _ptr(vec), K, ctypes.byref(t) if t is not None else None,
                                                 ctypes.byref(st) if st is not None else None, _ptr(out))
        del keep
        if rc:
            self._raise(rc)
        return out

    def leaf_census_device(self, feat_ptr, n_cands, vec_ptr, n_vec, truth, strata, out_ptr, stream=0):
        """duet_tune_leaf_census_device on resident arrays (devmem.DeviceTune.leaf_census); truth / strata: the structures or None."""
        rc = self.lib.duet_tune_leaf_census_device(self.handle, ctypes.c_void_p(feat_ptr), int(n_cands), ctypes.c_void_p(vec_ptr),
                                                   int(n_vec), ctypes.byref(truth) if truth is not None else None,
                                                   ctypes.byref(strata) if strata is not None else None, ctypes.c_void_p(out_ptr),
                                                   ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)

    # -- the evidence table (duet_evidence.hip) ---------------------------------------------------------------------------------
    def leaves_host(self, feat, vector):
        """duet_tune_leaves_host: feat FEATURE_DTYPE[C], one vector float64[14] -> (leaf u8[C], pred u8[C]): 0 .. 17, LEAF_NO_SEED,
        LEAF_FILTERED, and the pred sweep_host returns for that vector."""
        feat = np.ascontiguousarray(feat, dtype=FEATURE_DTYPE)
        vec = np.ascontiguousarray(vector, dtype=np.float64).reshape(len(TUNE_NAMES))
        leaf, pred = np.zeros(len(feat), dtype=np.uint8), np.zeros(len(feat), dtype=np.uint8)
        rc = self.lib.duet_tune_leaves_host(self.handle, _ptr(feat), len(feat), _ptr(vec), _ptr(leaf), _ptr(pred))
        if rc:
            self._raise(rc)
        return leaf, pred

    def leaves_device(self, feat_ptr, n_cands, vector, leaf_ptr, pred_ptr, stream=0):
        """duet_tune_leaves_device on resident arrays; the vector (float64[14]) is host memory."""
        vec = np.ascontiguousarray(vector, dtype=np.float64).reshape(len(TUNE_NAMES))
        rc = self.lib.duet_tune_leaves_device(self.handle, ctypes.c_void_p(feat_ptr), int(n_cands), _ptr(vec), ctypes.c_void_p(leaf_ptr),
                                              ctypes.c_void_p(pred_ptr), ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)

    def evidence_rows_host(self, feat, leaf, pred, cand_pos, cand_svlen, rows=None, cand_contig=None, cand_type=None, chrom_texts=None):
        """duet_evidence_rows_host: the data rows of the evidence table (EVIDENCE_COLUMNS) for host arrays -> bytes.
        Text form: rows = dict(pool, str_off, pool_bytes) as NativeIngest.rows() gives it.  Table form: cand_contig u16[C],
        cand_type u8[C] (0 .. 3 = DEL, INS, INV, DUP) and chrom_texts, the CHROM text per contig."""
        feat = np.ascontiguousarray(feat, dtype=FEATURE_DTYPE)
        C = len(feat)
        arr = [np.ascontiguousarray(a, dtype=dt) for a, dt in ((leaf, np.uint8), (pred, np.uint8), (cand_pos, np.uint32),
                                                               (cand_svlen, np.uint32))]
        for a in arr:
            assert len(a) == C, 'one entry per candidate'
        p = EvidenceProblem()
        p.n_cands = C
        p.feat = feat.ctypes.data if C else None
        p.leaf, p.pred, p.cand_pos, p.cand_svlen = [a.ctypes.data if C else None for a in arr]
        keep = [feat, arr]
        if rows is not None:
            pool = np.ascontiguousarray(rows['pool'], dtype=np.uint8)
            str_off = np.ascontiguousarray(rows['str_off'], dtype=np.uint32)
            assert len(str_off) >= 4 * C + 1, 'str_off holds 4 C + 1 offsets'
            p.pool_bytes = int(rows.get('pool_bytes', len(pool)))
            if len(pool) == 0:
                pool = np.zeros(1, dtype=np.uint8)          # (an empty pool is still the text form: a readable address)
            p.pool, p.str_off = pool.ctypes.data, str_off.ctypes.data
            keep += [pool, str_off]
            d = np.diff(str_off[:4 * C + 1].astype(np.int64)) if C else np.zeros(0, dtype=np.int64)
            cap = evidence_bound(C, max(int(d[0::4].max()), 0) if C else 0, max(int(d[3::4].max()), 0) if C else 0)
        else:
            contig = np.ascontiguousarray(cand_contig, dtype=np.uint16)
            ctype = np.ascontiguousarray(cand_type, dtype=np.uint8)
            assert len(contig) == C and len(ctype) == C, 'one entry per candidate'
            texts = [None if c is None else (c if isinstance(c, bytes) else c.encode()) for c in chrom_texts]
            chrom = (ctypes.c_char_p * max(len(texts), 1))(*texts)
            p.n_contigs = len(texts)
            p.cand_contig, p.cand_type = (a.ctypes.data if C else None for a in (contig, ctype))
            p.chrom = chrom
            keep += [contig, ctype, chrom]
            cap = evidence_bound(C, max([len(c) for c in texts if c is not None] + [0]))
        out = np.empty(max(cap, 1), dtype=np.uint8)
        n = ctypes.c_uint64(0)
        rc = self.lib.duet_evidence_rows_host(self.handle, ctypes.byref(p), out.ctypes.data, ctypes.c_uint64(cap), ctypes.byref(n))
        del keep
        if rc:
            self._raise(rc)
        return out[:n.value].tobytes()

    def evidence_rows_device(self, prob, out_ptr, cap, stream=0):
        """duet_evidence_rows_device on resident arrays (an EvidenceProblem of device pointers) -> the text's exact size; raises
        when cap is smaller (nothing is written then)."""
        n = ctypes.c_uint64(0)
        rc = self.lib.duet_evidence_rows_device(self.handle, ctypes.byref(prob), ctypes.c_void_p(out_ptr), ctypes.c_uint64(cap),
                                                ctypes.byref(n), ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)
        return n.value

    # -- phase-set links (duet_pslinks.hip) -------------------------------------------------------------------------------------
    def ps_links_host(self, soa, svlen_thres, suppread_thres, pc_cap=None):
        """duet_ps_links_host: the links of an EfSoA -> structured array of PS_LINK_DTYPE, ascending by (contig, ps_a, ps_b).
        pc_cap: the PC cap of the voters (None: the reference's 8100)."""
        cap = check_pc_cap(pc_cap)
        prob, keep = problem_from_arrays(soa, svlen_thres, suppread_thres)
        room = ps_links_room(soa.n_marks)
        out = np.zeros(room, dtype=PS_LINK_DTYPE)
        n = ctypes.c_uint32(0)
        rc = self.lib.duet_ps_links_host(self.handle, ctypes.byref(prob), PC_MAX if cap is None else cap, _ptr(out), room, ctypes.byref(n))
        del keep
        if rc:
            self._raise(rc)
        return out[:n.value].copy()

    def ps_links_device(self, prob, out_ptr, out_cap, stream=0, pc_cap=None):
        """duet_ps_links_device on a resident EfProblem (devmem.DeviceProblem.problem); out_ptr: device room for out_cap records
        -> the record count."""
        cap = check_pc_cap(pc_cap)
        n = ctypes.c_uint32(0)
        rc = self.lib.duet_ps_links_device(self.handle, ctypes.byref(prob), PC_MAX if cap is None else cap, ctypes.c_void_p(out_ptr),
                                           int(out_cap), ctypes.byref(n), ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)
        return n.value

    def svim_ps_links_device(self, sv_problem, result, out_ptr, out_cap, stream=0, pc_cap=None):
        """duet_svim_ps_links_device on a resident SvimProblem (devmem.DeviceSvim) -> (record count, candidate count)."""
        cap = check_pc_cap(pc_cap)
        n, n_cands = ctypes.c_uint32(0), ctypes.c_uint32(0)
        rc = self.lib.duet_svim_ps_links_device(self.handle, ctypes.byref(sv_problem), ctypes.byref(result), PC_MAX if cap is None else cap,
                                                ctypes.c_void_p(out_ptr), int(out_cap), ctypes.byref(n), ctypes.byref(n_cands),
                                                ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)
        return n.value, n_cands.value

    def svim_ps_links_host(self, marks, read_tag, depth, depth_off, depth_bin, svlen_thres, suppread_thres, max_dist=0.9, part_gap=1000,
                           part_max=100, normalizer=900.0, pc_cap=None, want_order=False):
        """duet_svim_ps_links_host: like svim_host, with the links (PS_LINK_DTYPE) of the clustered candidates in place of pred / ps
        -> dict(cluster arrays trimmed to the candidate count, links)."""
        cap = check_pc_cap(pc_cap)
        p, res, out, order, n, keep = self._svim_host_problem(marks, read_tag, depth, depth_off, depth_bin, svlen_thres, suppread_thres,
                                                              max_dist, part_gap, part_max, normalizer, want_order)
        room = ps_links_room(p.marks.n_marks)
        links = np.zeros(room, dtype=PS_LINK_DTYPE)
        n_links = ctypes.c_uint32(0)
        rc = self.lib.duet_svim_ps_links_host(self.handle, ctypes.byref(p), ctypes.byref(res), PC_MAX if cap is None else cap, _ptr(links),
                                              room, ctypes.byref(n_links))
        del keep
        if rc:
            self._raise(rc)
        got = dict(self._svim_trim(out, n.value), links=links[:n_links.value].copy())
        if want_order:
            got['order'] = order[:p.marks.n_marks]
        return got

    # -- read tags from phased SVs (duet_readtags.hip) ---------------------------------------------------------------------------
    def read_tags_host(self, cand_off, mark_read, mark_name, n_names, pred, ps, cand_pos, read_tag, cand_ctg_off=None, cand_contig=None,
                       mark_order=None, pc_cap=None, out_cap=None):
        """duet_read_tags_host over host arrays -> structured array of READ_TAG_DTYPE, ascending by (name, ps).  Exactly one of
        cand_ctg_off / cand_contig names the candidates' contigs; mark_order: the CSR slots' raw marks (None: identity); pc_cap: the
        PC cap of a usable tag (None: the reference's 8100); out_cap: the room offered (None: n_marks, which always suffices) --
        when it is too small the DuetLibraryError carries the exact count as `n_recs`."""
        conv = lambda a, dt: None if a is None else np.ascontiguousarray(a, dtype=dt)
        arrays = dict(cand_off=conv(cand_off, np.uint32), mark_order=conv(mark_order, np.uint32), mark_read=conv(mark_read, np.uint32),
                      mark_name=conv(mark_name, np.uint32), pred=conv(pred, np.uint8), ps=conv(ps, np.uint32),
                      cand_pos=conv(cand_pos, np.uint32), cand_ctg_off=conv(cand_ctg_off, np.uint32),
                      cand_contig=conv(cand_contig, np.uint16), read_tag=conv(read_tag, np.uint64))
        prob = ReadTagsProblem()
        prob.n_cands, prob.n_marks = len(arrays['pred']), len(arrays['mark_read'])
        prob.n_reads, prob.n_names = len(arrays['read_tag']), int(n_names)
        prob.n_contigs = len(arrays['cand_ctg_off']) - 1 if cand_ctg_off is not None else 0
        spare = np.zeros(1, dtype=np.uint64)
        for k, a in arrays.items():
            # (an empty array still has an address: which contig form is meant must not depend on the candidate count)
            setattr(prob, k, None if a is None else a.ctypes.data if a.size else spare.ctypes.data)
        room = prob.n_marks if out_cap is None else int(out_cap)
        out = np.zeros(max(room, 1), dtype=READ_TAG_DTYPE)
        n = ctypes.c_uint32(0)
        cap = PC_MAX if pc_cap is None else int(pc_cap)
        if not 0 <= cap <= 0xFFFFFFFF:
            raise ValueError('pc_cap: %r' % (pc_cap,))
        rc = self.lib.duet_read_tags_host(self.handle, ctypes.byref(prob), cap, _ptr(out), room, ctypes.byref(n))
        del arrays
        if rc:
            try:
                self._raise(rc)
            except DuetLibraryError as e:
                e.n_recs, e.out = n.value, out
                raise
        return out[:n.value].copy()

    def read_tags_device(self, prob, out_ptr, out_cap, stream=0, pc_cap=None):
        """duet_read_tags_device on a resident ReadTagsProblem (cand_ctg_off host memory); out_ptr: device room for out_cap records
        -> the record count."""
        n = ctypes.c_uint32(0)
        rc = self.lib.duet_read_tags_device(self.handle, ctypes.byref(prob), PC_MAX if pc_cap is None else int(pc_cap),
                                            ctypes.c_void_p(out_ptr), int(out_cap), ctypes.byref(n), ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)
        return n.value

    def read_tags_rows_host(self, records, name_off, name_pool, chrom_texts, read_tag, cap=None):
        """duet_read_tags_rows_host: the data rows of phased_sv.read_tags.tsv for `records` (READ_TAG_DTYPE) -> bytes.  name_off
        (uint64, n_names + 1) and name_pool (bytes or uint8 array): the read names; cap: the room offered (None: read_tags_bound) --
        when it is too small the DuetLibraryError carries the exact size as `out_len`."""
        records = np.ascontiguousarray(records, dtype=READ_TAG_DTYPE)
        name_off = np.ascontiguousarray(name_off, dtype=np.uint64)
        pool = np.frombuffer(bytes(name_pool), dtype=np.uint8) if isinstance(name_pool, (bytes, bytearray)) else \
            np.ascontiguousarray(name_pool, dtype=np.uint8)
        pool = pool if pool.size else np.zeros(1, dtype=np.uint8)
        read_tag = np.ascontiguousarray(read_tag, dtype=np.uint64)
        keep = []
        names = callset_names(np.zeros(0, dtype=np.uint32), name_off, pool, chrom_texts, keep)
        names.n_names = max(len(name_off), 1) - 1
        room = read_tags_bound(len(records), name_off, chrom_texts) if cap is None else int(cap)
        out = np.zeros(max(room, 1), dtype=np.uint8)
        n = ctypes.c_uint64(0)
        rc = self.lib.duet_read_tags_rows_host(self.handle, _ptr(records), len(records), ctypes.byref(names), _ptr(read_tag), len(read_tag),
                                               _ptr(out), ctypes.c_uint64(room), ctypes.byref(n))
        del keep
        if rc:
            try:
                self._raise(rc)
            except DuetLibraryError as e:
                e.out_len, e.out = n.value, out
                raise
        return out[:n.value].tobytes()

    def read_tags_rows_device(self, recs_ptr, n_recs, names, read_tag_ptr, n_reads, out_ptr, cap, stream=0):
        """duet_read_tags_rows_device on resident arrays (names: a CallsetNames of device pointers, chrom host) -> the text's exact
        size; raises when cap is smaller (nothing is written then)."""
        n = ctypes.c_uint64(0)
        rc = self.lib.duet_read_tags_rows_device(self.handle, ctypes.c_void_p(recs_ptr), int(n_recs), ctypes.byref(names),
                                                 ctypes.c_void_p(read_tag_ptr), int(n_reads), ctypes.c_void_p(out_ptr), ctypes.c_uint64(cap),
                                                 ctypes.byref(n), ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)
        return n.value

    # -- joined phase sets (duet_psjoin.hip) -------------------------------------------------------------------------------------
    @staticmethod
    def _ps_blocks(blocks):
        return np.ascontiguousarray(blocks, dtype=PS_BLOCK_DTYPE)

    def ps_join_tags_host(self, read_tag, read_off, blocks, out=None):
        """duet_ps_join_tags_host: the read tags (uint64) under the table `blocks` (PS_BLOCK_DTYPE; duet_amd/ps_join.py: table);
        read_off: the reads of contig k are read_off[k] .. read_off[k + 1].  out: the array written (None: a new one; read_tag itself
        is allowed) -> (out, n_changed)"""
        read_tag = np.ascontiguousarray(read_tag, dtype=np.uint64)
        read_off = np.ascontiguousarray(read_off, dtype=np.uint32)
        blocks = self._ps_blocks(blocks)
        if out is None:
            out = np.zeros(len(read_tag), dtype=np.uint64)
        n = ctypes.c_uint32(0)
        rc = self.lib.duet_ps_join_tags_host(self.handle, _ptr(read_tag), _ptr(read_off), max(len(read_off), 1) - 1, len(read_tag),
                                             _ptr(blocks), len(blocks), _ptr(out), ctypes.byref(n))
        if rc:
            self._raise(rc)
        return out, n.value

    def ps_join_tags_device(self, read_tag_ptr, read_off, n_reads, blocks, out_ptr, stream=0):
        """duet_ps_join_tags_device on resident tag words (read_off and blocks host arrays); out_ptr may be read_tag_ptr
        -> n_changed"""
        read_off = np.ascontiguousarray(read_off, dtype=np.uint32)
        blocks = self._ps_blocks(blocks)
        n = ctypes.c_uint32(0)
        rc = self.lib.duet_ps_join_tags_device(self.handle, ctypes.c_void_p(read_tag_ptr), _ptr(read_off), max(len(read_off), 1) - 1,
                                               int(n_reads), _ptr(blocks), len(blocks), ctypes.c_void_p(out_ptr), ctypes.byref(n),
                                               ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)
        return n.value

    def ps_join_diff_host(self, pred0, ps0, pred1, ps1, blocks, n_contigs, cand_ctg_off=None, cand_contig=None):
        """duet_ps_join_diff_host: the change code of every candidate between the calls (pred0, ps0) and (pred1, ps1) under the
        table `blocks`.  Exactly one of cand_ctg_off / cand_contig names the candidates' contigs -> (change u8[C], counts u32[8])"""
        conv = lambda a, dt: None if a is None else np.ascontiguousarray(a, dtype=dt)
        pred0, pred1, ps0, ps1 = conv(pred0, np.uint8), conv(pred1, np.uint8), conv(ps0, np.uint32), conv(ps1, np.uint32)
        off, col = conv(cand_ctg_off, np.uint32), conv(cand_contig, np.uint16)
        blocks = self._ps_blocks(blocks)
        C = len(pred0)
        change, counts = np.zeros(C, dtype=np.uint8), np.zeros(8, dtype=np.uint32)
        spare = np.zeros(1, dtype=np.uint64)
        # (an empty column still has an address: which contig form is meant must not depend on the candidate count)
        ptr = lambda a: None if a is None else a.ctypes.data if a.size else spare.ctypes.data
        rc = self.lib.duet_ps_join_diff_host(self.handle, C, ptr(pred0), ptr(ps0), ptr(pred1), ptr(ps1), ptr(off), ptr(col), int(n_contigs),
                                             _ptr(blocks), len(blocks), ptr(change), counts.ctypes.data)
        if rc:
            self._raise(rc)
        return change, counts

    def ps_join_diff_device(self, n_cands, pred0_ptr, ps0_ptr, pred1_ptr, ps1_ptr, blocks, n_contigs, change_ptr, cand_ctg_off=None,
                            cand_contig_ptr=None, stream=0):
        """duet_ps_join_diff_device on resident calls; cand_ctg_off a host array, or cand_contig_ptr the resident uint16 column;
        change_ptr: device room for n_cands bytes -> counts u32[8]"""
        off = None if cand_ctg_off is None else np.ascontiguousarray(cand_ctg_off, dtype=np.uint32)
        blocks = self._ps_blocks(blocks)
        counts = np.zeros(8, dtype=np.uint32)
        rc = self.lib.duet_ps_join_diff_device(self.handle, int(n_cands), ctypes.c_void_p(pred0_ptr), ctypes.c_void_p(ps0_ptr),
                                               ctypes.c_void_p(pred1_ptr), ctypes.c_void_p(ps1_ptr),
                                               None if off is None else off.ctypes.data,
                                               None if cand_contig_ptr is None else ctypes.c_void_p(cand_contig_ptr), int(n_contigs),
                                               _ptr(blocks), len(blocks), ctypes.c_void_p(change_ptr), counts.ctypes.data,
                                               ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)
        return counts

    # -- blocks of the phase-set links, on the device (duet_psblocks.hip) -------------------------------------------------------
    def ps_blocks_host(self, records, n_contigs, min_sv=1, rows=None, conflicts=None):
        """duet_ps_blocks_host: the table of ps_links.blocks(records, min_sv) from host records (PS_LINK_DTYPE)
        -> (rows PS_BLOCK_DTYPE, conflicts u32 in rank order, counts dict).  rows / conflicts: the arrays written (None: new ones
        with room for everything) -- a refused call leaves them as they were."""
        records = np.ascontiguousarray(records, dtype=PS_LINK_DTYPE)
        n = len(records)
        if rows is None:
            rows = np.zeros(2 * n, dtype=PS_BLOCK_DTYPE)
        if conflicts is None:
            conflicts = np.zeros(n, dtype=np.uint32)
        c = PsBlocksCounts()
        rc = self.lib.duet_ps_blocks_host(self.handle, _ptr(records), n, int(n_contigs), int(min_sv), _ptr(rows), len(rows),
                                          _ptr(conflicts), len(conflicts), ctypes.byref(c))
        if rc:
            self._raise(rc)
        return rows[:c.n_rows].copy(), conflicts[:c.n_conflicts].copy(), c.as_dict()

    def ps_blocks_device(self, links_ptr, n_links, n_contigs, min_sv, rows_ptr, rows_cap, conflicts_ptr=0, conflicts_cap=0, stream=0):
        """duet_ps_blocks_device on resident records (as ps_links_device left them); rows_ptr: device room for rows_cap rows
        (2 * n_links always suffice), conflicts_ptr: device room for conflicts_cap indices, or 0 -> counts dict."""
        c = PsBlocksCounts()
        rc = self.lib.duet_ps_blocks_device(self.handle, ctypes.c_void_p(links_ptr), int(n_links), int(n_contigs), int(min_sv),
                                            ctypes.c_void_p(rows_ptr), int(rows_cap), ctypes.c_void_p(conflicts_ptr), int(conflicts_cap),
                                            ctypes.byref(c), ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)
        return c.as_dict()

    def ps_join_links_device(self, links_ptr, n_links, min_sv, read_tag_ptr, read_off, n_reads, out_ptr, stream=0):
        """duet_ps_join_links_device: the table of the resident records built on the device and applied to the resident tag
        words (read_off a host array); out_ptr may be read_tag_ptr -> (n_changed, counts dict)."""
        read_off = np.ascontiguousarray(read_off, dtype=np.uint32)
        c, n = PsBlocksCounts(), ctypes.c_uint32(0)
        rc = self.lib.duet_ps_join_links_device(self.handle, ctypes.c_void_p(links_ptr), int(n_links), int(min_sv),
                                                ctypes.c_void_p(read_tag_ptr), _ptr(read_off), max(len(read_off), 1) - 1, int(n_reads),
                                                ctypes.c_void_p(out_ptr), ctypes.byref(c), ctypes.byref(n), ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)
        return n.value, c.as_dict()

    # -- tags from other SVs (duet_svtags.hip) -------------------------------------------------------------------------------------
    def sv_tags_host(self, cand_off, mark_read, mark_name, n_names, pred, ps, read_tag, cand_ctg_off=None, cand_contig=None,
                     mark_order=None, cand_pos=None, pc_cap=None, min_votes=1, pc_new=0, out_tag=None, out_index=None):
        """duet_sv_tags_host over host arrays (those of read_tags_host; cand_pos is not read) -> (out_tag u64[M], out_index u32[M],
        counts): one tag word per raw mark, the identity index of the second run, and (n_untagged, n_given, n_own_only).  out_tag /
        out_index: the arrays written (None: new ones, all-ones and zeros) -- a refused call leaves them as they were."""
        conv = lambda a, dt: None if a is None else np.ascontiguousarray(a, dtype=dt)
        arrays = dict(cand_off=conv(cand_off, np.uint32), mark_order=conv(mark_order, np.uint32), mark_read=conv(mark_read, np.uint32),
                      mark_name=conv(mark_name, np.uint32), pred=conv(pred, np.uint8), ps=conv(ps, np.uint32),
                      cand_pos=conv(cand_pos, np.uint32), cand_ctg_off=conv(cand_ctg_off, np.uint32),
                      cand_contig=conv(cand_contig, np.uint16), read_tag=conv(read_tag, np.uint64))
        prob = ReadTagsProblem()
        prob.n_cands, prob.n_marks = len(arrays['pred']), len(arrays['mark_read'])
        prob.n_reads, prob.n_names = len(arrays['read_tag']), int(n_names)
        prob.n_contigs = len(arrays['cand_ctg_off']) - 1 if cand_ctg_off is not None else 0
        spare = np.zeros(1, dtype=np.uint64)
        for k, a in arrays.items():
            # (an empty array still has an address: which contig form is meant must not depend on the candidate count)
            setattr(prob, k, None if a is None else a.ctypes.data if a.size else spare.ctypes.data)
        M = prob.n_marks
        if out_tag is None:
            out_tag = np.full(M, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        if out_index is None:
            out_index = np.zeros(M, dtype=np.uint32)
        assert out_tag.dtype == np.uint64 and out_index.dtype == np.uint32 and len(out_tag) == M and len(out_index) == M
        counts = np.zeros(3, dtype=np.uint32)
        args = [PC_MAX if pc_cap is None else pc_cap, min_votes, pc_new]
        if not all(0 <= int(x) <= 0xFFFFFFFF for x in args):
            raise ValueError('pc_cap, min_votes, pc_new: %r' % (args,))
        rc = self.lib.duet_sv_tags_host(self.handle, ctypes.byref(prob), int(args[0]), int(args[1]), int(args[2]),
                                        out_tag.ctypes.data if M else spare.ctypes.data, out_index.ctypes.data if M else spare.ctypes.data,
                                        counts.ctypes.data)
        del arrays
        if rc:
            self._raise(rc)
        return out_tag, out_index, tuple(int(x) for x in counts)

    def sv_tags_device(self, prob, out_tag_ptr, out_index_ptr, pc_cap=None, min_votes=1, pc_new=0, stream=0):
        """duet_sv_tags_device on a resident ReadTagsProblem (cand_ctg_off host memory); out_tag_ptr / out_index_ptr: device room for
        n_marks words of 8 / 4 bytes -> (n_untagged, n_given, n_own_only)"""
        counts = np.zeros(3, dtype=np.uint32)
        rc = self.lib.duet_sv_tags_device(self.handle, ctypes.byref(prob), PC_MAX if pc_cap is None else int(pc_cap), int(min_votes),
                                          int(pc_new), ctypes.c_void_p(out_tag_ptr), ctypes.c_void_p(out_index_ptr), counts.ctypes.data,
                                          ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)
        return tuple(int(x) for x in counts)

    # -- tags from other SVs, planned (duet_svtags_plan.hip) ------------------------------------------------------------------------
    def sv_tags_plan_host(self, cand_off, mark_read, mark_name, n_names, ps, read_tag, cand_mask=None, cand_ctg_off=None, cand_contig=None,
                          mark_order=None, cand_pos=None, pred=None, pc_cap=None, out_tag=None, out_index=None):
        """duet_sv_tags_plan_host over host arrays (those of sv_tags_host; pred and cand_pos are not read; cand_mask u8[C] or None =
        every candidate) -> (out_tag u64[M] the base words, out_index u32[M], info dict(n_untagged, n_records, n_runs,
        n_contributing)).  The plan stays on the context for sv_tags_apply_*.  out_tag / out_index: the arrays written (None: new
        ones) -- a refused call leaves them as they were."""
        conv = lambda a, dt: None if a is None else np.ascontiguousarray(a, dtype=dt)
        arrays = dict(cand_off=conv(cand_off, np.uint32), mark_order=conv(mark_order, np.uint32), mark_read=conv(mark_read, np.uint32),
                      mark_name=conv(mark_name, np.uint32), ps=conv(ps, np.uint32), cand_ctg_off=conv(cand_ctg_off, np.uint32),
                      cand_contig=conv(cand_contig, np.uint16), read_tag=conv(read_tag, np.uint64))
        mask = conv(cand_mask, np.uint8)
        prob = ReadTagsProblem()
        prob.n_cands, prob.n_marks = len(arrays['ps']), len(arrays['mark_read'])
        prob.n_reads, prob.n_names = len(arrays['read_tag']), int(n_names)
        prob.n_contigs = len(arrays['cand_ctg_off']) - 1 if cand_ctg_off is not None else 0
        assert mask is None or len(mask) == prob.n_cands
        spare = np.zeros(1, dtype=np.uint64)
        ptr = lambda a: None if a is None else a.ctypes.data if a.size else spare.ctypes.data
        for k, a in arrays.items():
            setattr(prob, k, ptr(a))
        M = prob.n_marks
        if out_tag is None:
            out_tag = np.full(M, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        if out_index is None:
            out_index = np.zeros(M, dtype=np.uint32)
        assert out_tag.dtype == np.uint64 and out_index.dtype == np.uint32 and len(out_tag) == M and len(out_index) == M
        cap = PC_MAX if pc_cap is None else int(pc_cap)
        if not 0 <= cap <= 0xFFFFFFFF:
            raise ValueError('pc_cap: %r' % (pc_cap,))
        info = SvTagsPlanInfo()
        rc = self.lib.duet_sv_tags_plan_host(self.handle, ctypes.byref(prob), ptr(mask), cap, ptr(out_tag), ptr(out_index),
                                             ctypes.byref(info))
        del arrays
        if rc:
            self._raise(rc)
        return out_tag, out_index, info.as_dict()

    def sv_tags_plan_device(self, prob, out_tag_ptr, out_index_ptr, cand_mask_ptr=None, pc_cap=None, stream=0):
        """duet_sv_tags_plan_device on a resident ReadTagsProblem (cand_ctg_off host memory; pred is not read); cand_mask_ptr:
        the resident u8[n_cands] mask, or None = every candidate; out_tag_ptr / out_index_ptr: device room for n_marks words of 8 /
        4 bytes -> info dict"""
        info = SvTagsPlanInfo()
        rc = self.lib.duet_sv_tags_plan_device(self.handle, ctypes.byref(prob), None if not cand_mask_ptr else ctypes.c_void_p(cand_mask_ptr),
                                               PC_MAX if pc_cap is None else int(pc_cap), ctypes.c_void_p(out_tag_ptr),
                                               ctypes.c_void_p(out_index_ptr), ctypes.byref(info), ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)
        return info.as_dict()

    def sv_tags_apply_host(self, pred, out_tag, min_votes=1, pc_new=0):
        """duet_sv_tags_apply_host: one vector's first-run calls on the context's plan; out_tag (u64[M], holding the plan's base
        words at the tagged marks) is written in place at the untagged marks -> (out_tag, counts u32[4]: n_untagged, n_given,
        n_own_only, and the candidates the plan cannot serve -- non-zero: the words are not to be used)"""
        pred = np.ascontiguousarray(pred, dtype=np.uint8)
        assert out_tag.dtype == np.uint64 and out_tag.flags['C_CONTIGUOUS']
        if not all(0 <= int(x) <= 0xFFFFFFFF for x in (min_votes, pc_new)):
            raise ValueError('min_votes, pc_new: %r' % ((min_votes, pc_new),))
        spare, counts = np.zeros(1, dtype=np.uint64), np.zeros(4, dtype=np.uint32)
        ptr = lambda a: a.ctypes.data if a.size else spare.ctypes.data
        rc = self.lib.duet_sv_tags_apply_host(self.handle, ptr(pred), int(min_votes), int(pc_new), ptr(out_tag), counts.ctypes.data)
        if rc:
            self._raise(rc)
        return out_tag, tuple(int(x) for x in counts)

    def sv_tags_apply_device(self, pred_ptr, out_tag_ptr, counts_ptr, min_votes=1, pc_new=0, stream=0):
        """duet_sv_tags_apply_device: asynchronous on `stream`, nothing is read back; counts_ptr: device room for four uint32"""
        rc = self.lib.duet_sv_tags_apply_device(self.handle, ctypes.c_void_p(pred_ptr), int(min_votes), int(pc_new),
                                                ctypes.c_void_p(out_tag_ptr), ctypes.c_void_p(counts_ptr), ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)

    def strata_build_device(self, prob, truth, chrom_stratum_ptr, n_strata, cand_stratum_ptr, group_stratum_ptr, stream=0):
        """duet_tune_strata_build_device on resident arrays (devmem.DeviceTune), after truth_build_device on the same prob / truth."""
        rc = self.lib.duet_tune_strata_build_device(self.handle, ctypes.byref(prob), ctypes.byref(truth), ctypes.c_void_p(chrom_stratum_ptr),
                                                    int(n_strata), ctypes.c_void_p(cand_stratum_ptr), ctypes.c_void_p(group_stratum_ptr),
                                                    ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)

    def sweep_strata_device(self, feat_ptr, n_cands, vec_ptr, n_vec, truth, strata, counts_ptr, stream=0):
        rc = self.lib.duet_tune_sweep_strata_device(self.handle, ctypes.c_void_p(feat_ptr), int(n_cands), ctypes.c_void_p(vec_ptr),
                                                    int(n_vec), ctypes.byref(truth), ctypes.byref(strata), ctypes.c_void_p(counts_ptr),
                                                    ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)

    def truth_build_device(self, prob, truth, stream=0):
        """duet_tune_truth_build_device on resident arrays (devmem.DeviceTune): fills truth.n_groups / n_pairs."""
        rc = self.lib.duet_tune_truth_build_device(self.handle, ctypes.byref(prob), ctypes.byref(truth), ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)

    def features_device(self, prob, out_ptr, stream=0, pc_cap=None):
        """duet_ef_features_device; raises ZeroDivisionError where E/F would (the records are written all the same).
        pc_cap: duet_ef_features_cap_device with that PC cap."""
        cap = check_pc_cap(pc_cap)
        if cap is None:
            rc = self.lib.duet_ef_features_device(self.handle, ctypes.byref(prob), ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream))
        else:
            rc = self.lib.duet_ef_features_cap_device(self.handle, ctypes.byref(prob), cap, ctypes.c_void_p(out_ptr),
                                                      ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)

    def svim_features_device(self, sv_problem, result, out_ptr, stream=0, pc_cap=None):
        """duet_svim_features_device (pc_cap: duet_svim_features_cap_device with that PC cap) -> the candidate count."""
        cap = check_pc_cap(pc_cap)
        n = ctypes.c_uint32(0)
        if cap is None:
            rc = self.lib.duet_svim_features_device(self.handle, ctypes.byref(sv_problem), ctypes.byref(result), ctypes.c_void_p(out_ptr),
                                                    ctypes.byref(n), ctypes.c_void_p(stream))
        else:
            rc = self.lib.duet_svim_features_cap_device(self.handle, ctypes.byref(sv_problem), ctypes.byref(result), cap,
                                                        ctypes.c_void_p(out_ptr), ctypes.byref(n), ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)
        return n.value

    def sweep_device(self, feat_ptr, n_cands, vec_ptr, n_vec, truth, counts_ptr, stream=0, out_pred_ptr=None, out_ps_ptr=None):
        """duet_tune_sweep_device; out_pred_ptr: device room for n_vec * n_cands bytes (vector-major), out_ps_ptr: for n_cands
        uint32; without a truth counts_ptr may be 0"""
        opt = lambda p: ctypes.c_void_p(p) if p else None
        rc = self.lib.duet_tune_sweep_device(self.handle, ctypes.c_void_p(feat_ptr), int(n_cands), ctypes.c_void_p(vec_ptr), int(n_vec),
                                             ctypes.byref(truth) if truth is not None else None, opt(counts_ptr), opt(out_pred_ptr),
                                             opt(out_ps_ptr), ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)

    def line_host(self, feat, base, axis, max_values=0):
        """duet_tune_line_host: feat FEATURE_DTYPE[C], base float64[14] -> (vectors float64[n_vec, 14], n_distinct): the line of
        field `axis` (its index in TUNE_NAMES) through `base`.  Raises ZeroDivisionError where a compared feature is not finite."""
        feat = np.ascontiguousarray(feat, dtype=FEATURE_DTYPE)
        base = np.ascontiguousarray(base, dtype=np.float64).reshape(len(TUNE_NAMES))
        out = np.zeros((len(feat) + 1, len(TUNE_NAMES)), dtype=np.float64)
        n_vec, n_distinct = ctypes.c_uint32(0), ctypes.c_uint32(0)
        rc = self.lib.duet_tune_line_host(self.handle, _ptr(feat), len(feat), _ptr(base), clamp_u32(axis), int(max_values), _ptr(out),
                                          ctypes.byref(n_vec), ctypes.byref(n_distinct))
        if rc:
            self._raise(rc)
        return out[:n_vec.value].copy(), n_distinct.value

    def line_device(self, feat_ptr, n_cands, base, axis, max_values, out_vec_ptr, stream=0):
        """duet_tune_line_device on resident arrays (devmem.DeviceTune.line); base float64[14] on the host
        -> (n_vec, n_distinct)."""
        base = np.ascontiguousarray(base, dtype=np.float64).reshape(len(TUNE_NAMES))
        n_vec, n_distinct = ctypes.c_uint32(0), ctypes.c_uint32(0)
        rc = self.lib.duet_tune_line_device(self.handle, ctypes.c_void_p(feat_ptr), int(n_cands), _ptr(base), clamp_u32(axis),
                                            int(max_values), ctypes.c_void_p(out_vec_ptr), ctypes.byref(n_vec), ctypes.byref(n_distinct),
                                            ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)
        return n_vec.value, n_distinct.value

    # -- the line of the PC cap (duet_tune_capline.hip) ------------------------------------------------------------------------
    def _cap_line(self, fn, prob, n_marks, max_values, out_ptr=None, stream=None):
        """One of the four cap-line entries: out_ptr None -> host form, (caps u32[n_caps], n_distinct); else the device form
        writing to out_ptr on `stream`, (n_caps, n_distinct)."""
        n_caps, n_distinct = ctypes.c_uint32(0), ctypes.c_uint32(0)
        if out_ptr is None:
            out = np.zeros(cap_line_room(n_marks, max_values), dtype=np.uint32)
            rc = fn(self.handle, ctypes.byref(prob), clamp_u32(max_values), _ptr(out), ctypes.byref(n_caps), ctypes.byref(n_distinct))
        else:
            rc = fn(self.handle, ctypes.byref(prob), clamp_u32(max_values), ctypes.c_void_p(out_ptr), ctypes.byref(n_caps),
                    ctypes.byref(n_distinct), ctypes.c_void_p(stream or 0))
        if rc:
            self._raise(rc)
        return (out[:n_caps.value].copy() if out_ptr is None else n_caps.value), n_distinct.value

    def cap_line_host(self, soa, svlen_thres, suppread_thres, max_values=0):
        """duet_tune_cap_line_host: the line of the PC cap of an EfSoA -> (caps u32[n_caps] ascending, n_distinct)."""
        prob, keep = problem_from_arrays(soa, svlen_thres, suppread_thres)
        got = self._cap_line(self.lib.duet_tune_cap_line_host, prob, soa.n_marks, max_values)
        del keep
        return got

    def cap_line_device(self, prob, max_values, out_ptr, stream=0):
        """duet_tune_cap_line_device on a resident EfProblem (devmem.DeviceProblem.problem); out_ptr: device room for
        cap_line_room(prob.n_marks, max_values) words -> (n_caps, n_distinct)."""
        return self._cap_line(self.lib.duet_tune_cap_line_device, prob, prob.n_marks, max_values, out_ptr, stream)

    def svim_cap_line_host(self, mark_read, read_tag, max_values=0):
        """duet_svim_cap_line_host: the line of the PC cap over the raw marks (read index per mark, tag word per read)
        -> (caps u32[n_caps] ascending, n_distinct)."""
        mr = np.ascontiguousarray(mark_read, dtype=np.uint32)
        tag = np.ascontiguousarray(read_tag, dtype=np.uint64)
        p = SvimProblem()
        p.marks.n_marks, p.n_reads = len(mr), len(tag)
        p.mark_read, p.read_tag = (a.ctypes.data if a.size else None for a in (mr, tag))
        return self._cap_line(self.lib.duet_svim_cap_line_host, p, len(mr), max_values)

    def svim_cap_line_device(self, sv_problem, max_values, out_ptr, stream=0):
        """duet_svim_cap_line_device on a resident SvimProblem (devmem.DeviceSvim.sv_problem) -> (n_caps, n_distinct)."""
        return self._cap_line(self.lib.duet_svim_cap_line_device, sv_problem, sv_problem.marks.n_marks, max_values, out_ptr, stream)

    def apply_device(self, feat_ptr, n_cands, vec_ptr, pred_ptr, ps_ptr, stream=0):
        """duet_tune_sweep_device with one vector and no truth set: pred u8[C] and ps u32[C] on the device, what
        duet_ef_run_device writes with the built-in constants."""
        rc = self.lib.duet_tune_sweep_device(self.handle, ctypes.c_void_p(feat_ptr), int(n_cands), ctypes.c_void_p(vec_ptr), 1, None, None,
                                             ctypes.c_void_p(pred_ptr), ctypes.c_void_p(ps_ptr), ctypes.c_void_p(stream))
        if rc:
            self._raise(rc)

    def seed_ps(self, contig, cap=1 << 20):
        out = np.zeros(cap, dtype=np.uint32)
        n = self.lib.duet_ef_get_seed_ps(self.handle, int(contig), _ptr(out), cap)
        if n < 0:
            self._raise(n)
        return out[:min(n, cap)].copy()

    # -- diagnostics: the shared device primitives on host arrays (include/duet_ef.h, "Diagnostics") ---------------
    def prims_sort(self, keys, vals=None, key_bits=64, first_shift=0, force_scan=False):
        """duet_prims_sort_host: radix_sort_pairs over keys u64[n] (and vals u32[n]) by the key bits [first_shift, key_bits)
        -> (sorted keys, sorted vals or None)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        out_keys = np.zeros(len(keys), dtype=np.uint64)
        out_vals = None
        if vals is not None:
            vals = np.ascontiguousarray(vals, dtype=np.uint32)
            if len(vals) != len(keys):
                raise ValueError('prims_sort: %d keys, %d values' % (len(keys), len(vals)))
            out_vals = np.zeros(len(vals), dtype=np.uint32)
        rc = self.lib.duet_prims_sort_host(self.handle, _ptr(keys), _ptr(vals), len(keys), int(key_bits), int(first_shift),
                                           1 if force_scan else 0, _ptr(out_keys), _ptr(out_vals))
        if rc:
            self._raise(rc)
        return out_keys, out_vals

    def prims_scan(self, values, op, n_dyn=None, force_spine=False, prefill=0xA5A5A5A5, zero14=True):
        """duet_prims_scan_host: launch_scan over values u32[n], op 0 the exclusive sum / 1 the inclusive maximum; n_dyn: the real
        count on the device, n being its bound.  -> (out u32[n], pre-filled with `prefill` before the scan; total; the 14 words
        the scan zeroes, pre-filled with ones, or None)."""
        values = np.ascontiguousarray(values, dtype=np.uint32)
        out = np.full(len(values), prefill, dtype=np.uint32)
        total = ctypes.c_uint32(0)
        z = np.ones(14, dtype=np.uint32) if zero14 else None
        rc = self.lib.duet_prims_scan_host(self.handle, _ptr(values), len(values), int(op), 0xFFFFFFFF if n_dyn is None else int(n_dyn),
                                           1 if force_spine else 0, _ptr(out), ctypes.byref(total), _ptr(z))
        if rc:
            self._raise(rc)
        return out, total.value, z

    def prims_local_sort(self, keys, key_bits, lo, cap=256, threads=1024):
        """duet_prims_local_sort_host: global passes over the key bits [lo, key_bits), rx_local<threads> and rx_big over the low
        ones -> keys u64[n] in the stable order of their low key_bits."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        out = np.zeros(len(keys), dtype=np.uint64)
        rc = self.lib.duet_prims_local_sort_host(self.handle, _ptr(keys), len(keys), int(key_bits), int(lo), int(cap), int(threads),
                                                 _ptr(out))
        if rc:
            self._raise(rc)
        return out


def check_pc_cap(pc_cap):
    """A PC cap argument: None (the entry without a cap), or an integer in 0 .. PC_CAP_MAX -> int; else ValueError."""
    if pc_cap is None:
        return None
    if isinstance(pc_cap, bool) or not isinstance(pc_cap, (int, np.integer)) or not 0 <= int(pc_cap) <= PC_CAP_MAX:
        raise ValueError('pc_cap: an integer in 0 .. 2^30 - 3 (%d), not %r' % (PC_CAP_MAX, pc_cap))
    return int(pc_cap)


def cap_line_room(n_marks, max_values=0):
    """The values a cap-line entry can write at most (include/duet_ef.h): what the caller allocates for out_caps."""
    room = min(int(n_marks), PC_CAP_MAX + 1) + 1
    return min(room, int(max_values)) if int(max_values) >= 2 else room


def clamp_u32(v):
    v = int(v)
    return 0 if v < 0 else (0xFFFFFFFF if v > 0xFFFFFFFF else v)


def problem_from_arrays(soa, svlen_thres, suppread_thres):
    """EfProblem over host numpy arrays; returns (problem, keepalive)."""
    p = EfProblem()
    p.n_contigs, p.n_cands, p.n_marks, p.n_reads = soa.n_contigs, soa.n_cands, soa.n_marks, soa.n_reads
    keep = [soa.cand_ctg_off, soa.read_tag, soa.cand_pos, soa.cand_svlen, soa.cand_svread, soa.cand_refread,
            soa.cand_gt_ok, soa.cand_off, soa.mark_read]
    (p.cand_ctg_off, p.read_tag, p.cand_pos, p.cand_svlen, p.cand_svread, p.cand_refread, p.cand_gt_ok,
     p.cand_off, p.mark_read) = [a.ctypes.data if a.size else None for a in keep]
    p.svlen_thres = clamp_u32(svlen_thres)
    p.suppread_thres = clamp_u32(suppread_thres)
    return p, keep


def problem_from_device(soa_host, dev_ptrs, svlen_thres, suppread_thres):
    """EfProblem whose arrays are device pointers (dict name -> int) and cand_ctg_off the host array."""
    p = EfProblem()
    p.n_contigs, p.n_cands, p.n_marks, p.n_reads = (soa_host.n_contigs, soa_host.n_cands, soa_host.n_marks,
                                                    soa_host.n_reads)
    p.cand_ctg_off = soa_host.cand_ctg_off.ctypes.data
    for name in ('read_tag', 'cand_pos', 'cand_svlen', 'cand_svread', 'cand_refread', 'cand_gt_ok', 'cand_off',
                 'mark_read'):
        setattr(p, name, dev_ptrs[name] or None)
    p.svlen_thres = clamp_u32(svlen_thres)
    p.suppread_thres = clamp_u32(suppread_thres)
    return p
