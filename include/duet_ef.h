/*
 * duet_ef.h -- C ABI of the MI355X (gfx950) implementation of Duet's step E/F:
 * integration of read-haplotype tags with SV support-read marks, per-candidate haplotype vote and
 * the T1-T5 threshold decision.
 *
 * The reference (yekaizhou/duet v0.6) is pure Python and has no FFI; the seam this library sits
 * behind is the body of
 *     generate_phased_callset(vcf_path, sam_home, svlen_thres, suppread_thres, thread, include_all_ctgs)
 *                                                                   src/duet/sv_phasing_fn.py:185-230
 * between "callset built" (generate_callinfo, :36-68) and "rows sorted" (:229):
 *     filter            sv_phasing_fn.py:189-190
 *     PS-class          sv_phasing_fn.py:191-194
 *     seed sets         sv_phasing_fn.py:195-203
 *     vote + features   sv_phasing_fn.py:70-140   (get_phase_info)
 *     decision          sv_phasing_fn.py:142-183  (predict_hp)
 *     contig drop       sv_phasing_fn.py:209-210
 * and the join of mark names against the per-contig tag dict (:46-48), which the host performs
 * while flattening names to indices.
 *
 * Conventions: plain pointers and sizes, no C++ or torch types; no exception crosses the ABI; every
 * call returns DUET_OK (0) or a negative duet_status and duet_last_error() describes the failure.
 * A context is driven by one host thread at a time.
 */
#ifndef DUET_EF_H
#define DUET_EF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DUET_ABI_VERSION 1

/* The library is built with -fvisibility=hidden: only the functions declared in this header are exported. */
#define DUET_API __attribute__((visibility("default")))

typedef enum duet_status {
    DUET_OK = 0,
    DUET_ERR_INVALID = -1,    /* bad argument (NULL pointer, inconsistent sizes) */
    DUET_ERR_NO_DEVICE = -2,  /* no usable gfx950 device / HIP runtime failure at context creation */
    DUET_ERR_HIP = -3,        /* a HIP call failed; duet_last_error has hipGetErrorString */
    DUET_ERR_OOM = -4,        /* device allocation failed */
    DUET_ERR_TIMEOUT = -6,    /* a collective step (communicator set-up, the all-gather) did not finish within the communicator's
                                 time limit: a peer is missing or stuck.  The communicator is unusable afterwards and the process
                                 should exit (a helper thread may still sit inside RCCL) */
    DUET_ERR_DIV_ZERO = -5    /* a candidate that reaches the decision has svread + refread == 0: the
                                 reference raises ZeroDivisionError there (sv_phasing_fn.py:123) */
} duet_status;

/*
 * Read tag word (one per read that is in its contig's tag dict, sv_phasing_fn.py:28-29):
 *     bits 63..62  hap   1 or 2 (HP:i); 3 = any other value (never counted as a haplotype vote)
 *     bits 61..32  pc    PC:i, saturated at 2^30-2 (only `pc <= 8100` and sums of such pc are used)
 *     bits 31..0   ps    PS:i
 */
#define DUET_TAG(hap, pc, ps) (((uint64_t)(hap) << 62) | ((uint64_t)(pc) << 32) | (uint64_t)(uint32_t)(ps))
#define DUET_MARK_ABSENT 0xFFFFFFFFu   /* mark whose read name is not in its contig's tag dict */
#define DUET_PC_MAX 8100u              /* sv_phasing_fn.py:76,88,201 */

/*
 * One E/F problem in structure-of-arrays form.  Candidates are in callset order
 * (generate_callinfo, sv_phasing_fn.py:50-67): contig-major in chrom-list order, file order inside a
 * contig; cand_ctg_off[k]..cand_ctg_off[k+1] are the candidates of contig k.
 * Marks of candidate c are mark_read[cand_off[c] .. cand_off[c+1]) in RNAMES/READS list order
 * (duplicates kept), each an index into read_tag (already resolved against the candidate's OWN
 * contig table, sv_phasing_fn.py:47-48) or DUET_MARK_ABSENT.  Every candidate has >= 1 mark.
 *
 * A mark has no tag when its index is DUET_MARK_ABSENT, when its index is >= n_reads, or when its tag
 * word is all-ones: the three mean the same, for every entry that takes this problem, and no entry
 * reads read_tag at an index >= n_reads.
 *
 * cand_ctg_off is ALWAYS a host pointer (K+1 small integers; the library stages it).  The other
 * arrays are device pointers for duet_ef_run_device and host pointers for duet_ef_run_host.
 */
typedef struct duet_ef_problem {
    uint32_t n_contigs;             /* K */
    uint32_t n_cands;               /* C */
    uint32_t n_marks;               /* M = cand_off[C] */
    uint32_t n_reads;               /* R = length of read_tag */
    const uint32_t *cand_ctg_off;   /* [K+1] HOST */
    const uint64_t *read_tag;       /* [R]   */
    const uint32_t *cand_pos;       /* [C]   VCF POS */
    const uint32_t *cand_svlen;     /* [C]   abs(SVLEN) (sv_phasing_fn.py:62) */
    const uint32_t *cand_svread;    /* [C]   INFO support count (read_file.py:40-47) */
    const uint32_t *cand_refread;   /* [C]   reference-read count as the reference derives it (read_file.py:56-76) */
    const uint8_t *cand_gt_ok;      /* [C]   1 unless the genotype string is exactly "./." (sv_phasing_fn.py:190) */
    const uint32_t *cand_off;       /* [C+1] CSR offsets into mark_read */
    const uint32_t *mark_read;      /* [M]   */
    uint32_t svlen_thres;           /* -s / --sv_min_size */
    uint32_t suppread_thres;        /* -r / --min_support_read */
} duet_ef_problem;

/* Kernels of one run, in launch order. */
enum { DUET_K_CLASSIFY = 0, DUET_K_SEEDS = 1, DUET_K_FINALIZE = 2, DUET_N_KERNELS = 3 };

typedef struct duet_ef_stats {
    uint64_t algorithmic_bytes;     /* 12*M + 27*C + 8*R */
    uint32_t n_seed_ps;             /* distinct seed phase sets over all contigs (valid after a host run) */
    uint32_t n_profiled_runs;       /* runs averaged into kernel_ms (profiling mode only) */
    float kernel_ms[DUET_N_KERNELS];/* mean duration per kernel from HIP events on the run's stream */
    float total_ms;                 /* mean first-kernel-start to last-kernel-end */
} duet_ef_stats;

typedef struct duet_ctx duet_ctx;

DUET_API int duet_abi_version(void);

/* Context on HIP device `device_id`. NULL on failure; duet_last_error(NULL) then holds the reason. */
DUET_API duet_ctx *duet_ctx_create(int device_id);
DUET_API void duet_ctx_destroy(duet_ctx *ctx);
DUET_API const char *duet_last_error(const duet_ctx *ctx);

/* HIP events attached to the kernels' own dispatches (hipExtLaunchKernelGGL start/stop events on the run's
 * stream), resolved by duet_ef_profile_collect: 0 = none, 1 = the dominant kernel (ef_classify) only -- two
 * events per run --, 2 = every kernel (kernel_ms[] complete, total_ms = first start to last end; serialises
 * the stream a little more), 3 = like 1 but only on every 8th run (what bench.py uses inside its timed
 * region: event pairs cost ~6 us of stream time each, a quarter of a config-2 step). */
DUET_API int duet_ctx_set_profiling(duet_ctx *ctx, int mode);

/*
 * Run E/F on device-resident inputs, asynchronously on `stream` (a hipStream_t passed as void*, NULL =
 * the null stream).  out_pred[C] (0 = filtered, 1 = "1|0", 2 = "0|1", 3 = "1|1") and out_ps[C] are
 * device pointers.  out_ps[c] is the PS predict_hp returns when the reference calls it for c, else 0.
 * The call does not synchronise; DUET_ERR_DIV_ZERO is reported by duet_ef_check (or by the host run).
 */
DUET_API int duet_ef_run_device(duet_ctx *ctx, const duet_ef_problem *prob, uint8_t *out_pred, uint32_t *out_ps,
                       void *stream);

/* Synchronise `stream` and return the deferred status of the runs issued on this context since the
 * last check (DUET_OK or DUET_ERR_DIV_ZERO / DUET_ERR_HIP). */
DUET_API int duet_ef_check(duet_ctx *ctx, void *stream);

/* Host convenience: copies the arrays to the device, runs, copies the results back, synchronises.
 * stats may be NULL. */
DUET_API int duet_ef_run_host(duet_ctx *ctx, const duet_ef_problem *prob, uint8_t *out_pred, uint32_t *out_ps,
                     duet_ef_stats *stats);

/* Profiling mode: synchronise, average the per-kernel event timings of the runs since the last
 * collect into *stats, and reset. */
DUET_API int duet_ef_profile_collect(duet_ctx *ctx, duet_ef_stats *stats);

/* Diagnostics: each bit forces a kernel path or launch structure other than the one the input would take (the outputs
 * are identical; tests use them to exercise every path), e.g. DUET_DBG_CLUSTER_EXACT sends every A0 partition through the exact linkage
 * instead of the bounding-box / threshold-graph fast paths.  0 in production.  The bit values 0x4
 * and 0x10000000 are unused and have no effect. */
#define DUET_DBG_EF_OWN_WIDE 0x1u        /* E/F: the two-launch path finalizes two tiles of 256 candidates per workgroup of 512 threads (ef_finalize_own_wide) whatever
                                            the size (default: where some contig spans more than 256 tiles and the problem has at most 512) */
#define DUET_DBG_EF_OWN_NARROW 0x2u      /* ... one tile per workgroup (ef_finalize_own) whatever the size; it wins over DUET_DBG_EF_OWN_WIDE */
#define DUET_DBG_EF_NO_SEED_HASH 0x40u   /* E/F: ef_seed_sort orders an unsorted seed list itself instead of taking its distinct values through a hash set first */
#define DUET_DBG_EF_FIN_TPB2 0x20u       /* E/F: ef_finalize takes two tiles of 256 candidates per workgroup whatever the size (default from 1 M candidates on) */
#define DUET_DBG_EF_FIN_TPB4 0x80u       /* ... four (default from 8 M candidates on) */
#define DUET_DBG_EF_HEAVY_ALL 0x80000u   /* E/F: ef_classify walks EVERY kept candidate wave-cooperatively (64 marks per step; default: those with more than 32 marks) */
#define DUET_DBG_EF_HEAVY_OFF 0x100000u  /* ... only those of more than 255 marks (the lane walk keeps its counts in bytes): every other candidate by its own lane, mark after mark */
#define DUET_DBG_EF_SPLIT_OFF 0x200000u  /* E/F: the two-launch path keeps ef_classify, one lane per candidate (default up to 512 tiles: ef_classify_split, two lanes
                                            per candidate; the bits that force three launches force ef_classify with them) */
#define DUET_DBG_EF_FP_DECIDE 0x400000u /* E/F: ef_classify takes every class-0 / class-1 decision through the binary64 expressions (rounds 1-4) instead of the
                                            integer form with the binary64 fallback */
#define DUET_DBG_EF_OWN_OFF 0x800000u     /* E/F: three launches (ef_classify, ef_seed_sort, ef_finalize) at every size; default up to 2048 tiles of 256 candidates
                                          * and 64 contigs: two -- every finalize tile builds its contig's seed set itself (ef_finalize_own) */
#define DUET_DBG_EF_OWN_ALL 0x1000000u    /* ... the two launches at every size (up to 64 contigs; host-planned runs only) */
#define DUET_DBG_EF_OWN_SMALLTAB 0x2000000u /* ... and their seed set in LDS holds 8 distinct seeds (default 1024): contigs with more take the array-free walk */
#define DUET_DBG_CLUSTER_EVENT_FORKS 0x4000000u /* A0: the side streams fork off behind hipEventRecord / hipStreamWaitEvent (rounds 1-5) instead of a signal kernel on the
                                          * main stream and a gate kernel on the side stream (round 6) */
#define DUET_DBG_CLUSTER_WIDE_OFF 0x8000000u /* A0: small inputs keep ONE wavefront per partition of more than 64 marks (rounds 1-5: cl_tight_big + cl_link_one) instead
                                              * of a workgroup of eight (cl_find_big + cl_wide_big: wide_unit) */
#define DUET_DBG_CLUSTER_EXACT 0x100u
#define DUET_DBG_CLUSTER_LARGE 0x200u   /* A0: take the launch structure of large inputs (> 4 M marks: one launch per size class,
                                           generic tile-offset scan in the sort, scans with a spine launch) whatever the size */
#define DUET_DBG_CLUSTER_PAIRS 0x400u   /* A0: sort (key, mark index) pairs even when the index fits the key's spare bits */
#define DUET_DBG_CLUSTER_NOBOX 0x800u   /* A0: no bounding-box test: every partition goes through the threshold-graph pair loops */
#define DUET_DBG_CLUSTER_KEYSORT 0x10000u /* A0: the key-only sort of rounds 1-3 (8-byte keys, the records gathered through the permutation afterwards)
                                            also where the 16-byte mark record could travel with the key (duet_recsort.hip.h) */
#define DUET_DBG_CLUSTER_RECSORT 0x40000u /* A0: the record sort also below 1.25 M marks (where the key-only sort is the default: launch-bound passes) */
#define DUET_DBG_CLUSTER_NOSYM 0x20000u  /* A0: the contracted linkage's pair tests column by column (every ordered pair) also where a unit holds one partition and
                                            could evaluate every unordered pair once */
#define DUET_DBG_CLUSTER_LSD 0x8000u     /* A0: plain LSD passes over all key bits also where small inputs would sort the low bits locally */
#define DUET_DBG_CLUSTER_SMALLCAP 0x4000u /* A0: the local sort of the low bits takes groups of at most 3 keys (default 128): the others go to the one-workgroup-per-group path */
#define DUET_DBG_CLUSTER_TIERS 0x2000u  /* A0: small inputs take the two-tier contracted linkage of large inputs in one launch per tier */
#define DUET_DBG_CLUSTER_KC2 0x1000u    /* A0: the contracted linkage keeps partitions with at most 2 groups (default 16); the others
                                           take the second lists (full-triangle linkage) */
DUET_API int duet_ctx_set_debug(duet_ctx *ctx, uint32_t flags);

/* Debug/inspection: copy contig k's sorted seed-PS array of the LAST run to `out` (capacity `cap`),
 * return its length (or a negative status). */
DUET_API int duet_ef_get_seed_ps(duet_ctx *ctx, uint32_t contig, uint32_t *out, uint32_t cap);

/* ------------------------------------------------------------------------------------------------------
 * Stage A0: span-position clustering of SV marks into candidates.
 *
 * Replaces what the reference delegates to the external `svim alignment ... --cluster_max_distance c`
 * (src/duet/sv_calling.py:13-15; help text src/duet/utils.py:27-28).  svim is not part of the reference
 * tree, so this stage follows this repository's own deterministic rule (oracle/cluster_oracle.c, DESIGN.md
 * section 9), modelled on SVIM 1.4.2: marks ordered by (contig, type, centre = pos + span/2); partitions
 * cut at a centre gap > part_gap or after part_max marks; span-position distance
 *     min(|dpos|, |dend|, |dcentre|) / normalizer + |dspan| / max(span)
 * in binary64; average linkage, merged while the closest pair is <= max_dist.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct duet_cluster_problem {
    uint32_t n_marks;               /* M */
    uint32_t part_gap;              /* 1000 */
    uint32_t part_max;              /* 100 (1..128) */
    uint32_t n_contigs_hint;        /* the four hints only narrow the sort key; when any is 0 the library measures the
                                     * maxima itself (one small kernel + one host round trip) */
    uint32_t n_types_hint;          /* 0 = unknown */
    uint32_t max_pos_hint;          /* 0 = unknown */
    uint32_t max_span_hint;         /* 0 = unknown */
    uint32_t reserved;
    double max_dist;                /* -c / --cluster_max_distance (0.9) */
    double normalizer;              /* 900 */
    const uint16_t *mark_contig;    /* [M] */
    const uint8_t *mark_type;       /* [M] caller-defined SV type code */
    const uint32_t *mark_pos;       /* [M] */
    const uint32_t *mark_span;      /* [M] */
} duet_cluster_problem;

/* Candidates in (contig, type, centre) order; members of candidate j are
 * order[cand_off[j] .. cand_off[j+1]) (mark indices, sorted order); cand_pos / cand_span are floor means.
 * All arrays need room for M entries (cand_off: M+1).  n_cands is a device word for duet_cluster_run_device
 * and a host word for duet_cluster_run_host. */
typedef struct duet_cluster_result {
    uint32_t *order;
    uint32_t *cand_off;
    uint16_t *cand_contig;
    uint8_t *cand_type;
    uint32_t *cand_pos;
    uint32_t *cand_span;
    uint32_t *n_cands;
} duet_cluster_result;

/* (Up to 4 M marks the stage's side-stream chains fork off and join through one-lane signal / gate kernels and a per-call epoch word
 * of the context, not through events -- an event record cost the main stream 7-14 us each.  Such a call cannot be captured into a
 * hipGraph: set DUET_DBG_CLUSTER_EVENT_FORKS with duet_ctx_set_debug for that; it also applies to duet_svim_phase_device.
 * A gate waits for a kernel of another queue, which needs the device to run the two side by side: the first such call of a context
 * tries that out once (three one-lane kernels on two internal streams, a bounded wait of at most 20 ms, two stream synchronisations)
 * and a context on a device that takes one kernel at a time -- under a counter-collecting profiler, AMD_SERIALIZE_KERNEL -- forks
 * behind events instead.) */
DUET_API int duet_cluster_run_device(duet_ctx *ctx, const duet_cluster_problem *prob, const duet_cluster_result *res,
                            void *stream);
DUET_API int duet_cluster_run_host(duet_ctx *ctx, const duet_cluster_problem *prob, const duet_cluster_result *res);

/* ------------------------------------------------------------------------------------------------------
 * Fused SVIM-mode pipeline: raw SV marks -> A0 clustering -> E/F phasing, everything resident in HBM, no VCF
 * round trip.  What upstream obtains from the SVIM VCF per candidate is derived
 * on the device from the clusters:
 *     POS      = floor mean of the members' pos          SVLEN   = floor mean of the members' span
 *     support  = number of member marks (svread)          GT      = called ("not ./.")
 *     marks    = the members' read indices in cluster order
 *     refread  = max(depth(contig, POS) - support, 0), depth read from a binned coverage array -- this
 *                repository's stand-in for SVIM's AD[0] (reads at the locus that do not support the SV);
 *                like A0 itself it has no pinned reference (svim is external).
 * Candidates come out grouped by contig, then by (type, centre); out_pred / out_ps are indexed like the
 * cluster result's candidate arrays.  The call synchronises `stream` once (candidate counts per contig come
 * back to the host to lay out the E/F workspace).
 * ---------------------------------------------------------------------------------------------------- */
typedef struct duet_svim_problem {
    duet_cluster_problem marks;     /* device arrays */
    const uint32_t *mark_read;      /* [M] device: read index of each raw mark (into read_tag) or DUET_MARK_ABSENT */
    const uint64_t *read_tag;       /* [R] device */
    uint32_t n_reads;
    uint32_t n_contigs;             /* K: mark_contig values are < K */
    const uint32_t *depth;          /* device: coverage bins, contig k at depth_off[k] .. depth_off[k+1] */
    const uint32_t *depth_off;      /* [K+1] HOST */
    uint32_t depth_bin;             /* bin width in bp (>= 1) */
    uint32_t svlen_thres, suppread_thres;
    uint32_t reserved;
} duet_svim_problem;

/* res: device arrays as for duet_cluster_run_device (n_cands a device word); out_pred[M], out_ps[M] device.
 * n_cands_host != NULL: the call waits once for the clustering to learn the candidate count, stores it there and
 * plans E/F on the host.  n_cands_host == NULL: nothing waits -- E/F is planned on the device for the upper bound of M
 * candidates and reads the count from res->n_cands; the caller gets the count from there after synchronising. */
DUET_API int duet_svim_phase_device(duet_ctx *ctx, const duet_svim_problem *prob, const duet_cluster_result *res,
                           uint8_t *out_pred, uint32_t *out_ps, uint32_t *n_cands_host, void *stream);

/* Host convenience (what a rank of `duet -b svim-gpu --gpus N` calls: no device-memory framework in the process): every
 * array of *prob and *res is HOST memory (res->order may be NULL; res->n_cands a host word; the arrays need room for M
 * entries, cand_off M + 1), out_pred[M] / out_ps[M] host; uploads, runs the fused pipeline, downloads, synchronises.
 * Returns DUET_ERR_DIV_ZERO like duet_ef_run_host. */
DUET_API int duet_svim_phase_host(duet_ctx *ctx, const duet_svim_problem *prob, const duet_cluster_result *res,
                         uint8_t *out_pred, uint32_t *out_ps);

/* ---------------------------------------------------------------------------------------------
 * Rows of sv_calling/variants.vcf in the svim-gpu mode (duet_callset.hip): one row per candidate of a
 * cluster result, in its order (contig-major, then type, then centre), phased or not -- this repository's own dialect modelled
 * on SVIM's:
 *     CHROM POS svim_gpu.<CHROM>.<i> N <T> . PASS SVTYPE=T;END=e;SVLEN=l;SUPPORT=n;READS=r1,...,rn GT:DP:AD gt:DP:ref,n
 * i = the row's 1-based number within its contig; T = DEL, INS, INV, DUP for type codes 0-3 (any other code: DUET_ERR_INVALID);
 * e = POS for INS, POS + span otherwise; l = -span for DEL, +span otherwise; n = member count; READS = the members' read names in
 * cluster order (res->order); ref = max(depth(contig, POS) - n, 0) as the fused adapter computes it (bin min(POS / depth_bin,
 * bins - 1), 0 on a contig without bins); DP = n + ref; gt = 1/1 if 5n >= 4 DP, else 0/1 if 5n >= DP, else 0/0.
 * The header lines stay with the host.
 * ---------------------------------------------------------------------------------------------------------------------- */
typedef struct duet_callset_names {
    const uint32_t *mark_name;      /* [M] per RAW mark (the order of prob->marks, like mark_read): index into name_off */
    const uint64_t *name_off;       /* [n_names + 1] name j = name_pool[name_off[j] .. name_off[j + 1]) */
    const char *name_pool;
    uint32_t n_names;
    uint32_t n_contigs;             /* must equal prob->n_contigs */
    const char *const *chrom;       /* [K] HOST: the CHROM text of every contig, NUL-terminated */
} duet_callset_names;

/* From *prob: depth, depth_off (HOST), depth_bin, n_contigs, marks.n_marks; from *res: order, cand_off, cand_contig, cand_type,
 * cand_pos, cand_span for n_cands candidates (res->n_cands is not read).
 * _device: device arrays (as duet_svim_phase_device leaves them), out_text device; asynchronous on `stream` apart from one host
 * round trip that learns the text's size.  _host: every array of *prob, *res and *names is HOST memory (res->order [M],
 * cand_off [n_cands + 1]); uploads, runs the same kernels, copies the text to out_text (host), synchronises.
 * Both: *out_len = the text's exact size; when out_cap is smaller nothing is written and the call returns DUET_ERR_INVALID.
 * A bound the caller can compute from its inputs: n_cands * (2 * longest CHROM text + 168) + sum over the members of
 * (name length + 1) -- e.g. M * (longest name + 1). */
DUET_API int duet_svim_vcf_rows_device(duet_ctx *ctx, const duet_svim_problem *prob, const duet_cluster_result *res, uint32_t n_cands,
                                       const duet_callset_names *names, char *out_text, uint64_t out_cap, uint64_t *out_len,
                                       void *stream);
DUET_API int duet_svim_vcf_rows_host(duet_ctx *ctx, const duet_svim_problem *prob, const duet_cluster_result *res, uint32_t n_cands,
                                     const duet_callset_names *names, char *out_text, uint64_t out_cap, uint64_t *out_len);

/* ---------------------------------------------------------------------------------------------
 * Rows of phased_sv.vcf in the svim-gpu mode (duet_svim_rows.hip): from a cluster result and its
 * (pred, ps) to the text of the data rows, as duet_amd/svim_mode.py rows_text writes them.
 *     CHROM POS Duet.<n> N <T> . PASS SVLEN=v;SVTYPE=<T> HP:PS hp:ps        (tab-separated, one '\n' behind each row)
 * Kept: the candidates with pred != 0.  Order: stable, by CHROM text (unsigned byte order, the shorter text first on a common
 * prefix -- how Python compares the strings) then POS; ties keep candidate order.  The library ranks the n_contigs texts itself,
 * on the host; two contigs with the same text share a rank.  n = the row's 1-based number after the sort; T = DEL, INS, INV, DUP
 * for type & 3 = 0, 1, 2, 3; v = span for INS and DUP, -span otherwise (a span of 0 prints 0); hp = 1|0, 0|1, 1|1 for pred 1, 2,
 * 3; POS, n, span and ps are full unsigned 32-bit values in decimal.  The header lines stay with the host.
 *
 * Reads res->cand_contig, cand_type, cand_pos, cand_span for n_cands candidates (order, cand_off, n_cands of *res are not read),
 * pred[n_cands], ps[n_cands].  chrom: [n_contigs] HOST, NUL-terminated CHROM text of every contig (each at most 1 MiB).
 * _device: device arrays (as duet_svim_phase_device leaves them), out_text device; asynchronous on `stream` apart from ONE host
 * round trip that learns the row count and the text's size.  _host: everything HOST; uploads, runs the same kernels, copies the
 * text back, synchronises.
 * Both: *n_rows = the row count, *out_len = the text's exact size; when out_cap is smaller nothing is written and the call
 * returns DUET_ERR_INVALID with *out_len still exact.  n_rows * (longest CHROM text + 96) always suffices: a row without CHROM is
 * at most 95 bytes.  Row offsets are 64-bit: a text of 4 GiB or more is legal.
 * DUET_ERR_INVALID, nothing written, duet_last_error names the case: a NULL array with n_cands > 0; n_contigs of 0 or more than
 * 65535; a NULL chrom[k]; a kept candidate with pred > 3; a kept candidate with cand_contig >= n_contigs.
 * n_cands == 0, or no kept candidate: DUET_OK, zero rows, zero bytes. */
DUET_API int duet_svim_phased_rows_device(duet_ctx *ctx, const duet_cluster_result *res, uint32_t n_cands, const uint8_t *pred,
                                          const uint32_t *ps, uint32_t n_contigs, const char *const *chrom, char *out_text,
                                          uint64_t out_cap, uint64_t *out_len, uint32_t *n_rows, void *stream);
DUET_API int duet_svim_phased_rows_host(duet_ctx *ctx, const duet_cluster_result *res, uint32_t n_cands, const uint8_t *pred,
                                        const uint32_t *ps, uint32_t n_contigs, const char *const *chrom, char *out_text,
                                        uint64_t out_cap, uint64_t *out_len, uint32_t *n_rows);

/* ---------------------------------------------------------------------------------------------
 * Rows of phased_sv.vcf on the device: from (pred, ps) to the text of the data rows.
 * Replaces, for the rows: the emission order of src/duet/sv_phasing_fn.py:204-228 (contig order, PS-class 0/1/2,
 * file order, pred 0 dropped), the stable sort of :229 (CHROM as text, POS as int), print_sv of
 * src/duet/write_file.py:6-17 and the SVLEN sign rule of sv_phasing_fn.py:225.  The header lines stay with the host.
 *
 * All pointers are device memory except cand_ctg_off.  The texts of candidate c are
 * pool[str_off[4c] .. str_off[4c+1]) = CHROM, then REF, ALT and SVTYPE up to str_off[4c+4].
 * cand_chrom_rank[c] = rank of c's CHROM text among the n_chrom_texts distinct CHROM texts in byte order
 * (shorter text first on a common prefix), which is how Python compares the strings at :229.
 *
 * The struct carries no n_reads: the caller of duet_rows_run_device vouches that every mark_read entry is
 * DUET_MARK_ABSENT or a valid index into read_tag (duet_ef_rows_run_host takes the size from *prob instead and
 * treats an index >= n_reads as no tag).  A tag word whose PS field is all-ones is no tag, as for duet_ef_problem. */
typedef struct duet_rows_problem {
    uint32_t n_contigs, n_cands;
    const uint32_t *cand_ctg_off;        /* HOST [K+1] */
    const uint8_t *pred;                 /* [C] from duet_ef_run_device */
    const uint32_t *ps;                  /* [C] */
    const uint32_t *cand_pos, *cand_svlen;
    const uint8_t *cand_plus;            /* [C] 1: SVTYPE is exactly INS or DUP, SVLEN is written positive */
    const uint16_t *cand_chrom_rank;     /* [C] */
    uint32_t n_chrom_texts;
    uint32_t max_pos;                    /* 0 = unknown (32 key bits for POS) */
    const char *pool;
    uint64_t pool_bytes;
    const uint32_t *str_off;             /* [4C+1] */
    const uint32_t *cand_off, *mark_read;/* the E/F problem's CSR and tag table: the PS-class is recomputed from them */
    const uint64_t *read_tag;
} duet_rows_problem;

/* Writes the rows, in final order, to out_text (device, out_cap bytes; pool_bytes + 96 * n_cands always suffices);
 * *out_len = bytes written, *n_rows = rows.  Synchronises `stream` (twice). */
DUET_API int duet_rows_run_device(duet_ctx *ctx, const duet_rows_problem *prob, char *out_text, uint64_t out_cap, uint64_t *out_len,
                         uint32_t *n_rows, void *stream);

/* Host-array convenience of the two together: *prob as for duet_ef_run_host, *rows with HOST arrays cand_plus,
 * cand_chrom_rank, pool, str_off (+ n_cands, n_chrom_texts, max_pos, pool_bytes; the other fields are filled in here);
 * uploads, runs E/F and the row emission on the device and copies the rows' text to out_text (host, out_cap bytes).
 * Returns what duet_ef_run_host would (e.g. DUET_ERR_DIV_ZERO) before writing any row. */
DUET_API int duet_ef_rows_run_host(duet_ctx *ctx, const duet_ef_problem *prob, const duet_rows_problem *rows, char *out_text,
                          uint64_t out_cap, uint64_t *out_len, uint32_t *n_rows);

/* ---------------------------------------------------------------------------------------------
 * Accuracy evaluator: a phased callset scored against a truth set, the arithmetic of
 * src/scripts/evaluation.py:99-159.  The host parses the two VCFs the way :35-97 does and flattens them:
 *   truth ("base") records grouped by list key = 2 * contig + type (0 INS, 1 DEL), position-sorted (stably) inside a list;
 *   calls that sit on a listed contig and have one of the two types, with their list key, their phase-set group
 *   (= distinct (contig, phase set) pair, :109-111) and their haplotype as a code: 0 '1|0', 1 '0|1', 2 '1|1', >= 3 any other
 *   string (compared for equality only); record ids (:51) as dense integers -- equal id strings share one integer, because
 *   upstream counts SETS of ids.
 * Out: the sizes of the six sets of :100 -- call_tp, base_tp, call_tp_gt, base_tp_gt, call_tp_hp, base_tp_hp.  The ten
 * numbers upstream prints are quotients of these and of len(callinfo) / len(baseinfo), taken on the host. */
typedef struct duet_eval_problem {
    uint32_t n_base, n_calls, n_groups, n_keys;      /* n_keys = 2 * contigs */
    uint32_t n_base_uid, n_call_uid;                 /* distinct ids on either side */
    uint32_t refdist;                                /* -r / --refdist (:126) */
    uint32_t reserved;
    double ratio;                                    /* -p / --pctsim (:127) */
    const uint32_t *base_off;                        /* [n_keys + 1] */
    const uint32_t *base_pos, *base_len, *base_uid;  /* [n_base] */
    const uint8_t *base_hp;                          /* [n_base] */
    const uint32_t *call_key;                        /* [n_calls]; every call's list must be non-empty (upstream raises
                                                        IndexError otherwise, :120-125: the host checks) */
    const uint32_t *call_pos, *call_len, *call_uid, *call_group;
    const uint8_t *call_hp;
} duet_eval_problem;

typedef struct duet_eval_counts {
    uint32_t call_tp, base_tp, call_gt, base_gt, call_hp, base_hp;
} duet_eval_counts;

/* All arrays are HOST pointers; uploads, runs four small kernels, synchronises. */
DUET_API int duet_eval_run_host(duet_ctx *ctx, const duet_eval_problem *prob, duet_eval_counts *counts);

/* The same scoring, said per record (duet_eval_details.hip): what became of every call and of every truth record.
 *
 * Call c (the order of the call arrays).  `base` is the truth record the call is compared with -- the nearest one of its list by
 * :117-125, an index into the base arrays --, `dist` = |call_pos[c] - base_pos[base]|, and `bits`:
 *   NEAR     dist <= refdist (:126)
 *   SIZE     min(len) / max(len) >= ratio, the binary64 quotient of :127 (0 / 0 is nan: refused)
 *   MATCHED  NEAR and SIZE: the pair the evaluator scores
 *   GT, SAME, FLIP   the tests of :130-131, :134 and :137-139 on a MATCHED pair (a '1|1' pair sets SAME and FLIP); never set without
 *            MATCHED, as the evaluator makes them on accepted pairs only
 *   LABEL    the labelling the call's phase-set group took (:143-148): 0 "same", 1 "flip" -- "same" only with strictly more ids,
 *            call ids plus truth ids; set on every call of the group, matched or not
 *   HP       MATCHED and the one of SAME / FLIP that LABEL names: the call is in call_tp_hp, its record in base_tp_hp
 * All bits but LABEL are about this record's own pair, not about its id: two calls with one id can differ.  A call whose
 * call_key is 0xFFFFFFFF is compared with nothing: base and dist all-ones, LABEL alone in bits.
 *
 * Truth record j (the order of the base arrays).  n_calls / n_gt / n_hp: the calls with base == j that have MATCHED / GT / HP.
 * `nearest`: the call of j's list key with the smallest |call_pos - base_pos[j]|, ties to the smaller call position, then to the
 * smaller call index; all-ones (and nearest_dist all-ones) when the key has no call.  `reason` says why a record with
 * n_calls == 0 was missed: NO_CALL the key has no call; FAR nearest_dist > refdist; SIZE the nearest call is within refdist and
 * the length ratio fails; ELSEWHERE the nearest call passes both tests against j and was compared with another record;
 * DUET_EVAL_HIT (255) when n_calls > 0. */
#define DUET_EVAL_NEAR 1u
#define DUET_EVAL_SIZE 2u
#define DUET_EVAL_MATCHED 4u
#define DUET_EVAL_GT 8u
#define DUET_EVAL_SAME 16u
#define DUET_EVAL_FLIP 32u
#define DUET_EVAL_LABEL 64u
#define DUET_EVAL_HP 128u

#define DUET_EVAL_NO_CALL 0
#define DUET_EVAL_FAR 1
#define DUET_EVAL_WRONG_SIZE 2
#define DUET_EVAL_ELSEWHERE 3
#define DUET_EVAL_HIT 255

typedef struct duet_eval_call_rec {
    uint32_t base, dist, bits;
} duet_eval_call_rec;                                /* 12 bytes */

typedef struct duet_eval_base_rec {
    uint32_t n_calls, n_gt, n_hp;
    uint32_t nearest, nearest_dist;
    uint8_t reason, reserved[3];                     /* reserved: 0 */
} duet_eval_base_rec;                                /* 24 bytes */

/* All arrays are HOST pointers.  counts: what duet_eval_run_host gives for *prob; calls[n_calls], base[n_base].  Checked on the
 * host before anything is uploaded (DUET_ERR_INVALID): n_keys in 1 .. 2^24 - 1; base_off ascends from 0 to n_base; every call_key
 * is 0xFFFFFFFF or names a non-empty list; every call_uid < n_call_uid and call_group < n_groups (of a call without a list key
 * too); every base_uid < n_base_uid.  n_calls == 0 launches nothing: every truth record is a NO_CALL. */
DUET_API int duet_eval_details_host(duet_ctx *ctx, const duet_eval_problem *prob, duet_eval_counts *counts, duet_eval_call_rec *calls,
                           duet_eval_base_rec *base);

/* ---------------------------------------------------------------------------------------------
 * Threshold sweep (duet_tune.hip): the T1-T5 tree of predict_hp (src/duet/sv_phasing_fn.py:142-183) with its constants
 * replaced by a vector of binary64 values, applied to K vectors at once and scored against a truth set.
 *
 * duet_tune_thresholds: 14 binary64 fields in this fixed order, each named after the reference line it replaces; the
 * defaults (DUET_TUNE_DEFAULTS) are the reference's constants.  Every comparison is the reference's, made in binary64 on
 * the binary64 features Python computes (hapread_ratio = allhap / deg, a1, a2, sv_ratio, totsc_ratio; an integer compared
 * with a double converts exactly), so NaN and +-inf behave as Python's <=, >=, > do.  Not in the vector: the `sv_ratio == 1`
 * test of :146 and ps_sr (fixed), the dead `sv_num >= 20` test of :157, and the PC cap 8100 of :76, :88, :201 -- it changes who
 * votes and the seed sets, not the tree, so it is a parameter of the feature export (duet_ef_features_cap_*, below), not a
 * field here.
 * ---------------------------------------------------------------------------------------------------------------------------- */
typedef struct duet_tune_thresholds {
    double c0_min_sv_num;           /* 4      :146  sv_num >= . (class 0) */
    double c2_min_sv_ratio;         /* 0.72   :149  sv_ratio >= . */
    double c2_max_avgsc_diff;       /* 1369.5 :150  hap_avgsc_diff <= . */
    double c2_min_sv_num;           /* 3      :151  sv_num >= . */
    double c2_min_hap0;             /* 6      :154  hap0 >= . */
    double c1_onehap_sv_ratio_lo;   /* 0.24   :160  sv_ratio <= . */
    double c1_onehap_sv_ratio_hi;   /* 0.9    :162  sv_ratio <= . */
    double c1_hapread_ratio;        /* 0.75   :163, :166 all four uses: hapread_ratio <= . / > . */
    double c1_max_avgsc_diff;       /* 2400   :163, :166  hap_avgsc_diff <= . */
    double c1_twohap_sv_ratio_1;    /* 0.3    :169  sv_ratio <= . */
    double c1_twohap_sv_ratio_2;    /* 0.45   :171  sv_ratio <= . */
    double c1_max_ref_num;          /* 10     :172  ref_num > . */
    double c1_twohap_sv_ratio_3;    /* 0.75   :176  sv_ratio <= . */
    double c1_max_totsc_ratio;      /* 9.72   :177  totsc_ratio <= . */
} duet_tune_thresholds;
#define DUET_TUNE_DEFAULTS {4.0, 0.72, 1369.5, 3.0, 6.0, 0.24, 0.9, 0.75, 2400.0, 0.3, 0.45, 10.0, 0.75, 9.72}

/* One candidate's features (56 bytes), in callset order.  `kept`: the filter of :189-190 holds; `eligible`: kept and the
 * candidate's contig has a non-empty seed set (:209-210) -- only eligible candidates reach predict_hp.  cls is the PS-class
 * (0 / 1 / 2, :191-194) of a kept candidate (0 otherwise).  The vote (hap1, hap2, hap0, allhap, t1, t2 = the PC sums, ps = the PS
 * predict_hp returns) is that of get_phase_info (:70-111) and is filled in for eligible candidates only (0 otherwise); deg is
 * the mark count, svread / refread the candidate's columns, for every candidate. */
typedef struct duet_tune_feature {
    uint64_t t1, t2;
    uint32_t hap1, hap2, hap0, allhap;
    uint32_t deg, svread, refread, ps;
    uint8_t eligible, kept, cls, reserved0;
    uint32_t reserved1;
} duet_tune_feature;

/* Runs E/F on the problem (device arrays as for duet_ef_run_device) for its seed sets, then one new kernel writes out[C]
 * (device).  Synchronises `stream`; returns what duet_ef_check would for the same problem (e.g. DUET_ERR_DIV_ZERO: the records
 * are written all the same).  _host: host arrays as for duet_ef_run_host, out[C] host. */
DUET_API int duet_ef_features_device(duet_ctx *ctx, const duet_ef_problem *prob, duet_tune_feature *out, void *stream);
DUET_API int duet_ef_features_host(duet_ctx *ctx, const duet_ef_problem *prob, duet_tune_feature *out);

/* The same records with the PC cap as a run parameter: a mark votes iff its read is tagged and pc <= pc_cap (the reference tests
 * `read[3] <= 8100`, sv_phasing_fn.py:76, :88, :201).  The PS-class is unchanged (:192-194 has no PC test); the seed set of a contig
 * is the set of PS values of its kept class-1 candidates that have at least one voter; eligible = kept and that set is not
 * empty; vote and ps follow get_phase_info with pc_cap in place of 8100.  pc_cap is 0 .. 2^30 - 3 (the tag word saturates pc at
 * 2^30 - 2, and a saturated value never votes): anything above is DUET_ERR_INVALID and nothing is written.  With
 * pc_cap == DUET_PC_MAX the records and the status are duet_ef_features_*'s, byte for byte.
 * These entries build the seed sets themselves (duet_tune_cap.hip) and never run E/F: the kernels of duet_ef_run_* keep the
 * reference's cap as a compile-time constant.  Their workspace is the context's own and not E/F's -- a call changes nothing of
 * what a later duet_ef_run_*, duet_ef_get_seed_ps or duet_ef_features_* on the same context returns.  Synchronises `stream`;
 * DUET_ERR_DIV_ZERO: an eligible candidate has svread + refread == 0 (the records are written all the same) -- eligibility
 * depends on the cap, so the status of one problem can differ between caps.  _host: host arrays, out[C] host. */
DUET_API int duet_ef_features_cap_device(duet_ctx *ctx, const duet_ef_problem *prob, uint32_t pc_cap, duet_tune_feature *out,
                                         void *stream);
DUET_API int duet_ef_features_cap_host(duet_ctx *ctx, const duet_ef_problem *prob, uint32_t pc_cap, duet_tune_feature *out);

/* A truth set prepared for the candidates (host work, once, independent of the thresholds; duet_amd/tune.py): the call a
 * candidate would be written as, read through the evaluator's own parser, matched once to its nearest truth record
 * (src/scripts/evaluation.py:99-159).  Per candidate c:
 *   cand_flags[c]  bit 12: the call is in the evaluator's call list; bit 13: it is, but the truth list of its (contig, type)
 *                  is empty (upstream raises IndexError when such a call is emitted); bit 14: it matches cand_uid[c];
 *                  bits 3 (p - 1) + {0, 1, 2}, p = pred 1..3: with that HP the match counts for genotyping / is "same" /
 *                  is "flip" (:131-142)
 *   cand_group[c]  the call's phase-set group (< n_groups) when bit 12 is set
 *   cand_uid[c]    the matched truth id (< n_uid) when bit 14 is set
 *   cand_pair[c]   dense id (< n_pairs) of the (group, uid) pair when bit 14 is set; pairs are numbered group-major:
 *                  group g owns pairs group_pair_off[g] .. group_pair_off[g + 1], pair_uid[] gives their truth ids. */
#define DUET_TUNE_IN_CALLS 0x1000u
#define DUET_TUNE_RAISES 0x2000u
#define DUET_TUNE_MATCHED 0x4000u
typedef struct duet_tune_truth {
    uint32_t n_uid, n_groups, n_pairs, reserved;
    const uint16_t *cand_flags;     /* [C] */
    const uint32_t *cand_group;     /* [C] */
    const uint32_t *cand_uid;       /* [C] */
    const uint32_t *cand_pair;      /* [C] */
    const uint32_t *group_pair_off; /* [n_groups + 1] */
    const uint32_t *pair_uid;       /* [n_pairs] */
} duet_tune_truth;

/* Per vector: what evaluation.py:99-159 reduces to its ten numbers.  n_calls = len(callinfo), n_groups = distinct phase-set
 * groups among the emitted calls, the six set sizes of :100, n_raise = emitted calls for which upstream raises IndexError.
 * Without a truth set only n_calls is filled in (then: every emitted candidate). */
typedef struct duet_tune_counts {
    uint32_t n_calls, n_groups, call_tp, base_tp, call_gt, base_gt, call_hp, base_hp, n_raise, reserved;
} duet_tune_counts;

/* K vectors over C candidates.  _device: feat[C], vec[K], the truth arrays (truth may be NULL), counts[K] (may be NULL when
 * truth is NULL), out_pred[K * C] (vector-major, may be NULL) and out_ps[C] (may be NULL; = ps of eligible candidates, else 0,
 * which is duet_ef_run_device's out_ps) are device memory; *truth itself is host memory.  Asynchronous on `stream` apart from
 * the workspace (grown, never shrunk; the vectors are processed in batches that fit it).  _host: the same with host arrays;
 * synchronises. */
DUET_API int duet_tune_sweep_device(duet_ctx *ctx, const duet_tune_feature *feat, uint32_t n_cands, const duet_tune_thresholds *vec,
                                    uint32_t n_vec, const duet_tune_truth *truth, duet_tune_counts *counts, uint8_t *out_pred,
                                    uint32_t *out_ps, void *stream);
DUET_API int duet_tune_sweep_host(duet_ctx *ctx, const duet_tune_feature *feat, uint32_t n_cands, const duet_tune_thresholds *vec,
                                  uint32_t n_vec, const duet_tune_truth *truth, duet_tune_counts *counts, uint8_t *out_pred,
                                  uint32_t *out_ps);

/* The features of the fused pipeline's candidates (for a sweep over -c, -s and -r without a callset file): clusters and adapts
 * as duet_svim_phase_device does with n_cands_host given, then runs E/F and the feature kernel on the adapted problem
 * (duet_ef_features_device) -- out_feat[M] in place of out_pred / out_ps, indexed like the cluster result's candidate arrays, which
 * stay in *res for duet_tune_truth_build_device's table form.  n_cands_host is mandatory.  Synchronises `stream`; the status is
 * duet_ef_features_device's (DUET_ERR_DIV_ZERO: the records are written all the same).  _host: arrays as for
 * duet_svim_phase_host, out_feat[M] host. */
DUET_API int duet_svim_features_device(duet_ctx *ctx, const duet_svim_problem *prob, const duet_cluster_result *res,
                                       duet_tune_feature *out_feat, uint32_t *n_cands_host, void *stream);
DUET_API int duet_svim_features_host(duet_ctx *ctx, const duet_svim_problem *prob, const duet_cluster_result *res,
                                     duet_tune_feature *out_feat);

/* duet_svim_features_* under a PC cap: clusters and adapts in exactly the same way (every call clusters again: the entry keeps
 * no state between caps), then duet_ef_features_cap_device in place of duet_ef_features_device. */
DUET_API int duet_svim_features_cap_device(duet_ctx *ctx, const duet_svim_problem *prob, const duet_cluster_result *res, uint32_t pc_cap,
                                           duet_tune_feature *out_feat, uint32_t *n_cands_host, void *stream);
DUET_API int duet_svim_features_cap_host(duet_ctx *ctx, const duet_svim_problem *prob, const duet_cluster_result *res, uint32_t pc_cap,
                                         duet_tune_feature *out_feat);

/* The truth arrays built on the device (duet_tune_truth.hip) -- what duet_amd/tune.py's prepare_truth computes on the host, which
 * stays the normative text.  Per candidate the caller says how the evaluator's parser sees the row the candidate would be
 * written as, which does not depend on -s, -r or the thresholds:
 *   cand_key[c]    the truth list key 2 * contig + type as in duet_eval_problem (< n_keys), or DUET_TUNE_KEY_NONE: the parser keeps
 *                  the row but no truth list can match it, or DUET_TUNE_KEY_SKIP: the parser drops the row (any other value
 *                  >= n_keys is taken as DUET_TUNE_KEY_NONE)
 *   cand_chrom[c]  dense id (< n_chrom) of the row's CHROM text; equal texts share an id
 *   cand_len[c]    abs(SVLEN): the parser also drops a row with a length below 50
 * or, with cand_key == NULL and cand_chrom == NULL (a cluster result: no per-candidate text exists), tables per contig:
 *   cand_contig[c] (< n_contigs), cand_type[c] (0..3: DEL, INS, INV, DUP; anything else is dropped), key_table[4 * contig + type]
 *   = the candidate's cand_key, chrom_id[contig] = its cand_chrom and, when bed_off != NULL, per contig the merged, sorted,
 *   closed ranges bed_lo[j] <= pos <= bed_hi[j], j in bed_off[contig] .. bed_off[contig + 1]: a candidate outside every range of
 *   its contig is DUET_TUNE_KEY_SKIP.
 * Of feat[c] `eligible` and `ps` are read.  The truth side is duet_eval_problem's: base_off[n_keys + 1], base_pos / base_len /
 * base_uid / base_hp [n_base] (position-sorted inside a list, base_uid < n_base_uid, base_hp codes 0 '1|0', 1 '0|1', 2 '1|1',
 * >= 3 anything else), refdist and ratio (the quotient min(len) / max(len) is taken in binary64).
 *
 * A candidate is in the call list iff it is eligible, not dropped and cand_len >= 50; every output of any other candidate is 0.
 * Groups are the distinct (cand_chrom, ps) among the calls, pairs the distinct (group, uid) among the matched calls.  The
 * numbering is that of one stable sort by (cand_chrom, ps, uid): it does not depend on the order in which anything arrives. */
#define DUET_TUNE_KEY_NONE 0xFFFFFFFEu
#define DUET_TUNE_KEY_SKIP 0xFFFFFFFFu
typedef struct duet_tune_truth_problem {
    uint32_t n_cands, n_keys, n_base, n_base_uid;
    uint32_t n_chrom;                   /* CHROM ids are < n_chrom */
    uint32_t n_contigs;                 /* table form only */
    uint32_t refdist;
    uint32_t reserved;
    double ratio;
    const duet_tune_feature *feat;      /* [C] */
    const uint32_t *cand_pos, *cand_len;/* [C] */
    const uint32_t *cand_key, *cand_chrom;      /* [C], or both NULL: the table form */
    const uint16_t *cand_contig;        /* [C] */
    const uint8_t *cand_type;           /* [C] */
    const uint32_t *key_table;          /* [4 * n_contigs] */
    const uint32_t *chrom_id;           /* [n_contigs] */
    const uint32_t *bed_off, *bed_lo, *bed_hi;  /* [n_contigs + 1], [bed_off[n_contigs]] x 2; bed_off NULL: no BED file */
    const uint32_t *base_off, *base_pos, *base_len, *base_uid;
    const uint8_t *base_hp;
} duet_tune_truth_problem;

/* Fills the six arrays *truth points to -- the caller's buffers, cand_* with room for C entries, group_pair_off for C + 1,
 * pair_uid for C -- and truth->n_uid (= n_base_uid), n_groups, n_pairs; *truth can then go to duet_tune_sweep_device as it is.
 * _device: every array of *prob and *truth is device memory; asynchronous on `stream` apart from ONE host round trip at the end
 * that learns n_groups and n_pairs.  _host: everything host memory; uploads, runs the same kernels, downloads, synchronises.
 * DUET_ERR_INVALID: a NULL array that is needed, or more key bits than 64 (bits of n_chrom - 1, 32 of ps, bits of n_base_uid, 1). */
DUET_API int duet_tune_truth_build_device(duet_ctx *ctx, const duet_tune_truth_problem *prob, duet_tune_truth *truth, void *stream);
DUET_API int duet_tune_truth_build_host(duet_ctx *ctx, const duet_tune_truth_problem *prob, duet_tune_truth *truth);

/* Strata: the sweep scored per set of CHROM texts in one pass.  A stratum is a set of CHROM texts; every row of the callset and
 * of the truth file belongs to exactly one stratum, by its CHROM text alone.  The record of (vector v, stratum s) is what
 * evaluation.py:99-159 forms when callset and truth set are both restricted to the rows whose CHROM text is in s -- the
 * evaluator matches, fills its six id sets and picks each phase-set group's labelling inside `for ch in range(24)`, so nothing
 * crosses a CHROM text.  A truth id is the text ID + CHROM + POS (:53), which two rows of different contigs can share ('.' at
 * chr1:2345678 and at chr12:345678): the restricted evaluator counts such an id once in a stratum that holds both contigs and
 * once in each stratum that holds one.  The caller therefore numbers the truth ids per (stratum, id text), stratum-major:
 * stratum s owns the ids uid_off[s] .. uid_off[s + 1], every offset a multiple of 32 (ids that name no record fill a range up),
 * so that a 32-bit word of the sweep's id sets belongs to one stratum.
 *   cand_stratum[c]   stratum (< n_strata) of candidate c; read for the candidates in the call list only
 *   group_stratum[g]  stratum of phase-set group g (all calls of a group share a CHROM id); read for groups with a call only */
#define DUET_TUNE_MAX_STRATA 64
typedef struct duet_tune_strata {
    uint32_t n_strata;              /* S, 1 .. DUET_TUNE_MAX_STRATA */
    uint32_t reserved;
    const uint8_t *cand_stratum;    /* [C] */
    const uint8_t *group_stratum;   /* [n_groups] */
    const uint32_t *uid_off;        /* [S + 1] HOST memory in both forms: uid_off[0] = 0, nondecreasing, every entry a multiple of 32,
                                       uid_off[S] == truth->n_uid */
} duet_tune_strata;

/* cand_stratum and group_stratum from the CHROM ids of a truth problem: runs after duet_tune_truth_build_* on the same *prob and
 * *truth.  The CHROM id of candidate c is prob->cand_chrom[c] (per-candidate form) or prob->chrom_id[prob->cand_contig[c]] (table
 * form); cand_stratum[c] = chrom_stratum[id] for every candidate and, for every call (DUET_TUNE_IN_CALLS in truth->cand_flags),
 * group_stratum[truth->cand_group[c]] too.  chrom_stratum[prob->n_chrom]; cand_stratum and group_stratum with room for C entries.
 * _device: every array is device memory; one kernel on `stream`, then the stream is synchronised for the kernel's status word
 * (4 bytes) -- a chrom_stratum entry >= n_strata, or a CHROM id >= n_chrom, writes stratum 0 and reports DUET_ERR_INVALID, it
 * never indexes past an array.  _host: host arrays; uploads, runs the same kernel, downloads cand_stratum[C] and
 * group_stratum[truth->n_groups].  DUET_ERR_INVALID also for n_strata of 0 or above DUET_TUNE_MAX_STRATA and for a NULL array
 * that is needed. */
DUET_API int duet_tune_strata_build_device(duet_ctx *ctx, const duet_tune_truth_problem *prob, const duet_tune_truth *truth,
                                           const uint8_t *chrom_stratum, uint32_t n_strata, uint8_t *cand_stratum,
                                           uint8_t *group_stratum, void *stream);
DUET_API int duet_tune_strata_build_host(duet_ctx *ctx, const duet_tune_truth_problem *prob, const duet_tune_truth *truth,
                                         const uint8_t *chrom_stratum, uint32_t n_strata, uint8_t *cand_stratum, uint8_t *group_stratum);

/* K vectors over C candidates, one duet_tune_counts record per (vector, stratum): counts[v * S + s].  truth and strata are
 * mandatory (pred and ps come from duet_tune_sweep_*); batching, workspace and the asynchrony of the _device form are
 * duet_tune_sweep_device's.  n_vec == 0 or n_cands == 0: DUET_OK, the counts zeroed.  DUET_ERR_INVALID: n_strata out of range,
 * uid_off not as described above, a NULL array that is needed and, in the _host form (which can read them), a cand_stratum entry
 * of a call or a group_stratum entry >= n_strata. */
DUET_API int duet_tune_sweep_strata_device(duet_ctx *ctx, const duet_tune_feature *feat, uint32_t n_cands, const duet_tune_thresholds *vec,
                                           uint32_t n_vec, const duet_tune_truth *truth, const duet_tune_strata *strata,
                                           duet_tune_counts *counts, void *stream);
DUET_API int duet_tune_sweep_strata_host(duet_ctx *ctx, const duet_tune_feature *feat, uint32_t n_cands, const duet_tune_thresholds *vec,
                                         uint32_t n_vec, const duet_tune_truth *truth, const duet_tune_strata *strata,
                                         duet_tune_counts *counts);

/* Leaf census (duet_tune_leaf.hip): which rule of the tree emits the calls, the wrong genotypes and the wrong haplotypes.  The
 * tree of predict_hp has 18 exits, numbered by its branch structure (a comparison that is false takes the else branch, for a nan
 * constant too, so the leaf a candidate ends at is the branch the code takes); a leaf fixes the pred up to the 1-or-2 choice:
 *    0 c0_call           class 0, sv_ratio == 1 and sv_num >= c0_min_sv_num                                   pred 3
 *    1 c0_drop           class 0 otherwise                                                                    0
 *    2 c2_low_ratio      class 2, not sv_ratio >= c2_min_sv_ratio                                             0
 *    3 c2_near_call      class 2, avgsc_diff <= c2_max_avgsc_diff, sv_num >= c2_min_sv_num                    3
 *    4 c2_near_few       ... not sv_num >= c2_min_sv_num                                                      0
 *    5 c2_far_call       class 2, not avgsc_diff <= c2_max_avgsc_diff, hap0 >= c2_min_hap0                    3
 *    6 c2_far_few        ... not hap0 >= c2_min_hap0                                                          0
 *    7 c1_one_low        class 1, one voting haplotype, sv_ratio <= c1_onehap_sv_ratio_lo                     0
 *    8 c1_one_het        ... <= c1_onehap_sv_ratio_hi, the hapread_ratio / avgsc_diff gate of :163 open       1 or 2
 *    9 c1_one_het_gated  ... the gate closed                                                                  0
 *   10 c1_one_hom        ... above c1_onehap_sv_ratio_hi, the gate open                                       3
 *   11 c1_one_hom_gated  ... the gate closed                                                                  0
 *   12 c1_two_low        class 1 otherwise, sv_ratio <= c1_twohap_sv_ratio_1                                  0
 *   13 c1_two_het_ref    ... <= c1_twohap_sv_ratio_2, ref_num > c1_max_ref_num                                0
 *   14 c1_two_het        ... <= c1_twohap_sv_ratio_2 otherwise                                                1 or 2
 *   15 c1_two_mid_hom    ... <= c1_twohap_sv_ratio_3, totsc_ratio <= c1_max_totsc_ratio                       3
 *   16 c1_two_mid_het    ... <= c1_twohap_sv_ratio_3 otherwise                                                1 or 2
 *   17 c1_two_hom        ... above c1_twohap_sv_ratio_3                                                       3
 * DUET_TUNE_LEAF_PRED gives the nominal pred, 1 standing for "1 or 2".
 *
 * One record per (vector v, stratum s, leaf): out[(v * S + s) * 18 + leaf], over the ELIGIBLE candidates of the stratum that end
 * at the leaf under the vector: n_cands all of them; n_listed those in the evaluator's call list (DUET_TUNE_IN_CALLS); n_matched
 * listed and DUET_TUNE_MATCHED -- neither depends on the pred: for a pred-0 leaf they say how many matchable candidates the rule
 * drops; n_calls listed and pred != 0; call_tp, call_gt, n_raise as duet_tune_counts has them, for those calls; call_hp the calls
 * whose same / flip bit agrees with the labelling their phase-set group takes in the plain sweep of that vector (decided over all
 * leaves together).  Summed over the leaves, n_calls, call_tp, call_gt, call_hp and n_raise are duet_tune_sweep_device's (S = 1)
 * and duet_tune_sweep_strata_device's (v, s); summed over the strata they are the S = 1 record.  Base-side set sizes are not
 * broken down: a truth id hit from two leaves belongs to neither.
 * truth may be NULL: only n_cands and n_calls (= pred != 0) are filled.  strata may be NULL: S = 1; otherwise only n_strata and
 * cand_stratum are read, cand_stratum for EVERY candidate (duet_tune_strata_build_* writes it so); a group lies inside one CHROM
 * id, hence one stratum, so the truth arrays may carry either id numbering.  Batching, workspace and asynchrony are
 * duet_tune_sweep_device's, which runs per batch for the groups' labellings: a census changes nothing a later sweep returns.
 * n_vec == 0 or n_cands == 0: DUET_OK, the records zeroed.  DUET_ERR_INVALID: n_strata of 0 or above DUET_TUNE_MAX_STRATA, a NULL
 * array that is needed and, in the _host form (which can read them), a cand_stratum entry >= n_strata or a call's group index
 * >= n_groups; the _device form counts a candidate with such a stratum in stratum 0.  _host: host arrays; synchronises. */
#define DUET_TUNE_N_LEAVES 18
#define DUET_TUNE_LEAF_NAMES                                                                                                      \
    {"c0_call", "c0_drop", "c2_low_ratio", "c2_near_call", "c2_near_few", "c2_far_call", "c2_far_few", "c1_one_low", "c1_one_het", \
     "c1_one_het_gated", "c1_one_hom", "c1_one_hom_gated", "c1_two_low", "c1_two_het_ref", "c1_two_het", "c1_two_mid_hom",        \
     "c1_two_mid_het", "c1_two_hom"}
#define DUET_TUNE_LEAF_PRED {3, 0, 0, 3, 0, 3, 0, 0, 1, 0, 3, 0, 0, 0, 1, 3, 1, 3}
typedef struct duet_tune_leaf_counts {
    uint32_t n_cands, n_listed, n_matched, n_calls, call_tp, call_gt, call_hp, n_raise;
} duet_tune_leaf_counts;
DUET_API int duet_tune_leaf_census_device(duet_ctx *ctx, const duet_tune_feature *feat, uint32_t n_cands, const duet_tune_thresholds *vec,
                                          uint32_t n_vec, const duet_tune_truth *truth, const duet_tune_strata *strata,
                                          duet_tune_leaf_counts *out, void *stream);
DUET_API int duet_tune_leaf_census_host(duet_ctx *ctx, const duet_tune_feature *feat, uint32_t n_cands, const duet_tune_thresholds *vec,
                                        uint32_t n_vec, const duet_tune_truth *truth, const duet_tune_strata *strata,
                                        duet_tune_leaf_counts *out);

/* Evidence table (duet_evidence.hip): per candidate the exit of the tree it takes under ONE vector, and
 * one text row per candidate -- its evidence, the rule that decided it and the call.
 *
 * duet_tune_leaves_*: out_leaf[c] = the leaf (0 .. 17, the numbering above: what duet_tune_leaf_census_* counts) of an eligible
 * candidate, DUET_TUNE_LEAF_NO_SEED for one that is kept but not eligible (its contig has no seed phase set),
 * DUET_TUNE_LEAF_FILTERED for one that is not kept; out_pred[c] = what duet_tune_sweep_device writes to out_pred for that vector
 * (0 for a candidate that is not eligible).  *vec is HOST memory in both forms.  _device: feat, out_leaf, out_pred device memory;
 * asynchronous on `stream`.  _host: host arrays; uploads, runs the same kernel, downloads, synchronises.  n_cands == 0: DUET_OK.
 * DUET_ERR_INVALID: a NULL array (or vector) with n_cands > 0. */
#define DUET_TUNE_LEAF_NO_SEED 0xFDu
#define DUET_TUNE_LEAF_FILTERED 0xFEu
DUET_API int duet_tune_leaves_device(duet_ctx *ctx, const duet_tune_feature *feat, uint32_t n_cands, const duet_tune_thresholds *vec,
                                     uint8_t *out_leaf, uint8_t *out_pred, void *stream);
DUET_API int duet_tune_leaves_host(duet_ctx *ctx, const duet_tune_feature *feat, uint32_t n_cands, const duet_tune_thresholds *vec,
                                   uint8_t *out_leaf, uint8_t *out_pred);

/* The rows: one per candidate, in candidate order (no sort, no compaction), tab-separated, one '\n' behind each row:
 *     CHROM POS SVTYPE SVLEN SVREAD REFREAD MARKS RULE CLASS HAP1 HAP2 HAP0 VOTERS PCSUM1 PCSUM2 PS HP
 * (DUET_EVIDENCE_COLUMNS; the header line stays with the host).  POS = cand_pos; SVLEN = cand_svlen, unsigned; SVREAD, REFREAD,
 * MARKS = the record's svread, refread, deg; RULE = `filtered`, `no_seed` or the leaf's name (DUET_TUNE_LEAF_NAMES) for leaf[c];
 * CLASS = cls where the record is kept, else `.`; HAP1 HAP2 HAP0 VOTERS PCSUM1 PCSUM2 PS = hap1, hap2, hap0, allhap, t1, t2, ps
 * where the record is eligible, else `.` each (t1, t2: full unsigned 64-bit decimals); HP = 1|0, 0|1, 1|1 for pred 1, 2, 3 and
 * `.` for pred 0.  Integers only: every binary64 feature the tree compares is a quotient of these columns.
 * Text form (pool != NULL; a caller's VCF): CHROM = pool[str_off[4c] .. str_off[4c+1]), SVTYPE = pool[str_off[4c+3] ..
 * str_off[4c+4]) -- the layout of duet_rows_problem; either piece may be empty.  Table form (pool == NULL; a cluster result):
 * CHROM = chrom[cand_contig[c]], SVTYPE = DEL, INS, INV, DUP for cand_type[c] = 0 .. 3, cand_svlen = the result's cand_span.
 * _device: every array device memory except chrom (HOST), out_text device; asynchronous on `stream` apart from ONE host round
 * trip that learns the text's size and the status word.  _host: everything HOST; uploads, runs the same kernels, copies the text
 * back, synchronises.
 * Both: *out_len = the text's exact size, always; when out_cap is smaller nothing is written and the call returns
 * DUET_ERR_INVALID.  A row is at most its CHROM and SVTYPE pieces + 180 bytes, so
 *     n_cands * (longest CHROM piece + longest SVTYPE piece + 180)           (table form: SVTYPE is 3 bytes)
 * always suffices.  Row offsets are 64-bit: a text of 4 GiB or more is legal.  out_text may sit at any byte address.
 * DUET_ERR_INVALID, nothing written, duet_last_error names the case: a NULL array that is needed; a leaf code other than 0 .. 17,
 * DUET_TUNE_LEAF_NO_SEED, DUET_TUNE_LEAF_FILTERED; pred > 3; string offsets that descend or leave the pool (text form); a type
 * code > 3, cand_contig >= n_contigs, n_contigs of 0 or more than 65535, a NULL chrom[k] (table form).  n_cands == 0: DUET_OK, zero
 * bytes.  The workspace is the context's own (grown, never shrunk) and not E/F's: a call changes nothing a later duet_ef_run_* or
 * duet_ef_features_* on the same context returns. */
#define DUET_EVIDENCE_COLUMNS                                                                                                     \
    {"CHROM", "POS", "SVTYPE", "SVLEN", "SVREAD", "REFREAD", "MARKS", "RULE", "CLASS", "HAP1", "HAP2", "HAP0", "VOTERS", "PCSUM1", \
     "PCSUM2", "PS", "HP"}
typedef struct duet_evidence_problem {
    uint32_t n_cands, n_contigs;            /* n_contigs: table form only */
    const duet_tune_feature *feat;          /* [C] */
    const uint8_t *leaf, *pred;             /* [C] from duet_tune_leaves_* */
    const uint32_t *cand_pos, *cand_svlen;  /* [C] */
    const char *pool;                       /* text form */
    uint64_t pool_bytes;
    const uint32_t *str_off;                /* [4C+1] */
    const uint16_t *cand_contig;            /* [C] table form */
    const uint8_t *cand_type;               /* [C] */
    const char *const *chrom;               /* HOST [n_contigs], NUL-terminated */
} duet_evidence_problem;
DUET_API int duet_evidence_rows_device(duet_ctx *ctx, const duet_evidence_problem *prob, char *out_text, uint64_t out_cap,
                                       uint64_t *out_len, void *stream);
DUET_API int duet_evidence_rows_host(duet_ctx *ctx, const duet_evidence_problem *prob, char *out_text, uint64_t out_cap,
                                     uint64_t *out_len);

/* The line of one axis (duet_tune_line.hip): with the other 13 constants fixed, every count of a sweep is a piecewise-constant
 * function of one constant and changes only where it crosses a value of the feature it is compared with, so one vector per
 * distinct value plus one sentinel covers every behaviour of the axis.  axis = the field's index in duet_tune_thresholds.  The
 * compared feature (binary64, the expressions of the sweep's own tree) and who takes part -- eligible candidates only:
 *   0 svread, class 0 (>=)      1 sv_ratio, 2 avgsc_diff, 3 svread, 4 hap0: class 2 (>=, <=, >=, >=)
 *   5, 6 sv_ratio, 7 hapread_ratio, 8 avgsc_diff: class 1 with one voting haplotype (<=; 7 also >)
 *   9, 10, 12 sv_ratio, 11 refread, 13 totsc_ratio: class 1 otherwise (<=; 11 >)
 * The participants do not depend on *base: a value no candidate is tested against under *base only adds a vector that scores like
 * its neighbour.  With x_1 < .. < x_D the distinct values, the line is -inf, x_1 .. x_D for the <= and > axes and x_1 .. x_D, +inf
 * for the >= axes: D + 1 values; out_vec[i] = *base with the axis field replaced by the i-th of them.  max_values = N >= 2 and
 * D + 1 > N: only the line's entries floor(i * D / (N - 1)), i = 0 .. N - 1, are written (both ends among them); 0: all.
 * *n_distinct = D, *n_vec = the vectors written.  n_cands == 0 or no participant: one vector, with the sentinel.
 * _device: feat[C] and out_vec (room for n_cands + 1 vectors) are device memory; base, n_vec and n_distinct host memory.  One host
 * round trip (D and the status word), then the vectors are written asynchronously on `stream`; the workspace is grown, never
 * shrunk.  _host: the same with host arrays; synchronises.
 * DUET_ERR_INVALID: axis > 13, max_values == 1, a NULL array that is needed.  DUET_ERR_DIV_ZERO: a participant's feature is not
 * finite (deg == 0, or svread + refread == 0 where duet_ef_features_device reports the same); no vector is written. */
DUET_API int duet_tune_line_device(duet_ctx *ctx, const duet_tune_feature *feat, uint32_t n_cands, const duet_tune_thresholds *base,
                                   uint32_t axis, uint32_t max_values, duet_tune_thresholds *out_vec, uint32_t *n_vec,
                                   uint32_t *n_distinct, void *stream);
DUET_API int duet_tune_line_host(duet_ctx *ctx, const duet_tune_feature *feat, uint32_t n_cands, const duet_tune_thresholds *base,
                                 uint32_t axis, uint32_t max_values, duet_tune_thresholds *out_vec, uint32_t *n_vec,
                                 uint32_t *n_distinct);

/* The line of the PC cap (duet_tune_capline.hip).  A mark votes iff its read is tagged and pc <= cap, so the feature records of
 * duet_ef_features_cap_* are a piecewise-constant function of the cap.  The participants are the marks of kept candidates
 * (cand_svlen >= svlen_thres, cand_svread >= suppread_thres, cand_gt_ok) whose read is tagged (index not DUET_MARK_ABSENT and
 * < n_reads, tag word not all-ones) with pc <= 2^30 - 3; the hap field plays no part, and a saturated pc of 2^30 - 2 never votes.
 * With x_1 < .. < x_D their distinct pc values, a cap in [x_i, x_i+1) gives the records of cap x_i byte for byte, a cap below
 * x_1 those of cap 0, a cap from x_D up those of x_D.  The line is x_1 .. x_D with 0 in front unless x_1 == 0: L = D or D + 1
 * values, ascending; no participant: the one value 0.  The best score on it is the exact optimum of the cap over 0 .. 2^30 - 3.
 * max_values = N >= 2 and L > N: only the line's entries floor(i * (L - 1) / (N - 1)), i = 0 .. N - 1, are written (both ends
 * among them); 0: all.  *n_distinct = D, *n_caps = the values written; out_caps needs room for max_values values when that is
 * non-zero, otherwise for min(n_marks, 2^30 - 2) + 1.
 * duet_svim_cap_line_*: the same for the raw marks of a duet_svim_problem, without clustering -- the participants are EVERY raw
 * mark whose read is tagged with pc <= 2^30 - 3, a superset of what any -c / -r setting of that extraction keeps, so one line
 * serves all of them.  The price: a value that no kept mark carries costs one evaluation and scores like its lower neighbour.
 * Of *prob only marks.n_marks, mark_read, read_tag and n_reads are read.
 * _device: the arrays of *prob (cand_ctg_off aside) and out_caps are device memory; n_caps and n_distinct host memory.  One host
 * round trip (D and x_1), then the values are written asynchronously on `stream`.  The workspace is the entry's own (16 bytes per
 * mark, the sort's histogram and scan partials; grown, never shrunk): a call changes nothing that a later duet_ef_run_*,
 * duet_ef_features_* or duet_ef_features_cap_* returns.  _host: the same with host arrays, out_caps host; synchronises.
 * DUET_ERR_INVALID: max_values == 1, a NULL array that is needed, whatever duet_ef_run_* refuses in *prob.  n_cands == 0 or
 * n_marks == 0: DUET_OK, the line [0]. */
DUET_API int duet_tune_cap_line_device(duet_ctx *ctx, const duet_ef_problem *prob, uint32_t max_values, uint32_t *out_caps,
                                       uint32_t *n_caps, uint32_t *n_distinct, void *stream);
DUET_API int duet_tune_cap_line_host(duet_ctx *ctx, const duet_ef_problem *prob, uint32_t max_values, uint32_t *out_caps,
                                     uint32_t *n_caps, uint32_t *n_distinct);
DUET_API int duet_svim_cap_line_device(duet_ctx *ctx, const duet_svim_problem *prob, uint32_t max_values, uint32_t *out_caps,
                                       uint32_t *n_caps, uint32_t *n_distinct, void *stream);
DUET_API int duet_svim_cap_line_host(duet_ctx *ctx, const duet_svim_problem *prob, uint32_t max_values, uint32_t *out_caps,
                                     uint32_t *n_caps, uint32_t *n_distinct);

/* ---------------------------------------------------------------------------------------------
 * Phase-set links (duet_pslinks.hip): how the SV candidates tie neighbouring phase sets together.  A
 * candidate whose supporting reads fall into two phase sets says which haplotype of the one is which haplotype of the other:
 * reads of haplotype 1 in phase set A and of haplotype 2 in phase set B mean that A's haplotype 1 and B's haplotype 2 are one
 * chromosome copy.  One record per pair of phase sets collects that over all candidates of a contig.  tests/ps_links_ref.py
 * states the rule in plain Python.
 *
 *   Candidates  the kept ones: cand_svlen >= svlen_thres, cand_svread >= suppread_thres, cand_gt_ok != 0.  Neither the seed sets
 *               nor the call play a part.
 *   Voters      a mark votes iff its read index is not DUET_MARK_ABSENT and < n_reads, its tag word is not all-ones,
 *               pc <= pc_cap and hap is 1 or 2 (a tagged read with hap 3 takes no part: unlike `allhap`).  A read marked twice
 *               counts twice, as in the vote.
 *   Groups      a candidate's voters grouped by PS: h1, h2 = the voters of haplotype 1, 2; d = h1 - h2.
 *   Pairs       the candidate's distinct PS values ascending (unsigned); each two neighbours (a, b), a < b, are one observation
 *               on the link (contig, a, b): a candidate with G groups gives G - 1 observations, none between non-neighbours.
 *   Kind        open when d_a == 0 or d_b == 0; same when both have the same sign; flip otherwise.  Weight w = min(|d_a|, |d_b|)
 *               (0 for an open observation).
 *   Record      one per distinct (contig, ps_a, ps_b): n_same, n_flip, n_open = the observations of each kind, n_sv their sum;
 *               w_same, w_flip = the weights summed over the same / flip observations; pos_min, pos_max over the cand_pos of
 *               the contributing candidates; contig = the contig index; reserved = 0.  Records ascend by (contig, ps_a, ps_b),
 *               the PS values compared as full unsigned 32-bit numbers.
 * Every sum is an integer sum and no kernel of the unit uses an atomic (the shared sort's histogram counts with integer atomics up
 * to 1024 tiles: sums), so nothing depends on the order in which anything arrives: two runs give identical bytes.
 *
 * pc_cap: 0 .. 2^30 - 3 (DUET_PC_MAX for the reference's cap); above: DUET_ERR_INVALID.
 * *n_links = the exact record count, always (0 on a refusal of the arguments).  n_links > out_cap: nothing is written to out and
 * the call returns DUET_ERR_INVALID.  max(n_marks, 1) - 1 records always suffice.  out may be NULL when out_cap is 0.
 * Whatever duet_ef_run_* refuses in *prob is refused here.  n_cands == 0 or n_marks == 0: DUET_OK, 0 links, no array is read.
 * _device: the arrays of *prob (cand_ctg_off aside: HOST, as always) and out are device memory, n_links host memory.  The call makes
 * up to THREE host round trips, each a few words: the number of voting marks of the candidates with two or more phase sets (sizes
 * the first sort; 0 ends the call), the number of observations (sizes the second and third sort), the number of records (checked
 * against out_cap before anything is written).  The records are written asynchronously on `stream`.
 * _host: host arrays, out host; uploads, runs the same kernels, copies the records back, synchronises.
 * The workspace is the entry's own (about 60 bytes per voting mark of a multi-phase-set candidate, 8 per candidate; grown, never
 * shrunk): a call changes nothing that a later duet_ef_run_*, duet_ef_features_* or duet_tune_* returns.
 *
 * duet_svim_ps_links_*: the same for the candidates of the fused pipeline -- clusters and adapts as duet_svim_features_device does
 * (every call clusters again: the entry keeps no state; one more host round trip for the candidates per contig), then the links
 * of the adapted problem.  The cluster result stays in *res; _device: *n_cands_host = the candidate count (mandatory); _host: arrays
 * as for duet_svim_phase_host, the count in *res->n_cands. */
typedef struct duet_ps_link {            /* 56 bytes */
    uint64_t w_same, w_flip;
    uint32_t contig, ps_a, ps_b;
    uint32_t n_sv, n_same, n_flip, n_open;
    uint32_t pos_min, pos_max;
    uint32_t reserved;                   /* 0 */
} duet_ps_link;
DUET_API int duet_ps_links_device(duet_ctx *ctx, const duet_ef_problem *prob, uint32_t pc_cap, duet_ps_link *out, uint32_t out_cap,
                                  uint32_t *n_links, void *stream);
DUET_API int duet_ps_links_host(duet_ctx *ctx, const duet_ef_problem *prob, uint32_t pc_cap, duet_ps_link *out, uint32_t out_cap,
                                uint32_t *n_links);
DUET_API int duet_svim_ps_links_device(duet_ctx *ctx, const duet_svim_problem *prob, const duet_cluster_result *res, uint32_t pc_cap,
                                       duet_ps_link *out, uint32_t out_cap, uint32_t *n_links, uint32_t *n_cands_host, void *stream);
DUET_API int duet_svim_ps_links_host(duet_ctx *ctx, const duet_svim_problem *prob, const duet_cluster_result *res, uint32_t pc_cap,
                                     duet_ps_link *out, uint32_t out_cap, uint32_t *n_links);

/* ---------------------------------------------------------------------------------------------
 * Read tags from phased SVs (duet_readtags.hip): which haplotype each supporting read lies on.  A
 * heterozygous call 1|0 in phase set P says that each of its supporting reads lies on haplotype 1 of P -- the reads without a
 * usable tag of their own included.  The mark CSR goes candidate -> reads; this is its transpose, read -> candidates, summed per
 * (read name, phase set).  tests/read_tags_ref.py states the rule in plain Python.
 *
 *   Slots       CSR slot i (cand_off[c] <= i < cand_off[c + 1]) is raw mark mark_order[i], or raw mark i when mark_order is NULL;
 *               mark_read and mark_name are indexed by raw mark.  mark_name is the read's identity: equal for all marks of one
 *               read and < n_names (names are interned per contig: one name, one contig, one read index).
 *   Marks       every mark of a candidate with pred 1 (1|0) or 2 (0|1) contributes; pred 0 and 3 say nothing about a read's
 *               haplotype.  A read listed twice in one candidate counts twice, as in the vote.
 *   Record      one per distinct (name, ps[c]) over the contributing marks: n_h1, n_h2 = its marks from 1|0 / 0|1 calls; pos_min,
 *               pos_max over cand_pos; contig = the candidates' contig (cand_contig[c], or the k with cand_ctg_off[k] <= c <
 *               cand_ctg_off[k + 1]); read = the mark_read of its marks; reserved = 0.  Records ascend by (name, ps), PS compared
 *               as a full unsigned 32-bit number.
 *   Status      sv = 1 if n_h1 > n_h2, 2 if n_h2 > n_h1, else 0.  The read's tag is usable when `read` is not DUET_MARK_ABSENT
 *               and < n_reads, the word is not all-ones, hap is 1 or 2 and pc <= pc_cap.  In this order:
 *                 DUET_READ_TAG_OTHER_PS   a usable tag whose PS is not the record's
 *                 DUET_READ_TAG_TIE        sv == 0, whatever the tag
 *                 DUET_READ_TAG_AGREE      a usable tag and sv == hap;  DUET_READ_TAG_DISAGREE  sv is the other haplotype
 *                 DUET_READ_TAG_NEW        no usable tag: the SVs place a read WhatsHap could not
 *   Refused     contributing marks of one name on two contigs, or with two different mark_read values: DUET_ERR_INVALID, nothing
 *               written, *n_recs = 0.  Found from the minimum and maximum inside the reduction, not by a pass of its own.
 * Integer sums, minima and maxima only, and no kernel of the unit uses an atomic (the shared sort's histogram counts with integer
 * atomics up to 1024 tiles: sums): two runs give identical bytes.
 *
 * pc_cap: 0 .. 2^30 - 3; above: DUET_ERR_INVALID.  Also refused, nothing written: both or neither of cand_ctg_off and cand_contig;
 * pred > 3; mark_name >= n_names; mark_order >= n_marks; a cand_ctg_off that does not ascend from 0 to n_cands; a NULL array that is
 * needed.  *n_recs = the exact record count, also when out_cap is smaller: then nothing is written and the call returns
 * DUET_ERR_INVALID.  n_marks records always suffice.  out may be NULL when out_cap is 0.  n_cands == 0, n_marks == 0 or no
 * candidate with pred 1 or 2: DUET_OK, 0 records.
 * _device: the arrays of *prob (cand_ctg_off aside: HOST) and out are device memory, n_recs host memory.  Up to THREE host round
 * trips, each a few words: the number of contributing marks V (sizes the sort; 0 ends the call), the record count (checked against
 * out_cap), the refusals of the reduction -- the records wait in the workspace until that word is read, then are copied to out
 * asynchronously on `stream`.  _host: host arrays, out host; uploads, runs the same kernels, copies the records back, synchronises.
 * The workspace is the entry's own (32 bytes per contributing mark + the sort's histogram, 8 per candidate, 40 per record; grown,
 * never shrunk): a call changes nothing that a later duet_ef_run_*, duet_ef_features_*, duet_tune_* or duet_ps_links_* returns.
 *
 * The rows (duet_read_tags_rows_*): one per record, in record order, tab-separated, one '\n' behind each row:
 *     CHROM READ PS N_SV N_H1 N_H2 HP_SV TAG_HP TAG_PS TAG_PC STATUS POS_MIN POS_MAX
 * (DUET_READ_TAG_COLUMNS; the header line stays with the host).  CHROM = names->chrom[contig]; READ = name_pool[name_off[name] ..
 * name_off[name + 1]); N_SV = n_h1 + n_h2; HP_SV = 1, 2 or `.` for sv; TAG_HP TAG_PS TAG_PC = the read's own tag word, whatever
 * the cap: all three `.` when `read` is DUET_MARK_ABSENT or >= n_reads or the word is all-ones, TAG_HP `.` for hap 0 and 3;
 * STATUS = DUET_READ_TAG_STATUS_NAMES[status].  Of *names only name_off, name_pool, n_names, n_contigs and chrom are read.
 * _device: recs, name_off, name_pool, read_tag and out_text device memory, chrom HOST; asynchronous on `stream` apart from ONE host
 * round trip that learns the text's size and the status words.  _host: everything HOST.
 * Both: *out_len = the text's exact size, always; when out_cap is smaller nothing is written and the call returns
 * DUET_ERR_INVALID.  A row is at most its CHROM and READ pieces + 103 bytes, so
 *     n_recs * (longest CHROM text + longest name + 104)
 * always suffices.  Row offsets are 64-bit.  DUET_ERR_INVALID, nothing written: a record's name >= n_names, contig >= n_contigs
 * or status > 4; name offsets that descend; n_contigs of 0 or more than 65535; a NULL array or text that is needed.  n_recs == 0:
 * DUET_OK, zero bytes.  The workspace is the entry's own. */
#define DUET_READ_TAG_AGREE 0u
#define DUET_READ_TAG_DISAGREE 1u
#define DUET_READ_TAG_TIE 2u
#define DUET_READ_TAG_NEW 3u
#define DUET_READ_TAG_OTHER_PS 4u
#define DUET_READ_TAG_STATUS_NAMES {"agree", "disagree", "tie", "new", "other_ps"}
#define DUET_READ_TAG_COLUMNS \
    {"CHROM", "READ", "PS", "N_SV", "N_H1", "N_H2", "HP_SV", "TAG_HP", "TAG_PS", "TAG_PC", "STATUS", "POS_MIN", "POS_MAX"}
typedef struct duet_read_tag_rec {       /* 40 bytes */
    uint32_t name, contig, ps, read;
    uint32_t n_h1, n_h2, pos_min, pos_max;
    uint32_t status;
    uint32_t reserved;                   /* 0 */
} duet_read_tag_rec;
typedef struct duet_read_tags_problem {
    uint32_t n_cands, n_marks, n_reads, n_names;
    uint32_t n_contigs, reserved;        /* n_contigs: with cand_ctg_off */
    const uint32_t *cand_off;            /* [C+1] */
    const uint32_t *mark_order;          /* [M] or NULL (identity) */
    const uint32_t *mark_read;           /* [M] per raw mark: index into read_tag, or DUET_MARK_ABSENT */
    const uint32_t *mark_name;           /* [M] per raw mark */
    const uint8_t *pred;                 /* [C] 0 .. 3 */
    const uint32_t *ps, *cand_pos;       /* [C] */
    const uint32_t *cand_ctg_off;        /* HOST [K+1], or NULL ... */
    const uint16_t *cand_contig;         /* ... then [C], non-descending */
    const uint64_t *read_tag;            /* [R] */
} duet_read_tags_problem;
DUET_API int duet_read_tags_device(duet_ctx *ctx, const duet_read_tags_problem *prob, uint32_t pc_cap, duet_read_tag_rec *out,
                                   uint32_t out_cap, uint32_t *n_recs, void *stream);
DUET_API int duet_read_tags_host(duet_ctx *ctx, const duet_read_tags_problem *prob, uint32_t pc_cap, duet_read_tag_rec *out,
                                 uint32_t out_cap, uint32_t *n_recs);
DUET_API int duet_read_tags_rows_device(duet_ctx *ctx, const duet_read_tag_rec *recs, uint32_t n_recs, const duet_callset_names *names,
                                        const uint64_t *read_tag, uint32_t n_reads, char *out_text, uint64_t out_cap, uint64_t *out_len,
                                        void *stream);
DUET_API int duet_read_tags_rows_host(duet_ctx *ctx, const duet_read_tag_rec *recs, uint32_t n_recs, const duet_callset_names *names,
                                      const uint64_t *read_tag, uint32_t n_reads, char *out_text, uint64_t out_cap, uint64_t *out_len);

/* ---------------------------------------------------------------------------------------------
 * Joined phase sets (duet_psjoin.hip): the phase-set links say which phase sets are one block and in which
 * sense; duet_amd/ps_links.py: blocks turns them into a table (contig, PS) -> (BLOCK, FLIP).  Here the table is applied to the read
 * tags -- a joined run is the ordinary run on the remapped tags -- and the calls of the two runs are compared candidate by
 * candidate.  tests/ps_join_ref.py states both rules in plain Python.
 *
 *   Table       n_blocks rows of duet_ps_block, ALWAYS host memory (like cand_ctg_off: thousands of rows; the library checks and
 *               stages them): strictly ascending by (contig, ps), PS compared as a full unsigned 32-bit number; contig < n_contigs;
 *               flip 0 or 1.  Otherwise DUET_ERR_INVALID, nothing written.  The same PS on two contigs: two keys.
 *   Tag word    read r of contig k (read_off[k] <= r < read_off[k + 1]) with tag word t.  The all-ones word is untouched,
 *               whatever the table holds.  (k, ps(t)) in the table: ps becomes BLOCK, and with FLIP == 1 hap 1 becomes 2 and 2
 *               becomes 1; hap 0 and 3 stay; pc is kept bit for bit.  A word whose key is not in the table is unchanged.
 *   Change      of a candidate called (p0, s0) before and (p1, s1) after (pred, ps of duet_ef_run_*), the first rule that holds:
 *                 DUET_PS_JOIN_NONE        p0 == 0 and p1 == 0
 *                 DUET_PS_JOIN_GAINED      p0 == 0
 *                 DUET_PS_JOIN_LOST        p1 == 0
 *                 DUET_PS_JOIN_SAME        (p1, s1) == (p0, s0)
 *                 DUET_PS_JOIN_RELABELLED  (p1, s1) == (p', s'): s' = BLOCK of (contig, s0), or s0 when the key is not in the table;
 *                                          p' = 3 - p0 when that row's FLIP is 1 and p0 is 1 or 2, else p0
 *                 DUET_PS_JOIN_TO_HET      p0 == 3 and p1 is 1 or 2
 *                 DUET_PS_JOIN_TO_HOM      p0 is 1 or 2 and p1 == 3
 *                 DUET_PS_JOIN_OTHER       everything else
 * Integers only.  The counts are sums of per-wavefront popcounts, added with integer atomics to words of the call's own: nothing
 * depends on the order of arrival, two runs give identical bytes.
 *
 * duet_ps_join_tags_*: out_tag[r] = the remapped read_tag[r] for every r < n_reads; out_tag may be read_tag itself.  *n_changed =
 * the number of words whose bits changed.  read_off is HOST memory, [n_contigs + 1], ascending from 0 to n_reads (empty contigs
 * are allowed); otherwise DUET_ERR_INVALID.  n_contigs == 0 is refused unless n_reads and n_blocks are 0 too.  Every refusal is
 * decided on the host before anything is written.  n_reads == 0 or n_blocks == 0: DUET_OK, out_tag a copy, *n_changed = 0.
 * _device: read_tag and out_tag device memory, n_changed host memory; ONE host round trip (the count).  _host: host arrays.
 *
 * duet_ps_join_diff_*: change[c] = the code of candidate c, counts[i] = the candidates with code i.  Exactly one of cand_ctg_off
 * (HOST, [n_contigs + 1], ascending from 0 to n_cands) and cand_contig ([n_cands], each < n_contigs) names the candidates' contigs;
 * both or neither: DUET_ERR_INVALID.  A pred above 3 or a cand_contig >= n_contigs is found on the device, through a word of its
 * own: DUET_ERR_INVALID, nothing written to change, counts zero.  n_cands == 0: DUET_OK, zero counts.
 * _device: pred0, ps0, pred1, ps1, cand_contig and change device memory, counts[8] host memory; ONE host round trip (the counts
 * and the refusals), after which the codes are copied to change asynchronously on `stream`.  _host: host arrays.
 * The workspace is the entries' own (16 bytes per table row, 1 per candidate; grown, never shrunk): a call changes nothing that
 * a later duet_ef_run_*, duet_ef_features_*, duet_tune_*, duet_ps_links_* or duet_read_tags_* returns. */
#define DUET_PS_JOIN_NONE 0u
#define DUET_PS_JOIN_GAINED 1u
#define DUET_PS_JOIN_LOST 2u
#define DUET_PS_JOIN_SAME 3u
#define DUET_PS_JOIN_RELABELLED 4u
#define DUET_PS_JOIN_TO_HET 5u
#define DUET_PS_JOIN_TO_HOM 6u
#define DUET_PS_JOIN_OTHER 7u
#define DUET_PS_JOIN_CHANGE_NAMES {"none", "gained", "lost", "same", "relabelled", "to_het", "to_hom", "other"}
typedef struct duet_ps_block {           /* 16 bytes */
    uint32_t contig, ps, block, flip;
} duet_ps_block;
DUET_API int duet_ps_join_tags_device(duet_ctx *ctx, const uint64_t *read_tag, const uint32_t *read_off, uint32_t n_contigs,
                                      uint32_t n_reads, const duet_ps_block *blocks, uint32_t n_blocks, uint64_t *out_tag,
                                      uint32_t *n_changed, void *stream);
DUET_API int duet_ps_join_tags_host(duet_ctx *ctx, const uint64_t *read_tag, const uint32_t *read_off, uint32_t n_contigs,
                                    uint32_t n_reads, const duet_ps_block *blocks, uint32_t n_blocks, uint64_t *out_tag,
                                    uint32_t *n_changed);
DUET_API int duet_ps_join_diff_device(duet_ctx *ctx, uint32_t n_cands, const uint8_t *pred0, const uint32_t *ps0, const uint8_t *pred1,
                                      const uint32_t *ps1, const uint32_t *cand_ctg_off, const uint16_t *cand_contig,
                                      uint32_t n_contigs, const duet_ps_block *blocks, uint32_t n_blocks, uint8_t *change,
                                      uint32_t *counts, void *stream);
DUET_API int duet_ps_join_diff_host(duet_ctx *ctx, uint32_t n_cands, const uint8_t *pred0, const uint32_t *ps0, const uint8_t *pred1,
                                    const uint32_t *ps1, const uint32_t *cand_ctg_off, const uint16_t *cand_contig,
                                    uint32_t n_contigs, const duet_ps_block *blocks, uint32_t n_blocks, uint8_t *change,
                                    uint32_t *counts);

/* ---------------------------------------------------------------------------------------------
 * Blocks of the phase-set links, on the device (duet_psblocks.hip): the table that duet_amd/ps_links.py:
 * blocks(records, min_sv) builds on the host -- that function is the normative text -- built from resident records, and applied
 * to the read tags without a host table in between.  For callers that rebuild it many times (duet_amd.tune under --join_ps).
 * tests/ps_blocks_ref.py states the round-based build in plain Python.
 *
 *   Nodes       every (contig, ps) that occurs as ps_a or ps_b of any record, trusted or not; one row per node, ascending by
 *               (contig, ps), PS compared as a full unsigned 32-bit number.
 *   Trusted     a record whose verdict is same or flip -- (n_same, w_same) against (n_flip, w_flip), lexicographically -- and
 *               whose winning side has n_win >= min_sv.
 *   Order       strict: (-n_win, -w_win, row index).
 *   Forest      Kruskal in that order: a link joins two components or is checked against the sense they imply; one that
 *               contradicts it is not applied and its row index goes to the conflicts, in the order met.  BLOCK = the smallest
 *               PS of the component, FLIP = the node's sense relative to that PS.
 * The device builds the same forest in rounds: every component takes its best-ranked outgoing link (the order is strict, so the
 * forest is unique); a trusted link outside the forest is a conflict exactly when the parities of its ends differ from its sense.
 * Integers only; the atomics are minima and sums, so two runs give identical bytes.
 *
 * duet_ps_blocks_*: links as duet_ps_links_* writes them (n_links records, strictly ascending by (contig, ps_a, ps_b), ps_a < ps_b,
 * contig < n_contigs).  out_rows: n_rows rows, 2 * n_links always suffice.  out_conflicts: the conflicting row indices in rank
 * order; it may be NULL (with conflicts_cap 0): none is written, counts->n_conflicts is still exact.  *counts (HOST): the rows, the
 * trusted records, the conflicts, the components (distinct BLOCK values per contig, summed).
 * DUET_ERR_INVALID, nothing written to either output, *counts zero: min_sv < 1; n_links >= 2^30; a record with ps_a >= ps_b, with
 * contig >= n_contigs, or not strictly above the record before it (found on the device, through a word of the call's own; the
 * results wait in the workspace until that word has been read); n_rows > rows_cap; out_conflicts given and n_conflicts >
 * conflicts_cap.  n_links == 0: DUET_OK, zero counts, no array is read.
 * _device: links, out_rows and out_conflicts device memory; ONE host round trip (the counts and the refusal word), after which the
 * results are copied out asynchronously on `stream`.  The number of rounds and of pointer jumps per round is fixed on the host
 * from the bound 2 * n_links on the nodes.  _host: host arrays.
 *
 * duet_ps_join_links_device: out_tag and *n_changed are what duet_ps_join_tags_device gives for the table of blocks(records,
 * min_sv); the table never visits the host.  read_tag, out_tag device memory (out_tag may be read_tag), read_off HOST as for
 * duet_ps_join_tags_*, counts and n_changed host memory.  ONE host round trip in all.  A refusal of the arguments is decided
 * before anything is written; a refusal found on the device (the three record checks) returns DUET_ERR_INVALID with zero counts
 * and *n_changed = 0, and out_tag then holds an unchanged copy of read_tag.  n_links == 0: out_tag a copy.
 * The workspace is the entries' own (about 110 bytes per record; grown, never shrunk): a call changes nothing that any other
 * entry later returns. */
typedef struct duet_ps_blocks_counts {
    uint32_t n_rows, n_trusted, n_conflicts, n_components;
} duet_ps_blocks_counts;
DUET_API int duet_ps_blocks_device(duet_ctx *ctx, const duet_ps_link *links, uint32_t n_links, uint32_t n_contigs, uint32_t min_sv,
                                   duet_ps_block *out_rows, uint32_t rows_cap, uint32_t *out_conflicts, uint32_t conflicts_cap,
                                   duet_ps_blocks_counts *counts, void *stream);
DUET_API int duet_ps_blocks_host(duet_ctx *ctx, const duet_ps_link *links, uint32_t n_links, uint32_t n_contigs, uint32_t min_sv,
                                 duet_ps_block *out_rows, uint32_t rows_cap, uint32_t *out_conflicts, uint32_t conflicts_cap,
                                 duet_ps_blocks_counts *counts);
DUET_API int duet_ps_join_links_device(duet_ctx *ctx, const duet_ps_link *links, uint32_t n_links, uint32_t min_sv,
                                       const uint64_t *read_tag, const uint32_t *read_off, uint32_t n_contigs, uint32_t n_reads,
                                       uint64_t *out_tag, duet_ps_blocks_counts *counts, uint32_t *n_changed, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Tags from other SVs (duet_svtags.hip): a mark whose read has no tag word is given the haplotype that the
 * OTHER heterozygous calls listing the read place it on.  A call must not vote for itself, so the tag is per mark and
 * leave-one-out: the evidence for mark (c, r) is every het call listing r except c.  The output is one tag word per RAW MARK, in
 * read_tag's layout (hap:2 | pc:30 | ps:32): the second run is the ordinary run with read_tag = out_tag, n_reads = n_marks and
 * mark_read = out_index (the identity, which the entry also writes).  tests/sv_tags_ref.py states the rule in plain Python.
 * Nothing here has been tried on real data; which reads get a tag, the PC they get and how ties break are CHOICES.
 *
 *   Problem     the duet_read_tags_problem of the section above (cand_pos is not read and may be NULL).  A raw mark belongs to the
 *               candidate whose CSR slot names it; a raw mark that no slot names belongs to none.
 *   Kept        a mark that has a tag (index not DUET_MARK_ABSENT, < n_reads, word not all-ones) keeps its word bit for bit,
 *               whatever hap and pc it holds: only reads without any tag word are given one (the narrow choice: the PS-class of
 *               every tagged mark stays what it was).
 *   Evidence    for an untagged mark m of candidate c with name n = mark_name[m]: the section-20 records of n, one per (n, P) over
 *               the marks of candidates with pred 1 or 2, with n_h1 and n_h2 (a read listed twice counts twice).
 *   Own part    k = the marks of c whose name is n.  pred[c] == 1: the record (n, ps[c]) loses k from n_h1; pred[c] == 2: from
 *               n_h2; otherwise nothing is taken out.
 *   Choice      d_P = n_h1' - n_h2' (signed 64-bit).  The P with the largest |d_P|, ties to the smaller P as a full unsigned
 *               32-bit number.  |d_P| < min_votes, or no record: out_tag[m] is all-ones.  Otherwise hap = 1 if d_P > 0 else 2,
 *               pc = pc_new, ps = P.
 *   Counts      counts[0] n_untagged: the marks without a tag; counts[1] n_given: those that received one; counts[2] n_own_only:
 *               those that would have received one with the own part left in and receive none without it.  Sums of popcounts
 *               added with integer atomics: independent of the order of arrival, two runs give identical bytes.
 *   Refused     DUET_ERR_INVALID, nothing written: pred > 3; a cand_off that descends or passes n_marks; a mark_name >= n_names (every raw mark is checked); a mark_order
 *               entry >= n_marks, or a raw mark named by two slots (its tag would depend on which slot is asked); a cand_ctg_off
 *               that does not ascend from 0 to n_cands; both or neither of cand_ctg_off and cand_contig; pc_cap or pc_new above
 *               2^30 - 3; min_votes == 0; a NULL array that is needed; section 20's contradiction (contributing marks of one
 *               name on two contigs or with two mark_read values).  pc_cap is the cap of the run the tags are made for; the rule
 *               itself does not read it.
 * n_cands == 0 or n_marks == 0: DUET_OK, zero counts, nothing written.  No candidate with pred 1 or 2: every untagged mark is
 * all-ones.
 * _device: the arrays of *prob (cand_ctg_off aside: HOST), out_tag[n_marks] and out_index[n_marks] are device memory, counts[3]
 * host memory.  THREE host round trips of a few words: the contributing marks V and the argument refusals; the record and run
 * counts; the contradiction words and the counters.  The words wait in the workspace until the last is read, then are copied to
 * out_tag asynchronously on `stream`.  _host: host arrays; uploads, runs the same kernels, copies back, synchronises.
 * The workspace is the entry's own (44 bytes per contributing mark + the sort's histogram, 12 per mark, 8 per candidate, 16 per
 * record; grown, never shrunk): a call changes nothing that any other entry returns. */
DUET_API int duet_sv_tags_device(duet_ctx *ctx, const duet_read_tags_problem *prob, uint32_t pc_cap, uint32_t min_votes, uint32_t pc_new,
                                 uint64_t *out_tag, uint32_t *out_index, uint32_t *counts, void *stream);
DUET_API int duet_sv_tags_host(duet_ctx *ctx, const duet_read_tags_problem *prob, uint32_t pc_cap, uint32_t min_votes, uint32_t pc_new,
                               uint64_t *out_tag, uint32_t *out_index, uint32_t *counts);

/* ---------------------------------------------------------------------------------------------
 * Tags from other SVs, planned (duet_svtags_plan.hip): the rule of the section above for MANY vectors of first-run
 * calls over one problem.  What does not read pred is done once (the plan); what reads it is done per vector (the apply) with no
 * sort, no allocation and no host round trip.  For callers that score the second run of many vectors (duet_amd.tune under
 * --vote_sv_tags).  tests/sv_tags_ref.py remains the rule; nothing new is chosen.
 *
 * duet_sv_tags_plan_*: prob as for duet_sv_tags_* -- pred is NOT read and may be NULL; ps[c] is read for the masked candidates.
 * cand_mask: u8[n_cands], non-zero = the candidate may be a het call (pred 1 or 2) under some vector; NULL = every candidate.
 *   Plan        everything of duet_sv_tags_device that does not read pred, over the masked candidates in place of the het ones: the
 *               owner of every raw mark; the (name << 32 | ps[c]) keys of the masked candidates' marks sorted stably once; the records
 *               numbered; the RUNS -- a record's members from one candidate -- kept as (candidate, k), so a candidate with 70,000
 *               marks under one name is one run; one compact record per UNTAGGED raw mark: the mark, its candidate (where masked),
 *               its own k, the range of records of its name.
 *   Base words  out_tag[m] = the word of every tagged mark bit for bit, all-ones for every untagged mark; out_index = the identity.
 *   Refused     DUET_ERR_INVALID, nothing written, no plan left: what duet_sv_tags_* refuses of the problem and of pc_cap (pred, min_votes
 *               and pc_new are the apply's).  Section 20's contradiction is checked over the MASKED candidates' marks: STRICTER than
 *               duet_sv_tags_*, which checks the het ones only -- a masked candidate that no vector calls het can refuse a plan.
 *   *info       (HOST) the untagged marks, the records, the runs, and the contributing marks V of the masked candidates.
 * n_cands == 0 or n_marks == 0: DUET_OK, zero info, nothing written; an apply then clears its counters and writes nothing else.
 * _device: the arrays of *prob (cand_ctg_off aside: HOST), cand_mask, out_tag[n_marks] and out_index[n_marks] device memory.  THREE host
 * round trips of a few words, as duet_sv_tags_device.  _host: host arrays.
 * The plan lives in a workspace of the context's own (8 bytes per run, 20 per record, 20 per untagged mark, 5 per candidate, beside the
 * build's transient 44 per contributing mark and 16 per mark; grown, never shrunk).  One plan per context: a later plan call
 * replaces it, accepted or not.  The plan holds COPIES (ps and the mask among them): nothing of *prob is read once the work queued
 * on `stream` has run, so the caller may point the problem at out_tag afterwards.
 *
 * duet_sv_tags_apply_*: pred u8[n_cands], one vector's first-run calls.  out_tag must hold the plan's base words at the tagged marks.
 *   Writes      the word of EVERY untagged mark -- given or all-ones -- on every call, and nothing else of out_tag: the bytes of a
 *               vector do not depend on the vectors applied before it.
 *   out_counts  u32[4]: n_untagged, n_given, n_own_only as duet_sv_tags_*; out_counts[3] = the candidates with pred > 3 or with pred 1
 *               or 2 outside the mask.  Non-zero: the words of this call are not to be used (the tagged marks still hold the base
 *               words).
 *   Contract    where the plan accepts and out_counts[3] is 0: out_tag, out_index and the three counters are those of
 *               duet_sv_tags_device with the same pred, min_votes and pc_new, byte for byte.
 *   Refused     DUET_ERR_INVALID, nothing written: no plan on the context; min_votes == 0; pc_new above 2^30 - 3; a NULL argument.
 * _device: pred, out_tag and out_counts device memory; ASYNCHRONOUS on `stream` -- four words cleared and two kernels, nothing read
 * back; calls on one plan are ordered by the stream (they share the plan's record sums).  _host: host arrays (out_tag is uploaded,
 * applied to, and copied back), synchronises. */
typedef struct duet_sv_tags_plan_info {
    uint32_t n_untagged, n_records, n_runs, n_contributing;
} duet_sv_tags_plan_info;
DUET_API int duet_sv_tags_plan_device(duet_ctx *ctx, const duet_read_tags_problem *prob, const uint8_t *cand_mask, uint32_t pc_cap,
                                      uint64_t *out_tag, uint32_t *out_index, duet_sv_tags_plan_info *info, void *stream);
DUET_API int duet_sv_tags_plan_host(duet_ctx *ctx, const duet_read_tags_problem *prob, const uint8_t *cand_mask, uint32_t pc_cap,
                                    uint64_t *out_tag, uint32_t *out_index, duet_sv_tags_plan_info *info);
DUET_API int duet_sv_tags_apply_device(duet_ctx *ctx, const uint8_t *pred, uint32_t min_votes, uint32_t pc_new, uint64_t *out_tag,
                                       uint32_t *out_counts, void *stream);
DUET_API int duet_sv_tags_apply_host(duet_ctx *ctx, const uint8_t *pred, uint32_t min_votes, uint32_t pc_new, uint64_t *out_tag,
                                     uint32_t *out_counts);

/* ---------------------------------------------------------------------------------------------
 * Diagnostics: the shared device primitives (duet_amd/csrc/duet_prims.hip.h) on host arrays, each run unchanged on the
 * context's own stream with a workspace sized as the primitive's comments prescribe (duet_amd/csrc/duet_prims_check.hip).  No
 * product path calls these; tests/test_gpu_prims.py compares them with numpy at every plan boundary.  n == 0: DUET_OK, nothing is
 * launched.  A null array or an argument outside the primitive's documented preconditions: DUET_ERR_INVALID, nothing is launched.
 *
 * duet_prims_sort_host: radix_sort_pairs -- the stable sort of n keys (with vals: of n (key, value) pairs) by the key bits
 *   [first_shift, key_bits); the bits above key_bits travel untouched.  1 <= key_bits <= 64, first_shift < key_bits; vals and
 *   out_vals are both given or both null; force_scan != 0: the tile offsets by the generic scan, as above 1024 tiles.
 * duet_prims_scan_host: launch_scan<op> over in[n] -- op 0 the exclusive sum (mod 2^32), op 1 the inclusive maximum; n_dyn: the
 *   real element count on the device, n being its bound (UINT32_MAX: none is passed); force_spine != 0: the path with a spine
 *   launch.  out[n] is uploaded before the scan and downloaded after it, so the caller sees what was left untouched; *total: the
 *   combination of every element; zero14 (may be null): 14 words uploaded before the scan, which zeroes them, and downloaded.
 * duet_prims_local_sort_host: the hybrid sort of the key-only clustering path -- global passes over the bits [lo, key_bits), then
 *   rx_local<threads> and rx_big over the low bits, groups of more than cap keys going to rx_big; the result is the stable sort
 *   by the bits [0, key_bits).  1 <= key_bits <= 64, 1 <= lo < 32, lo < key_bits, 1 <= cap <= 256, threads 256 or 1024. */
DUET_API int duet_prims_sort_host(duet_ctx *ctx, const uint64_t *keys, const uint32_t *vals, uint32_t n, uint32_t key_bits,
                                  uint32_t first_shift, int force_scan, uint64_t *out_keys, uint32_t *out_vals);
DUET_API int duet_prims_scan_host(duet_ctx *ctx, const uint32_t *in, uint32_t n, int op, uint32_t n_dyn, int force_spine,
                                  uint32_t *out, uint32_t *total, uint32_t *zero14);
DUET_API int duet_prims_local_sort_host(duet_ctx *ctx, const uint64_t *keys, uint32_t n, uint32_t key_bits, uint32_t lo, uint32_t cap,
                                        uint32_t threads, uint64_t *out_keys);

/* ---------------------------------------------------------------------------------------------
 * The collective of the contig-sharded path: candidates shard by contig over the GPUs of one node,
 * one process and one context per GPU, and ONE all-gather of fixed-size record blocks reassembles the call set
 * (src/duet/sv_phasing_fn.py:15-18, 195-210: nothing crosses contigs before the final sort at :229).  RCCL over xGMI,
 * loaded at run time (the library has no link-time dependency on it; these calls fail with DUET_ERR_NO_DEVICE where it is
 * missing).  The caller hands the 128-byte unique id of rank 0 to every rank by its own means (duet_amd/comm.py: a TCP
 * star on MASTER_ADDR:MASTER_PORT); duet_comm_create is collective (ncclCommInitRank) and returns NULL on failure
 * (duet_last_error(ctx)). */
#define DUET_COMM_ID_BYTES 128
typedef struct duet_comm duet_comm;
DUET_API int duet_comm_rccl_version(duet_ctx *ctx);      /* ncclGetVersion's code (e.g. 22707) of the RCCL the library loaded, or a negative status */
DUET_API int duet_comm_unique_id(duet_ctx *ctx, unsigned char *id /* [DUET_COMM_ID_BYTES] */);
DUET_API duet_comm *duet_comm_create(duet_ctx *ctx, const unsigned char *id, int rank, int world);
/* Every blocking step is bounded: duet_comm_create and the synchronising calls below give up after the time limit -- the
 * environment's DUET_RDZV_TIMEOUT in seconds (default 300) at creation, duet_comm_set_timeout afterwards -- with
 * DUET_ERR_TIMEOUT (duet_comm_create: NULL and that text in duet_last_error) instead of waiting for a rank that never comes. */
DUET_API int duet_comm_set_timeout(duet_comm *comm, double seconds);
/* every rank contributes `bytes` bytes, every rank receives world * bytes (rank-major).  _device: device pointers,
 * asynchronous on `stream`; _host: host pointers, staged through device buffers of the communicator, synchronises. */
DUET_API int duet_comm_allgather_device(duet_comm *comm, const void *send, uint64_t bytes, void *recv, void *stream);
DUET_API int duet_comm_allgather_host(duet_comm *comm, const void *send, uint64_t bytes, void *recv);
/* One rank's whole data path of the contig-sharded run, results never leaving the device before the collective
 * (src/duet/sv_phasing_fn.py:189-228 on the rank's contigs, then the reassembly in front of :229):
 *   *prob (HOST arrays, the rank's shard) is uploaded, ef_classify -> ef_seed_sort -> ef_finalize write straight into the
 *   rank's record block on the device,
 *       ps u32[n_max] | pred u8[n_max] | pad to 16 | status u32, 12 bytes pad | kept u64[n_slots]
 *   (n_max = the largest shard's candidate count, the same on every rank; status = 5 when a candidate that reaches the
 *   decision has svread + refread == 0, else 0; kept[s] = candidates c with pred != 0 and cand_slot[c] == s: the rows each
 *   CHROM text contributes, which is what tells every rank where its rows' numbering starts), ONE ncclAllGather of the
 *   blocks on the kernels' stream, one copy of the world * block bytes to `gathered` (host), bounded wait.
 * duet_comm_block_bytes gives the block size.  cand_slot may be NULL when n_slots == 0. */
DUET_API uint64_t duet_comm_block_bytes(uint32_t n_max, uint32_t n_slots);
DUET_API int duet_comm_ef_allgather(duet_comm *comm, const duet_ef_problem *prob, const uint32_t *cand_slot, uint32_t n_slots,
                                    uint32_t n_max, uint8_t *gathered);
/* A rank whose own part of duet_comm_ef_allgather fails (arguments, memory, upload, a launch) still contributes a block to
 * the collective -- zeros, with this bit set in the status word and the negated duet_status in the low 16 bits -- so that its
 * peers fail at once instead of waiting for the time limit; the failing rank returns its own error after the collective. */
#define DUET_COMM_STATUS_RANK_FAILED 0x80000000u
/* What RCCL itself says about the communicator (ncclCommCount / ncclCommUserRank / ncclCommCuDevice; -1 where the loaded RCCL
 * lacks the call): `rccl_ranks` == world is the evidence that RCCL, not a stand-in, connected every rank. */
DUET_API int duet_comm_info(duet_comm *comm, int *rank, int *world, int *rccl_ranks, int *rccl_rank, int *rccl_device);
/* Every rank all-gathers `words` 32-bit words of a pattern that names its rank and the word's place, and checks every slot
 * of what comes back (collective: every rank must call it with the same `words`).  DUET_OK or the first wrong word. */
DUET_API int duet_comm_selftest(duet_comm *comm, uint32_t words);
/* Frees the communicator.  On one that timed out (DUET_ERR_TIMEOUT) nothing of the device is touched -- a collective may be
 * stuck on the stream, ncclCommDestroy and hipFree would wait for it: its buffers are leaked, the process is expected to exit. */
DUET_API void duet_comm_destroy(duet_comm *comm);

#ifdef __cplusplus
}
#endif
#endif /* DUET_EF_H */
