/*
 * duet_ingest.h -- C ABI of the native host-side ingest/emit of Duet's step E/F (libduet_ingest.so, plain C++,
 * no GPU dependency): caller VCF + per-contig haplotagged BAMs -> the structure-of-arrays problem of
 * duet_ef.h, and (pred, ps) -> the rows of phased_sv.vcf.
 *
 * It restates, for well-formed ASCII input, what the reference does in Python:
 *     read_hap_bam        src/duet/sv_phasing_fn.py:11-34   (tag dict per contig, later lines win)
 *     parse_vcf           src/duet/read_file.py:25-77       (three caller dialects, first-record layout)
 *     generate_callinfo   src/duet/sv_phasing_fn.py:36-68   (join of mark names, callset order)
 *     emission + sort     src/duet/sv_phasing_fn.py:213-229
 *     print_sv_header/print_sv  src/duet/write_file.py:6-45
 * Anything it is not sure to reproduce exactly (non-ASCII bytes, blank lines, malformed numbers, missing
 * fields, out-of-range values ...) makes the call return DUET_INGEST_UNSUPPORTED; the Python host path
 * (duet_amd/read_file.py, sv_phasing_fn.py) then handles the input and raises what upstream would raise.
 */
#ifndef DUET_INGEST_H
#define DUET_INGEST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DUET_INGEST_OK 0
#define DUET_INGEST_UNSUPPORTED 1      /* fall back to the Python path */
#define DUET_INGEST_IO (-1)            /* file could not be read */
#define DUET_INGEST_INVALID (-2)       /* bad argument / call order */

typedef struct duet_ingest duet_ingest;

typedef struct duet_ingest_arrays {     /* views into memory owned by the duet_ingest object */
    uint32_t n_contigs, n_cands, n_marks, n_reads;
    const uint32_t *cand_ctg_off;       /* [K+1] */
    const uint32_t *read_off;           /* [K+1] */
    const uint64_t *read_tag;           /* [R]   */
    const uint32_t *cand_pos, *cand_svlen, *cand_svread, *cand_refread;   /* [C] */
    const uint8_t *cand_gt_ok;          /* [C]   */
    const uint32_t *cand_off;           /* [C+1] */
    const uint32_t *mark_read;          /* [M]   */
} duet_ingest_arrays;

/* contig_names: the chrom list (read_file.py:6-16), n_contigs entries. */
duet_ingest *duet_ingest_create(int n_contigs, const char *const *contig_names);
void duet_ingest_destroy(duet_ingest *ing);
const char *duet_ingest_error(const duet_ingest *ing);

/* Tag dict of contig k from a BAM file (built-in BGZF/BAM reader, `threads` inflate workers). */
int duet_ingest_add_bam(duet_ingest *ing, int contig, const char *bam_path, int threads);
/* The same for n contigs in one call, `threads` workers in all (src/duet/sv_phasing_fn.py:15-29 is a loop over independent contigs:
 * every contig has a dict of its own): whole contigs are dealt to the workers, the largest files first; with fewer contigs than
 * workers each contig keeps threads / n of them.  Returns the status of the first contig in the caller's order that failed. */
int duet_ingest_add_bams(duet_ingest *ing, int n, const int *contigs, const char *const *bam_paths, int threads);

/* 1 when the BAM added for contig k held at least one alignment (the reference logs '  signatures extracted from k'
 * then, '  no signature from k' otherwise: src/duet/sv_phasing_fn.py:30-33), 0 when it held none or none was added. */
int duet_ingest_bam_has_alignments(const duet_ingest *ing, int contig);

/* Parse the caller VCF (`threads` workers) and join its mark names against the tag dicts added so far. */
int duet_ingest_parse_vcf(duet_ingest *ing, const char *vcf_path, int threads);
/* The same in two calls, so that a caller can run the first half -- read, tokenise, pick the listed contigs' records: it
 * touches nothing the BAM side uses -- on another thread BESIDE its duet_ingest_add_bam calls, and the second half (numbers,
 * join of the mark names against the tag dicts) once both are done.  _begin's failure is reported by _finish (error text
 * included), which must be called exactly once after it. */
int duet_ingest_parse_vcf_begin(duet_ingest *ing, const char *vcf_path, int threads);
int duet_ingest_parse_vcf_finish(duet_ingest *ing);
int duet_ingest_get_arrays(const duet_ingest *ing, duet_ingest_arrays *out);

/* Text of phased_sv.vcf: header (write_file.py:19-45; include_all_ctgs selects which ##contig lines are
 * copied; a negative value leaves the header out -- the caller has written it already, as the reference does before
 * it evaluates anything, src/duet/sv_phasing.py:16) followed by the rows of every candidate with pred != 0.  Returns a malloc'ed buffer in *text
 * (free with duet_ingest_free) and its length in *len. */
int duet_ingest_emit(duet_ingest *ing, const uint8_t *pred, const uint32_t *ps, int include_all_ctgs,
                     char **text, uint64_t *len);
void duet_ingest_free(void *p);

/* Sharded runs (one rank per GPU, contigs owned whole: src/duet/sv_phasing_fn.py:15-29,195-229 are per contig).
 * _vcf_precount: records and line bytes of every listed contig in the caller VCF -- one memchr pass, no tokenising; every
 *   rank runs it (same result everywhere), which gives the contig -> rank assignment and every rank's candidate count
 *   before anything is parsed.  The file stays loaded for the parse that follows.
 * _set_owned (before the parse): owned[k] == 0 -> contig k's records are left to another rank (dropped after their first
 *   token; that rank vouches for them); header lines and the contig list stay complete.
 * _count_kept: rows (pred != 0) per CHROM-text slot, slot = 2 * contig + (0: spelled chr<name>, 1: spelled <name>).
 * _cand_slots: every candidate's slot (what duet_comm_ef_allgather of duet_ef.h counts the kept rows by, on the device).
 * _emit_blocks: the rank's rows, the rows of slot s numbered id_base[s], id_base[s] + 1, ... ; slot_off / slot_len [2K]
 *   give each slot's byte range in *text.  A CHROM text belongs to one contig, the final file is the blocks in the byte
 *   order of their texts (sv_phasing_fn.py:229 sorts CHROM as text first). */
int duet_ingest_vcf_precount(duet_ingest *ing, const char *vcf_path, uint64_t *n_records /* [K] */, uint64_t *n_bytes /* [K] */);
int duet_ingest_set_owned(duet_ingest *ing, const uint8_t *owned /* [K] or NULL = all */);
int duet_ingest_count_kept(duet_ingest *ing, const uint8_t *pred, uint64_t *kept /* [2K] */);
int duet_ingest_cand_slots(duet_ingest *ing, uint32_t *slot /* [C] */);
int duet_ingest_emit_blocks(duet_ingest *ing, const uint8_t *pred, const uint32_t *ps, const uint64_t *id_base /* [2K] */,
                            char **text, uint64_t *len, uint64_t *slot_off /* [2K] */, uint64_t *slot_len /* [2K] */);

/* The header lines alone (write_file.py:19-45), for callers that produce the rows elsewhere (duet_rows_run_device). */
int duet_ingest_header(duet_ingest *ing, int include_all_ctgs, char **text, uint64_t *len);

/* What duet_rows_run_device (duet_ef.h) needs besides the arrays above: the CHROM / REF / ALT / SVTYPE texts of every
 * candidate in one pool (4 offsets per candidate), the byte-order rank of each candidate's CHROM text among the
 * distinct CHROM texts (the sort of sv_phasing_fn.py:229 compares them as strings), and the SVLEN sign flags
 * (sv_phasing_fn.py:225).  Views into memory owned by the duet_ingest object. */
typedef struct duet_ingest_rows {
    uint32_t n_cands, n_chrom_texts, max_pos;
    const char *pool;
    uint64_t pool_bytes;
    const uint32_t *str_off;            /* [4C+1] */
    const uint16_t *cand_chrom_rank;    /* [C] */
    const uint8_t *cand_plus;           /* [C] */
} duet_ingest_rows;
int duet_ingest_get_rows(duet_ingest *ing, duet_ingest_rows *out);

/* SVIM-mode signature extraction (the reference delegates it to the external `svim
 * alignment`, src/duet/sv_calling.py:13-15, so this is the repository's own rule, parity unpinned -- normative text:
 * oracle/svim_oracle.py).  When enabled BEFORE duet_ingest_add_bam, every primary or supplementary alignment with
 * MAPQ >= min_mapq contributes (a) one raw SV mark per CIGAR insertion / deletion of at least min_sv_size bases:
 * type 1 = INS / 0 = DEL, pos = 1-based reference position of the event, span = its length, read = the alignment's
 * entry in the contig's tag table (or 0xFFFFFFFF); (b) +1 to depth[b] of every bin b of depth_bin bases whose
 * middle it covers.  The marks are what duet_cluster_run_* / duet_svim_phase_device (duet_ef.h) take. */
int duet_ingest_set_extraction(duet_ingest *ing, int enable, uint32_t min_sv_size, uint32_t min_mapq, uint32_t depth_bin);

typedef struct duet_ingest_marks {      /* views into memory owned by the duet_ingest object */
    uint32_t n_marks, n_contigs, n_reads, depth_bin;
    const uint16_t *mark_contig;        /* [M] */
    const uint8_t *mark_type;           /* [M] */
    const uint32_t *mark_pos, *mark_span, *mark_read;   /* [M] */
    const uint64_t *read_tag;           /* [R] all contigs' tag tables, concatenated */
    const uint32_t *read_off;           /* [K+1] */
    const uint32_t *depth;              /* [depth_off[K]] */
    const uint32_t *depth_off;          /* [K+1] */
} duet_ingest_marks;
int duet_ingest_get_marks(duet_ingest *ing, duet_ingest_marks *out);

/* Read names of the raw marks (what sv_calling/variants.vcf lists in READS=; duet_svim_vcf_rows_* of duet_ef.h).  Opt-in: call
 * duet_ingest_keep_mark_names(ing, 1) BEFORE the BAMs are added (DUET_INGEST_INVALID once marks exist); without it the extraction
 * keeps no names and duet_ingest_get_mark_names returns DUET_INGEST_INVALID.  Names are interned per contig: mark_name[i] is the
 * name of mark i of duet_ingest_get_marks (same order), an index into name_off; name n is name_pool[name_off[n] .. name_off[n + 1]).
 * A read that supplies marks on two contigs has one entry per contig.
 * The VCF path takes the same opt-in: enabled BEFORE duet_ingest_parse_vcf* (DUET_INGEST_INVALID afterwards), the join also interns
 * the name of every mark of the caller VCF per contig, tagged or not, and on an ingest without extraction
 * duet_ingest_get_mark_names returns them: mark_name[i] is the name of mark i of duet_ingest_arrays.mark_read (same order), the
 * pool laid out as above, in order of first mark.  Without the call nothing is kept and the parse does what it did. */
typedef struct duet_ingest_mark_names {  /* views into memory owned by the duet_ingest object */
    uint32_t n_marks, n_names;
    const uint32_t *mark_name;          /* [M] */
    const uint64_t *name_off;           /* [n_names + 1] */
    const char *name_pool;              /* [pool_bytes] */
    uint64_t pool_bytes;
} duet_ingest_mark_names;
int duet_ingest_keep_mark_names(duet_ingest *ing, int enable);
int duet_ingest_get_mark_names(duet_ingest *ing, duet_ingest_mark_names *out);

#ifdef __cplusplus
}
#endif
#endif
