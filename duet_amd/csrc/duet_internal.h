// duet_internal.h -- host-side state shared by the translation units of libduet_ef.so (not part of the ABI).
#ifndef DUET_INTERNAL_H
#define DUET_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "duet_ef.h"

struct DevBuf {
    void *ptr = nullptr;
    size_t cap = 0;
};

// device buffers freed with their owner (hipFree after duet_ctx_destroy's device synchronisation)
struct DuetOwnedBufs {
    DevBuf b[16];
    DuetOwnedBufs() = default;
    DuetOwnedBufs(const DuetOwnedBufs &) = delete;
    DuetOwnedBufs &operator=(const DuetOwnedBufs &) = delete;
    ~DuetOwnedBufs()
    {
        for (DevBuf &x : b)
            if (x.ptr) (void)hipFree(x.ptr);
    }
};

// the plan of duet_sv_tags_plan_* (duet_svtags_plan.hip): counts, and where its pieces lie in svplan_ws
struct DuetSvPlan {
    bool valid = false;
    uint32_t C = 0, M = 0, U = 0, N = 0, R = 0, V = 0;       // candidates, marks, untagged marks, records, runs, contributing marks
    void *runs = nullptr, *rec_h = nullptr, *ps = nullptr, *mask = nullptr;
    uint32_t *rec_first = nullptr, *rec_ps = nullptr, *u_mark = nullptr, *u_cand = nullptr, *u_k = nullptr, *u_lo = nullptr, *u_hi = nullptr;
};

struct duet_ctx {
    int device = 0;
    std::string err;
    int profiling = 0;                     // 0 off, 1 ef_classify events, 2 every kernel, 3 ef_classify on every 8th run
    int ev_mode = 0;                       // mode the pooled events were recorded with
    uint32_t prof_tick = 0;                // run counter of the sampled mode
    uint32_t dbg = 0;
    uint32_t ef_heavy_t = 32;              // ef_classify: candidates with more marks take the wave-cooperative walk (DUET_EF_HEAVY_T overrides)
    unsigned long long *d_stamps = nullptr;
    hipStream_t own_stream = nullptr;
    uint64_t *d_untagged = nullptr;                           // one all-ones word: what ef_classify gathers for a mark without a tag
    uint32_t *rx_dtot = nullptr;                              // [256] digit totals of a radix pass (zero between passes)
    // E/F plan (workspace keyed by the contig layout)
    std::vector<uint32_t> plan_off;        // cached cand_ctg_off
    uint32_t plan_C = 0;
    uint32_t plan_max_span = 0;            // tiles of 256 candidates that the plan's longest contig touches (selects ef_finalize_own_wide)
    hipStream_t plan_stream = (hipStream_t)-1;   // the stream the plan was built on
    uint32_t *plan_stage = nullptr;        // pinned staging block for the plan uploads
    size_t plan_stage_cap = 0;
    hipEvent_t plan_ev = nullptr;          // recorded after the staging block has been read
    DevBuf ws_small;                        // ctg_off | n_one | status | blk_ctg | blk_cnt
    DevBuf ws_start, ws_ent, ws_one, ws_tmp, ws_c2;
    uint32_t *d_ctg_off = nullptr, *d_n_one = nullptr, *d_status = nullptr, *d_blk_ctg = nullptr,
             *d_blk_cnt = nullptr;
    // host-run staging
    DevBuf h_in[9], h_out[2];
    // clustering (A0) workspace and host-run staging
    DevBuf cl_ws[16], cl_in[4], cl_out[6];
    DevBuf rows_ws[8];                     // device-side row emission
    DevBuf rows_in[5];                     // host-array entry: uploaded text pool, offsets, ranks, sign flags; the rows
    DevBuf eval_ws;                        // evaluator (duet_eval.hip): one arena
    DevBuf sv_ws[5];
    DevBuf sv_in[3], sv_out[2];            // duet_svim_phase_host: mark read indices, read tags, depth bins; pred, ps
    std::vector<uint32_t> sv_depth_off;    // the depth offsets the device copy in sv_ws[0] holds (uploaded only when they change)
    hipStream_t sv_depth_off_stream = nullptr;             // ... and the stream that upload is ordered on (compared, never used: the
                                                           // caller may have destroyed it since)
    hipEvent_t sv_depth_off_ev = nullptr;                  // ... recorded behind that upload: what a run on another stream waits for
    void *sv_depth_off_at = nullptr;                       // fused SVIM-mode pipeline: contig offsets, adapted columns, gathered marks
    hipStream_t cl_side[3] = {nullptr, nullptr, nullptr};     // the size classes of A0 agglomerate side by side
    hipEvent_t cl_fork = nullptr, cl_join[3] = {nullptr, nullptr, nullptr};
    uint32_t *cl_flags = nullptr;                             // [16] device words: what the side streams' gate kernels wait for (stage A0's forks, round 6)
    int cl_gates = 0;                                         // 0: not tried yet; 1: a gate on one stream sees a signal from another (the device runs them side by side); -1: it does not
    uint32_t cl_epoch = 0;                                    // ... the value the current run's forks write there
    // profiling events: 6 per run
    std::vector<hipEvent_t> ev_pool;
    std::vector<uint8_t> ev_kmask;         // per profiled run: the kernels that ran (bit i = kernel i; the two-launch E/F has no ef_seed_sort)
    size_t ev_used = 0;
    // the two-launch E/F (ef_finalize_own) leaves no ascending seed arrays behind: what duet_ef_get_seed_ps / duet_ef_stats need is
    // made on demand by ef_seed_sort from the same seed entries, with the last run's kernel arguments on the last run's stream
    std::vector<unsigned char> ef_last_params;
    hipStream_t ef_last_stream = nullptr;
    bool ef_seeds_stale = false;
    bool pending_check = false;
    DuetOwnedBufs tune_ws;                 // threshold sweep (duet_tune.hip): E/F outputs of the feature export, sweep workspace, host-run staging
    DuetOwnedBufs tune_truth_in, tune_truth_out;   // duet_tune_truth_build_host: staged inputs; base_hp and the six truth arrays (the build's own workspace is tune_ws 15)
    DuetOwnedBufs tune_strata_ws;          // strata of the sweep: host-run staging of cand_stratum 0 and group_stratum 1; the build's status word 2 and host-run staging 3-8
    DuetOwnedBufs tune_leaf_ws;            // leaf census (duet_tune_leaf.hip): the sweep's scratch counts 0, the groups' label bits 1; host-run staging of the features 2, the vectors 3, cand_stratum 4, the records 5, the truth arrays 6-11
    DuetOwnedBufs tune_line_ws;           // the line of one axis (duet_tune_line.hip): workspace 0; host-run staging of the features 1 and the vectors 2
    DuetOwnedBufs tune_cap_ws;             // feature export under a PC cap (duet_tune_cap.hip): workspace 0; host-run staging of the features 1
    DuetOwnedBufs tune_capline_ws;         // the line of the PC cap (duet_tune_capline.hip): workspace 0; host-run staging of the values 1, of a svim problem's mark reads 2 and read tags 3
    DuetOwnedBufs callset_ws;            // svim-gpu callset rows (duet_callset.hip): workspace 0-4, host-run staging 5-14, text 15
    DuetOwnedBufs evidence_ws;             // evidence table (duet_evidence.hip): row lengths 0, row offsets 1, tile sums 2, status words and CHROM texts 3; host-run staging 4-12, text 13
    DuetOwnedBufs svim_rows_ws;            // svim-gpu rows of phased_sv.vcf (duet_svim_rows.hip): workspace 0-8, host-run staging 9-14, text 15
    DuetOwnedBufs pslinks_ws;              // phase-set links (duet_pslinks.hip): per-candidate workspace 0, per-voter workspace 1; host-run staging of the records 2
    DuetOwnedBufs readtags_ws;             // read tags (duet_readtags.hip): per-candidate workspace 0, per-mark workspace 1, the records before they are released 2; host-run staging 3-11
    DuetOwnedBufs readtags_rows_ws;        // ... its rows: row lengths 0, row offsets 1, tile sums 2, status words and CHROM texts 3; host-run staging 4-7, text 8
    DuetOwnedBufs psjoin_ws;               // joined phase sets (duet_psjoin.hip): the header words, the offsets and the staged table 0, the change codes before they are released 1; host-run staging of the read tags 2, of pred0, ps0, pred1, ps1, cand_contig 3-7
    DuetOwnedBufs psblocks_ws;             // blocks of the links (duet_psblocks.hip): the header words and the whole workspace 0; host-run staging of the records 1
    DuetOwnedBufs svtags_ws;               // tags from other SVs (duet_svtags.hip): per-candidate workspace 0, per-mark workspace and the staged words 1, per-contributing-mark workspace 2, the records 3; host-run staging 4-11
    DuetOwnedBufs svplan_ws;               // tags from other SVs, planned (duet_svtags_plan.hip): the build's per-candidate workspace 0, per-mark workspace and the staged base words 1, per-contributing-mark workspace 2; KEPT between calls: the runs and records 3, the untagged marks 4, the copies of ps and the mask 5
    DuetOwnedBufs svplan_in;               // ... host-run staging: the plan's arrays 0-7; the apply's pred, words and counters 8-10
    DuetSvPlan svplan;                     // ... the one plan of the context
    DuetOwnedBufs prims_ws;               // diagnostics of the shared primitives (duet_prims_check.hip): one arena, 0
};

extern thread_local std::string duet_g_last_error;

inline int duet_fail(duet_ctx *ctx, int code, const std::string &msg)
{
    if (ctx) ctx->err = msg;
    duet_g_last_error = msg;
    return code;
}

#define HIP_TRY(ctx, expr)                                                                      \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return duet_fail(ctx, e_ == hipErrorOutOfMemory ? DUET_ERR_OOM : DUET_ERR_HIP,      \
                             std::string(#expr) + ": " + hipGetErrorString(e_));                \
    } while (0)

// device-planned E/F run (duet_ef.hip), for the fused pipeline in duet_svim.hip.  _prepare sizes the workspace for the bound
// and names the plan's place in it: ctg_off[K + 1], and K + 8 words to zero (seeds per contig, status words) -- the producer
// (stage A0's cl_emit) writes both itself, and the run launches no plan kernel
int duet_ef_plan_on_device_prepare(duet_ctx *ctx, uint32_t K, uint32_t c_max, hipStream_t stream, uint32_t **ctg_off_out,
                                   uint32_t **zero_out);
int duet_ef_run_planned_on_device(duet_ctx *ctx, const duet_ef_problem *pr, uint32_t c_max, const uint32_t *d_n_cands,
                                  const uint16_t *d_cand_contig /* the candidates' contig column */, uint8_t *out_pred, uint32_t *out_ps,
                                  hipStream_t stream);

int duet_ef_materialise_seeds(duet_ctx *ctx);

// argument checks of an E/F problem (host or device arrays alike: pointers and counts only)
int duet_ef_validate(duet_ctx *ctx, const duet_ef_problem *pr);

// host arrays of an E/F problem -> the context's staging buffers (duet_ef.hip)
int duet_ef_upload(duet_ctx *ctx, const duet_ef_problem *pr, duet_ef_problem *d, hipStream_t s);

// phase-set links (duet_pslinks.hip) of a device-resident problem, checked by the caller; out is device memory, or with
// out_on_host host memory (the records are staged and copied, the stream synchronised).  For the SVIM drivers in duet_svim.hip.
int duet_ps_links_run(duet_ctx *ctx, const duet_ef_problem *pr, uint32_t pc_cap, duet_ps_link *out, uint32_t out_cap, uint32_t *n_links,
                      hipStream_t st, bool out_on_host);

// pj_tags (duet_psjoin.hip) over a table that is already on the device in its staged layout, for duet_psblocks.hip: slice k of the
// keys (PS, ascending) and values (flip << 32 | block) is d_slice_off[k] .. d_slice_off[k + 1]; n_bound: an index no row has (the
// row count or above); d_read_off: the device copy of read_off; d_hdr: 16 zeroed words, word 0 receives the changed tag words.
// K >= 1, R >= 1, the arguments checked by the caller; nothing is read back.
int duet_ps_join_tags_staged(duet_ctx *ctx, const uint64_t *read_tag, const uint32_t *d_read_off, uint32_t K, uint32_t R,
                             const uint32_t *d_slice_off, const uint32_t *d_key, const uint64_t *d_val, uint32_t n_bound, uint64_t *out_tag,
                             uint32_t *d_hdr, hipStream_t st);

inline int duet_reserve(duet_ctx *ctx, DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap) return DUET_OK;
    if (b.ptr) HIP_TRY(ctx, hipFree(b.ptr));
    b.ptr = nullptr;
    b.cap = 0;
    size_t want = bytes + bytes / 8 + 256;
    HIP_TRY(ctx, hipMalloc(&b.ptr, want));
    b.cap = want;
    return DUET_OK;
}

// host arrays -> the staging buffers bufs[0..n): each reserved (with 64 spare bytes, so an empty array still has a readable
// address), copied on s when it has bytes; dev[i] = its device address
inline int duet_stage_arrays(duet_ctx *ctx, DevBuf *bufs, const void *const *src, const size_t *bytes, int n, hipStream_t s, void **dev)
{
    for (int i = 0; i < n; ++i) {
        int rc = duet_reserve(ctx, bufs[i], bytes[i] + 64);
        if (rc) return rc;
        if (bytes[i]) HIP_TRY(ctx, hipMemcpyAsync(bufs[i].ptr, src[i], bytes[i], hipMemcpyHostToDevice, s));
        dev[i] = bufs[i].ptr;
    }
    return DUET_OK;
}

// Stage A0 (duet_cluster.hip) as the fused pipeline (duet_svim.hip) runs it: with sv, cl_emit also writes what a caller VCF
// would have carried and the marks' read indices in output order.  sv == nullptr: duet_cluster_run_device.
struct SvExtra {
    const uint32_t *mark_in, *depth, *depth_off;
    uint32_t depth_bin;
    uint32_t *mark_out, *svread, *refread;
    uint8_t *gt;
    uint32_t *ef_ctg_off, *ef_zero;       // step E/F's plan, written by cl_emit (null: E/F plans for itself)
    uint32_t n_contigs;
};
int duet_cluster_run(duet_ctx *ctx, const duet_cluster_problem *pr, const duet_cluster_result *res, void *stream_, const SvExtra *sv);

// Host staging of the clustering's host entries (duet_cluster_run_host, and the SVIM host entries of duet_svim.hip).
// The four mark arrays of a host problem -> cl_in; *d = the problem over them
inline int duet_stage_marks(duet_ctx *ctx, const duet_cluster_problem *pr, duet_cluster_problem *d, hipStream_t s)
{
    const size_t M = pr->n_marks;
    const void *src[4] = {pr->mark_contig, pr->mark_type, pr->mark_pos, pr->mark_span};
    const size_t bytes[4] = {M * 2, M, M * 4, M * 4};
    void *dev[4];
    for (int i = 0; i < 4; ++i)
        if (!src[i] && bytes[i]) return duet_fail(ctx, DUET_ERR_INVALID, "null array");
    int rc = duet_stage_arrays(ctx, ctx->cl_in, src, bytes, 4, s, dev);
    if (rc) return rc;
    *d = *pr;
    d->mark_contig = (const uint16_t *)dev[0];
    d->mark_type = (const uint8_t *)dev[1];
    d->mark_pos = (const uint32_t *)dev[2];
    d->mark_span = (const uint32_t *)dev[3];
    return DUET_OK;
}

// cl_out reserved for M marks; *r = the device result in it
inline int duet_bind_cluster_result(duet_ctx *ctx, size_t M, duet_cluster_result *r)
{
    const size_t ob[6] = {M * 4, (M + 1) * 4 + 16, M * 2, M, M * 4, M * 4};
    for (int i = 0; i < 6; ++i) {
        int rc = duet_reserve(ctx, ctx->cl_out[i], ob[i]);
        if (rc) return rc;
    }
    r->order = (uint32_t *)ctx->cl_out[0].ptr;
    r->cand_off = (uint32_t *)ctx->cl_out[1].ptr;
    r->cand_contig = (uint16_t *)ctx->cl_out[2].ptr;
    r->cand_type = (uint8_t *)ctx->cl_out[3].ptr;
    r->cand_pos = (uint32_t *)ctx->cl_out[4].ptr;
    r->cand_span = (uint32_t *)ctx->cl_out[5].ptr;
    r->n_cands = (uint32_t *)((char *)ctx->cl_out[1].ptr + (M + 1) * 4);        // spare word after cand_off
    return DUET_OK;
}

// n candidates of the device result r -> the host arrays of res (order[M] only where the caller wants it); the device is idle
inline int duet_fetch_cluster_result(duet_ctx *ctx, size_t M, size_t n, const duet_cluster_result *r, const duet_cluster_result *res)
{
    if (res->order) HIP_TRY(ctx, hipMemcpy(res->order, r->order, M * 4, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(res->cand_off, r->cand_off, (n + 1) * 4, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(res->cand_contig, r->cand_contig, n * 2, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(res->cand_type, r->cand_type, n, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(res->cand_pos, r->cand_pos, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(res->cand_span, r->cand_span, n * 4, hipMemcpyDeviceToHost));
    return DUET_OK;
}

// The CHROM texts of K contigs (NUL-terminated, none null) in one pool, contig k at off[k] .. off[k + 1].  With want_rank also
// rank[k] = the text's rank among the distinct texts in unsigned byte order, the shorter text first on a common prefix (how
// Python compares the strings; equal texts share a rank), and n_texts = the number of distinct texts.
struct DuetChromTable {
    std::string pool;
    std::vector<uint32_t> off;
    std::vector<uint16_t> rank;
    uint32_t n_texts = 0;
};

inline DuetChromTable duet_chrom_table(const char *const *chrom, uint32_t K, bool want_rank)
{
    DuetChromTable t;
    t.off.assign((size_t)K + 1, 0);
    for (uint32_t k = 0; k < K; ++k) {
        t.pool += chrom[k];
        t.off[k + 1] = (uint32_t)t.pool.size();
    }
    if (!want_rank) return t;
    std::vector<uint32_t> by_text(K);
    for (uint32_t k = 0; k < K; ++k) by_text[k] = k;
    auto less = [&](uint32_t a, uint32_t b) {
        const size_t la = t.off[a + 1] - t.off[a], lb = t.off[b + 1] - t.off[b];
        const int c = memcmp(t.pool.data() + t.off[a], t.pool.data() + t.off[b], la < lb ? la : lb);
        return c ? c < 0 : la < lb;
    };
    std::sort(by_text.begin(), by_text.end(), less);
    t.rank.assign(K, 0);
    for (uint32_t i = 0; i < K; ++i) {
        if (i && less(by_text[i - 1], by_text[i])) ++t.n_texts;
        t.rank[by_text[i]] = (uint16_t)t.n_texts;
    }
    ++t.n_texts;
    return t;
}

#endif
