// duet_svim.hip -- the fused SVIM-mode pipeline: raw marks -> clusters (stage A0, duet_cluster.hip) -> the arrays step E/F reads
// -> its decisions (duet_ef.hip) or the candidates' features (duet_tune.hip).  Host drivers and one small kernel; DESIGN.md
// section 9 has the pipeline and its measurements.
//
// Every entry is the same front -- checks, workspace, the cached depth_off upload, the clustering whose emit kernel also writes
// what a caller VCF would have carried -- and then one of three ends: E/F planned on the device (fully asynchronous), E/F
// planned on the host from the candidates per contig (one round trip), or the feature export behind that same plan.  The host
// entries stage their arrays (duet_internal.h) around the device entries.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#include "duet_ef.h"
#include "duet_internal.h"

namespace {

// ctg_off[k] = first candidate whose contig is >= k (candidates are sorted by contig); ctg_off[K] = N
__global__ void sv_contig_offsets(const uint16_t *cand_contig, const uint32_t *n_cands, uint32_t K, uint32_t *ctg_off)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > K) return;
    const uint32_t N = *n_cands;
    uint32_t lo = 0, hi = N;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (cand_contig[mid] < k) lo = mid + 1; else hi = mid;
    }
    ctg_off[k] = k == K ? N : lo;
}

// The front of every device entry: the clustering on `st` and ef = the cluster result plus sv_ws written as E/F's candidate
// columns -- everything but n_cands and cand_ctg_off, which the plan gives.  ef.n_marks == 0 on return: the empty problem,
// nothing to run.  outputs_given: whether the entry's own output pointers are there.  n_cands_host: zeroed when given; null:
// E/F plans on the device (cl_emit writes its plan).
int svim_front(duet_ctx *ctx, const duet_svim_problem *pr, const duet_cluster_result *res, bool outputs_given, uint32_t *n_cands_host,
               hipStream_t st, duet_ef_problem &ef)
{
    memset(&ef, 0, sizeof(ef));
    if (!ctx) return duet_fail(nullptr, DUET_ERR_INVALID, "null context");
    if (!pr || !res || !outputs_given) return duet_fail(ctx, DUET_ERR_INVALID, "null argument");
    if (!pr->depth_off || pr->depth_bin == 0 || pr->n_contigs == 0 || pr->n_contigs > 65535)
        return duet_fail(ctx, DUET_ERR_INVALID, "bad depth / contig description");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t M = pr->marks.n_marks, K = pr->n_contigs;
    if (n_cands_host) *n_cands_host = 0;
    if (M == 0) {
        if (res->n_cands) HIP_TRY(ctx, hipMemsetAsync(res->n_cands, 0, 4, st));
        return DUET_OK;
    }
    if (!pr->mark_read || !pr->depth) return duet_fail(ctx, DUET_ERR_INVALID, "null array");
    // workspace: ctg_off + depth_off on the device, the adapted candidate columns, the gathered marks
    int rc;
    const size_t sz[5] = {((size_t)K + 1) * 4 * 2, (size_t)M * 4, (size_t)M * 4, (size_t)M, (size_t)M * 4};
    for (int i = 0; i < 5; ++i)
        if ((rc = duet_reserve(ctx, ctx->sv_ws[i], sz[i]))) return rc;
    // (reserved first: a reallocation moves d_depth_off, which the comparison below then takes for a change)
    uint32_t *d_depth_off = (uint32_t *)ctx->sv_ws[0].ptr + (K + 1);
    // (uploaded only when they change: a pageable host-to-device copy in front of every run keeps the host from queueing the
    // run's thirty launches ahead of the device -- 45 us of gaps per 0.37 ms run at 1 M marks)
    // (the copy is ordered on the stream it was issued on: a run on ANOTHER stream uploads again -- after waiting for that
    // stream, whose pageable copy may still be reading the host vector)
    if (ctx->sv_depth_off_at != (void *)d_depth_off || ctx->sv_depth_off.size() != (size_t)K + 1 || ctx->sv_depth_off_stream != st ||
        memcmp(ctx->sv_depth_off.data(), pr->depth_off, ((size_t)K + 1) * 4) != 0) {
        // (the previous copy's source is about to change: wait for THAT COPY -- an event recorded behind it, not the stream it
        // was issued on, which the caller may have destroyed in the meantime)
        if (!ctx->sv_depth_off_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->sv_depth_off_ev, hipEventDisableTiming));
        if (ctx->sv_depth_off_at) HIP_TRY(ctx, hipEventSynchronize(ctx->sv_depth_off_ev));
        ctx->sv_depth_off.assign(pr->depth_off, pr->depth_off + K + 1);
        HIP_TRY(ctx, hipMemcpyAsync(d_depth_off, ctx->sv_depth_off.data(), ((size_t)K + 1) * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipEventRecord(ctx->sv_depth_off_ev, st));
        ctx->sv_depth_off_at = (void *)d_depth_off;
        ctx->sv_depth_off_stream = st;
    }
    // clustering; its emit kernel also writes what a caller VCF would have carried (support, reference reads, GT)
    // and the marks' read indices in output order
    SvExtra sv;
    sv.mark_in = pr->mark_read; sv.depth = pr->depth; sv.depth_off = d_depth_off; sv.depth_bin = pr->depth_bin;
    sv.mark_out = (uint32_t *)ctx->sv_ws[4].ptr; sv.svread = (uint32_t *)ctx->sv_ws[1].ptr;
    sv.refread = (uint32_t *)ctx->sv_ws[2].ptr; sv.gt = (uint8_t *)ctx->sv_ws[3].ptr;
    sv.ef_ctg_off = nullptr; sv.ef_zero = nullptr; sv.n_contigs = K;
    // (fully asynchronous runs: cl_emit writes step E/F's plan into E/F's workspace, sized for the bound of M candidates)
    if (!n_cands_host && (rc = duet_ef_plan_on_device_prepare(ctx, K, M, st, &sv.ef_ctg_off, &sv.ef_zero))) return rc;
    if ((rc = duet_cluster_run(ctx, &pr->marks, res, st, &sv))) return rc;
    ef.n_contigs = K; ef.n_marks = M; ef.n_reads = pr->n_reads;
    ef.read_tag = pr->read_tag;
    ef.cand_pos = res->cand_pos; ef.cand_svlen = res->cand_span; ef.cand_svread = sv.svread; ef.cand_refread = sv.refread;
    ef.cand_gt_ok = sv.gt; ef.cand_off = res->cand_off; ef.mark_read = sv.mark_out;
    ef.svlen_thres = pr->svlen_thres; ef.suppread_thres = pr->suppread_thres;
    return DUET_OK;
}

// The host plan behind the front: candidates per contig -> ctg_off[K + 1], which ef then points to, and ef.n_cands = N.
// The one host round trip of a host-planned run.
int svim_host_plan(duet_ctx *ctx, const duet_cluster_result *res, hipStream_t st, std::vector<uint32_t> &ctg_off, duet_ef_problem &ef)
{
    const uint32_t K = ef.n_contigs;
    uint32_t *d_ctg_off = (uint32_t *)ctx->sv_ws[0].ptr;
    hipLaunchKernelGGL(sv_contig_offsets, dim3((K + 1 + 255) / 256), dim3(256), 0, st, (const uint16_t *)res->cand_contig,
                       (const uint32_t *)res->n_cands, K, d_ctg_off);
    ctg_off.resize((size_t)K + 1);
    HIP_TRY(ctx, hipMemcpyAsync(ctg_off.data(), d_ctg_off, ((size_t)K + 1) * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    ef.n_cands = ctg_off[K];
    ef.cand_ctg_off = ctg_off.data();
    return DUET_OK;
}

// What both host entries check once their own output pointers are known to be there: every array is on the host here, so what
// the device entry has to trust is checked -- a contig id beyond the depth description would index sv_depth_off / the E/F plan
// outside their K + 1 entries.  Zeroes *res->n_cands; nothing more for the empty problem.
int svim_host_check(duet_ctx *ctx, const duet_svim_problem *pr, const duet_cluster_result *res, bool outputs_given)
{
    if (!pr || !res || !res->n_cands || !outputs_given) return duet_fail(ctx, DUET_ERR_INVALID, "null argument");
    if (!pr->depth_off || pr->n_contigs == 0) return duet_fail(ctx, DUET_ERR_INVALID, "bad depth / contig description");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t M = pr->marks.n_marks;
    *res->n_cands = 0;
    if (M == 0) return DUET_OK;
    if (!res->cand_off || !res->cand_contig || !res->cand_type || !res->cand_pos || !res->cand_span)
        return duet_fail(ctx, DUET_ERR_INVALID, "null result array");
    for (uint32_t k = 0; k < pr->n_contigs; ++k)
        if (pr->depth_off[k] > pr->depth_off[k + 1]) return duet_fail(ctx, DUET_ERR_INVALID, "depth_off must be non-decreasing");
    if (!pr->marks.mark_contig) return duet_fail(ctx, DUET_ERR_INVALID, "null array");
    for (uint32_t i = 0; i < M; ++i)
        if (pr->marks.mark_contig[i] >= pr->n_contigs)
            return duet_fail(ctx, DUET_ERR_INVALID, "a mark's contig id is not below n_contigs (the depth description's contig count)");
    return DUET_OK;
}

// host arrays of a SVIM problem -> cl_in and sv_in, *d = the problem over them; *r = the device result in cl_out
int svim_stage(duet_ctx *ctx, const duet_svim_problem *pr, duet_svim_problem *d, duet_cluster_result *r, hipStream_t s)
{
    const uint32_t M = pr->marks.n_marks;
    *d = *pr;
    int rc = duet_stage_marks(ctx, &pr->marks, &d->marks, s);
    if (rc) return rc;
    const void *src[3] = {pr->mark_read, pr->read_tag, pr->depth};
    const size_t bytes[3] = {(size_t)M * 4, (size_t)pr->n_reads * 8, (size_t)pr->depth_off[pr->n_contigs] * 4};
    void *dev[3];
    for (int i = 0; i < 3; ++i)
        if (!src[i] && bytes[i]) return duet_fail(ctx, DUET_ERR_INVALID, "null array");
    if ((rc = duet_stage_arrays(ctx, ctx->sv_in, src, bytes, 3, s, dev))) return rc;
    d->mark_read = (const uint32_t *)dev[0];
    d->read_tag = (const uint64_t *)dev[1];
    d->depth = (const uint32_t *)dev[2];
    return duet_bind_cluster_result(ctx, M, r);
}

// the first check of the feature entries, in front of the null-argument check (pc_cap == nullptr: the reference's cap)
int svim_cap_check(duet_ctx *ctx, const uint32_t *pc_cap)
{
    if (!ctx) return duet_fail(nullptr, DUET_ERR_INVALID, "null context");
    if (pc_cap && *pc_cap > (1u << 30) - 3u) return duet_fail(ctx, DUET_ERR_INVALID, "pc_cap is above 2^30 - 3 (the tag word saturates pc at 2^30 - 2)");
    return DUET_OK;
}

// (pc_cap == nullptr: the reference's cap through duet_ef_features_device; else duet_ef_features_cap_device with *pc_cap)
int svim_features_device(duet_ctx *ctx, const duet_svim_problem *pr, const duet_cluster_result *res, duet_tune_feature *out_feat,
                         uint32_t *n_cands_host, void *stream_, const uint32_t *pc_cap)
{
    int rc = svim_cap_check(ctx, pc_cap);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream_;
    duet_ef_problem ef;
    std::vector<uint32_t> ctg_off;
    rc = svim_front(ctx, pr, res, out_feat && n_cands_host, n_cands_host, st, ef);
    if (rc || ef.n_marks == 0) return rc;
    if ((rc = svim_host_plan(ctx, res, st, ctg_off, ef))) return rc;
    *n_cands_host = ef.n_cands;
    if (ef.n_cands == 0) return DUET_OK;
    return pc_cap ? duet_ef_features_cap_device(ctx, &ef, *pc_cap, out_feat, st) : duet_ef_features_device(ctx, &ef, out_feat, st);
}

int svim_features_host(duet_ctx *ctx, const duet_svim_problem *pr, const duet_cluster_result *res, duet_tune_feature *out_feat,
                       const uint32_t *pc_cap)
{
    int rc = svim_cap_check(ctx, pc_cap);
    if (rc) return rc;
    rc = svim_host_check(ctx, pr, res, out_feat != nullptr);
    if (rc || pr->marks.n_marks == 0) return rc;
    hipStream_t s = ctx->own_stream;
    const uint32_t M = pr->marks.n_marks;
    duet_svim_problem d;
    duet_cluster_result r;
    if ((rc = svim_stage(ctx, pr, &d, &r, s))) return rc;
    DevBuf &bf = ctx->tune_ws.b[2];                     // (the feature staging of duet_ef_features_host)
    if ((rc = duet_reserve(ctx, bf, (size_t)M * sizeof(duet_tune_feature)))) return rc;
    uint32_t n = 0;
    rc = svim_features_device(ctx, &d, &r, (duet_tune_feature *)bf.ptr, &n, s, pc_cap);
    if (rc && rc != DUET_ERR_DIV_ZERO) return rc;
    // (a division by zero names its candidate: the results come back all the same, and the message with them)
    const std::string msg = ctx->err;
    *res->n_cands = n;
    int rc2 = duet_fetch_cluster_result(ctx, M, n, &r, res);
    if (rc2) return rc2;
    HIP_TRY(ctx, hipMemcpy(out_feat, bf.ptr, (size_t)n * sizeof(duet_tune_feature), hipMemcpyDeviceToHost));
    if (rc) ctx->err = msg;
    return rc;
}

// The phase-set links of the fused pipeline's candidates (duet_pslinks.hip): the front, the host plan, then the links of the
// adapted problem -- as svim_features_device reaches the feature export.  out_on_host: the records go to host memory.
int svim_ps_links_device(duet_ctx *ctx, const duet_svim_problem *pr, const duet_cluster_result *res, uint32_t pc_cap, duet_ps_link *out,
                         uint32_t out_cap, uint32_t *n_links, uint32_t *n_cands_host, hipStream_t st, bool out_on_host)
{
    if (n_links) *n_links = 0;
    int rc = svim_cap_check(ctx, &pc_cap);
    if (rc) return rc;
    duet_ef_problem ef;
    std::vector<uint32_t> ctg_off;
    rc = svim_front(ctx, pr, res, n_links && n_cands_host && (out || !out_cap), n_cands_host, st, ef);
    if (rc || ef.n_marks == 0) return rc;
    if ((rc = svim_host_plan(ctx, res, st, ctg_off, ef))) return rc;
    *n_cands_host = ef.n_cands;
    if (ef.n_cands == 0) return DUET_OK;
    return duet_ps_links_run(ctx, &ef, pc_cap, out, out_cap, n_links, st, out_on_host);
}

int svim_ps_links_host(duet_ctx *ctx, const duet_svim_problem *pr, const duet_cluster_result *res, uint32_t pc_cap, duet_ps_link *out,
                       uint32_t out_cap, uint32_t *n_links)
{
    if (n_links) *n_links = 0;
    int rc = svim_cap_check(ctx, &pc_cap);
    if (rc) return rc;
    rc = svim_host_check(ctx, pr, res, n_links && (out || !out_cap));
    if (rc || pr->marks.n_marks == 0) return rc;
    hipStream_t s = ctx->own_stream;
    const uint32_t M = pr->marks.n_marks;
    duet_svim_problem d;
    duet_cluster_result r;
    if ((rc = svim_stage(ctx, pr, &d, &r, s))) return rc;
    uint32_t n = 0;
    rc = svim_ps_links_device(ctx, &d, &r, pc_cap, out, out_cap, n_links, &n, s, true);
    // (a record buffer that is too small: the cluster result comes back all the same, and the message with the exact count)
    if (rc && !(rc == DUET_ERR_INVALID && *n_links > out_cap)) return rc;
    const std::string msg = ctx->err;
    HIP_TRY(ctx, hipStreamSynchronize(s));
    *res->n_cands = n;
    int rc2 = duet_fetch_cluster_result(ctx, M, n, &r, res);
    if (rc2) return rc2;
    if (rc) ctx->err = msg;
    return rc;
}

}  // namespace

extern "C" {

int duet_svim_ps_links_device(duet_ctx *ctx, const duet_svim_problem *pr, const duet_cluster_result *res, uint32_t pc_cap, duet_ps_link *out,
                              uint32_t out_cap, uint32_t *n_links, uint32_t *n_cands_host, void *stream_)
{
    return svim_ps_links_device(ctx, pr, res, pc_cap, out, out_cap, n_links, n_cands_host, (hipStream_t)stream_, false);
}

int duet_svim_ps_links_host(duet_ctx *ctx, const duet_svim_problem *pr, const duet_cluster_result *res, uint32_t pc_cap, duet_ps_link *out,
                            uint32_t out_cap, uint32_t *n_links)
{
    return svim_ps_links_host(ctx, pr, res, pc_cap, out, out_cap, n_links);
}

int duet_svim_phase_device(duet_ctx *ctx, const duet_svim_problem *pr, const duet_cluster_result *res, uint8_t *out_pred,
                           uint32_t *out_ps, uint32_t *n_cands_host, void *stream_)
{
    hipStream_t st = (hipStream_t)stream_;
    duet_ef_problem ef;
    int rc = svim_front(ctx, pr, res, out_pred && out_ps, n_cands_host, st, ef);
    if (rc || ef.n_marks == 0) return rc;
    if (!n_cands_host) {
        // fully asynchronous: E/F is planned on the device from the candidates' contig column; buffers and grids are
        // sized for the upper bound (a candidate has at least one mark) and the kernels read the real count
        ef.n_cands = ef.n_marks;
        return duet_ef_run_planned_on_device(ctx, &ef, ef.n_marks, (const uint32_t *)res->n_cands, (const uint16_t *)res->cand_contig, out_pred, out_ps, st);
    }
    std::vector<uint32_t> ctg_off;
    if ((rc = svim_host_plan(ctx, res, st, ctg_off, ef))) return rc;
    *n_cands_host = ef.n_cands;
    if (ef.n_cands == 0) return DUET_OK;
    return duet_ef_run_device(ctx, &ef, out_pred, out_ps, st);
}

int duet_svim_phase_host(duet_ctx *ctx, const duet_svim_problem *pr, const duet_cluster_result *res, uint8_t *out_pred, uint32_t *out_ps)
{
    if (!ctx) return duet_fail(nullptr, DUET_ERR_INVALID, "null context");
    int rc = svim_host_check(ctx, pr, res, out_pred && out_ps);
    if (rc || pr->marks.n_marks == 0) return rc;
    hipStream_t s = ctx->own_stream;
    const uint32_t M = pr->marks.n_marks;
    duet_svim_problem d;
    duet_cluster_result r;
    if ((rc = svim_stage(ctx, pr, &d, &r, s))) return rc;
    if ((rc = duet_reserve(ctx, ctx->sv_out[0], (size_t)M + 16))) return rc;
    if ((rc = duet_reserve(ctx, ctx->sv_out[1], (size_t)M * 4 + 16))) return rc;
    uint32_t n = 0;
    if ((rc = duet_svim_phase_device(ctx, &d, &r, (uint8_t *)ctx->sv_out[0].ptr, (uint32_t *)ctx->sv_out[1].ptr, &n, s))) return rc;
    if ((rc = duet_ef_check(ctx, s))) return rc;                                        // (synchronises; DUET_ERR_DIV_ZERO comes out here)
    *res->n_cands = n;
    if ((rc = duet_fetch_cluster_result(ctx, M, n, &r, res))) return rc;
    HIP_TRY(ctx, hipMemcpy(out_pred, ctx->sv_out[0].ptr, (size_t)n, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(out_ps, ctx->sv_out[1].ptr, (size_t)n * 4, hipMemcpyDeviceToHost));
    return DUET_OK;
}

int duet_svim_features_device(duet_ctx *ctx, const duet_svim_problem *pr, const duet_cluster_result *res, duet_tune_feature *out_feat,
                              uint32_t *n_cands_host, void *stream_)
{
    return svim_features_device(ctx, pr, res, out_feat, n_cands_host, stream_, nullptr);
}

int duet_svim_features_cap_device(duet_ctx *ctx, const duet_svim_problem *pr, const duet_cluster_result *res, uint32_t pc_cap,
                                  duet_tune_feature *out_feat, uint32_t *n_cands_host, void *stream_)
{
    return svim_features_device(ctx, pr, res, out_feat, n_cands_host, stream_, &pc_cap);
}

int duet_svim_features_host(duet_ctx *ctx, const duet_svim_problem *pr, const duet_cluster_result *res, duet_tune_feature *out_feat)
{
    return svim_features_host(ctx, pr, res, out_feat, nullptr);
}

int duet_svim_features_cap_host(duet_ctx *ctx, const duet_svim_problem *pr, const duet_cluster_result *res, uint32_t pc_cap,
                                duet_tune_feature *out_feat)
{
    return svim_features_host(ctx, pr, res, out_feat, &pc_cap);
}

}  // extern "C"
