// duet_callset.hip -- gfx950 kernels and C ABI for sv_calling/variants.vcf of the svim-gpu mode: the rows of every clustered
// candidate, formatted on the device from the arrays the fused pipeline (duet_svim_phase_device) leaves
// resident -- the cluster result, the binned depth -- and the raw marks' read names.
//
// Pipeline (one stream):
//   cs_first        first candidate of every contig (the row numbers of the ID column count per contig)
//   cs_len          per candidate: decimal digit counts + CHROM twice + the members' name lengths (order -> mark_name -> name_off)
//   64-bit scan     cs_scan_reduce (tile sums) -> scan_spine_u64 (one workgroup) -> cs_scan_apply: row offsets and the total
//   (one host round trip: the total and the type-code check)
//   cs_write        one wavefront per row: lane 0 formats the numeric pieces into LDS, the lanes copy the pieces and the names
//                   (consecutive lanes on consecutive bytes)

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#include "duet_ef.h"
#include "duet_internal.h"

namespace {

#include "duet_text.hip.h"

constexpr uint32_t kCsThreads = 256, kCsItems = 8, kCsTile = kCsThreads * kCsItems;

struct CsParams {
    uint32_t N, K, depth_bin;
    const uint32_t *cand_off, *order;
    const uint16_t *cand_contig;
    const uint8_t *cand_type;
    const uint32_t *cand_pos, *cand_span;
    const uint32_t *mark_name;
    const uint64_t *name_off;
    const char *name_pool;
    const uint32_t *depth, *depth_off;          // depth_off: device copy [K + 1]
    const char *chrom_pool;
    const uint32_t *chrom_off;                  // [K + 1]
    uint32_t *first;                            // [K] first candidate of each contig that has one
    uint32_t *len;                              // [N] row lengths
    uint64_t *row_off;                          // [N]
    uint64_t *part;                             // [tiles]
    uint64_t *total;                            // [1]
    uint32_t *flag;                             // [1] bit 0: type code > 3, bit 1: a row of 4 GiB or more, bit 2: output overrun
    char *out;
    uint64_t cap;
};

// the numbers of a row
struct CsRow {
    uint32_t k, t, pos, span, n, row;
    uint64_t end, dp, ref;
    uint32_t gt;                                // 2: 1/1, 1: 0/1, 0: 0/0
};

__device__ __forceinline__ CsRow cs_row(const CsParams &p, uint32_t c)
{
    CsRow r;
    r.k = p.cand_contig[c];
    r.t = p.cand_type[c];
    r.pos = p.cand_pos[c];
    r.span = p.cand_span[c];
    r.n = p.cand_off[c + 1] - p.cand_off[c];
    r.row = c - p.first[r.k] + 1u;
    r.end = r.t == 1u ? (uint64_t)r.pos : (uint64_t)r.pos + r.span;
    const uint32_t b0 = p.depth_off[r.k], bins = p.depth_off[r.k + 1] - b0;
    uint64_t d = 0;
    if (bins) {
        const uint32_t b = r.pos / p.depth_bin;
        d = p.depth[b0 + (b < bins - 1u ? b : bins - 1u)];
    }
    r.ref = d > r.n ? d - r.n : 0u;
    r.dp = r.n + r.ref;
    const uint64_t n5 = 5ull * r.n;
    r.gt = n5 >= 4ull * r.dp ? 2u : (n5 >= r.dp ? 1u : 0u);
    return r;
}

__global__ __launch_bounds__(256) void cs_first(const CsParams p)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= p.N) return;
    const uint16_t k = p.cand_contig[c];
    if (c == 0 || p.cand_contig[c - 1] != k) p.first[k] = c;
}

__global__ __launch_bounds__(256) void cs_len(const CsParams p)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= p.N) return;
    const CsRow r = cs_row(p, c);
    if (r.t > 3u) {
        atomicOr(p.flag, 1u);
        p.len[c] = 0;
        return;
    }
    uint64_t names = 0;
    for (uint32_t j = p.cand_off[c]; j < p.cand_off[c + 1]; ++j) {
        const uint32_t nm = p.mark_name[p.order[j]];
        names += p.name_off[nm + 1] - p.name_off[nm];
    }
    const uint32_t L = p.chrom_off[r.k + 1] - p.chrom_off[r.k];
    const uint32_t neg = (r.t == 0u && r.span != 0u) ? 1u : 0u;
    //   CHROM \t POS \t svim_gpu. CHROM . i \t N \t <T> \t . \t PASS \t
    uint64_t n = (uint64_t)L + 1 + digits_u64(r.pos) + 1 + 9 + L + 1 + digits_u64(r.row) + 1 + 1 + 1 + 5 + 1 + 1 + 1 + 4 + 1;
    //   SVTYPE=T ;END=e ;SVLEN=[-]l ;SUPPORT=n ;READS= names (n - 1 commas)
    n += 7 + 3 + 5 + digits_u64(r.end) + 7 + neg + digits_u64(r.span) + 9 + digits_u64(r.n) + 7 + names + (r.n ? r.n - 1u : 0u);
    //   \t GT:DP:AD \t gt : DP : ref , n \n
    n += 1 + 8 + 1 + 3 + 1 + digits_u64(r.dp) + 1 + digits_u64(r.ref) + 1 + digits_u64(r.n) + 1;
    if (n > 0xFFFFFFFFull) {
        atomicOr(p.flag, 2u);
        n = 0;
    }
    p.len[c] = (uint32_t)n;
}

// 64-bit exclusive scan of len[] (row lengths are 32-bit, their sums are not)
__global__ __launch_bounds__(kCsThreads) void cs_scan_reduce(const CsParams p)
{
    __shared__ uint64_t s_w[kCsThreads / 64];
    const uint32_t tid = threadIdx.x, base = blockIdx.x * kCsTile + tid * kCsItems;
    uint64_t acc = 0;
#pragma unroll
    for (uint32_t j = 0; j < kCsItems; ++j)
        if (base + j < p.N) acc += p.len[base + j];
    acc = wave_sum(acc);
    if ((tid & 63u) == 0) s_w[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) p.part[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ __launch_bounds__(kCsThreads) void cs_scan_apply(const CsParams p)
{
    __shared__ uint64_t s_w[kCsThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t base = blockIdx.x * kCsTile + tid * kCsItems;
    uint32_t v[kCsItems];
    uint64_t acc = 0;
#pragma unroll
    for (uint32_t j = 0; j < kCsItems; ++j) {
        v[j] = base + j < p.N ? p.len[base + j] : 0u;
        acc += v[j];
    }
    const uint64_t x = wave_scan(acc, lane);
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    uint64_t run = p.part[blockIdx.x] + x - acc;
    for (uint32_t w = 0; w < wave; ++w) run += s_w[w];
#pragma unroll
    for (uint32_t j = 0; j < kCsItems; ++j) {
        if (base + j < p.N) p.row_off[base + j] = run;
        run += v[j];
    }
}

__device__ __constant__ const char kTypes[4][4] = {"DEL", "INS", "INV", "DUP"};

__global__ __launch_bounds__(256) void cs_write(const CsParams p)
{
    __shared__ char s_a[4][32], s_b[4][128], s_c[4][64];
    __shared__ uint32_t s_len[4][3];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t c = blockIdx.x * 4 + wave; c < p.N; c += gridDim.x * 4) {
        const uint32_t k = p.cand_contig[c];
        const uint32_t m0 = p.cand_off[c], n = p.cand_off[c + 1] - m0;
        if (lane == 0) {
            const CsRow r = cs_row(p, c);
            const char *T = kTypes[r.t & 3u];
            char *a = s_a[wave];
            uint32_t q = 0;
            a[q++] = '\t';
            q += put_u64(a + q, r.pos);
            a[q++] = '\t';
            q += put_str(a + q, "svim_gpu.");
            s_len[wave][0] = q;
            char *b = s_b[wave];
            q = 0;
            b[q++] = '.';
            q += put_u64(b + q, r.row);
            q += put_str(b + q, "\tN\t<");
            q += put_str(b + q, T);
            q += put_str(b + q, ">\t.\tPASS\tSVTYPE=");
            q += put_str(b + q, T);
            q += put_str(b + q, ";END=");
            q += put_u64(b + q, r.end);
            q += put_str(b + q, ";SVLEN=");
            if (r.t == 0u && r.span != 0u) b[q++] = '-';
            q += put_u64(b + q, r.span);
            q += put_str(b + q, ";SUPPORT=");
            q += put_u64(b + q, r.n);
            q += put_str(b + q, ";READS=");
            s_len[wave][1] = q;
            char *e = s_c[wave];
            q = 0;
            q += put_str(e + q, "\tGT:DP:AD\t");
            e[q++] = r.gt == 2u ? '1' : '0';
            e[q++] = '/';
            e[q++] = r.gt >= 1u ? '1' : '0';
            e[q++] = ':';
            q += put_u64(e + q, r.dp);
            e[q++] = ':';
            q += put_u64(e + q, r.ref);
            e[q++] = ',';
            q += put_u64(e + q, r.n);
            e[q++] = '\n';
            s_len[wave][2] = q;
        }
        wave_publish();
        const uint32_t la = s_len[wave][0], lb = s_len[wave][1], lc = s_len[wave][2];
        const uint32_t c0 = p.chrom_off[k], L = p.chrom_off[k + 1] - c0;
        uint64_t cur = p.row_off[c];
        const uint64_t stop = cur + p.len[c];
        if (stop > p.cap || p.len[c] == 0) {
            if (lane == 0) atomicOr(p.flag, 4u);
            __builtin_amdgcn_wave_barrier();
            continue;
        }
        char *out = p.out;
        wave_copy(out + cur, p.chrom_pool + c0, L, lane);                                         // CHROM
        cur += L;
        wave_copy(out + cur, s_a[wave], la, lane);                                                // \t POS \t svim_gpu.
        cur += la;
        wave_copy(out + cur, p.chrom_pool + c0, L, lane);                                         // CHROM
        cur += L;
        wave_copy(out + cur, s_b[wave], lb, lane);                                                // .i ... ;READS=
        cur += lb;
        // the members' names in cluster order, 64 at a time: each lane looks one up, a wave scan places them, then all lanes
        // copy each name (consecutive lanes on consecutive bytes)
        for (uint32_t j0 = 0; j0 < n; j0 += 64) {
            const uint32_t j = j0 + lane;
            uint64_t src = 0;
            uint32_t ln = 0, w = 0;
            if (j < n) {
                const uint32_t nm = p.mark_name[p.order[m0 + j]];
                src = p.name_off[nm];
                ln = (uint32_t)(p.name_off[nm + 1] - src);
                w = ln + (j + 1 < n ? 1u : 0u);
            }
            const uint32_t x = wave_scan(w, lane);
            const uint32_t at = x - w;
            const uint32_t cnt = n - j0 < 64u ? n - j0 : 64u;
            for (uint32_t q = 0; q < cnt; ++q) {
                const uint32_t lo = __shfl((uint32_t)src, q, 64), hi = __shfl((uint32_t)(src >> 32), q, 64);
                const uint32_t qln = __shfl(ln, q, 64), qat = __shfl(at, q, 64);
                const uint64_t qsrc = ((uint64_t)hi << 32) | lo;
                wave_copy(out + cur + qat, p.name_pool + qsrc, qln, lane);
                if (lane == 0 && j0 + q + 1 < n) out[cur + qat + qln] = ',';
            }
            cur += __shfl(x, 63, 64);
        }
        wave_copy(out + cur, s_c[wave], lc, lane);                                                // \tGT:DP:AD\t ... \n
        __builtin_amdgcn_wave_barrier();                                                          // before lane 0 rewrites the LDS pieces
    }
}

// inputs of one call, all device pointers except depth_off (HOST, K + 1) and the CHROM texts (HOST)
struct CsInputs {
    uint32_t N, M, K, depth_bin;
    const uint32_t *cand_off, *order;
    const uint16_t *cand_contig;
    const uint8_t *cand_type;
    const uint32_t *cand_pos, *cand_span, *mark_name;
    const uint64_t *name_off;
    const char *name_pool;
    const uint32_t *depth;
    const uint32_t *depth_off_host;
    const char *const *chrom;
};

// steps 1-3 and the round trip; *need = the text's size.  `small` holds the scalars, the depth offsets and the CHROM texts
int cs_plan(duet_ctx *ctx, const CsInputs &in, CsParams &p, hipStream_t st, uint64_t *need)
{
    const uint32_t N = in.N, K = in.K;
    for (uint32_t k = 0; k < K; ++k)
        if (!in.chrom[k]) return duet_fail(ctx, DUET_ERR_INVALID, "null CHROM text");
    const DuetChromTable ct = duet_chrom_table(in.chrom, K, false);
    const std::string &chrom_pool = ct.pool;
    const uint32_t nb = (N + kCsTile - 1) / kCsTile;
    const size_t small = 64 + ((size_t)K + 1) * 8 + chrom_pool.size() + 64;
    const size_t sizes[5] = {(size_t)K * 4 + 64, (size_t)N * 4, (size_t)N * 8, (size_t)nb * 8 + 64, small};
    int rc;
    for (int i = 0; i < 5; ++i)
        if ((rc = duet_reserve(ctx, ctx->callset_ws.b[i], sizes[i]))) return rc;
    char *sm = (char *)ctx->callset_ws.b[4].ptr;
    uint32_t *d_depth_off = (uint32_t *)(sm + 64), *d_chrom_off = d_depth_off + (K + 1);
    char *d_chrom = (char *)(d_chrom_off + (K + 1));
    HIP_TRY(ctx, hipMemsetAsync(sm, 0, 64, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_depth_off, in.depth_off_host, ((size_t)K + 1) * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_chrom_off, ct.off.data(), ((size_t)K + 1) * 4, hipMemcpyHostToDevice, st));
    if (!chrom_pool.empty()) HIP_TRY(ctx, hipMemcpyAsync(d_chrom, chrom_pool.data(), chrom_pool.size(), hipMemcpyHostToDevice, st));
    memset(&p, 0, sizeof(p));
    p.N = N; p.K = K; p.depth_bin = in.depth_bin;
    p.cand_off = in.cand_off; p.order = in.order; p.cand_contig = in.cand_contig; p.cand_type = in.cand_type;
    p.cand_pos = in.cand_pos; p.cand_span = in.cand_span; p.mark_name = in.mark_name; p.name_off = in.name_off;
    p.name_pool = in.name_pool; p.depth = in.depth; p.depth_off = d_depth_off; p.chrom_pool = d_chrom; p.chrom_off = d_chrom_off;
    p.first = (uint32_t *)ctx->callset_ws.b[0].ptr;
    p.len = (uint32_t *)ctx->callset_ws.b[1].ptr;
    p.row_off = (uint64_t *)ctx->callset_ws.b[2].ptr;
    p.part = (uint64_t *)ctx->callset_ws.b[3].ptr;
    p.total = (uint64_t *)sm;
    p.flag = (uint32_t *)(sm + 8);
    const uint32_t g = (N + 255) / 256;
    hipLaunchKernelGGL(cs_first, dim3(g), dim3(256), 0, st, p);
    hipLaunchKernelGGL(cs_len, dim3(g), dim3(256), 0, st, p);
    hipLaunchKernelGGL(cs_scan_reduce, dim3(nb), dim3(kCsThreads), 0, st, p);
    hipLaunchKernelGGL(scan_spine_u64, dim3(1), dim3(1024), 0, st, p.part, nb, p.total);
    hipLaunchKernelGGL(cs_scan_apply, dim3(nb), dim3(kCsThreads), 0, st, p);
    HIP_TRY(ctx, hipGetLastError());
    uint64_t fin[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(fin, sm, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (fin[1] & 1u) return duet_fail(ctx, DUET_ERR_INVALID, "candidate type code other than 0-3 (DEL, INS, INV, DUP)");
    if (fin[1] & 2u) return duet_fail(ctx, DUET_ERR_INVALID, "a row of 4 GiB or more");
    *need = fin[0];
    return DUET_OK;
}

int cs_write_rows(duet_ctx *ctx, CsParams &p, char *out, uint64_t cap, hipStream_t st)
{
    p.out = out;
    p.cap = cap;
    const uint32_t wb = (p.N + 3) / 4;
    hipLaunchKernelGGL(cs_write, dim3(wb < 8192u ? wb : 8192u), dim3(256), 0, st, p);
    HIP_TRY(ctx, hipGetLastError());
    return DUET_OK;
}

int cs_check(duet_ctx *ctx, const duet_svim_problem *prob, const duet_cluster_result *res, const duet_callset_names *names,
             uint64_t *out_len)
{
    if (!ctx) return duet_fail(nullptr, DUET_ERR_INVALID, "null context");
    if (!prob || !res || !names || !out_len) return duet_fail(ctx, DUET_ERR_INVALID, "null argument");
    *out_len = 0;
    if (prob->n_contigs == 0 || prob->n_contigs > 65535 || !prob->depth_off || !names->chrom || names->n_contigs != prob->n_contigs)
        return duet_fail(ctx, DUET_ERR_INVALID, "bad contig count or missing contig arrays");
    if (prob->depth_bin == 0) return duet_fail(ctx, DUET_ERR_INVALID, "depth_bin must be >= 1");
    return DUET_OK;
}

}  // namespace

extern "C" {

int duet_svim_vcf_rows_device(duet_ctx *ctx, const duet_svim_problem *prob, const duet_cluster_result *res, uint32_t n_cands,
                              const duet_callset_names *names, char *out_text, uint64_t out_cap, uint64_t *out_len, void *stream_)
{
    int rc;
    if ((rc = cs_check(ctx, prob, res, names, out_len))) return rc;
    if (n_cands == 0) return DUET_OK;
    if (!res->order || !res->cand_off || !res->cand_contig || !res->cand_type || !res->cand_pos || !res->cand_span ||
        !names->mark_name || !names->name_off || !names->name_pool || !out_text ||
        (prob->depth_off[prob->n_contigs] && !prob->depth))
        return duet_fail(ctx, DUET_ERR_INVALID, "null array");
    hipStream_t st = (hipStream_t)stream_;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    CsInputs in = {n_cands, prob->marks.n_marks, prob->n_contigs, prob->depth_bin, res->cand_off, res->order, res->cand_contig,
                   res->cand_type, res->cand_pos, res->cand_span, names->mark_name, names->name_off, names->name_pool, prob->depth,
                   prob->depth_off, names->chrom};
    CsParams p;
    uint64_t need = 0;
    if ((rc = cs_plan(ctx, in, p, st, &need))) return rc;
    *out_len = need;
    if (need > out_cap) return duet_fail(ctx, DUET_ERR_INVALID, "output buffer too small for the callset rows (*out_len = size needed)");
    return cs_write_rows(ctx, p, out_text, out_cap, st);
}

int duet_svim_vcf_rows_host(duet_ctx *ctx, const duet_svim_problem *prob, const duet_cluster_result *res, uint32_t n_cands,
                            const duet_callset_names *names, char *out_text, uint64_t out_cap, uint64_t *out_len)
{
    int rc;
    if ((rc = cs_check(ctx, prob, res, names, out_len))) return rc;
    if (n_cands == 0) return DUET_OK;
    const uint32_t M = prob->marks.n_marks, K = prob->n_contigs, N = n_cands;
    if (N > M) return duet_fail(ctx, DUET_ERR_INVALID, "more candidates than marks");
    if (!res->order || !res->cand_off || !res->cand_contig || !res->cand_type || !res->cand_pos || !res->cand_span ||
        !names->mark_name || !names->name_off || !out_text)
        return duet_fail(ctx, DUET_ERR_INVALID, "null array");
    const uint64_t pool_bytes = names->name_off[names->n_names];
    if (pool_bytes && !names->name_pool) return duet_fail(ctx, DUET_ERR_INVALID, "null name pool");
    const uint64_t n_bins = prob->depth_off[K];
    if (n_bins && !prob->depth) return duet_fail(ctx, DUET_ERR_INVALID, "null depth array");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->own_stream;
    const void *src[10] = {res->cand_off, res->order, res->cand_contig, res->cand_type, res->cand_pos, res->cand_span,
                           names->mark_name, names->name_off, names->name_pool, prob->depth};
    const size_t bytes[10] = {((size_t)N + 1) * 4, (size_t)M * 4, (size_t)N * 2, (size_t)N, (size_t)N * 4, (size_t)N * 4,
                              (size_t)M * 4, ((size_t)names->n_names + 1) * 8, (size_t)pool_bytes, (size_t)n_bins * 4};
    void *dev[10];
    if ((rc = duet_stage_arrays(ctx, ctx->callset_ws.b + 5, src, bytes, 10, s, dev))) return rc;
    CsInputs in = {N, M, K, prob->depth_bin, (const uint32_t *)dev[0], (const uint32_t *)dev[1], (const uint16_t *)dev[2],
                   (const uint8_t *)dev[3], (const uint32_t *)dev[4], (const uint32_t *)dev[5], (const uint32_t *)dev[6],
                   (const uint64_t *)dev[7], (const char *)dev[8], (const uint32_t *)dev[9], prob->depth_off, names->chrom};
    CsParams p;
    uint64_t need = 0;
    if ((rc = cs_plan(ctx, in, p, s, &need))) return rc;
    *out_len = need;
    if (need > out_cap) return duet_fail(ctx, DUET_ERR_INVALID, "output buffer too small for the callset rows (*out_len = size needed)");
    DevBuf &ob = ctx->callset_ws.b[15];
    if ((rc = duet_reserve(ctx, ob, need + 64))) return rc;
    if ((rc = cs_write_rows(ctx, p, (char *)ob.ptr, need, s))) return rc;
    uint32_t flag = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&flag, p.flag, 4, hipMemcpyDeviceToHost, s));
    if (need) HIP_TRY(ctx, hipMemcpyAsync(out_text, ob.ptr, need, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (flag & 4u) return duet_fail(ctx, DUET_ERR_INVALID, "callset rows overran their offsets");
    return DUET_OK;
}

}  // extern "C"
