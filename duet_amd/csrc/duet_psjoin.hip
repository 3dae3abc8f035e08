// duet_psjoin.hip -- joined phase sets (include/duet_ef.h: duet_ps_join_tags_device, duet_ps_join_diff_device):
// the table (contig, PS) -> (BLOCK, FLIP) that duet_amd/ps_links.py: blocks builds from the phase-set links, applied to the read tags,
// and the per-candidate comparison of the calls before and after.
//
//   the host checks the table and the offsets, lays out one slice of the table per contig and stages it: keys (the PS values,
//   ascending inside a slice) and values (flip << 32 | block)
//   pj_tags      one lane per read: its contig from read_off, its PS looked up by bisection in the contig's slice (a workgroup whose
//                reads lie inside one contig and whose slice holds at most kLdsSlice keys bisects a copy in LDS); PS -> BLOCK, hap 1 <-> 2
//                under FLIP; the changed words counted by ballot, one integer add per wavefront
//   pj_diff      one lane per candidate: the change code of (pred0, ps0) -> (pred1, ps1), the table looked up for `relabelled` alone;
//                the eight counts by ballots, one integer add per wavefront and code
// Integers only.  The adds are integer atomics on words of the call's own header: sums, whatever the order of arrival.  A refusal
// found on the device is a plain store of 1 to a word of its own.
#include "duet_internal.h"

#include <cstring>

namespace {

#include "duet_seeds.hip.h"                // kUntagged, tag_ps, tag_hap, lower_bound_u32

struct Arena {                      // pieces of one allocation, each at a multiple of 256 bytes
    size_t total = 0;
    size_t take(size_t bytes) { const size_t at = total; total += (bytes + 255) & ~(size_t)255; return at; }
};

constexpr uint32_t kThreads = 256;                    // reads (candidates) per workgroup
constexpr uint32_t kLdsSlice = 2048;                  // keys of one contig's slice that pj_tags copies into LDS at most (8 KiB)
// header words of a call
constexpr uint32_t kHdrChanged = 0, kHdrCounts = 1, kBadPred = 9, kBadContig = 10, kHdrWords = 16;

int fail(duet_ctx *ctx, int code, const char *msg) { return duet_fail(ctx, code, msg); }

struct Table {                      // the staged table: slice k = [slice_off[k], slice_off[k + 1])
    uint32_t K, n;
    const uint32_t *slice_off;      // [K + 1]
    const uint32_t *key;            // [n] PS
    const uint64_t *val;            // [n] flip << 32 | block
};

// the first k with off[k + 1] > i (empty contigs own nothing); off ascends from 0 to the element count, i below it
__device__ __forceinline__ uint32_t contig_of(const uint32_t *off, uint32_t K, uint32_t i)
{
    uint32_t lo = 0, hi = K - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (off[mid + 1] <= i) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the row of (k, ps): its index, or t.n when the table has none
__device__ __forceinline__ uint32_t find_row(const Table &t, uint32_t k, uint32_t ps)
{
    const uint32_t s0 = t.slice_off[k], s1 = t.slice_off[k + 1];
    const uint32_t i = s0 + lower_bound_u32(t.key + s0, s1 - s0, ps);
    return (i < s1 && t.key[i] == ps) ? i : t.n;
}

// the tag word under row value v: ps -> block; hap 1 <-> 2 under flip; pc bit for bit
__device__ __forceinline__ uint64_t remap(uint64_t w, uint64_t v)
{
    const uint32_t hap = tag_hap(w);
    uint64_t out = (w & 0xFFFFFFFF00000000ull) | (uint32_t)v;
    if ((v >> 32) != 0 && (hap == 1u || hap == 2u)) out ^= 3ull << 62;
    return out;
}

__global__ __launch_bounds__(kThreads) void pj_tags(const uint64_t *read_tag, uint64_t *out_tag, uint32_t R, const uint32_t *read_off,
                                                     const Table t, uint32_t *hdr)
{
    __shared__ uint32_t s_key[kLdsSlice];
    const uint64_t r64 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const bool live = r64 < R;
    const uint32_t r = (uint32_t)r64;
    // the tile's first and last read: the same contig means one slice for the whole workgroup (uniform: every lane computes it)
    const uint32_t first = blockIdx.x * kThreads, last = (R - first > kThreads ? first + kThreads : R) - 1u;
    const uint32_t k_first = contig_of(read_off, t.K, first), k_last = contig_of(read_off, t.K, last);
    const uint32_t s0 = t.slice_off[k_first], len = t.slice_off[k_first + 1] - s0;
    const bool in_lds = k_first == k_last && len != 0 && len <= kLdsSlice;
    if (in_lds) {
        for (uint32_t i = threadIdx.x; i < len; i += kThreads) s_key[i] = t.key[s0 + i];
        __syncthreads();
    }
    bool changed = false;
    if (live) {
        const uint64_t w = read_tag[r];
        uint64_t o = w;
        if (w != kUntagged) {
            const uint32_t ps = tag_ps(w);
            uint32_t row;
            if (in_lds) {
                const uint32_t i = lower_bound_u32(s_key, len, ps);
                row = (i < len && s_key[i] == ps) ? s0 + i : t.n;
            } else if (k_first == k_last) row = len ? find_row(t, k_first, ps) : t.n;
            else row = find_row(t, contig_of(read_off, t.K, r), ps);
            if (row < t.n) o = remap(w, t.val[row]);
        }
        changed = o != w;
        out_tag[r] = o;
    }
    const unsigned long long m = __ballot(changed);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(hdr + kHdrChanged, (uint32_t)__popcll(m));
}

struct DiffArgs {
    uint32_t C, K;
    const uint8_t *pred0, *pred1;
    const uint32_t *ps0, *ps1;
    const uint32_t *ctg_off;        // [K + 1], or null ...
    const uint16_t *cand_contig;    // ... then [C]
    Table t;
    uint8_t *change;
    uint32_t *hdr;
};

__global__ __launch_bounds__(kThreads) void pj_diff(const DiffArgs a)
{
    const uint64_t c64 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const bool live = c64 < a.C;
    const uint32_t c = (uint32_t)c64;
    uint32_t code = 8;                                           // (no lane of the table's eight)
    if (live) {
        const uint32_t p0 = a.pred0[c], p1 = a.pred1[c], s0 = a.ps0[c], s1 = a.ps1[c];
        if (p0 > 3u || p1 > 3u) {
            a.hdr[kBadPred] = 1u;
            code = DUET_PS_JOIN_OTHER;
        } else if (p0 == 0 && p1 == 0) code = DUET_PS_JOIN_NONE;
        else if (p0 == 0) code = DUET_PS_JOIN_GAINED;
        else if (p1 == 0) code = DUET_PS_JOIN_LOST;
        else if (p1 == p0 && s1 == s0) code = DUET_PS_JOIN_SAME;
        else {
            const uint32_t k = a.cand_contig ? a.cand_contig[c] : contig_of(a.ctg_off, a.K, c);
            uint32_t pe = p0, se = s0;                           // what the table alone makes of (p0, s0)
            if (k >= a.K) a.hdr[kBadContig] = 1u;
            else {
                const uint32_t row = find_row(a.t, k, s0);
                if (row < a.t.n) {
                    const uint64_t v = a.t.val[row];
                    se = (uint32_t)v;
                    if ((v >> 32) != 0 && (p0 == 1u || p0 == 2u)) pe = 3u - p0;
                }
            }
            if (p1 == pe && s1 == se) code = DUET_PS_JOIN_RELABELLED;
            else if (p0 == 3u && (p1 == 1u || p1 == 2u)) code = DUET_PS_JOIN_TO_HET;
            else if ((p0 == 1u || p0 == 2u) && p1 == 3u) code = DUET_PS_JOIN_TO_HOM;
            else code = DUET_PS_JOIN_OTHER;
        }
        a.change[c] = (uint8_t)code;
    }
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) {
        const unsigned long long m = __ballot(code == i);
        if ((threadIdx.x & 63u) == 0 && m) atomicAdd(a.hdr + kHdrCounts + i, (uint32_t)__popcll(m));
    }
}

// off[0 .. K] ascends from 0 to n
bool ascends(const uint32_t *off, uint32_t K, uint32_t n)
{
    bool ok = off[0] == 0 && off[K] == n;
    for (uint32_t k = 0; ok && k < K; ++k) ok = off[k] <= off[k + 1];
    return ok;
}

// the table's rows: strictly ascending by (contig, ps), contig < K, flip 0 or 1
int check_table(duet_ctx *ctx, const duet_ps_block *blocks, uint32_t n_blocks, uint32_t K)
{
    if (n_blocks && !blocks) return fail(ctx, DUET_ERR_INVALID, "ps join: null table");
    for (uint32_t i = 0; i < n_blocks; ++i) {
        const duet_ps_block &b = blocks[i];
        if (b.contig >= K) return fail(ctx, DUET_ERR_INVALID, "ps join: a table row's contig not below the contig count");
        if (b.flip > 1u) return fail(ctx, DUET_ERR_INVALID, "ps join: a table row's flip above 1");
        if (i && !(blocks[i - 1].contig < b.contig || (blocks[i - 1].contig == b.contig && blocks[i - 1].ps < b.ps)))
            return fail(ctx, DUET_ERR_INVALID, "ps join: the table does not strictly ascend by (contig, ps)");
    }
    return DUET_OK;
}

// header | off[K + 1] (the caller's offsets; may be null) | slice_off[K + 1] | key[n] | val[n] -> workspace 0, staged on st.
// *d_off: the device copy of `off`.  The pageable host block is copied synchronously with respect to the host (hipMemcpyAsync
// from pageable memory returns once the block has been read)
int stage_table(duet_ctx *ctx, const duet_ps_block *blocks, uint32_t n, uint32_t K, const uint32_t *off, hipStream_t st, Table &t,
                const uint32_t **d_off, uint32_t **d_hdr)
{
    Arena a;
    const size_t o_hdr = a.take(kHdrWords * 4), o_off = a.take(((size_t)K + 1) * 4), o_sl = a.take(((size_t)K + 1) * 4),
                 o_val = a.take((size_t)n * 8 + 8), o_key = a.take((size_t)n * 4 + 4);
    DevBuf &ws = ctx->psjoin_ws.b[0];
    int rc;
    if ((rc = duet_reserve(ctx, ws, a.total))) return rc;
    std::vector<unsigned char> h(a.total, 0);
    uint32_t *h_sl = (uint32_t *)(h.data() + o_sl), *h_key = (uint32_t *)(h.data() + o_key);
    uint64_t *h_val = (uint64_t *)(h.data() + o_val);
    if (off) memcpy(h.data() + o_off, off, ((size_t)K + 1) * 4);
    for (uint32_t i = 0; i < n; ++i) {
        ++h_sl[blocks[i].contig + 1];
        h_key[i] = blocks[i].ps;
        h_val[i] = ((uint64_t)blocks[i].flip << 32) | blocks[i].block;
    }
    for (uint32_t k = 0; k < K; ++k) h_sl[k + 1] += h_sl[k];
    HIP_TRY(ctx, hipMemcpyAsync(ws.ptr, h.data(), a.total, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                      // (h leaves scope with this function)
    char *w = (char *)ws.ptr;
    t.K = K; t.n = n;
    t.slice_off = (const uint32_t *)(w + o_sl);
    t.key = (const uint32_t *)(w + o_key);
    t.val = (const uint64_t *)(w + o_val);
    *d_off = (const uint32_t *)(w + o_off);
    *d_hdr = (uint32_t *)(w + o_hdr);
    return DUET_OK;
}

int tags_check(duet_ctx *ctx, const uint64_t *read_tag, const uint32_t *read_off, uint32_t K, uint32_t R, const duet_ps_block *blocks,
               uint32_t n_blocks, const uint64_t *out_tag, uint32_t *n_changed)
{
    if (n_changed) *n_changed = 0;
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    if (!n_changed || !read_off || (R && (!read_tag || !out_tag))) return fail(ctx, DUET_ERR_INVALID, "null argument");
    if (K == 0 && (R || n_blocks)) return fail(ctx, DUET_ERR_INVALID, "ps join: no contig (n_contigs is 0)");
    if (!ascends(read_off, K, R)) return fail(ctx, DUET_ERR_INVALID, "ps join: read_off does not ascend from 0 to n_reads");
    return check_table(ctx, blocks, n_blocks, K);
}

// read_tag, out_tag: device memory (may be one array); the arguments are checked
int tags_run(duet_ctx *ctx, const uint64_t *read_tag, const uint32_t *read_off, uint32_t K, uint32_t R, const duet_ps_block *blocks,
             uint32_t n_blocks, uint64_t *out_tag, uint32_t *n_changed, hipStream_t st)
{
    if (R == 0) return DUET_OK;
    if (n_blocks == 0) {
        if (out_tag != read_tag) HIP_TRY(ctx, hipMemcpyAsync(out_tag, read_tag, (size_t)R * 8, hipMemcpyDeviceToDevice, st));
        return DUET_OK;
    }
    Table t;
    const uint32_t *d_off = nullptr;
    uint32_t *d_hdr = nullptr;
    int rc;
    if ((rc = stage_table(ctx, blocks, n_blocks, K, read_off, st, t, &d_off, &d_hdr))) return rc;
    hipLaunchKernelGGL(pj_tags, dim3((R + kThreads - 1) / kThreads), dim3(kThreads), 0, st, read_tag, out_tag, R, d_off, t, d_hdr);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(n_changed, d_hdr + kHdrChanged, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                      // the one round trip: the count
    return DUET_OK;
}

int diff_check(duet_ctx *ctx, uint32_t C, const uint8_t *pred0, const uint32_t *ps0, const uint8_t *pred1, const uint32_t *ps1,
               const uint32_t *cand_ctg_off, const uint16_t *cand_contig, uint32_t K, const duet_ps_block *blocks, uint32_t n_blocks,
               const uint8_t *change, uint32_t *counts)
{
    if (counts) memset(counts, 0, 8 * 4);
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    if (!counts) return fail(ctx, DUET_ERR_INVALID, "null argument");
    if ((cand_ctg_off != nullptr) == (cand_contig != nullptr))
        return fail(ctx, DUET_ERR_INVALID, "ps join: exactly one of cand_ctg_off and cand_contig names the candidates' contigs");
    if (C && (!pred0 || !ps0 || !pred1 || !ps1 || !change)) return fail(ctx, DUET_ERR_INVALID, "null array");
    if (K == 0 && (C || n_blocks)) return fail(ctx, DUET_ERR_INVALID, "ps join: no contig (n_contigs is 0)");
    if (cand_ctg_off && !ascends(cand_ctg_off, K, C))
        return fail(ctx, DUET_ERR_INVALID, "ps join: cand_ctg_off does not ascend from 0 to n_cands");
    return check_table(ctx, blocks, n_blocks, K);
}

// the arrays: device memory; change: device memory, or with change_on_host host memory.  The codes wait in the workspace until the
// refusals have been read: a refused call writes nothing
int diff_run(duet_ctx *ctx, uint32_t C, const uint8_t *pred0, const uint32_t *ps0, const uint8_t *pred1, const uint32_t *ps1,
             const uint32_t *cand_ctg_off, const uint16_t *cand_contig, uint32_t K, const duet_ps_block *blocks, uint32_t n_blocks,
             uint8_t *change, uint32_t *counts, hipStream_t st, bool change_on_host)
{
    if (C == 0) return DUET_OK;
    DiffArgs a;
    memset(&a, 0, sizeof(a));
    const uint32_t *d_off = nullptr;
    uint32_t *d_hdr = nullptr;
    int rc;
    if ((rc = stage_table(ctx, blocks, n_blocks, K, cand_ctg_off, st, a.t, &d_off, &d_hdr))) return rc;
    DevBuf &cb = ctx->psjoin_ws.b[1];
    if ((rc = duet_reserve(ctx, cb, (size_t)C))) return rc;
    a.C = C; a.K = K; a.pred0 = pred0; a.pred1 = pred1; a.ps0 = ps0; a.ps1 = ps1;
    a.ctg_off = cand_ctg_off ? d_off : nullptr;
    a.cand_contig = cand_contig;
    a.change = (uint8_t *)cb.ptr;
    a.hdr = d_hdr;
    hipLaunchKernelGGL(pj_diff, dim3((C + kThreads - 1) / kThreads), dim3(kThreads), 0, st, a);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t hdr[kHdrWords];
    HIP_TRY(ctx, hipMemcpyAsync(hdr, d_hdr, sizeof(hdr), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                      // the one round trip: the counts and the refusals
    if (hdr[kBadPred]) return fail(ctx, DUET_ERR_INVALID, "ps join: pred above 3");
    if (hdr[kBadContig]) return fail(ctx, DUET_ERR_INVALID, "ps join: cand_contig not below the contig count");
    memcpy(counts, hdr + kHdrCounts, 8 * 4);
    HIP_TRY(ctx, hipMemcpyAsync(change, cb.ptr, (size_t)C, change_on_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    if (change_on_host) HIP_TRY(ctx, hipStreamSynchronize(st));
    return DUET_OK;
}

}  // namespace

int duet_ps_join_tags_staged(duet_ctx *ctx, const uint64_t *read_tag, const uint32_t *d_read_off, uint32_t K, uint32_t R,
                             const uint32_t *d_slice_off, const uint32_t *d_key, const uint64_t *d_val, uint32_t n_bound, uint64_t *out_tag,
                             uint32_t *d_hdr, hipStream_t st)
{
    Table t;
    t.K = K; t.n = n_bound;
    t.slice_off = d_slice_off; t.key = d_key; t.val = d_val;
    hipLaunchKernelGGL(pj_tags, dim3((R + kThreads - 1) / kThreads), dim3(kThreads), 0, st, read_tag, out_tag, R, d_read_off, t, d_hdr);
    HIP_TRY(ctx, hipGetLastError());
    return DUET_OK;
}

extern "C" {

int duet_ps_join_tags_device(duet_ctx *ctx, const uint64_t *read_tag, const uint32_t *read_off, uint32_t n_contigs, uint32_t n_reads,
                             const duet_ps_block *blocks, uint32_t n_blocks, uint64_t *out_tag, uint32_t *n_changed, void *stream_)
{
    int rc = tags_check(ctx, read_tag, read_off, n_contigs, n_reads, blocks, n_blocks, out_tag, n_changed);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return tags_run(ctx, read_tag, read_off, n_contigs, n_reads, blocks, n_blocks, out_tag, n_changed, (hipStream_t)stream_);
}

int duet_ps_join_tags_host(duet_ctx *ctx, const uint64_t *read_tag, const uint32_t *read_off, uint32_t n_contigs, uint32_t n_reads,
                           const duet_ps_block *blocks, uint32_t n_blocks, uint64_t *out_tag, uint32_t *n_changed)
{
    int rc = tags_check(ctx, read_tag, read_off, n_contigs, n_reads, blocks, n_blocks, out_tag, n_changed);
    if (rc) return rc;
    if (n_reads == 0) return DUET_OK;
    if (n_blocks == 0) {
        if (out_tag != read_tag) memmove(out_tag, read_tag, (size_t)n_reads * 8);
        return DUET_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->own_stream;
    // staging 2: the read tags, remapped in place
    const void *src[1] = {read_tag};
    const size_t bytes[1] = {(size_t)n_reads * 8};
    void *dev[1];
    if ((rc = duet_stage_arrays(ctx, ctx->psjoin_ws.b + 2, src, bytes, 1, s, dev))) return rc;
    if ((rc = tags_run(ctx, (const uint64_t *)dev[0], read_off, n_contigs, n_reads, blocks, n_blocks, (uint64_t *)dev[0], n_changed, s)))
        return rc;
    HIP_TRY(ctx, hipMemcpy(out_tag, dev[0], (size_t)n_reads * 8, hipMemcpyDeviceToHost));
    return DUET_OK;
}

int duet_ps_join_diff_device(duet_ctx *ctx, uint32_t n_cands, const uint8_t *pred0, const uint32_t *ps0, const uint8_t *pred1,
                             const uint32_t *ps1, const uint32_t *cand_ctg_off, const uint16_t *cand_contig, uint32_t n_contigs,
                             const duet_ps_block *blocks, uint32_t n_blocks, uint8_t *change, uint32_t *counts, void *stream_)
{
    int rc = diff_check(ctx, n_cands, pred0, ps0, pred1, ps1, cand_ctg_off, cand_contig, n_contigs, blocks, n_blocks, change, counts);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return diff_run(ctx, n_cands, pred0, ps0, pred1, ps1, cand_ctg_off, cand_contig, n_contigs, blocks, n_blocks, change, counts,
                    (hipStream_t)stream_, false);
}

int duet_ps_join_diff_host(duet_ctx *ctx, uint32_t n_cands, const uint8_t *pred0, const uint32_t *ps0, const uint8_t *pred1,
                           const uint32_t *ps1, const uint32_t *cand_ctg_off, const uint16_t *cand_contig, uint32_t n_contigs,
                           const duet_ps_block *blocks, uint32_t n_blocks, uint8_t *change, uint32_t *counts)
{
    int rc = diff_check(ctx, n_cands, pred0, ps0, pred1, ps1, cand_ctg_off, cand_contig, n_contigs, blocks, n_blocks, change, counts);
    if (rc) return rc;
    const size_t C = n_cands;
    if (C == 0) return DUET_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->own_stream;
    // staging 3-7: pred0, ps0, pred1, ps1, cand_contig
    const void *src[5] = {pred0, ps0, pred1, ps1, cand_contig};
    const size_t bytes[5] = {C, C * 4, C, C * 4, cand_contig ? C * 2 : 0};
    void *dev[5];
    if ((rc = duet_stage_arrays(ctx, ctx->psjoin_ws.b + 3, src, bytes, 5, s, dev))) return rc;
    return diff_run(ctx, n_cands, (const uint8_t *)dev[0], (const uint32_t *)dev[1], (const uint8_t *)dev[2], (const uint32_t *)dev[3],
                    cand_ctg_off, cand_contig ? (const uint16_t *)dev[4] : nullptr, n_contigs, blocks, n_blocks, change, counts, s, true);
}

}  // extern "C"
