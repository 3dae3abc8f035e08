// duet_evidence.hip -- gfx950 kernels and C ABI of the evidence table (include/duet_ef.h, "Evidence table"):
// per candidate the exit of predict_hp's tree it takes under one vector, and one text row per candidate with its evidence, the
// rule that decided it and the call.  The tree is the sweep's: derive (duet_tune_derive.hip.h) and leaf_of
// (duet_tune_sweep.hip.h), whose verdict duet_tune_sweep_device writes and whose exits duet_tune_leaf_census_* counts.
//
//   ev_leaves           one lane per candidate: filtered / no_seed / leaf_of under the vector (a kernel argument), and the pred
//
// The rows (one stream):
//   ev_len              one lane per candidate: the codes checked (status word) and the row's length
//   64-bit scan         rows_scan_reduce (tile sums) -> scan_spine_u64 (one workgroup) -> rows_scan_apply: row offsets, the total
//   (one host round trip: the total and the status word)
//   ev_write            one wavefront per row: lane i formats column i of the fourteen behind SVTYPE into LDS at the place a wave
//                       scan of the columns' lengths gives it, one more lane formats POS; then the lanes copy CHROM, the POS
//                       piece, SVTYPE and the rest (consecutive lanes on consecutive bytes)
#include "duet_internal.h"

#include <cmath>
#include <cstring>

namespace {

int fail(duet_ctx *ctx, int code, const char *msg) { return duet_fail(ctx, code, msg); }

#include "duet_tune_sweep.hip.h"           // derive, leaf_of
#include "duet_text.hip.h"

constexpr uint32_t kLeaves = DUET_TUNE_N_LEAVES;
constexpr uint32_t kNoSeed = DUET_TUNE_LEAF_NO_SEED, kFiltered = DUET_TUNE_LEAF_FILTERED;

__global__ __launch_bounds__(256) void ev_leaves(const duet_tune_feature *feat, uint32_t C, const duet_tune_thresholds t,
                                                 uint8_t *out_leaf, uint8_t *out_pred)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= C) return;
    const duet_tune_feature f = feat[c];
    uint32_t leaf = kFiltered, pred = 0;
    if (f.kept && !f.eligible) leaf = kNoSeed;
    else if (f.eligible) leaf = leaf_of(derive(f), t, &pred);       // (eligible: what the sweep and the census test)
    out_leaf[c] = (uint8_t)leaf;
    out_pred[c] = (uint8_t)pred;
}

// ---- the rows ----------------------------------------------------------------------------------------------------------------

constexpr uint32_t kEvThreads = 256, kEvItems = 8, kEvTile = kEvThreads * kEvItems;
constexpr uint32_t kEvCols = 14;                // the columns behind SVTYPE: SVLEN .. HP
constexpr uint32_t kEvTail = 192;               // their bytes at most, separators included: 14 + 1 + 4 * 10 + 16 + 3 + 4 * 10 + 2 * 20 + 10 + 3 = 167
// status word
constexpr uint32_t kBadLeaf = 1u, kBadPred = 2u, kBadType = 4u, kBadContig = 8u, kBadStr = 16u, kLongRow = 32u, kOverrun = 64u;

struct EvParams {
    uint32_t N, K;
    const duet_tune_feature *feat;
    const uint8_t *leaf, *pred;
    const uint32_t *cand_pos, *cand_svlen;
    const char *pool;                           // text form, else null
    uint64_t pool_bytes;
    const uint32_t *str_off;
    const uint16_t *cand_contig;                // table form
    const uint8_t *cand_type;
    const char *chrom_pool;
    const uint32_t *chrom_off;                  // [K + 1]
    uint32_t *len;                              // [N] row lengths
    uint64_t *row_off;                          // [N]
    uint64_t *part;                             // [tiles]
    uint64_t *total;                            // [1]
    uint32_t *flag;                             // [1] status word
    char *out;
    uint64_t cap;
};

// RULE by code: the 18 leaves, then no_seed, then filtered
struct EvNames {
    char text[kLeaves + 2][20];
    uint8_t len[kLeaves + 2];
};
__device__ __constant__ const EvNames kEvNames = {
    {"c0_call", "c0_drop", "c2_low_ratio", "c2_near_call", "c2_near_few", "c2_far_call", "c2_far_few", "c1_one_low", "c1_one_het",
     "c1_one_het_gated", "c1_one_hom", "c1_one_hom_gated", "c1_two_low", "c1_two_het_ref", "c1_two_het", "c1_two_mid_hom",
     "c1_two_mid_het", "c1_two_hom", "no_seed", "filtered"},
    {7, 7, 12, 12, 11, 11, 10, 10, 10, 16, 10, 16, 10, 14, 10, 14, 14, 10, 7, 8}};
__device__ __constant__ const char kEvTypes[4][4] = {"DEL", "INS", "INV", "DUP"};
__device__ __constant__ const char kEvHp[4][4] = {".", "1|0", "0|1", "1|1"};

// the row's two text pieces: where they are and how long
struct EvText {
    const char *chrom, *type;
    uint32_t n_chrom, n_type, bad;
};

__device__ __forceinline__ EvText ev_text(const EvParams &p, uint32_t c)
{
    EvText t;
    t.chrom = t.type = nullptr;
    t.n_chrom = t.n_type = t.bad = 0;
    if (p.pool) {
        const uint32_t *o = p.str_off + 4 * (size_t)c;
        const uint32_t o0 = o[0], o1 = o[1], o3 = o[3], o4 = o[4];
        if (o0 > o1 || o1 > o3 || o3 > o4 || o4 > p.pool_bytes) {
            t.bad = kBadStr;
            return t;
        }
        t.chrom = p.pool + o0; t.n_chrom = o1 - o0;
        t.type = p.pool + o3; t.n_type = o4 - o3;
    } else {
        const uint32_t k = p.cand_contig[c], ty = p.cand_type[c];
        if (ty > 3u) t.bad |= kBadType;
        if (k >= p.K) t.bad |= kBadContig;
        if (t.bad) return t;
        const uint32_t c0 = p.chrom_off[k];
        t.chrom = p.chrom_pool + c0; t.n_chrom = p.chrom_off[k + 1] - c0;
        t.type = kEvTypes[ty]; t.n_type = 3;
    }
    return t;
}

// the index into kEvNames, or kLeaves + 2 for a code that is none
__device__ __forceinline__ uint32_t ev_rule(uint32_t leaf)
{
    return leaf < kLeaves ? leaf : (leaf == kNoSeed ? kLeaves : (leaf == kFiltered ? kLeaves + 1u : kLeaves + 2u));
}

// Column i (0 SVLEN .. 13 HP) of a row: a decimal number (s null) or n bytes of text at s
struct EvCol {
    uint64_t v;
    const char *s;
    uint32_t n;
};

__device__ __forceinline__ EvCol ev_col(const duet_tune_feature &f, uint32_t svlen, uint32_t rule, uint32_t pred, uint32_t i)
{
    EvCol col;
    col.s = nullptr;
    col.v = 0;
    bool shown = true;
    switch (i) {
    case 0: col.v = svlen; break;
    case 1: col.v = f.svread; break;
    case 2: col.v = f.refread; break;
    case 3: col.v = f.deg; break;
    case 4: col.s = kEvNames.text[rule]; col.n = kEvNames.len[rule]; return col;
    case 5: col.v = f.cls; shown = f.kept != 0; break;
    case 6: col.v = f.hap1; shown = f.eligible != 0; break;
    case 7: col.v = f.hap2; shown = f.eligible != 0; break;
    case 8: col.v = f.hap0; shown = f.eligible != 0; break;
    case 9: col.v = f.allhap; shown = f.eligible != 0; break;
    case 10: col.v = f.t1; shown = f.eligible != 0; break;
    case 11: col.v = f.t2; shown = f.eligible != 0; break;
    case 12: col.v = f.ps; shown = f.eligible != 0; break;
    default: col.s = kEvHp[pred & 3u]; col.n = pred ? 3u : 1u; return col;
    }
    if (!shown) {
        col.s = kEvHp[0];
        col.n = 1;
        return col;
    }
    col.n = (i == 10u || i == 11u) ? digits_u64(col.v) : digits_u32((uint32_t)col.v);
    return col;
}

__global__ __launch_bounds__(256) void ev_len(const EvParams p)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= p.N) return;
    const uint32_t rule = ev_rule(p.leaf[c]), pred = p.pred[c];
    const EvText t = ev_text(p, c);
    const uint32_t bad = t.bad | (rule >= kLeaves + 2u ? kBadLeaf : 0u) | (pred > 3u ? kBadPred : 0u);
    if (bad) {
        atomicOr(p.flag, bad);
        p.len[c] = 0;
        return;
    }
    const duet_tune_feature f = p.feat[c];
    //   CHROM \t POS \t SVTYPE, then per column a tab in front, \n behind the last
    uint64_t n = (uint64_t)t.n_chrom + 1 + digits_u32(p.cand_pos[c]) + 1 + t.n_type + kEvCols + 1;
    const uint32_t svlen = p.cand_svlen[c];
#pragma unroll
    for (uint32_t i = 0; i < kEvCols; ++i) n += ev_col(f, svlen, rule, pred, i).n;
    if (n > 0xFFFFFFFFull) {
        atomicOr(p.flag, kLongRow);
        n = 0;
    }
    p.len[c] = (uint32_t)n;
}

__global__ __launch_bounds__(256) void ev_write(const EvParams p)
{
    __shared__ char s_a[4][16], s_b[4][kEvTail];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t c = blockIdx.x * 4 + wave; c < p.N; c += gridDim.x * 4) {
        const uint32_t rowlen = p.len[c];
        uint64_t cur = p.row_off[c];
        if (rowlen == 0 || cur + rowlen > p.cap) {                 // (the host checked the status word and the total: not reached)
            if (lane == 0) atomicOr(p.flag, kOverrun);
            continue;
        }
        const EvText t = ev_text(p, c);
        const uint32_t rule = ev_rule(p.leaf[c]), pred = p.pred[c];
        // lane i < 14: column i with its tab in front (the last one with \n behind); lane 14: \t POS \t
        uint32_t n = 0;
        EvCol col;
        col.s = nullptr; col.v = 0; col.n = 0;
        if (lane < kEvCols) {
            col = ev_col(p.feat[c], p.cand_svlen[c], rule, pred, lane);
            n = col.n + 1u + (lane == kEvCols - 1u ? 1u : 0u);
        }
        const uint32_t x = wave_scan(n, lane);
        const uint32_t lb = __shfl(x, 63, 64);
        uint32_t la = 0;
        if (lane < kEvCols) {
            char *d = s_b[wave] + (x - n);
            *d++ = '\t';
            if (col.s) for (uint32_t i = 0; i < col.n; ++i) d[i] = col.s[i];
            else put_u64(d, col.v);
            if (lane == kEvCols - 1u) d[col.n] = '\n';
        } else if (lane == kEvCols) {
            char *a = s_a[wave];
            a[la++] = '\t';
            la += put_u32(a + la, p.cand_pos[c]);
            a[la++] = '\t';
        }
        la = __shfl(la, (int)kEvCols, 64);
        wave_publish();
        char *out = p.out;
        wave_copy(out + cur, t.chrom, t.n_chrom, lane);                                          // CHROM
        cur += t.n_chrom;
        wave_copy(out + cur, s_a[wave], la, lane);                                               // \t POS \t
        cur += la;
        wave_copy(out + cur, t.type, t.n_type, lane);                                            // SVTYPE
        cur += t.n_type;
        wave_copy(out + cur, s_b[wave], lb, lane);                                               // \t SVLEN ... \t HP \n
        __builtin_amdgcn_wave_barrier();                                                         // before the LDS pieces are rewritten
    }
}

// what one call reads: device pointers, except the CHROM texts (HOST)
struct EvInputs {
    uint32_t N, K;
    const duet_tune_feature *feat;
    const uint8_t *leaf, *pred;
    const uint32_t *cand_pos, *cand_svlen;
    const char *pool;
    uint64_t pool_bytes;
    const uint32_t *str_off;
    const uint16_t *cand_contig;
    const uint8_t *cand_type;
    const char *const *chrom;
};

int ev_check(duet_ctx *ctx, const duet_evidence_problem *pr, const char *out_text, uint64_t *out_len)
{
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    if (!pr || !out_len) return fail(ctx, DUET_ERR_INVALID, "null argument");
    *out_len = 0;
    if (pr->n_cands == 0) return DUET_OK;
    if (!pr->feat || !pr->leaf || !pr->pred || !pr->cand_pos || !pr->cand_svlen || !out_text)
        return fail(ctx, DUET_ERR_INVALID, "null array");
    if (pr->pool) {
        if (!pr->str_off) return fail(ctx, DUET_ERR_INVALID, "null string offsets");
        return DUET_OK;
    }
    if (!pr->cand_contig || !pr->cand_type) return fail(ctx, DUET_ERR_INVALID, "null array (no text pool: cand_contig and cand_type are needed)");
    if (pr->n_contigs == 0 || pr->n_contigs > 65535) return fail(ctx, DUET_ERR_INVALID, "bad contig count (1 to 65535)");
    if (!pr->chrom) return fail(ctx, DUET_ERR_INVALID, "null CHROM text array");
    uint64_t bytes = 0;
    for (uint32_t k = 0; k < pr->n_contigs; ++k) {
        if (!pr->chrom[k]) return fail(ctx, DUET_ERR_INVALID, "null CHROM text");
        bytes += strlen(pr->chrom[k]);
    }
    if (bytes > 0xFFFFFFFFull) return fail(ctx, DUET_ERR_INVALID, "CHROM texts of 4 GiB or more");
    return DUET_OK;
}

// the length kernel, the scan and the round trip; *need = the text's size
int ev_plan(duet_ctx *ctx, const EvInputs &in, EvParams &p, hipStream_t st, uint64_t *need)
{
    const uint32_t N = in.N, K = in.pool ? 0u : in.K;
    DuetChromTable ct;
    if (!in.pool) ct = duet_chrom_table(in.chrom, K, false);
    const uint32_t nb = (N + kEvTile - 1) / kEvTile;
    // `small`: total and status word | chrom_off[K + 1] | the CHROM texts
    const size_t small = 64 + ((size_t)K + 1) * 4 + ct.pool.size() + 64;
    const size_t sizes[4] = {(size_t)N * 4, (size_t)N * 8, (size_t)nb * 8 + 64, small};
    DevBuf *ws = ctx->evidence_ws.b;
    int rc;
    for (int i = 0; i < 4; ++i)
        if ((rc = duet_reserve(ctx, ws[i], sizes[i]))) return rc;
    char *sm = (char *)ws[3].ptr;
    uint32_t *d_chrom_off = (uint32_t *)(sm + 64);
    char *d_chrom = (char *)(d_chrom_off + (K + 1));
    HIP_TRY(ctx, hipMemsetAsync(sm, 0, 64, st));
    if (!in.pool) {
        HIP_TRY(ctx, hipMemcpyAsync(d_chrom_off, ct.off.data(), ((size_t)K + 1) * 4, hipMemcpyHostToDevice, st));
        if (!ct.pool.empty()) HIP_TRY(ctx, hipMemcpyAsync(d_chrom, ct.pool.data(), ct.pool.size(), hipMemcpyHostToDevice, st));
    }
    memset(&p, 0, sizeof(p));
    p.N = N; p.K = K;
    p.feat = in.feat; p.leaf = in.leaf; p.pred = in.pred; p.cand_pos = in.cand_pos; p.cand_svlen = in.cand_svlen;
    p.pool = in.pool; p.pool_bytes = in.pool_bytes; p.str_off = in.str_off;
    p.cand_contig = in.cand_contig; p.cand_type = in.cand_type; p.chrom_pool = d_chrom; p.chrom_off = d_chrom_off;
    p.len = (uint32_t *)ws[0].ptr;
    p.row_off = (uint64_t *)ws[1].ptr;
    p.part = (uint64_t *)ws[2].ptr;
    p.total = (uint64_t *)sm;
    p.flag = (uint32_t *)(sm + 8);
    hipLaunchKernelGGL(ev_len, dim3((N + 255) / 256), dim3(256), 0, st, p);
    hipLaunchKernelGGL((rows_scan_reduce<kEvThreads, kEvItems>), dim3(nb), dim3(kEvThreads), 0, st, (const uint32_t *)p.len, N, p.part);
    hipLaunchKernelGGL(scan_spine_u64, dim3(1), dim3(1024), 0, st, p.part, nb, p.total);
    hipLaunchKernelGGL((rows_scan_apply<kEvThreads, kEvItems>), dim3(nb), dim3(kEvThreads), 0, st, (const uint32_t *)p.len, N,
                       (const uint64_t *)p.part, p.row_off);
    HIP_TRY(ctx, hipGetLastError());
    uint64_t fin[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(fin, sm, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    // (before the first failure: a caller that sizes its buffer from *out_len never sees a partial sum)
    const uint32_t flag = (uint32_t)fin[1];
    if (flag & kBadLeaf) return fail(ctx, DUET_ERR_INVALID, "leaf code other than 0-17, DUET_TUNE_LEAF_NO_SEED, DUET_TUNE_LEAF_FILTERED");
    if (flag & kBadPred) return fail(ctx, DUET_ERR_INVALID, "pred above 3");
    if (flag & kBadType) return fail(ctx, DUET_ERR_INVALID, "candidate type code other than 0-3 (DEL, INS, INV, DUP)");
    if (flag & kBadContig) return fail(ctx, DUET_ERR_INVALID, "cand_contig not below n_contigs");
    if (flag & kBadStr) return fail(ctx, DUET_ERR_INVALID, "string offsets that descend or leave the text pool");
    if (flag & kLongRow) return fail(ctx, DUET_ERR_INVALID, "a row of 4 GiB or more");
    *need = fin[0];
    return DUET_OK;
}

int ev_write_rows(duet_ctx *ctx, EvParams &p, char *out, uint64_t cap, hipStream_t st)
{
    p.out = out;
    p.cap = cap;
    const uint32_t wb = (p.N + 3) / 4;
    hipLaunchKernelGGL(ev_write, dim3(wb < 8192u ? wb : 8192u), dim3(256), 0, st, p);
    HIP_TRY(ctx, hipGetLastError());
    return DUET_OK;
}

const char kTooSmall[] = "output buffer too small for the evidence rows (*out_len = size needed)";

}  // namespace

extern "C" {

int duet_tune_leaves_device(duet_ctx *ctx, const duet_tune_feature *feat, uint32_t n_cands, const duet_tune_thresholds *vec,
                            uint8_t *out_leaf, uint8_t *out_pred, void *stream_)
{
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    if (n_cands == 0) return DUET_OK;
    if (!feat) return fail(ctx, DUET_ERR_INVALID, "null feature array");
    if (!vec) return fail(ctx, DUET_ERR_INVALID, "null threshold vector");
    if (!out_leaf || !out_pred) return fail(ctx, DUET_ERR_INVALID, "null output array");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(ev_leaves, dim3((n_cands + 255) / 256), dim3(256), 0, (hipStream_t)stream_, feat, n_cands, *vec, out_leaf, out_pred);
    HIP_TRY(ctx, hipGetLastError());
    return DUET_OK;
}

int duet_tune_leaves_host(duet_ctx *ctx, const duet_tune_feature *feat, uint32_t n_cands, const duet_tune_thresholds *vec,
                          uint8_t *out_leaf, uint8_t *out_pred)
{
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    if (n_cands == 0) return DUET_OK;
    if (!feat) return fail(ctx, DUET_ERR_INVALID, "null feature array");
    if (!vec) return fail(ctx, DUET_ERR_INVALID, "null threshold vector");
    if (!out_leaf || !out_pred) return fail(ctx, DUET_ERR_INVALID, "null output array");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->own_stream;
    const size_t C = n_cands;
    DevBuf *B = ctx->evidence_ws.b + 4;                           // staging: the features, the leaves, the preds
    const void *src[1] = {feat};
    const size_t bytes[1] = {C * sizeof(duet_tune_feature)};
    void *dev[1];
    int rc;
    if ((rc = duet_stage_arrays(ctx, B, src, bytes, 1, s, dev)) || (rc = duet_reserve(ctx, B[1], C + 64)) ||
        (rc = duet_reserve(ctx, B[2], C + 64)))
        return rc;
    if ((rc = duet_tune_leaves_device(ctx, (const duet_tune_feature *)dev[0], n_cands, vec, (uint8_t *)B[1].ptr, (uint8_t *)B[2].ptr, s)))
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out_leaf, B[1].ptr, C, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(out_pred, B[2].ptr, C, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return DUET_OK;
}

int duet_evidence_rows_device(duet_ctx *ctx, const duet_evidence_problem *pr, char *out_text, uint64_t out_cap, uint64_t *out_len,
                              void *stream_)
{
    int rc;
    if ((rc = ev_check(ctx, pr, out_text, out_len))) return rc;
    if (pr->n_cands == 0) return DUET_OK;
    hipStream_t st = (hipStream_t)stream_;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const EvInputs in = {pr->n_cands, pr->n_contigs, pr->feat, pr->leaf, pr->pred, pr->cand_pos, pr->cand_svlen, pr->pool,
                         pr->pool_bytes, pr->str_off, pr->cand_contig, pr->cand_type, pr->chrom};
    EvParams p;
    uint64_t need = 0;
    if ((rc = ev_plan(ctx, in, p, st, &need))) return rc;
    *out_len = need;
    if (need > out_cap) return fail(ctx, DUET_ERR_INVALID, kTooSmall);
    return ev_write_rows(ctx, p, out_text, out_cap, st);
}

int duet_evidence_rows_host(duet_ctx *ctx, const duet_evidence_problem *pr, char *out_text, uint64_t out_cap, uint64_t *out_len)
{
    int rc;
    if ((rc = ev_check(ctx, pr, out_text, out_len))) return rc;
    if (pr->n_cands == 0) return DUET_OK;
    const size_t C = pr->n_cands;
    const bool text = pr->pool != nullptr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->own_stream;
    // staging 4-12: features, leaf, pred, pos, svlen | pool, str_off | cand_contig, cand_type
    const void *src[9] = {pr->feat, pr->leaf, pr->pred, pr->cand_pos, pr->cand_svlen, pr->pool, pr->str_off, pr->cand_contig, pr->cand_type};
    const size_t bytes[9] = {C * sizeof(duet_tune_feature), C, C, C * 4, C * 4, text ? (size_t)pr->pool_bytes : 0,
                             text ? (4 * C + 1) * 4 : 0, text ? 0 : C * 2, text ? 0 : C};
    void *dev[9];
    if ((rc = duet_stage_arrays(ctx, ctx->evidence_ws.b + 4, src, bytes, 9, s, dev))) return rc;
    const EvInputs in = {pr->n_cands, pr->n_contigs, (const duet_tune_feature *)dev[0], (const uint8_t *)dev[1], (const uint8_t *)dev[2],
                         (const uint32_t *)dev[3], (const uint32_t *)dev[4], text ? (const char *)dev[5] : nullptr, pr->pool_bytes,
                         (const uint32_t *)dev[6], (const uint16_t *)dev[7], (const uint8_t *)dev[8], pr->chrom};
    EvParams p;
    uint64_t need = 0;
    if ((rc = ev_plan(ctx, in, p, s, &need))) return rc;
    *out_len = need;
    if (need > out_cap) return fail(ctx, DUET_ERR_INVALID, kTooSmall);
    DevBuf &ob = ctx->evidence_ws.b[13];
    if ((rc = duet_reserve(ctx, ob, need + 64))) return rc;
    if ((rc = ev_write_rows(ctx, p, (char *)ob.ptr, need, s))) return rc;
    uint32_t flag = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&flag, p.flag, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (flag & kOverrun) return fail(ctx, DUET_ERR_INVALID, "evidence rows overran their offsets");
    if (need) HIP_TRY(ctx, hipMemcpy(out_text, ob.ptr, need, hipMemcpyDeviceToHost));
    return DUET_OK;
}

}  // extern "C"
