// duet_readtags.hip -- read tags from phased SVs (include/duet_ef.h: duet_read_tags_device): which haplotype
// each supporting read of a heterozygous call lies on.  The mark CSR goes candidate -> reads; this unit transposes it to read ->
// candidates and sums each (read name, phase set) into one record.
//
//   rt_count     per candidate: its mark count when pred is 1 or 2, else 0 (no mark is read)
//   a scan over those counts: where each het candidate's marks go, and their total V -- host round trip 1
//   rt_keys      one wavefront per het candidate: per mark the pair (name << 32 | ps[c], place), the candidate beside it; a
//                candidate's marks keep their order
//   a stable radix sort over exactly 32 + bits_for(n_names - 1) bits
//   head flags on the key, scanned: the records numbered, each one's first position stored -- host round trip 2, the record count
//   checked against out_cap
//   rt_reduce    one wavefront per record strides over its members: the counts, min and max of pos, contig and read index by
//                shuffles; the status; lane 0 writes the record into the staging block.  Two contigs or two read indices under
//                one name are seen here, from the min and max (and from the first member of the name's next record)
//   host round trip 3, one status word; then the records are copied from the staging block to `out`
//   rr_len, a 64-bit scan, rr_write: one text row per record (the structure of ev_len / ev_write in duet_evidence.hip)
// Integers only and no atomic in the unit's own kernels: a refusal is a plain store of 1 to a word of its own, whoever stores it.
// (The shared sort's rx_hist accumulates its digit totals with integer atomics up to 1024 tiles: sums.)
#include "duet_internal.h"

#include <cstring>

namespace {

#include "duet_prims.hip.h"
#include "duet_seeds.hip.h"                // kEmpty, kUntagged, tag_ps, tag_pc, tag_hap
#include "duet_text.hip.h"

constexpr uint32_t kCapMax = (1u << 30) - 3u;         // the tag word saturates pc at 2^30 - 2: a saturated value is never usable
constexpr int kWaves = 4;                             // wavefronts (candidates, records) per workgroup
// header words of a call: the counts, then one word per refusal
constexpr uint32_t kHdrV = 0, kHdrRecs = 1, kBadPred = 4, kBadName = 5, kBadOrder = 6, kTwoContigs = 7, kTwoReads = 8, kHdrWords = 16;

int fail(duet_ctx *ctx, int code, const char *msg) { return duet_fail(ctx, code, msg); }

struct Prob {                       // the device's view of the problem
    uint32_t C, M, K, n_reads, n_names, pc_cap;
    const uint32_t *cand_off, *mark_order, *mark_read, *mark_name, *ps, *cand_pos, *ctg_off;
    const uint8_t *pred;
    const uint16_t *cand_contig;
    const uint64_t *read_tag;
};

// the CSR slots of candidate c, kept inside the marks whatever the offsets say
__device__ __forceinline__ void cand_range(const Prob &a, uint32_t c, uint32_t &b, uint32_t &e)
{
    e = a.cand_off[c + 1];
    e = e < a.M ? e : a.M;
    b = a.cand_off[c];
    b = b < e ? b : e;
}

__global__ __launch_bounds__(256) void rt_count(const Prob a, uint32_t *cnt, uint32_t *hdr)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= a.C) return;
    const uint32_t pr = a.pred[c];
    uint32_t n = 0;
    if (pr > 3u) hdr[kBadPred] = 1u;
    else if (pr == 1u || pr == 2u) {
        uint32_t b, e;
        cand_range(a, c, b, e);
        n = e - b;
    }
    cnt[c] = n;
}

__global__ __launch_bounds__(64 * kWaves) void rt_keys(const Prob a, const uint32_t *cnt, const uint32_t *start, uint32_t V, uint64_t *keys,
                                                        uint32_t *vals, uint32_t *cand_of, uint32_t *hdr)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t c64 = (uint64_t)blockIdx.x * kWaves + wave; c64 < a.C; c64 += (uint64_t)gridDim.x * kWaves) {
        const uint32_t c = (uint32_t)c64;
        if (cnt[c] == 0) continue;                               // (not a het call, or no mark)
        uint32_t b, e;
        cand_range(a, c, b, e);
        const uint64_t at = start[c], ps = a.ps[c];
        for (uint64_t m = (uint64_t)b + lane; m < e; m += 64) {
            const uint64_t mine = at + (m - b);
            if (mine >= V) continue;                             // (the count kernel saw the same range: the bound is for safety)
            uint32_t raw = a.mark_order ? a.mark_order[m] : (uint32_t)m, name = 0;
            if (raw >= a.M) hdr[kBadOrder] = 1u;
            else if ((name = a.mark_name[raw]) >= a.n_names) {
                hdr[kBadName] = 1u;
                name = 0;
            }
            keys[mine] = ((uint64_t)name << 32) | ps;
            vals[mine] = (uint32_t)mine;
            cand_of[mine] = c;
        }
    }
}

// the sorted (name, ps) keys: position i opens a record
struct LoadRecHead {
    const uint64_t *keys;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return (i == 0 || keys[i - 1] != keys[i]) ? 1u : 0u; }
};
struct StoreHeadAt {                // start[number] = position, for the heads
    uint32_t *start;
    __device__ __forceinline__ void operator()(uint32_t i, uint32_t before, uint32_t head) const
    {
        if (head) start[before] = i;
    }
};

struct ReduceArgs {
    Prob a;
    const uint64_t *keys;           // sorted: name << 32 | ps
    const uint32_t *perm, *cand_of, *start, *rstart;
    uint32_t n_recs, V;
    duet_read_tag_rec *out;
    uint32_t *hdr;
};

// member i of the sorted order: its candidate and its read index
__device__ __forceinline__ void member(const ReduceArgs &r, uint32_t i, uint32_t &c, uint32_t &rd)
{
    uint32_t p = r.perm[i];
    p = p < r.V ? p : r.V - 1u;
    c = r.cand_of[p];
    uint32_t b, e;
    cand_range(r.a, c, b, e);
    const uint64_t slot = (uint64_t)b + (p - r.start[c]);
    rd = kEmpty;
    if (slot < e) {
        const uint32_t raw = r.a.mark_order ? r.a.mark_order[slot] : (uint32_t)slot;
        if (raw < r.a.M) rd = r.a.mark_read[raw];
    }
}

// the candidate's contig: its column, or the first k with ctg_off[k + 1] > c (empty contigs own nothing)
__device__ __forceinline__ uint32_t contig_of(const Prob &a, uint32_t c)
{
    if (a.cand_contig) return a.cand_contig[c];
    uint32_t lo = 0, hi = a.K - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a.ctg_off[mid + 1] <= c) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// is the read's own tag usable: index present and inside the table, word not all-ones, hap 1 or 2, pc <= cap
__device__ __forceinline__ bool usable_tag(const Prob &a, uint32_t rd, uint64_t &t)
{
    if (rd == kEmpty || rd >= a.n_reads) return false;
    t = a.read_tag[rd];
    if (t == kUntagged) return false;
    const uint32_t hap = tag_hap(t);
    return (hap == 1u || hap == 2u) && tag_pc(t) <= a.pc_cap;
}

__global__ __launch_bounds__(64 * kWaves) void rt_reduce(const ReduceArgs r)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t j64 = (uint64_t)blockIdx.x * kWaves + wave; j64 < r.n_recs; j64 += (uint64_t)gridDim.x * kWaves) {
        const uint32_t j = (uint32_t)j64;
        const uint32_t s = r.rstart[j];
        uint32_t e = j + 1 < r.n_recs ? r.rstart[j + 1] : r.V;
        e = e < r.V ? e : r.V;
        if (s >= e) continue;                                    // (a record has a member: not reached)
        uint32_t n_h1 = 0, n_h2 = 0, pos_min = 0xFFFFFFFFu, pos_max = 0, k_min = 0xFFFFFFFFu, k_max = 0, rd_min = 0xFFFFFFFFu, rd_max = 0;
        for (uint64_t i = (uint64_t)s + lane; i < e; i += 64) {
            uint32_t c, rd;
            member(r, (uint32_t)i, c, rd);
            const uint32_t pr = r.a.pred[c], pos = r.a.cand_pos[c], k = contig_of(r.a, c);
            n_h1 += pr == 1u;
            n_h2 += pr == 2u;
            pos_min = pos < pos_min ? pos : pos_min;
            pos_max = pos > pos_max ? pos : pos_max;
            k_min = k < k_min ? k : k_min;
            k_max = k > k_max ? k : k_max;
            rd_min = rd < rd_min ? rd : rd_min;
            rd_max = rd > rd_max ? rd : rd_max;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            n_h1 += __shfl_xor(n_h1, o, 64);
            n_h2 += __shfl_xor(n_h2, o, 64);
            const uint32_t pn = __shfl_xor(pos_min, o, 64), px = __shfl_xor(pos_max, o, 64), kn = __shfl_xor(k_min, o, 64),
                           kx = __shfl_xor(k_max, o, 64), rn = __shfl_xor(rd_min, o, 64), rx = __shfl_xor(rd_max, o, 64);
            pos_min = pn < pos_min ? pn : pos_min;
            pos_max = px > pos_max ? px : pos_max;
            k_min = kn < k_min ? kn : k_min;
            k_max = kx > k_max ? kx : k_max;
            rd_min = rn < rd_min ? rn : rd_min;
            rd_max = rx > rd_max ? rx : rd_max;
        }
        if (lane != 0) continue;
        const uint64_t key = r.keys[s];
        const uint32_t name = (uint32_t)(key >> 32), ps = (uint32_t)key;
        bool two_k = k_min != k_max, two_rd = rd_min != rd_max;
        if (e < r.V && (uint32_t)(r.keys[e] >> 32) == name) {    // the name's next record: its first member has to agree too
            uint32_t c2, rd2;
            member(r, e, c2, rd2);
            two_k = two_k || contig_of(r.a, c2) != k_min;
            two_rd = two_rd || rd2 != rd_min;
        }
        if (two_k) r.hdr[kTwoContigs] = 1u;
        if (two_rd) r.hdr[kTwoReads] = 1u;
        const uint32_t sv = n_h1 > n_h2 ? 1u : (n_h2 > n_h1 ? 2u : 0u);
        uint64_t t = 0;
        const bool usable = usable_tag(r.a, rd_min, t);
        uint32_t status;
        if (usable && tag_ps(t) != ps) status = DUET_READ_TAG_OTHER_PS;
        else if (sv == 0) status = DUET_READ_TAG_TIE;
        else if (usable) status = tag_hap(t) == sv ? DUET_READ_TAG_AGREE : DUET_READ_TAG_DISAGREE;
        else status = DUET_READ_TAG_NEW;
        duet_read_tag_rec o;
        o.name = name; o.contig = k_min; o.ps = ps; o.read = rd_min; o.n_h1 = n_h1; o.n_h2 = n_h2;
        o.pos_min = pos_min; o.pos_max = pos_max; o.status = status; o.reserved = 0;
        r.out[j] = o;
    }
}

uint32_t wave_grid(uint32_t n)      // workgroups of kWaves wavefronts for n wavefront-sized jobs (grid-stride beyond 2^18)
{
    const uint32_t nb = (n + kWaves - 1) / kWaves;
    return nb < (1u << 18) ? (nb ? nb : 1u) : (1u << 18);
}

int check_args(duet_ctx *ctx, const duet_read_tags_problem *pr, uint32_t pc_cap, const duet_read_tag_rec *out, uint32_t out_cap,
               uint32_t *n_recs)
{
    if (n_recs) *n_recs = 0;
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    if (pc_cap > kCapMax) return fail(ctx, DUET_ERR_INVALID, "pc_cap is above 2^30 - 3 (the tag word saturates pc at 2^30 - 2)");
    if (!pr || !n_recs || (!out && out_cap)) return fail(ctx, DUET_ERR_INVALID, "null argument");
    if ((pr->cand_ctg_off != nullptr) == (pr->cand_contig != nullptr))
        return fail(ctx, DUET_ERR_INVALID, "read tags: exactly one of cand_ctg_off and cand_contig names the candidates' contigs");
    if (pr->n_cands == 0 || pr->n_marks == 0) return DUET_OK;
    if (!pr->cand_off || !pr->mark_read || !pr->mark_name || !pr->pred || !pr->ps || !pr->cand_pos || (!pr->read_tag && pr->n_reads))
        return fail(ctx, DUET_ERR_INVALID, "null array");
    if (pr->n_names == 0) return fail(ctx, DUET_ERR_INVALID, "read tags: marks without a single name (n_names is 0)");
    if (pr->cand_ctg_off) {
        const uint32_t K = pr->n_contigs;
        if (K == 0) return fail(ctx, DUET_ERR_INVALID, "read tags: no contig (n_contigs is 0)");
        bool ok = pr->cand_ctg_off[0] == 0 && pr->cand_ctg_off[K] == pr->n_cands;
        for (uint32_t k = 0; ok && k < K; ++k) ok = pr->cand_ctg_off[k] <= pr->cand_ctg_off[k + 1];
        if (!ok) return fail(ctx, DUET_ERR_INVALID, "read tags: cand_ctg_off does not ascend from 0 to n_cands");
    }
    return DUET_OK;
}

// the records of a device-resident problem, checked by the caller; out is device memory, or with out_on_host host memory
int run(duet_ctx *ctx, const duet_read_tags_problem *pr, uint32_t pc_cap, duet_read_tag_rec *out, uint32_t out_cap, uint32_t *n_recs,
        hipStream_t st, bool out_on_host)
{
    const uint32_t C = pr->n_cands, M = pr->n_marks, K = pr->cand_ctg_off ? pr->n_contigs : 0u;
    if (C == 0 || M == 0) return DUET_OK;
    int rc;
    Prob a;
    memset(&a, 0, sizeof(a));
    a.C = C; a.M = M; a.K = K; a.n_reads = pr->n_reads; a.n_names = pr->n_names; a.pc_cap = pc_cap;
    a.cand_off = pr->cand_off; a.mark_order = pr->mark_order; a.mark_read = pr->mark_read; a.mark_name = pr->mark_name;
    a.ps = pr->ps; a.cand_pos = pr->cand_pos; a.pred = pr->pred; a.cand_contig = pr->cand_contig; a.read_tag = pr->read_tag;

    // ---- the candidates: the het calls and how many marks they hold ----
    Arena a1;
    const size_t o_hdr = a1.take(kHdrWords * 4), o_ctg = a1.take(((size_t)K + 1) * 4), o_cnt = a1.take((size_t)C * 4),
                 o_start = a1.take((size_t)C * 4), o_part1 = a1.take(((size_t)(C + kScanTile - 1) / kScanTile + 1) * 4);
    DevBuf &ws1 = ctx->readtags_ws.b[0];
    if ((rc = duet_reserve(ctx, ws1, a1.total))) return rc;
    char *w1 = (char *)ws1.ptr;
    uint32_t *d_hdr = (uint32_t *)(w1 + o_hdr), *d_ctg_off = (uint32_t *)(w1 + o_ctg), *cnt = (uint32_t *)(w1 + o_cnt),
             *start = (uint32_t *)(w1 + o_start), *part1 = (uint32_t *)(w1 + o_part1);
    HIP_TRY(ctx, hipMemsetAsync(d_hdr, 0, kHdrWords * 4, st));
    if (K) {
        HIP_TRY(ctx, hipMemcpyAsync(d_ctg_off, pr->cand_ctg_off, ((size_t)K + 1) * 4, hipMemcpyHostToDevice, st));
        a.ctg_off = d_ctg_off;
    }
    hipLaunchKernelGGL(rt_count, dim3((C + 255u) / 256u), dim3(256), 0, st, a, cnt, d_hdr);
    launch_scan<0>(LoadPlain{cnt}, C, part1, StorePlain{start}, d_hdr + kHdrV, st);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t hdr[kHdrWords];
    HIP_TRY(ctx, hipMemcpyAsync(hdr, d_hdr, sizeof(hdr), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                                   // round trip 1
    if (hdr[kBadPred]) return fail(ctx, DUET_ERR_INVALID, "read tags: pred above 3");
    const uint32_t V = hdr[kHdrV];
    if (V == 0) return DUET_OK;
    if (V > M) return fail(ctx, DUET_ERR_INVALID, "read tags: more contributing marks than marks (cand_off does not ascend)");

    // ---- marks -> (name, ps) keys -> sorted -> records numbered ----
    const uint32_t nb_rx = (V + kRxTile - 1) / kRxTile, nb_sc = (V + kScanTile - 1) / kScanTile;
    const uint32_t nb_hs = (256u * nb_rx + kScanTile - 1) / kScanTile;
    Arena a2;
    const size_t o_ka = a2.take((size_t)V * 8), o_kb = a2.take((size_t)V * 8), o_va = a2.take((size_t)V * 4), o_vb = a2.take((size_t)V * 4),
                 o_co = a2.take((size_t)V * 4), o_rs = a2.take((size_t)V * 4), o_hist = a2.take((size_t)256 * nb_rx * 4),
                 o_part = a2.take(((size_t)(nb_sc > nb_hs ? nb_sc : nb_hs) + 1) * 4);
    DevBuf &ws2 = ctx->readtags_ws.b[1];
    if ((rc = duet_reserve(ctx, ws2, a2.total))) return rc;
    char *w2 = (char *)ws2.ptr;
    uint64_t *keysA = (uint64_t *)(w2 + o_ka), *keysB = (uint64_t *)(w2 + o_kb);
    uint32_t *valsA = (uint32_t *)(w2 + o_va), *valsB = (uint32_t *)(w2 + o_vb), *cand_of = (uint32_t *)(w2 + o_co),
             *rstart = (uint32_t *)(w2 + o_rs), *hist = (uint32_t *)(w2 + o_hist), *spart = (uint32_t *)(w2 + o_part);
    hipLaunchKernelGGL(rt_keys, dim3(wave_grid(C)), dim3(64 * kWaves), 0, st, a, (const uint32_t *)cnt, (const uint32_t *)start, V, keysA,
                       valsA, cand_of, d_hdr);
    uint64_t *sk = nullptr;
    uint32_t *sv = nullptr;
    radix_sort_pairs(keysA, keysB, valsA, valsB, V, 32u + bits_for((uint64_t)pr->n_names - 1u), hist, spart, ctx->rx_dtot, st, &sk, &sv,
                     nullptr);
    launch_scan<0>(LoadRecHead{sk}, V, spart, StoreHeadAt{rstart}, d_hdr + kHdrRecs, st);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(hdr, d_hdr, sizeof(hdr), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                                   // round trip 2
    if (hdr[kBadOrder]) return fail(ctx, DUET_ERR_INVALID, "read tags: mark_order not below n_marks");
    if (hdr[kBadName]) return fail(ctx, DUET_ERR_INVALID, "read tags: mark_name not below n_names");
    const uint32_t N = hdr[kHdrRecs];
    if (N == 0 || N > V) return fail(ctx, DUET_ERR_HIP, "read tags: the record count left its range");
    *n_recs = N;
    if (N > out_cap) return fail(ctx, DUET_ERR_INVALID, "read tags: the record buffer is too small (out_cap below *n_recs)");

    // ---- the records, into the staging block: a refusal found here leaves `out` as it was ----
    DevBuf &bo = ctx->readtags_ws.b[2];
    if ((rc = duet_reserve(ctx, bo, (size_t)N * sizeof(duet_read_tag_rec)))) return rc;
    ReduceArgs r;
    memset(&r, 0, sizeof(r));
    r.a = a; r.keys = sk; r.perm = sv; r.cand_of = cand_of; r.start = start; r.rstart = rstart; r.n_recs = N; r.V = V;
    r.out = (duet_read_tag_rec *)bo.ptr; r.hdr = d_hdr;
    hipLaunchKernelGGL(rt_reduce, dim3(wave_grid(N)), dim3(64 * kWaves), 0, st, r);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(hdr, d_hdr, sizeof(hdr), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                                   // round trip 3
    if (hdr[kTwoContigs] || hdr[kTwoReads]) *n_recs = 0;
    if (hdr[kTwoContigs]) return fail(ctx, DUET_ERR_INVALID, "read tags: the marks of one name lie on two contigs");
    if (hdr[kTwoReads]) return fail(ctx, DUET_ERR_INVALID, "read tags: the marks of one name carry two read indices");
    HIP_TRY(ctx, hipMemcpyAsync(out, bo.ptr, (size_t)N * sizeof(duet_read_tag_rec), out_on_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                                st));
    if (out_on_host) HIP_TRY(ctx, hipStreamSynchronize(st));
    return DUET_OK;
}

// ---- the rows ----------------------------------------------------------------------------------------------------------------------

constexpr uint32_t kRrThreads = 256, kRrItems = 8, kRrTile = kRrThreads * kRrItems;
constexpr uint32_t kRrCols = 11;                // the columns behind READ: PS .. POS_MAX
constexpr uint32_t kRrTail = 112;               // their bytes at most, separators included: 11 + 8 * 10 + 1 + 1 + 8 + 1 = 102
// status words of the rows
constexpr uint32_t kRowBadName = 2, kRowBadContig = 3, kRowBadStatus = 4, kRowBadOff = 5, kRowLong = 6, kRowOverrun = 7;

struct RrParams {
    uint32_t N, K, n_names, n_reads;
    const duet_read_tag_rec *recs;
    const uint64_t *name_off, *read_tag;
    const char *name_pool, *chrom_pool;
    const uint32_t *chrom_off;                  // [K + 1]
    uint32_t *len;                              // [N] row lengths
    uint64_t *row_off;                          // [N]
    uint64_t *part;                             // [tiles]
    uint64_t *total;                            // [1]
    uint32_t *flag;                             // the status words (indices kRow*; words 0 and 1 hold *total)
    char *out;
    uint64_t cap;
};

struct RrNames {
    char text[5][12];
    uint8_t len[5];
};
__device__ __constant__ const RrNames kRrStatus = {{"agree", "disagree", "tie", "new", "other_ps"}, {5, 8, 3, 3, 8}};
__device__ __constant__ const char kRrHap[3][2] = {".", "1", "2"};

// Column i (0 PS .. 10 POS_MAX) of a row: a decimal number (s null) or n bytes of text at s.  t: the read's own tag word, all-ones
// when it has none
struct RrCol {
    uint64_t v;
    const char *s;
    uint32_t n;
};

__device__ __forceinline__ RrCol rr_col(const duet_read_tag_rec &r, uint64_t t, uint32_t i)
{
    RrCol col;
    col.s = nullptr;
    col.v = 0;
    const bool tagged = t != kUntagged;
    switch (i) {
    case 0: col.v = r.ps; break;
    case 1: col.v = (uint64_t)r.n_h1 + r.n_h2; break;
    case 2: col.v = r.n_h1; break;
    case 3: col.v = r.n_h2; break;
    case 4: col.s = kRrHap[r.n_h1 > r.n_h2 ? 1 : (r.n_h2 > r.n_h1 ? 2 : 0)]; col.n = 1; return col;
    case 5: {
        const uint32_t hap = tagged ? tag_hap(t) : 0u;
        col.s = kRrHap[hap == 1u || hap == 2u ? hap : 0u]; col.n = 1;
        return col;
    }
    case 6: col.v = tag_ps(t); break;
    case 7: col.v = tag_pc(t); break;
    case 8: col.s = kRrStatus.text[r.status]; col.n = kRrStatus.len[r.status]; return col;
    case 9: col.v = r.pos_min; break;
    default: col.v = r.pos_max; break;
    }
    if ((i == 6u || i == 7u) && !tagged) {
        col.s = kRrHap[0];
        col.n = 1;
        return col;
    }
    col.n = digits_u64(col.v);
    return col;
}

// the read's own tag word, all-ones when the index is absent or outside the table
__device__ __forceinline__ uint64_t rr_tag(const RrParams &p, uint32_t rd)
{
    return (rd == kEmpty || rd >= p.n_reads) ? kUntagged : p.read_tag[rd];
}

__global__ __launch_bounds__(256) void rr_len(const RrParams p)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= p.N) return;
    const duet_read_tag_rec r = p.recs[j];
    uint32_t bad = 0;
    if (r.name >= p.n_names) bad = kRowBadName;
    else if (r.contig >= p.K) bad = kRowBadContig;
    else if (r.status > DUET_READ_TAG_OTHER_PS) bad = kRowBadStatus;
    uint64_t n = 0;
    if (!bad) {
        const uint64_t n0 = p.name_off[r.name], n1 = p.name_off[r.name + 1];
        if (n1 < n0) bad = kRowBadOff;
        else {
            //   CHROM \t READ, then per column a tab in front, \n behind the last
            n = (uint64_t)(p.chrom_off[r.contig + 1] - p.chrom_off[r.contig]) + 1 + (n1 - n0) + kRrCols + 1;
            const uint64_t t = rr_tag(p, r.read);
#pragma unroll
            for (uint32_t i = 0; i < kRrCols; ++i) n += rr_col(r, t, i).n;
            if (n > 0xFFFFFFFFull) bad = kRowLong;
        }
    }
    if (bad) {
        p.flag[bad] = 1u;
        n = 0;
    }
    p.len[j] = (uint32_t)n;
}

__global__ __launch_bounds__(256) void rr_write(const RrParams p)
{
    __shared__ char s_b[4][kRrTail];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t j = blockIdx.x * 4 + wave; j < p.N; j += gridDim.x * 4) {
        const uint32_t rowlen = p.len[j];
        uint64_t cur = p.row_off[j];
        if (rowlen == 0 || cur + rowlen > p.cap) {                 // (the host checked the status words and the total: not reached)
            if (lane == 0) p.flag[kRowOverrun] = 1u;
            continue;
        }
        const duet_read_tag_rec r = p.recs[j];
        const uint64_t t = rr_tag(p, r.read);
        // lane i < 11: column i with its tab in front (the last one with \n behind)
        uint32_t n = 0;
        RrCol col;
        col.s = nullptr; col.v = 0; col.n = 0;
        if (lane < kRrCols) {
            col = rr_col(r, t, lane);
            n = col.n + 1u + (lane == kRrCols - 1u ? 1u : 0u);
        }
        const uint32_t x = wave_scan(n, lane);
        const uint32_t lb = __shfl(x, 63, 64);
        if (lane < kRrCols && x <= kRrTail) {
            char *d = s_b[wave] + (x - n);
            *d++ = '\t';
            if (col.s) for (uint32_t i = 0; i < col.n; ++i) d[i] = col.s[i];
            else put_u64(d, col.v);
            if (lane == kRrCols - 1u) d[col.n] = '\n';
        }
        wave_publish();
        const uint32_t c0 = p.chrom_off[r.contig], n_chrom = p.chrom_off[r.contig + 1] - c0;
        const uint64_t n0 = p.name_off[r.name];
        const uint32_t n_name = rowlen - n_chrom - 1u - lb;          // (what rr_len counted)
        char *out = p.out;
        wave_copy(out + cur, p.chrom_pool + c0, n_chrom, lane);                                  // CHROM
        cur += n_chrom;
        if (lane == 0) out[cur] = '\t';
        cur += 1;
        wave_copy(out + cur, p.name_pool + n0, n_name, lane);                                    // READ
        cur += n_name;
        wave_copy(out + cur, s_b[wave], lb, lane);                                               // \t PS ... \t POS_MAX \n
        __builtin_amdgcn_wave_barrier();                                                         // before the LDS piece is rewritten
    }
}

int rows_check(duet_ctx *ctx, const duet_read_tag_rec *recs, uint32_t n_recs, const duet_callset_names *names, const uint64_t *read_tag,
               uint32_t n_reads, const char *out_text, uint64_t *out_len)
{
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    if (!out_len) return fail(ctx, DUET_ERR_INVALID, "null argument");
    *out_len = 0;
    if (n_recs == 0) return DUET_OK;
    if (!recs || !names || !names->name_off || !names->name_pool || !out_text || (!read_tag && n_reads))
        return fail(ctx, DUET_ERR_INVALID, "null array");
    if (names->n_contigs == 0 || names->n_contigs > 65535) return fail(ctx, DUET_ERR_INVALID, "bad contig count (1 to 65535)");
    if (!names->chrom) return fail(ctx, DUET_ERR_INVALID, "null CHROM text array");
    uint64_t bytes = 0;
    for (uint32_t k = 0; k < names->n_contigs; ++k) {
        if (!names->chrom[k]) return fail(ctx, DUET_ERR_INVALID, "null CHROM text");
        bytes += strlen(names->chrom[k]);
    }
    if (bytes > 0xFFFFFFFFull) return fail(ctx, DUET_ERR_INVALID, "CHROM texts of 4 GiB or more");
    return DUET_OK;
}

// the length kernel, the scan and the round trip; *need = the text's size.  recs, name_off, name_pool, read_tag: device memory
int rows_plan(duet_ctx *ctx, const duet_read_tag_rec *recs, uint32_t N, const duet_callset_names *names, const uint64_t *name_off,
              const char *name_pool, const uint64_t *read_tag, uint32_t n_reads, RrParams &p, hipStream_t st, uint64_t *need)
{
    const uint32_t K = names->n_contigs;
    const DuetChromTable ct = duet_chrom_table(names->chrom, K, false);
    const uint32_t nb = (N + kRrTile - 1) / kRrTile;
    // `small`: total and status words | chrom_off[K + 1] | the CHROM texts
    const size_t small = 64 + ((size_t)K + 1) * 4 + ct.pool.size() + 64;
    const size_t sizes[4] = {(size_t)N * 4, (size_t)N * 8, (size_t)nb * 8 + 64, small};
    DevBuf *ws = ctx->readtags_rows_ws.b;
    int rc;
    for (int i = 0; i < 4; ++i)
        if ((rc = duet_reserve(ctx, ws[i], sizes[i]))) return rc;
    char *sm = (char *)ws[3].ptr;
    uint32_t *d_chrom_off = (uint32_t *)(sm + 64);
    char *d_chrom = (char *)(d_chrom_off + (K + 1));
    HIP_TRY(ctx, hipMemsetAsync(sm, 0, 64, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_chrom_off, ct.off.data(), ((size_t)K + 1) * 4, hipMemcpyHostToDevice, st));
    if (!ct.pool.empty()) HIP_TRY(ctx, hipMemcpyAsync(d_chrom, ct.pool.data(), ct.pool.size(), hipMemcpyHostToDevice, st));
    memset(&p, 0, sizeof(p));
    p.N = N; p.K = K; p.n_names = names->n_names; p.n_reads = n_reads;
    p.recs = recs; p.name_off = name_off; p.read_tag = read_tag; p.name_pool = name_pool; p.chrom_pool = d_chrom; p.chrom_off = d_chrom_off;
    p.len = (uint32_t *)ws[0].ptr;
    p.row_off = (uint64_t *)ws[1].ptr;
    p.part = (uint64_t *)ws[2].ptr;
    p.total = (uint64_t *)sm;
    p.flag = (uint32_t *)sm;
    hipLaunchKernelGGL(rr_len, dim3((N + 255) / 256), dim3(256), 0, st, p);
    hipLaunchKernelGGL((rows_scan_reduce<kRrThreads, kRrItems>), dim3(nb), dim3(kRrThreads), 0, st, (const uint32_t *)p.len, N, p.part);
    hipLaunchKernelGGL(scan_spine_u64, dim3(1), dim3(1024), 0, st, p.part, nb, p.total);
    hipLaunchKernelGGL((rows_scan_apply<kRrThreads, kRrItems>), dim3(nb), dim3(kRrThreads), 0, st, (const uint32_t *)p.len, N,
                       (const uint64_t *)p.part, p.row_off);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t fin[8];
    HIP_TRY(ctx, hipMemcpyAsync(fin, sm, sizeof(fin), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    // (before the first failure: a caller that sizes its buffer from *out_len never sees a partial sum)
    if (fin[kRowBadName]) return fail(ctx, DUET_ERR_INVALID, "read tag rows: a record's name not below n_names");
    if (fin[kRowBadContig]) return fail(ctx, DUET_ERR_INVALID, "read tag rows: a record's contig not below n_contigs");
    if (fin[kRowBadStatus]) return fail(ctx, DUET_ERR_INVALID, "read tag rows: a status code above DUET_READ_TAG_OTHER_PS");
    if (fin[kRowBadOff]) return fail(ctx, DUET_ERR_INVALID, "read tag rows: name offsets that descend");
    if (fin[kRowLong]) return fail(ctx, DUET_ERR_INVALID, "a row of 4 GiB or more");
    *need = ((uint64_t)fin[1] << 32) | fin[0];
    return DUET_OK;
}

int rows_write(duet_ctx *ctx, RrParams &p, char *out, uint64_t cap, hipStream_t st)
{
    p.out = out;
    p.cap = cap;
    const uint32_t wb = (p.N + 3) / 4;
    hipLaunchKernelGGL(rr_write, dim3(wb < 8192u ? wb : 8192u), dim3(256), 0, st, p);
    HIP_TRY(ctx, hipGetLastError());
    return DUET_OK;
}

const char kTooSmall[] = "output buffer too small for the read tag rows (*out_len = size needed)";

}  // namespace

extern "C" {

int duet_read_tags_device(duet_ctx *ctx, const duet_read_tags_problem *pr, uint32_t pc_cap, duet_read_tag_rec *out, uint32_t out_cap,
                          uint32_t *n_recs, void *stream_)
{
    int rc = check_args(ctx, pr, pc_cap, out, out_cap, n_recs);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return run(ctx, pr, pc_cap, out, out_cap, n_recs, (hipStream_t)stream_, false);
}

int duet_read_tags_host(duet_ctx *ctx, const duet_read_tags_problem *pr, uint32_t pc_cap, duet_read_tag_rec *out, uint32_t out_cap,
                        uint32_t *n_recs)
{
    int rc = check_args(ctx, pr, pc_cap, out, out_cap, n_recs);
    if (rc) return rc;
    const size_t C = pr->n_cands, M = pr->n_marks;
    if (C == 0 || M == 0) return DUET_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->own_stream;
    // staging 3-11: cand_off, mark_order, mark_read, mark_name, pred, ps, cand_pos, cand_contig, read_tag
    const void *src[9] = {pr->cand_off, pr->mark_order, pr->mark_read, pr->mark_name, pr->pred, pr->ps, pr->cand_pos, pr->cand_contig,
                          pr->read_tag};
    const size_t bytes[9] = {(C + 1) * 4, pr->mark_order ? M * 4 : 0, M * 4, M * 4, C, C * 4, C * 4, pr->cand_contig ? C * 2 : 0,
                             (size_t)pr->n_reads * 8};
    void *dev[9];
    if ((rc = duet_stage_arrays(ctx, ctx->readtags_ws.b + 3, src, bytes, 9, s, dev))) return rc;
    duet_read_tags_problem d = *pr;
    d.cand_off = (const uint32_t *)dev[0];
    d.mark_order = pr->mark_order ? (const uint32_t *)dev[1] : nullptr;
    d.mark_read = (const uint32_t *)dev[2];
    d.mark_name = (const uint32_t *)dev[3];
    d.pred = (const uint8_t *)dev[4];
    d.ps = (const uint32_t *)dev[5];
    d.cand_pos = (const uint32_t *)dev[6];
    d.cand_contig = pr->cand_contig ? (const uint16_t *)dev[7] : nullptr;
    d.read_tag = (const uint64_t *)dev[8];
    return run(ctx, &d, pc_cap, out, out_cap, n_recs, s, true);
}

int duet_read_tags_rows_device(duet_ctx *ctx, const duet_read_tag_rec *recs, uint32_t n_recs, const duet_callset_names *names,
                               const uint64_t *read_tag, uint32_t n_reads, char *out_text, uint64_t out_cap, uint64_t *out_len,
                               void *stream_)
{
    int rc;
    if ((rc = rows_check(ctx, recs, n_recs, names, read_tag, n_reads, out_text, out_len))) return rc;
    if (n_recs == 0) return DUET_OK;
    hipStream_t st = (hipStream_t)stream_;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RrParams p;
    uint64_t need = 0;
    if ((rc = rows_plan(ctx, recs, n_recs, names, names->name_off, names->name_pool, read_tag, n_reads, p, st, &need))) return rc;
    *out_len = need;
    if (need > out_cap) return fail(ctx, DUET_ERR_INVALID, kTooSmall);
    return rows_write(ctx, p, out_text, out_cap, st);
}

int duet_read_tags_rows_host(duet_ctx *ctx, const duet_read_tag_rec *recs, uint32_t n_recs, const duet_callset_names *names,
                             const uint64_t *read_tag, uint32_t n_reads, char *out_text, uint64_t out_cap, uint64_t *out_len)
{
    int rc;
    if ((rc = rows_check(ctx, recs, n_recs, names, read_tag, n_reads, out_text, out_len))) return rc;
    if (n_recs == 0) return DUET_OK;
    const size_t n_off = (size_t)names->n_names + 1;
    for (size_t j = 0; j + 1 < n_off; ++j)
        if (names->name_off[j] > names->name_off[j + 1]) return fail(ctx, DUET_ERR_INVALID, "read tag rows: name offsets that descend");
    const uint64_t pool_bytes = names->name_off[names->n_names];
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->own_stream;
    // staging 4-7: the records, the name offsets, the name pool, the read tags
    const void *src[4] = {recs, names->name_off, names->name_pool, read_tag};
    const size_t bytes[4] = {(size_t)n_recs * sizeof(duet_read_tag_rec), n_off * 8, (size_t)pool_bytes, (size_t)n_reads * 8};
    void *dev[4];
    if ((rc = duet_stage_arrays(ctx, ctx->readtags_rows_ws.b + 4, src, bytes, 4, s, dev))) return rc;
    RrParams p;
    uint64_t need = 0;
    if ((rc = rows_plan(ctx, (const duet_read_tag_rec *)dev[0], n_recs, names, (const uint64_t *)dev[1], (const char *)dev[2],
                        (const uint64_t *)dev[3], n_reads, p, s, &need)))
        return rc;
    *out_len = need;
    if (need > out_cap) return fail(ctx, DUET_ERR_INVALID, kTooSmall);
    DevBuf &ob = ctx->readtags_rows_ws.b[8];
    if ((rc = duet_reserve(ctx, ob, need + 64))) return rc;
    if ((rc = rows_write(ctx, p, (char *)ob.ptr, need, s))) return rc;
    uint32_t flag = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&flag, p.flag + kRowOverrun, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (flag) return fail(ctx, DUET_ERR_INVALID, "read tag rows overran their offsets");
    if (need) HIP_TRY(ctx, hipMemcpy(out_text, ob.ptr, need, hipMemcpyDeviceToHost));
    return DUET_OK;
}

}  // extern "C"
