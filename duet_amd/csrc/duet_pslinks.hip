// duet_pslinks.hip -- phase-set links (include/duet_ef.h: duet_ps_links_device): which phase sets the SV
// candidates tie together, in which sense and how strongly, built on the device from the resident E/F problem.  A kept candidate
// whose voting marks fall into G >= 2 phase sets gives G - 1 observations, one per pair of neighbouring PS values; the observations
// of one (contig, ps_a, ps_b) are summed into one record.
//
//   pl_count     one wavefront per candidate, 64 marks at a time like features_body: the number of its voting marks when they
//                carry two different PS values (min != max over the voters), 0 otherwise and for a candidate that is not kept
//   a scan over those counts: where each candidate's voters go, and their total V -- host round trip 1
//   pl_keys      the same walk over the multi-PS candidates: one (candidate << 32 | ps, hap - 1) pair per voter, compacted by ballot
//   a stable radix sort over exactly 32 + bits_for(C - 1) bits
//   head flags on (candidate, ps), scanned: the groups numbered, each group's first position stored; a second scan over the hap
//   bits: with it a group's h2 is a difference of two prefix sums, h1 = its size - h2 (integer, no atomics)
//   a scan over the groups that share their candidate with the group in front: those pairs numbered, and each written as one
//   observation -- contig (from the contig offsets), ps_a, ps_b, kind, weight, pos; their number -- round trip 2
//   order by (contig, ps_a, ps_b), wider than 64 bits: two stable sorts with the permutation as the value, first by ps_b (32 bits),
//   then by contig << 32 | ps_a (32 + bits_for(K - 1) bits)
//   head flags over the ordered observations, scanned: the records numbered -- round trip 3, checked against out_cap
//   pl_reduce    one wavefront per record: the sums, min and max over its observations (shuffles; integer)
// No float and no atomic in the unit's own kernels (the shared sort's rx_hist accumulates its digit totals with integer atomics up
// to 1024 tiles: sums, so nothing depends on the order of arrival).
#include "duet_internal.h"

#include <cstring>

namespace {

#include "duet_prims.hip.h"
#include "duet_seeds.hip.h"                // kEmpty, kUntagged, tag_ps, tag_pc, tag_hap

constexpr uint32_t kCapMax = (1u << 30) - 3u;         // the tag word saturates pc at 2^30 - 2: a saturated value never votes
constexpr int kWaves = 4;                             // wavefronts (candidates, records) per workgroup
constexpr uint32_t kSame = 0, kFlip = 1, kOpen = 2;

int fail(duet_ctx *ctx, int code, const char *msg) { return duet_fail(ctx, code, msg); }

struct Prob {                       // the device's view of the problem
    uint32_t C, M, K, n_reads, svlen_thres, suppread_thres, pc_cap;
    const uint64_t *read_tag;
    const uint32_t *cand_pos, *cand_svlen, *cand_svread, *cand_off, *mark_read;
    const uint8_t *cand_gt_ok;
};

// does mark m vote: its read tagged, pc <= cap, hap 1 or 2 (a tagged read with hap 3 takes no part)
__device__ __forceinline__ bool voter(const Prob &a, uint32_t m, uint32_t &ps, uint32_t &hap)
{
    const uint32_t r = a.mark_read[m];
    if (r == kEmpty || r >= a.n_reads) return false;
    const uint64_t t = a.read_tag[r];
    if (t == kUntagged) return false;
    ps = tag_ps(t);
    hap = tag_hap(t);
    return tag_pc(t) <= a.pc_cap && (hap == 1u || hap == 2u);
}

// the kept test as features_body states it (duet_tune_feat.hip.h, sv_phasing_fn.py:189-190)
__device__ __forceinline__ bool kept(const Prob &a, uint32_t c)
{
    return a.cand_svlen[c] >= a.svlen_thres && a.cand_svread[c] >= a.suppread_thres && a.cand_gt_ok[c] != 0;
}

__global__ __launch_bounds__(64 * kWaves) void pl_count(const Prob a, uint32_t *cnt)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t c64 = (uint64_t)blockIdx.x * kWaves + wave; c64 < a.C; c64 += (uint64_t)gridDim.x * kWaves) {
        const uint32_t c = (uint32_t)c64;
        uint32_t n = 0, lo = 0xFFFFFFFFu, hi = 0;
        if (kept(a, c)) {
            const uint32_t b = a.cand_off[c];
            uint32_t e = a.cand_off[c + 1];
            e = e < a.M ? e : a.M;                               // (nothing is read past the marks, whatever the offsets say)
            for (uint64_t m0 = b; m0 < e; m0 += 64) {
                const uint64_t m = m0 + lane;
                uint32_t ps = 0, hap = 0;
                if (m < e && voter(a, (uint32_t)m, ps, hap)) {
                    ++n;
                    lo = ps < lo ? ps : lo;
                    hi = ps > hi ? ps : hi;
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            n += __shfl_xor(n, o, 64);
            const uint32_t l2 = __shfl_xor(lo, o, 64), h2 = __shfl_xor(hi, o, 64);
            lo = l2 < lo ? l2 : lo;
            hi = h2 > hi ? h2 : hi;
        }
        if (lane == 0) cnt[c] = (n != 0 && lo != hi) ? n : 0u;
    }
}

__global__ __launch_bounds__(64 * kWaves) void pl_keys(const Prob a, const uint32_t *cnt, const uint32_t *start, uint32_t V, uint64_t *keys,
                                                        uint32_t *vals)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (uint64_t c64 = (uint64_t)blockIdx.x * kWaves + wave; c64 < a.C; c64 += (uint64_t)gridDim.x * kWaves) {
        const uint32_t c = (uint32_t)c64;
        if (cnt[c] == 0) continue;                               // (not kept, no voter, or one phase set)
        const uint32_t b = a.cand_off[c];
        uint32_t e = a.cand_off[c + 1];
        e = e < a.M ? e : a.M;
        uint64_t at = start[c];
        for (uint64_t m0 = b; m0 < e; m0 += 64) {
            const uint64_t m = m0 + lane;
            uint32_t ps = 0, hap = 0;
            const bool v = m < e && voter(a, (uint32_t)m, ps, hap);
            const unsigned long long mask = __ballot(v);
            const uint64_t mine = at + (uint32_t)__popcll(mask & lt);
            if (v && mine < V) {                                 // (the count kernel saw the same marks: the bound is for safety)
                keys[mine] = ((uint64_t)c << 32) | ps;
                vals[mine] = hap - 1u;
            }
            at += (uint32_t)__popcll(mask);
        }
    }
}

// the sorted (candidate, ps) keys: position i opens a group
struct LoadGroupHead {
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

// the groups: group g holds the sorted positions gstart[g] .. gstart[g + 1] (the last one up to V); p2[i] = the hap-2 voters in
// front of position i (p2[V]: all of them)
struct Groups {
    const uint64_t *keys;
    const uint32_t *gstart, *p2, *n_groups;
    uint32_t V;
    __device__ __forceinline__ uint32_t cand(uint32_t g) const { return (uint32_t)(keys[gstart[g]] >> 32); }
    __device__ __forceinline__ int64_t diff(uint32_t s, uint32_t e) const       // h1 - h2 of the positions s .. e
    {
        const int64_t n = (int64_t)e - (int64_t)s, h2 = (int64_t)p2[e] - (int64_t)p2[s];
        return n - 2 * h2;
    }
};
struct LoadPair {                   // group g > 0 forms a pair with the group in front: they share the candidate
    Groups q;
    __device__ __forceinline__ uint32_t operator()(uint32_t g) const { return (g > 0 && q.cand(g) == q.cand(g - 1)) ? 1u : 0u; }
};
struct Obs {                        // the observations, one array per field
    uint64_t *key;                  // contig << 32 | ps_a
    uint32_t *ps_b, *pos, *w, *kind;
};
struct StoreObs {
    Groups q;
    const uint32_t *ctg_off, *cand_pos;
    uint32_t K;
    Obs o;
    __device__ __forceinline__ void operator()(uint32_t g, uint32_t before, uint32_t pair) const
    {
        if (!pair || before >= q.V) return;
        const uint32_t G = *q.n_groups;
        const uint32_t sa = q.gstart[g - 1], sb = q.gstart[g], eb = g + 1 < G ? q.gstart[g + 1] : q.V;
        const int64_t da = q.diff(sa, sb), db = q.diff(sb, eb);
        const uint64_t ka = q.keys[sa], kb = q.keys[sb];
        const uint32_t c = (uint32_t)(ka >> 32);
        // the candidate's contig: the first k with ctg_off[k + 1] > c (empty contigs own nothing)
        uint32_t lo = 0, hi = K - 1u;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (ctg_off[mid + 1] <= c) lo = mid + 1; else hi = mid;
        }
        const uint64_t ma = (uint64_t)(da < 0 ? -da : da), mb = (uint64_t)(db < 0 ? -db : db);
        o.key[before] = ((uint64_t)lo << 32) | (uint32_t)ka;
        o.ps_b[before] = (uint32_t)kb;
        o.pos[before] = cand_pos[c];
        o.w[before] = (uint32_t)(ma < mb ? ma : mb);
        o.kind[before] = (da == 0 || db == 0) ? kOpen : ((da > 0) == (db > 0) ? kSame : kFlip);
    }
};

// first ordering pass: the key is ps_b, the value the observation's index
__global__ __launch_bounds__(256) void pl_key_b(const uint32_t *ps_b, uint32_t n, uint64_t *keys, uint32_t *vals)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) {
        keys[i] = ps_b[i];
        vals[i] = i;
    }
}

// second ordering pass: contig << 32 | ps_a of the observations as the first pass left them (the permutation stays the value)
__global__ __launch_bounds__(256) void pl_key_a(const uint64_t *obs_key, const uint32_t *perm, uint32_t n, uint64_t *keys)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) keys[i] = obs_key[perm[i]];
}

// the ordered observations: position i opens the run of one (contig, ps_a, ps_b)
struct LoadLinkHead {
    const uint64_t *keys;
    const uint32_t *perm, *ps_b;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const
    {
        return (i == 0 || keys[i - 1] != keys[i] || ps_b[perm[i - 1]] != ps_b[perm[i]]) ? 1u : 0u;
    }
};

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int o)
{
    const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
    return ((uint64_t)hi << 32) | lo;
}

struct ReduceArgs {
    const uint64_t *keys;           // ordered: contig << 32 | ps_a
    const uint32_t *perm, *lstart;
    Obs o;
    uint32_t n_links, n_obs;
    duet_ps_link *out;
};

__global__ __launch_bounds__(64 * kWaves) void pl_reduce(const ReduceArgs a)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t l64 = (uint64_t)blockIdx.x * kWaves + wave; l64 < a.n_links; l64 += (uint64_t)gridDim.x * kWaves) {
        const uint32_t l = (uint32_t)l64;
        const uint32_t s = a.lstart[l];
        uint32_t e = l + 1 < a.n_links ? a.lstart[l + 1] : a.n_obs;
        e = e < a.n_obs ? e : a.n_obs;
        uint32_t n_same = 0, n_flip = 0, n_open = 0, pos_min = 0xFFFFFFFFu, pos_max = 0;
        uint64_t w_same = 0, w_flip = 0;
        for (uint64_t i = (uint64_t)s + lane; i < e; i += 64) {
            const uint32_t j = a.perm[i];
            const uint32_t kind = a.o.kind[j], w = a.o.w[j], pos = a.o.pos[j];
            n_same += kind == kSame;
            n_flip += kind == kFlip;
            n_open += kind == kOpen;
            w_same += kind == kSame ? w : 0u;
            w_flip += kind == kFlip ? w : 0u;
            pos_min = pos < pos_min ? pos : pos_min;
            pos_max = pos > pos_max ? pos : pos_max;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            n_same += __shfl_xor(n_same, o, 64);
            n_flip += __shfl_xor(n_flip, o, 64);
            n_open += __shfl_xor(n_open, o, 64);
            w_same += shfl_xor_u64(w_same, o);
            w_flip += shfl_xor_u64(w_flip, o);
            const uint32_t mn = __shfl_xor(pos_min, o, 64), mx = __shfl_xor(pos_max, o, 64);
            pos_min = mn < pos_min ? mn : pos_min;
            pos_max = mx > pos_max ? mx : pos_max;
        }
        if (lane == 0 && s < a.n_obs) {
            const uint64_t k = a.keys[s];
            duet_ps_link r;
            r.w_same = w_same; r.w_flip = w_flip;
            r.contig = (uint32_t)(k >> 32); r.ps_a = (uint32_t)k; r.ps_b = a.o.ps_b[a.perm[s]];
            r.n_sv = n_same + n_flip + n_open; r.n_same = n_same; r.n_flip = n_flip; r.n_open = n_open;
            r.pos_min = pos_min; r.pos_max = pos_max;
            r.reserved = 0;
            a.out[l] = r;
        }
    }
}

uint32_t wave_grid(uint32_t n)      // workgroups of kWaves wavefronts for n wavefront-sized jobs (grid-stride beyond 2^18)
{
    const uint32_t nb = (n + kWaves - 1) / kWaves;
    return nb < (1u << 18) ? (nb ? nb : 1u) : (1u << 18);
}

int check_args(duet_ctx *ctx, const void *prob, uint32_t pc_cap, const duet_ps_link *out, uint32_t out_cap, uint32_t *n_links)
{
    if (n_links) *n_links = 0;
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    if (pc_cap > kCapMax) return fail(ctx, DUET_ERR_INVALID, "pc_cap is above 2^30 - 3 (the tag word saturates pc at 2^30 - 2)");
    if (!prob || !n_links || (!out && out_cap)) return fail(ctx, DUET_ERR_INVALID, "null argument");
    return DUET_OK;
}

// (candidates without a single mark: no array is read, there is no link whatever the arrays are)
int check_ef(duet_ctx *ctx, const duet_ef_problem *pr) { return pr->n_cands && !pr->n_marks ? DUET_OK : duet_ef_validate(ctx, pr); }

}  // namespace

int duet_ps_links_run(duet_ctx *ctx, const duet_ef_problem *pr, uint32_t pc_cap, duet_ps_link *out, uint32_t out_cap, uint32_t *n_links,
                      hipStream_t st, bool out_on_host)
{
    *n_links = 0;
    const uint32_t C = pr->n_cands, M = pr->n_marks, K = pr->n_contigs;
    if (C == 0 || M == 0) return DUET_OK;
    int rc;
    Prob a;
    memset(&a, 0, sizeof(a));
    a.C = C; a.M = M; a.K = K; a.n_reads = pr->n_reads;
    a.svlen_thres = pr->svlen_thres; a.suppread_thres = pr->suppread_thres; a.pc_cap = pc_cap;
    a.read_tag = pr->read_tag;
    a.cand_pos = pr->cand_pos; a.cand_svlen = pr->cand_svlen; a.cand_svread = pr->cand_svread; a.cand_off = pr->cand_off;
    a.mark_read = pr->mark_read; a.cand_gt_ok = pr->cand_gt_ok;

    // ---- the candidates: who has voters in two phase sets, and how many voters ----
    Arena a1;
    const size_t o_hdr = a1.take(64), o_ctg = a1.take(((size_t)K + 1) * 4), o_cnt = a1.take((size_t)C * 4), o_start = a1.take((size_t)C * 4),
                 o_part1 = a1.take(((size_t)(C + kScanTile - 1) / kScanTile + 1) * 4);
    DevBuf &ws1 = ctx->pslinks_ws.b[0];
    if ((rc = duet_reserve(ctx, ws1, a1.total))) return rc;
    char *w1 = (char *)ws1.ptr;
    // header words: [0] V, the voters of the multi-PS candidates; [1] the groups; [3] the observations; [4] the records
    uint32_t *d_hdr = (uint32_t *)(w1 + o_hdr), *d_ctg_off = (uint32_t *)(w1 + o_ctg), *cnt = (uint32_t *)(w1 + o_cnt),
             *start = (uint32_t *)(w1 + o_start), *part1 = (uint32_t *)(w1 + o_part1);
    HIP_TRY(ctx, hipMemsetAsync(d_hdr, 0, 64, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_ctg_off, pr->cand_ctg_off, ((size_t)K + 1) * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(pl_count, dim3(wave_grid(C)), dim3(64 * kWaves), 0, st, a, cnt);
    launch_scan<0>(LoadPlain{cnt}, C, part1, StorePlain{start}, d_hdr, st);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t V = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&V, d_hdr, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                                   // round trip 1
    if (V == 0) return DUET_OK;
    if (V > M) return fail(ctx, DUET_ERR_HIP, "ps links: more voters than marks (cand_off does not describe mark_read)");

    // ---- voters -> groups -> observations ----
    const uint32_t nb_rx = (V + kRxTile - 1) / kRxTile, nb_sc = (V + kScanTile - 1) / kScanTile;
    const uint32_t nb_hs = (256u * nb_rx + kScanTile - 1) / kScanTile;
    Arena a2;
    const size_t o_ka = a2.take((size_t)V * 8), o_kb = a2.take((size_t)V * 8), o_va = a2.take((size_t)V * 4), o_vb = a2.take((size_t)V * 4),
                 o_p2 = a2.take(((size_t)V + 1) * 4), o_gs = a2.take((size_t)V * 4), o_ok = a2.take((size_t)V * 8),
                 o_ob = a2.take((size_t)V * 4), o_op = a2.take((size_t)V * 4), o_ow = a2.take((size_t)V * 4), o_oq = a2.take((size_t)V * 4),
                 o_ls = a2.take((size_t)V * 4), o_hist = a2.take((size_t)256 * nb_rx * 4),
                 o_part = a2.take(((size_t)(nb_sc > nb_hs ? nb_sc : nb_hs) + 1) * 4);
    DevBuf &ws2 = ctx->pslinks_ws.b[1];
    if ((rc = duet_reserve(ctx, ws2, a2.total))) return rc;
    char *w2 = (char *)ws2.ptr;
    uint64_t *keysA = (uint64_t *)(w2 + o_ka), *keysB = (uint64_t *)(w2 + o_kb);
    uint32_t *valsA = (uint32_t *)(w2 + o_va), *valsB = (uint32_t *)(w2 + o_vb), *p2 = (uint32_t *)(w2 + o_p2),
             *gstart = (uint32_t *)(w2 + o_gs), *lstart = (uint32_t *)(w2 + o_ls), *hist = (uint32_t *)(w2 + o_hist),
             *spart = (uint32_t *)(w2 + o_part);
    Obs ob;
    ob.key = (uint64_t *)(w2 + o_ok); ob.ps_b = (uint32_t *)(w2 + o_ob); ob.pos = (uint32_t *)(w2 + o_op);
    ob.w = (uint32_t *)(w2 + o_ow); ob.kind = (uint32_t *)(w2 + o_oq);
    hipLaunchKernelGGL(pl_keys, dim3(wave_grid(C)), dim3(64 * kWaves), 0, st, a, (const uint32_t *)cnt, (const uint32_t *)start, V, keysA, valsA);
    uint64_t *sk = nullptr;
    uint32_t *sv = nullptr;
    radix_sort_pairs(keysA, keysB, valsA, valsB, V, 32u + bits_for((uint64_t)C - 1u), hist, spart, ctx->rx_dtot, st, &sk, &sv, nullptr);
    launch_scan<0>(LoadGroupHead{sk}, V, spart, StoreHeadAt{gstart}, d_hdr + 1, st);
    launch_scan<0>(LoadPlain{sv}, V, spart, StorePlain{p2}, p2 + V, st);
    Groups q;
    q.keys = sk; q.gstart = gstart; q.p2 = p2; q.n_groups = d_hdr + 1; q.V = V;
    StoreObs so;
    so.q = q; so.ctg_off = d_ctg_off; so.cand_pos = pr->cand_pos; so.K = K; so.o = ob;
    launch_scan<0>(LoadPair{q}, V, spart, so, d_hdr + 3, st, nullptr, false, d_hdr + 1);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t n_obs = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&n_obs, d_hdr + 3, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                                   // round trip 2
    if (n_obs == 0) return DUET_OK;
    if (n_obs >= V) return fail(ctx, DUET_ERR_HIP, "ps links: more observations than voters");

    // ---- order by (contig, ps_a, ps_b): two stable sorts, the permutation as the value; the records numbered ----
    const uint32_t nb_o = (n_obs + 255u) / 256u;
    hipLaunchKernelGGL(pl_key_b, dim3(nb_o), dim3(256), 0, st, (const uint32_t *)ob.ps_b, n_obs, keysA, valsA);
    uint64_t *k1 = nullptr, *k1_spare = nullptr;
    uint32_t *perm1 = nullptr;
    radix_sort_pairs(keysA, keysB, valsA, valsB, n_obs, 32u, hist, spart, ctx->rx_dtot, st, &k1, &perm1, &k1_spare);
    uint32_t *perm1_spare = perm1 == valsA ? valsB : valsA;
    hipLaunchKernelGGL(pl_key_a, dim3(nb_o), dim3(256), 0, st, (const uint64_t *)ob.key, (const uint32_t *)perm1, n_obs, k1_spare);
    uint64_t *k2 = nullptr;
    uint32_t *perm = nullptr;
    radix_sort_pairs(k1_spare, k1, perm1, perm1_spare, n_obs, 32u + bits_for((uint64_t)K - 1u), hist, spart, ctx->rx_dtot, st, &k2, &perm,
                     nullptr);
    launch_scan<0>(LoadLinkHead{k2, perm, ob.ps_b}, n_obs, spart, StoreHeadAt{lstart}, d_hdr + 4, st);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t L = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&L, d_hdr + 4, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                                   // round trip 3
    *n_links = L;
    if (L > out_cap) return fail(ctx, DUET_ERR_INVALID, "ps links: the record buffer is too small (out_cap below *n_links)");
    if (L == 0) return DUET_OK;

    // ---- the records ----
    ReduceArgs r;
    memset(&r, 0, sizeof(r));
    r.keys = k2; r.perm = perm; r.lstart = lstart; r.o = ob; r.n_links = L; r.n_obs = n_obs;
    r.out = out;
    if (out_on_host) {
        DevBuf &bo = ctx->pslinks_ws.b[2];
        if ((rc = duet_reserve(ctx, bo, (size_t)L * sizeof(duet_ps_link)))) return rc;
        r.out = (duet_ps_link *)bo.ptr;
    }
    hipLaunchKernelGGL(pl_reduce, dim3(wave_grid(L)), dim3(64 * kWaves), 0, st, r);
    HIP_TRY(ctx, hipGetLastError());
    if (out_on_host) {
        HIP_TRY(ctx, hipMemcpyAsync(out, r.out, (size_t)L * sizeof(duet_ps_link), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    return DUET_OK;
}

extern "C" {

int duet_ps_links_device(duet_ctx *ctx, const duet_ef_problem *pr, uint32_t pc_cap, duet_ps_link *out, uint32_t out_cap, uint32_t *n_links,
                         void *stream_)
{
    int rc = check_args(ctx, pr, pc_cap, out, out_cap, n_links);
    if (rc || (rc = check_ef(ctx, pr))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return duet_ps_links_run(ctx, pr, pc_cap, out, out_cap, n_links, (hipStream_t)stream_, false);
}

int duet_ps_links_host(duet_ctx *ctx, const duet_ef_problem *pr, uint32_t pc_cap, duet_ps_link *out, uint32_t out_cap, uint32_t *n_links)
{
    int rc = check_args(ctx, pr, pc_cap, out, out_cap, n_links);
    if (rc || (rc = check_ef(ctx, pr))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->own_stream;
    duet_ef_problem d = *pr;
    if (pr->n_cands && pr->n_marks && (rc = duet_ef_upload(ctx, pr, &d, s))) return rc;
    return duet_ps_links_run(ctx, &d, pc_cap, out, out_cap, n_links, s, true);
}

}  // extern "C"
