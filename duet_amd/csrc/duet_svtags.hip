// duet_svtags.hip -- tags from other SVs (include/duet_ef.h: duet_sv_tags_device): a mark whose read has no
// tag word is given the haplotype that the OTHER heterozygous calls listing the read place it on -- per mark, leave-one-out, so
// that no call votes for itself.  The output is one tag word per raw mark: a second E/F run reads it through an identity index.
//
//   st_count     per candidate: its mark count when pred is 1 or 2, else 0; offsets that descend or pass the marks are refused
//   st_owner     per CSR slot: owner[raw mark] = slot; per raw mark: the name is checked.  st_owner_check: a raw mark that two
//                slots name is refused (its tag would depend on which slot wins)
//   a scan over the counts: where each het candidate's marks go, and their total V -- host round trip 1
//   st_keys      one wavefront per het candidate: per mark the pair (name << 32 | ps[c], place), the candidate beside it
//   a stable radix sort over exactly 32 + bits_for(n_names - 1) bits
//   head flags on the key, scanned: the records numbered.  Head flags on (key, candidate), scanned: the RUNS numbered -- the sort
//   is stable and places ascend with the candidate, so a candidate's members of one record are adjacent; a run's length is k, the
//   candidate's own contribution to the record -- host round trip 2, the two counts
//   st_runs      per sorted position: k of its run, stored at the mark's place (4 bytes per contributing mark, no walk)
//   st_reduce    one wavefront per record: n_h1, n_h2; contig and read index by minimum and maximum (section 20's contradiction)
//   st_derive    one lane per raw mark: the word is copied, or chosen from the name's records with the own k taken out; three
//                counters, one ballot and one integer atomic per wavefront and counter
//   host round trip 3: the contradiction words and the counters; only then the staged words are copied to out_tag
// Integers only.  The counters are sums of popcounts: nothing depends on the order of arrival.
#include "duet_internal.h"

#include <cstring>

namespace {

#include "duet_prims.hip.h"
#include "duet_seeds.hip.h"                // kEmpty, kUntagged

constexpr uint32_t kCapMax = (1u << 30) - 3u;         // the tag word saturates pc at 2^30 - 2
constexpr int kWaves = 4;                             // wavefronts (candidates, records) per workgroup
// header words of a call: the counts, one word per refusal, the three counters
constexpr uint32_t kHdrV = 0, kHdrRecs = 1, kHdrRuns = 2, kBadPred = 4, kBadName = 5, kBadOrder = 6, kTwoContigs = 7, kTwoReads = 8,
                   kDupOrder = 9, kCntUntagged = 10, kCntGiven = 11, kCntOwnOnly = 12, kBadOff = 13, kHdrWords = 16;

int fail(duet_ctx *ctx, int code, const char *msg) { return duet_fail(ctx, code, msg); }

struct Prob {                       // the device's view of the problem
    uint32_t C, M, K, n_reads, n_names;
    const uint32_t *cand_off, *mark_order, *mark_read, *mark_name, *ps, *ctg_off;
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

__global__ __launch_bounds__(256) void st_count(const Prob a, uint32_t *cnt, uint32_t *hdr)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= a.C) return;
    const uint32_t pr = a.pred[c];
    uint32_t n = 0;
    if (a.cand_off[c] > a.cand_off[c + 1] || a.cand_off[c + 1] > a.M) hdr[kBadOff] = 1u;
    if (pr > 3u) hdr[kBadPred] = 1u;
    else if (pr == 1u || pr == 2u) {
        uint32_t b, e;
        cand_range(a, c, b, e);
        n = e - b;
    }
    cnt[c] = n;
}

// owner: all-ones on entry.  Lane i is slot i and raw mark i
__global__ __launch_bounds__(256) void st_owner(const Prob a, uint32_t *owner, uint32_t *hdr)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i64 >= a.M) return;
    const uint32_t i = (uint32_t)i64;
    if (a.mark_name[i] >= a.n_names) hdr[kBadName] = 1u;
    uint32_t slots = a.cand_off[a.C];
    slots = slots < a.M ? slots : a.M;
    const uint32_t raw = a.mark_order ? a.mark_order[i] : i;     // (an order is checked over all its M entries)
    if (raw >= a.M) hdr[kBadOrder] = 1u;
    else if (i < slots) owner[raw] = i;
}

__global__ __launch_bounds__(256) void st_owner_check(const Prob a, const uint32_t *owner, uint32_t *hdr)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t slots = a.cand_off[a.C];
    slots = slots < a.M ? slots : a.M;
    if (i64 >= slots) return;
    const uint32_t i = (uint32_t)i64, raw = a.mark_order[i];
    if (raw < a.M && owner[raw] != i) hdr[kDupOrder] = 1u;
}

__global__ __launch_bounds__(64 * kWaves) void st_keys(const Prob a, const uint32_t *cnt, const uint32_t *start, uint32_t V, uint64_t *keys,
                                                        uint32_t *vals, uint32_t *cand_of)
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
            const uint32_t raw = a.mark_order ? a.mark_order[m] : (uint32_t)m;
            uint32_t name = raw < a.M ? a.mark_name[raw] : 0u;   // (round trip 1 refused a bad order or name: not reached)
            name = name < a.n_names ? name : 0u;
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
// ... position i opens a run: a record's members from one candidate
struct LoadRunHead {
    const uint64_t *keys;
    const uint32_t *perm, *cand_of;
    uint32_t V;
    __device__ __forceinline__ uint32_t cand(uint32_t i) const
    {
        const uint32_t p = perm[i];
        return cand_of[p < V ? p : V - 1u];
    }
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const
    {
        return (i == 0 || keys[i - 1] != keys[i] || cand(i - 1) != cand(i)) ? 1u : 0u;
    }
};
struct StoreRun {                   // the run's number at every position, its first position for the heads
    uint32_t *run_start, *run_id;
    __device__ __forceinline__ void operator()(uint32_t i, uint32_t before, uint32_t head) const
    {
        run_id[i] = before + head - 1u;                          // (position 0 is a head)
        if (head) run_start[before] = i;
    }
};

__global__ __launch_bounds__(256) void st_runs(const uint32_t *perm, const uint32_t *run_id, const uint32_t *run_start, uint32_t n_runs,
                                                uint32_t V, uint32_t *kplace)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i64 >= V) return;
    const uint32_t i = (uint32_t)i64, r = run_id[i], p = perm[i];
    if (r >= n_runs || p >= V) return;                           // (not reached)
    const uint32_t e = r + 1u < n_runs ? run_start[r + 1u] : V;
    kplace[p] = e - run_start[r];
}

struct ReduceArgs {
    Prob a;
    const uint64_t *keys;           // sorted: name << 32 | ps
    const uint32_t *perm, *cand_of, *start, *rstart;
    uint32_t n_recs, V;
    uint32_t *rec_name, *rec_ps, *rec_h1, *rec_h2;
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

__global__ __launch_bounds__(64 * kWaves) void st_reduce(const ReduceArgs r)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t j64 = (uint64_t)blockIdx.x * kWaves + wave; j64 < r.n_recs; j64 += (uint64_t)gridDim.x * kWaves) {
        const uint32_t j = (uint32_t)j64;
        const uint32_t s = r.rstart[j];
        uint32_t e = j + 1 < r.n_recs ? r.rstart[j + 1] : r.V;
        e = e < r.V ? e : r.V;
        if (s >= e) continue;                                    // (a record has a member: not reached)
        uint32_t n_h1 = 0, n_h2 = 0, k_min = 0xFFFFFFFFu, k_max = 0, rd_min = 0xFFFFFFFFu, rd_max = 0;
        for (uint64_t i = (uint64_t)s + lane; i < e; i += 64) {
            uint32_t c, rd;
            member(r, (uint32_t)i, c, rd);
            const uint32_t pr = r.a.pred[c], k = contig_of(r.a, c);
            n_h1 += pr == 1u;
            n_h2 += pr == 2u;
            k_min = k < k_min ? k : k_min;
            k_max = k > k_max ? k : k_max;
            rd_min = rd < rd_min ? rd : rd_min;
            rd_max = rd > rd_max ? rd : rd_max;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            n_h1 += __shfl_xor(n_h1, o, 64);
            n_h2 += __shfl_xor(n_h2, o, 64);
            const uint32_t kn = __shfl_xor(k_min, o, 64), kx = __shfl_xor(k_max, o, 64), rn = __shfl_xor(rd_min, o, 64),
                           rx = __shfl_xor(rd_max, o, 64);
            k_min = kn < k_min ? kn : k_min;
            k_max = kx > k_max ? kx : k_max;
            rd_min = rn < rd_min ? rn : rd_min;
            rd_max = rx > rd_max ? rx : rd_max;
        }
        if (lane != 0) continue;
        const uint64_t key = r.keys[s];
        const uint32_t name = (uint32_t)(key >> 32);
        bool two_k = k_min != k_max, two_rd = rd_min != rd_max;
        if (e < r.V && (uint32_t)(r.keys[e] >> 32) == name) {    // the name's next record: its first member has to agree too
            uint32_t c2, rd2;
            member(r, e, c2, rd2);
            two_k = two_k || contig_of(r.a, c2) != k_min;
            two_rd = two_rd || rd2 != rd_min;
        }
        if (two_k) r.hdr[kTwoContigs] = 1u;
        if (two_rd) r.hdr[kTwoReads] = 1u;
        r.rec_name[j] = name;
        r.rec_ps[j] = (uint32_t)key;
        r.rec_h1[j] = n_h1;
        r.rec_h2[j] = n_h2;
    }
}

struct DeriveArgs {
    Prob a;
    const uint32_t *owner, *start, *kplace, *rec_name, *rec_ps, *rec_h1, *rec_h2;
    uint32_t n_recs, V, min_votes, pc_new;
    uint64_t *out;                  // [M] the staged words
    uint32_t *hdr;
};

__device__ __forceinline__ uint64_t abs_i64(long long d) { return d < 0 ? (uint64_t)0 - (uint64_t)d : (uint64_t)d; }

__global__ __launch_bounds__(256) void st_derive(const DeriveArgs r)
{
    const Prob &a = r.a;
    const uint64_t m64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool live = m64 < a.M;
    const uint32_t m = live ? (uint32_t)m64 : 0u;
    bool untagged = false, given = false, own_only = false;
    if (live) {
        const uint32_t rd = a.mark_read[m];
        uint64_t word = kUntagged;
        if (rd != kEmpty && rd < a.n_reads) word = a.read_tag[rd];
        untagged = word == kUntagged;
        if (untagged) {
            // the mark's candidate: the last c with cand_off[c] <= slot; the own contribution when that one is a het call
            const uint32_t slot = r.owner[m];
            uint32_t k = 0, own_ps = 0, own_pred = 0;
            if (slot != kEmpty) {
                uint32_t lo = 0, hi = a.C;                       // cand_off[lo] <= slot < cand_off[hi] where the offsets ascend
                while (hi - lo > 1u) {
                    const uint32_t mid = lo + ((hi - lo) >> 1);
                    if (a.cand_off[mid] <= slot) lo = mid; else hi = mid;
                }
                uint32_t b, e;
                cand_range(a, lo, b, e);
                const uint32_t pr = a.pred[lo];
                if (slot >= b && slot < e && (pr == 1u || pr == 2u)) {
                    const uint64_t place = (uint64_t)r.start[lo] + (slot - b);
                    if (place < r.V) {
                        k = r.kplace[place];
                        own_ps = a.ps[lo];
                        own_pred = pr;
                    }
                }
            }
            const uint32_t name = a.mark_name[m];
            uint32_t j = 0, hi = r.n_recs;                       // the first record whose name is not below the mark's
            while (j < hi) {
                const uint32_t mid = j + ((hi - j) >> 1);
                if (r.rec_name[mid] < name) j = mid + 1; else hi = mid;
            }
            // records ascend by PS inside a name: a strictly larger |d| replaces, so ties stay with the smaller PS
            uint64_t best = 0, best_in = 0;
            uint32_t best_ps = 0;
            bool best_h1 = false;
            for (; j < r.n_recs && r.rec_name[j] == name; ++j) {
                const uint32_t ps = r.rec_ps[j];
                const long long d_in = (long long)r.rec_h1[j] - (long long)r.rec_h2[j];
                long long d = d_in;
                if (own_pred && ps == own_ps) d += own_pred == 1u ? -(long long)k : (long long)k;
                const uint64_t ad = abs_i64(d), ad_in = abs_i64(d_in);
                best_in = ad_in > best_in ? ad_in : best_in;
                if (ad > best) {
                    best = ad;
                    best_ps = ps;
                    best_h1 = d > 0;
                }
            }
            given = best >= r.min_votes;                         // (min_votes >= 1: a name without a record gives nothing)
            own_only = !given && best_in >= r.min_votes;
            if (given) word = ((uint64_t)(best_h1 ? 1u : 2u) << 62) | ((uint64_t)r.pc_new << 32) | best_ps;
        }
        r.out[m] = word;
    }
    const unsigned long long b_un = __ballot(untagged), b_gv = __ballot(given), b_oo = __ballot(own_only);
    if ((threadIdx.x & 63u) == 0) {
        if (b_un) atomicAdd(&r.hdr[kCntUntagged], (uint32_t)__popcll(b_un));
        if (b_gv) atomicAdd(&r.hdr[kCntGiven], (uint32_t)__popcll(b_gv));
        if (b_oo) atomicAdd(&r.hdr[kCntOwnOnly], (uint32_t)__popcll(b_oo));
    }
}

__global__ __launch_bounds__(256) void st_iota(uint32_t *out, uint32_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = (uint32_t)i;
}

uint32_t wave_grid(uint32_t n)      // workgroups of kWaves wavefronts for n wavefront-sized jobs (grid-stride beyond 2^18)
{
    const uint32_t nb = (n + kWaves - 1) / kWaves;
    return nb < (1u << 18) ? (nb ? nb : 1u) : (1u << 18);
}

int check_args(duet_ctx *ctx, const duet_read_tags_problem *pr, uint32_t pc_cap, uint32_t min_votes, uint32_t pc_new, const uint64_t *out_tag,
               const uint32_t *out_index, uint32_t *counts)
{
    if (counts) counts[0] = counts[1] = counts[2] = 0;
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    if (pc_cap > kCapMax) return fail(ctx, DUET_ERR_INVALID, "pc_cap is above 2^30 - 3 (the tag word saturates pc at 2^30 - 2)");
    if (pc_new > kCapMax) return fail(ctx, DUET_ERR_INVALID, "sv tags: pc_new is above 2^30 - 3 (the tag word saturates pc at 2^30 - 2)");
    if (min_votes == 0) return fail(ctx, DUET_ERR_INVALID, "sv tags: min_votes is 0 (a tag needs at least one vote)");
    if (!pr || !counts) return fail(ctx, DUET_ERR_INVALID, "null argument");
    if ((pr->cand_ctg_off != nullptr) == (pr->cand_contig != nullptr))
        return fail(ctx, DUET_ERR_INVALID, "sv tags: exactly one of cand_ctg_off and cand_contig names the candidates' contigs");
    if (pr->cand_ctg_off) {
        const uint32_t K = pr->n_contigs;
        bool ok = pr->cand_ctg_off[0] == 0 && pr->cand_ctg_off[K] == pr->n_cands;
        for (uint32_t k = 0; ok && k < K; ++k) ok = pr->cand_ctg_off[k] <= pr->cand_ctg_off[k + 1];
        if (!ok) return fail(ctx, DUET_ERR_INVALID, "sv tags: cand_ctg_off does not ascend from 0 to n_cands");
    }
    if (pr->n_cands == 0 || pr->n_marks == 0) return DUET_OK;
    if (!out_tag || !out_index) return fail(ctx, DUET_ERR_INVALID, "null argument");
    if (!pr->cand_off || !pr->mark_read || !pr->mark_name || !pr->pred || !pr->ps || (!pr->read_tag && pr->n_reads))
        return fail(ctx, DUET_ERR_INVALID, "null array");
    if (pr->n_names == 0) return fail(ctx, DUET_ERR_INVALID, "sv tags: marks without a single name (n_names is 0)");
    if (pr->cand_ctg_off && pr->n_contigs == 0) return fail(ctx, DUET_ERR_INVALID, "sv tags: no contig (n_contigs is 0)");
    return DUET_OK;
}

// the tag words of a device-resident problem, checked by the caller; out_tag and out_index are device memory, or with on_host
// host memory
int run(duet_ctx *ctx, const duet_read_tags_problem *pr, uint32_t min_votes, uint32_t pc_new, uint64_t *out_tag, uint32_t *out_index,
        uint32_t *counts, hipStream_t st, bool on_host)
{
    const uint32_t C = pr->n_cands, M = pr->n_marks, K = pr->cand_ctg_off ? pr->n_contigs : 0u;
    int rc;
    Prob a;
    memset(&a, 0, sizeof(a));
    a.C = C; a.M = M; a.K = K; a.n_reads = pr->n_reads; a.n_names = pr->n_names;
    a.cand_off = pr->cand_off; a.mark_order = pr->mark_order; a.mark_read = pr->mark_read; a.mark_name = pr->mark_name;
    a.ps = pr->ps; a.pred = pr->pred; a.cand_contig = pr->cand_contig; a.read_tag = pr->read_tag;
    DevBuf *ws = ctx->svtags_ws.b;
    const uint32_t nb_m = (uint32_t)(((uint64_t)M + 255u) / 256u);

    // ---- the candidates: the het calls and how many marks they hold; the marks: whose slot each raw mark is ----
    Arena a1;
    const size_t o_hdr = a1.take(kHdrWords * 4), o_ctg = a1.take(((size_t)K + 1) * 4), o_cnt = a1.take((size_t)C * 4),
                 o_start = a1.take((size_t)C * 4), o_part1 = a1.take(((size_t)(C + kScanTile - 1) / kScanTile + 1) * 4);
    if ((rc = duet_reserve(ctx, ws[0], a1.total))) return rc;
    Arena am;
    const size_t o_owner = am.take((size_t)M * 4), o_stage = am.take((size_t)M * 8), o_iota = am.take(on_host ? (size_t)M * 4 : 0);
    if ((rc = duet_reserve(ctx, ws[1], am.total))) return rc;
    char *w1 = (char *)ws[0].ptr, *wm = (char *)ws[1].ptr;
    uint32_t *d_hdr = (uint32_t *)(w1 + o_hdr), *d_ctg_off = (uint32_t *)(w1 + o_ctg), *cnt = (uint32_t *)(w1 + o_cnt),
             *start = (uint32_t *)(w1 + o_start), *part1 = (uint32_t *)(w1 + o_part1);
    uint32_t *owner = (uint32_t *)(wm + o_owner), *iota = (uint32_t *)(wm + o_iota);
    uint64_t *stage = (uint64_t *)(wm + o_stage);
    HIP_TRY(ctx, hipMemsetAsync(d_hdr, 0, kHdrWords * 4, st));
    HIP_TRY(ctx, hipMemsetAsync(owner, 0xFF, (size_t)M * 4, st));
    if (K) {
        HIP_TRY(ctx, hipMemcpyAsync(d_ctg_off, pr->cand_ctg_off, ((size_t)K + 1) * 4, hipMemcpyHostToDevice, st));
        a.ctg_off = d_ctg_off;
    }
    hipLaunchKernelGGL(st_count, dim3((C + 255u) / 256u), dim3(256), 0, st, a, cnt, d_hdr);
    hipLaunchKernelGGL(st_owner, dim3(nb_m), dim3(256), 0, st, a, owner, d_hdr);
    if (a.mark_order) hipLaunchKernelGGL(st_owner_check, dim3(nb_m), dim3(256), 0, st, a, (const uint32_t *)owner, d_hdr);
    launch_scan<0>(LoadPlain{cnt}, C, part1, StorePlain{start}, d_hdr + kHdrV, st);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t hdr[kHdrWords];
    HIP_TRY(ctx, hipMemcpyAsync(hdr, d_hdr, sizeof(hdr), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                                   // round trip 1
    if (hdr[kBadPred]) return fail(ctx, DUET_ERR_INVALID, "sv tags: pred above 3");
    if (hdr[kBadOff]) return fail(ctx, DUET_ERR_INVALID, "sv tags: cand_off does not ascend within n_marks");
    if (hdr[kBadOrder]) return fail(ctx, DUET_ERR_INVALID, "sv tags: mark_order not below n_marks");
    if (hdr[kDupOrder]) return fail(ctx, DUET_ERR_INVALID, "sv tags: mark_order names a raw mark twice");
    if (hdr[kBadName]) return fail(ctx, DUET_ERR_INVALID, "sv tags: mark_name not below n_names");
    const uint32_t V = hdr[kHdrV];
    if (V > M) return fail(ctx, DUET_ERR_INVALID, "sv tags: more contributing marks than marks (cand_off does not ascend)");

    DeriveArgs d;
    memset(&d, 0, sizeof(d));
    if (V) {
        // ---- marks -> (name, ps) keys -> sorted -> records and runs numbered ----
        const uint32_t nb_rx = (V + kRxTile - 1) / kRxTile, nb_sc = (V + kScanTile - 1) / kScanTile;
        const uint32_t nb_hs = (256u * nb_rx + kScanTile - 1) / kScanTile;
        Arena a2;
        const size_t o_ka = a2.take((size_t)V * 8), o_kb = a2.take((size_t)V * 8), o_va = a2.take((size_t)V * 4),
                     o_vb = a2.take((size_t)V * 4), o_co = a2.take((size_t)V * 4), o_rs = a2.take((size_t)V * 4),
                     o_us = a2.take((size_t)V * 4), o_ui = a2.take((size_t)V * 4), o_kp = a2.take((size_t)V * 4),
                     o_hist = a2.take((size_t)256 * nb_rx * 4), o_part = a2.take(((size_t)(nb_sc > nb_hs ? nb_sc : nb_hs) + 1) * 4);
        if ((rc = duet_reserve(ctx, ws[2], a2.total))) return rc;
        char *w2 = (char *)ws[2].ptr;
        uint64_t *keysA = (uint64_t *)(w2 + o_ka), *keysB = (uint64_t *)(w2 + o_kb);
        uint32_t *valsA = (uint32_t *)(w2 + o_va), *valsB = (uint32_t *)(w2 + o_vb), *cand_of = (uint32_t *)(w2 + o_co),
                 *rstart = (uint32_t *)(w2 + o_rs), *run_start = (uint32_t *)(w2 + o_us), *run_id = (uint32_t *)(w2 + o_ui),
                 *kplace = (uint32_t *)(w2 + o_kp), *hist = (uint32_t *)(w2 + o_hist), *spart = (uint32_t *)(w2 + o_part);
        hipLaunchKernelGGL(st_keys, dim3(wave_grid(C)), dim3(64 * kWaves), 0, st, a, (const uint32_t *)cnt, (const uint32_t *)start, V, keysA,
                           valsA, cand_of);
        uint64_t *sk = nullptr;
        uint32_t *sv = nullptr;
        radix_sort_pairs(keysA, keysB, valsA, valsB, V, 32u + bits_for((uint64_t)pr->n_names - 1u), hist, spart, ctx->rx_dtot, st, &sk, &sv,
                         nullptr);
        launch_scan<0>(LoadRecHead{sk}, V, spart, StoreHeadAt{rstart}, d_hdr + kHdrRecs, st);
        launch_scan<0>(LoadRunHead{sk, sv, cand_of, V}, V, spart, StoreRun{run_start, run_id}, d_hdr + kHdrRuns, st);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(hdr, d_hdr, sizeof(hdr), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));                               // round trip 2
        const uint32_t N = hdr[kHdrRecs], R = hdr[kHdrRuns];
        if (N == 0 || N > V || R < N || R > V) return fail(ctx, DUET_ERR_HIP, "sv tags: the record or run count left its range");

        // ---- k of every contributing mark; the records ----
        Arena a3;
        const size_t o_rn = a3.take((size_t)N * 4), o_rp = a3.take((size_t)N * 4), o_r1 = a3.take((size_t)N * 4),
                     o_r2 = a3.take((size_t)N * 4);
        if ((rc = duet_reserve(ctx, ws[3], a3.total))) return rc;
        char *w3 = (char *)ws[3].ptr;
        ReduceArgs r;
        memset(&r, 0, sizeof(r));
        r.a = a; r.keys = sk; r.perm = sv; r.cand_of = cand_of; r.start = start; r.rstart = rstart; r.n_recs = N; r.V = V;
        r.rec_name = (uint32_t *)(w3 + o_rn); r.rec_ps = (uint32_t *)(w3 + o_rp); r.rec_h1 = (uint32_t *)(w3 + o_r1);
        r.rec_h2 = (uint32_t *)(w3 + o_r2); r.hdr = d_hdr;
        hipLaunchKernelGGL(st_runs, dim3((V + 255u) / 256u), dim3(256), 0, st, (const uint32_t *)sv, (const uint32_t *)run_id,
                           (const uint32_t *)run_start, R, V, kplace);
        hipLaunchKernelGGL(st_reduce, dim3(wave_grid(N)), dim3(64 * kWaves), 0, st, r);
        d.kplace = kplace; d.rec_name = r.rec_name; d.rec_ps = r.rec_ps; d.rec_h1 = r.rec_h1; d.rec_h2 = r.rec_h2; d.n_recs = N;
    }

    // ---- the words, into the staging block: a refusal found here leaves out_tag as it was ----
    d.a = a; d.owner = owner; d.start = start; d.V = V; d.min_votes = min_votes; d.pc_new = pc_new; d.out = stage; d.hdr = d_hdr;
    hipLaunchKernelGGL(st_derive, dim3(nb_m), dim3(256), 0, st, d);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(hdr, d_hdr, sizeof(hdr), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                                   // round trip 3
    if (hdr[kTwoContigs]) return fail(ctx, DUET_ERR_INVALID, "sv tags: the marks of one name lie on two contigs");
    if (hdr[kTwoReads]) return fail(ctx, DUET_ERR_INVALID, "sv tags: the marks of one name carry two read indices");
    counts[0] = hdr[kCntUntagged];
    counts[1] = hdr[kCntGiven];
    counts[2] = hdr[kCntOwnOnly];
    if (on_host) {
        hipLaunchKernelGGL(st_iota, dim3(nb_m), dim3(256), 0, st, iota, M);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(out_tag, stage, (size_t)M * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(out_index, iota, (size_t)M * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        return DUET_OK;
    }
    HIP_TRY(ctx, hipMemcpyAsync(out_tag, stage, (size_t)M * 8, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(st_iota, dim3(nb_m), dim3(256), 0, st, out_index, M);
    HIP_TRY(ctx, hipGetLastError());
    return DUET_OK;
}

}  // namespace

extern "C" {

int duet_sv_tags_device(duet_ctx *ctx, const duet_read_tags_problem *pr, uint32_t pc_cap, uint32_t min_votes, uint32_t pc_new,
                        uint64_t *out_tag, uint32_t *out_index, uint32_t *counts, void *stream_)
{
    int rc = check_args(ctx, pr, pc_cap, min_votes, pc_new, out_tag, out_index, counts);
    if (rc) return rc;
    if (pr->n_cands == 0 || pr->n_marks == 0) return DUET_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return run(ctx, pr, min_votes, pc_new, out_tag, out_index, counts, (hipStream_t)stream_, false);
}

int duet_sv_tags_host(duet_ctx *ctx, const duet_read_tags_problem *pr, uint32_t pc_cap, uint32_t min_votes, uint32_t pc_new,
                      uint64_t *out_tag, uint32_t *out_index, uint32_t *counts)
{
    int rc = check_args(ctx, pr, pc_cap, min_votes, pc_new, out_tag, out_index, counts);
    if (rc) return rc;
    const size_t C = pr->n_cands, M = pr->n_marks;
    if (C == 0 || M == 0) return DUET_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->own_stream;
    // staging 4-11: cand_off, mark_order, mark_read, mark_name, pred, ps, cand_contig, read_tag
    const void *src[8] = {pr->cand_off, pr->mark_order, pr->mark_read, pr->mark_name, pr->pred, pr->ps, pr->cand_contig, pr->read_tag};
    const size_t bytes[8] = {(C + 1) * 4, pr->mark_order ? M * 4 : 0, M * 4, M * 4, C, C * 4, pr->cand_contig ? C * 2 : 0,
                             (size_t)pr->n_reads * 8};
    void *dev[8];
    if ((rc = duet_stage_arrays(ctx, ctx->svtags_ws.b + 4, src, bytes, 8, s, dev))) return rc;
    duet_read_tags_problem d = *pr;
    d.cand_off = (const uint32_t *)dev[0];
    d.mark_order = pr->mark_order ? (const uint32_t *)dev[1] : nullptr;
    d.mark_read = (const uint32_t *)dev[2];
    d.mark_name = (const uint32_t *)dev[3];
    d.pred = (const uint8_t *)dev[4];
    d.ps = (const uint32_t *)dev[5];
    d.cand_contig = pr->cand_contig ? (const uint16_t *)dev[6] : nullptr;
    d.read_tag = (const uint64_t *)dev[7];
    return run(ctx, &d, min_votes, pc_new, out_tag, out_index, counts, s, true);
}

}  // extern "C"
