// duet_svtags_plan.hip -- tags from other SVs for MANY first-run vectors (include/duet_ef.h: duet_sv_tags_plan_device,
// duet_sv_tags_apply_device).  duet_svtags.hip restated along one line: what does not read pred is done once
// (the PLAN, over the candidates of a mask instead of the het ones), what reads pred is done per vector (the APPLY) without a sort,
// an allocation or a host round trip.
//
// The plan:
//   sp_count, sp_owner, sp_owner_check, sp_keys    as st_count .. st_keys, the mask in pred's place
//   a scan over the untagged flags of the raw marks: where each untagged mark's record goes, and their number U -- host round trip 1
//   the stable radix sort, the records and the runs numbered as in duet_svtags.hip -- host round trip 2
//   sp_runs      per sorted position: k of its run at the mark's place; the run's head stores the run itself, (candidate, k)
//   sp_records   one wavefront per record: name, PS, its first run; contig and read index by minimum and maximum (section 20's
//                contradiction, over the MASKED candidates)
//   sp_marks     one lane per raw mark: the base word (the tag word, or all-ones); for an untagged mark its record -- the mark, its
//                candidate when that one is masked, its own k, the records of its name
//   host round trip 3: the contradiction words; only then the base words are copied to out_tag
// The apply:
//   sa_records   one lane per record: n_h1 = sum of k over its runs whose candidate has pred 1, n_h2 likewise.  A record of up to
//                kLight runs is summed by its lane; the longer ones of a wavefront are then taken one after the other by all 64
//                lanes (a ballot names them, the record's range travels by a lane read, the sums by a butterfly)
//   sa_marks     one lane per untagged mark: st_derive's choice from the plan, pred and the plan's copy of ps; lane i < C also
//                judges candidate i for the fourth counter.  Four counters, one ballot and one integer atomic per wavefront each
// Integers only.  The counters are sums of popcounts: nothing depends on the order of arrival.
#include "duet_internal.h"

#include <cstring>

namespace {

#include "duet_prims.hip.h"
#include "duet_seeds.hip.h"                // kEmpty, kUntagged

constexpr uint32_t kCapMax = (1u << 30) - 3u;         // the tag word saturates pc at 2^30 - 2
constexpr int kWaves = 4;                             // wavefronts (candidates, records) per workgroup
constexpr uint32_t kLight = 8;                        // sa_records: a record of more runs is summed by the whole wavefront
// header words of a plan: the counts, one word per refusal
constexpr uint32_t kHdrV = 0, kHdrRecs = 1, kHdrRuns = 2, kHdrUntagged = 3, kBadName = 5, kBadOrder = 6, kTwoContigs = 7, kTwoReads = 8,
                   kDupOrder = 9, kBadOff = 13, kHdrWords = 16;

int fail(duet_ctx *ctx, int code, const char *msg) { return duet_fail(ctx, code, msg); }

struct Prob {                       // the device's view of the problem
    uint32_t C, M, K, n_reads, n_names;
    const uint32_t *cand_off, *mark_order, *mark_read, *mark_name, *ps, *ctg_off;
    const uint8_t *mask;            // null: every candidate
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

__global__ __launch_bounds__(256) void sp_count(const Prob a, uint32_t *cnt, uint32_t *hdr)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= a.C) return;
    uint32_t n = 0;
    if (a.cand_off[c] > a.cand_off[c + 1] || a.cand_off[c + 1] > a.M) hdr[kBadOff] = 1u;
    if (!a.mask || a.mask[c]) {
        uint32_t b, e;
        cand_range(a, c, b, e);
        n = e - b;
    }
    cnt[c] = n;
}

// owner: all-ones on entry.  Lane i is slot i and raw mark i
__global__ __launch_bounds__(256) void sp_owner(const Prob a, uint32_t *owner, uint32_t *hdr)
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

__global__ __launch_bounds__(256) void sp_owner_check(const Prob a, const uint32_t *owner, uint32_t *hdr)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t slots = a.cand_off[a.C];
    slots = slots < a.M ? slots : a.M;
    if (i64 >= slots) return;
    const uint32_t i = (uint32_t)i64, raw = a.mark_order[i];
    if (raw < a.M && owner[raw] != i) hdr[kDupOrder] = 1u;
}

__global__ __launch_bounds__(64 * kWaves) void sp_keys(const Prob a, const uint32_t *cnt, const uint32_t *start, uint32_t V, uint64_t *keys,
                                                        uint32_t *vals, uint32_t *cand_of)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t c64 = (uint64_t)blockIdx.x * kWaves + wave; c64 < a.C; c64 += (uint64_t)gridDim.x * kWaves) {
        const uint32_t c = (uint32_t)c64;
        if (cnt[c] == 0) continue;                               // (not masked, or no mark)
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

// raw mark i has no tag: the header's one definition
__device__ __forceinline__ uint64_t base_word(const Prob &a, uint32_t i)
{
    const uint32_t rd = a.mark_read[i];
    return (rd != kEmpty && rd < a.n_reads) ? a.read_tag[rd] : kUntagged;
}
struct LoadUntagged {
    Prob a;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return base_word(a, i) == kUntagged ? 1u : 0u; }
};
struct StoreUpos {                  // upos[raw mark] = the number of its record, for the untagged marks
    uint32_t *upos;
    __device__ __forceinline__ void operator()(uint32_t i, uint32_t before, uint32_t flag) const
    {
        if (flag) upos[i] = before;
    }
};

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

// the plan as the kernels see it (host copy: duet_ctx::svplan)
struct Plan {
    uint32_t C, M, U, N, R;
    const uint2 *runs;              // [R] (candidate, k), by record
    const uint32_t *rec_first;      // [N + 1] the first run of every record
    const uint32_t *rec_ps;         // [N]
    uint2 *rec_h;                   // [N] (n_h1, n_h2) of the vector being applied
    const uint32_t *u_mark, *u_cand, *u_k, *u_lo, *u_hi;         // [U] the untagged marks
    const uint32_t *ps;             // [C] the plan's copy
    const uint8_t *mask;            // [C] the plan's copy, or null
};

__global__ __launch_bounds__(256) void sp_runs(const uint32_t *perm, const uint32_t *run_id, const uint32_t *run_start, const uint32_t *cand_of,
                                                uint32_t n_runs, uint32_t V, uint32_t *kplace, uint2 *runs)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i64 >= V) return;
    const uint32_t i = (uint32_t)i64, r = run_id[i], p = perm[i];
    if (r >= n_runs || p >= V) return;                           // (not reached)
    const uint32_t s = run_start[r], e = r + 1u < n_runs ? run_start[r + 1u] : V;
    kplace[p] = e - s;
    if (i == s) runs[r] = make_uint2(cand_of[p], e - s);
}

struct RecordArgs {
    Prob a;
    const uint64_t *keys;           // sorted: name << 32 | ps
    const uint32_t *perm, *cand_of, *start, *rstart, *run_id;
    uint32_t n_recs, n_runs, V;
    uint32_t *rec_name, *rec_ps, *rec_first;
    uint32_t *hdr;
};

// member i of the sorted order: its candidate and its read index
__device__ __forceinline__ void member(const RecordArgs &r, uint32_t i, uint32_t &c, uint32_t &rd)
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

__global__ __launch_bounds__(64 * kWaves) void sp_records(const RecordArgs r)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t j64 = (uint64_t)blockIdx.x * kWaves + wave; j64 < r.n_recs; j64 += (uint64_t)gridDim.x * kWaves) {
        const uint32_t j = (uint32_t)j64;
        const uint32_t s = r.rstart[j];
        uint32_t e = j + 1 < r.n_recs ? r.rstart[j + 1] : r.V;
        e = e < r.V ? e : r.V;
        if (s >= e) continue;                                    // (a record has a member: not reached)
        uint32_t k_min = 0xFFFFFFFFu, k_max = 0, rd_min = 0xFFFFFFFFu, rd_max = 0;
        for (uint64_t i = (uint64_t)s + lane; i < e; i += 64) {
            uint32_t c, rd;
            member(r, (uint32_t)i, c, rd);
            const uint32_t k = contig_of(r.a, c);
            k_min = k < k_min ? k : k_min;
            k_max = k > k_max ? k : k_max;
            rd_min = rd < rd_min ? rd : rd_min;
            rd_max = rd > rd_max ? rd : rd_max;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
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
        const uint32_t first = r.run_id[s];                      // (a record's head is a run's head)
        r.rec_first[j] = first < r.n_runs ? first : r.n_runs;
        if (j + 1u == r.n_recs) r.rec_first[r.n_recs] = r.n_runs;
    }
}

struct MarkArgs {
    Prob a;
    const uint32_t *owner, *cnt, *start, *kplace, *upos, *rec_name;
    uint32_t n_recs, V, U;
    uint64_t *stage;                // [M] the base words
    uint32_t *u_mark, *u_cand, *u_k, *u_lo, *u_hi;
};

__global__ __launch_bounds__(256) void sp_marks(const MarkArgs r)
{
    const Prob &a = r.a;
    const uint64_t m64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (m64 >= a.M) return;
    const uint32_t m = (uint32_t)m64;
    const uint64_t word = base_word(a, m);
    r.stage[m] = word;
    if (word != kUntagged) return;
    const uint32_t u = r.upos[m];
    if (u >= r.U) return;                                        // (the scan counted the same flags: not reached)
    // the mark's candidate: the last c with cand_off[c] <= slot; kept with its own contribution when that one is masked
    const uint32_t slot = r.owner[m];
    uint32_t cand = kEmpty, k = 0;
    if (slot != kEmpty) {
        uint32_t lo = 0, hi = a.C;                               // cand_off[lo] <= slot < cand_off[hi] where the offsets ascend
        while (hi - lo > 1u) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (a.cand_off[mid] <= slot) lo = mid; else hi = mid;
        }
        uint32_t b, e;
        cand_range(a, lo, b, e);
        if (slot >= b && slot < e && r.cnt[lo] != 0) {
            const uint64_t place = (uint64_t)r.start[lo] + (slot - b);
            if (place < r.V) {
                cand = lo;
                k = r.kplace[place];
            }
        }
    }
    const uint32_t name = a.mark_name[m];
    uint32_t lo = 0, hi = r.n_recs;                              // the first record whose name is not below the mark's
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (r.rec_name[mid] < name) lo = mid + 1; else hi = mid;
    }
    uint32_t end = lo;
    hi = r.n_recs;                                               // ... and the first whose name is above it
    while (end < hi) {
        const uint32_t mid = end + ((hi - end) >> 1);
        if (r.rec_name[mid] <= name) end = mid + 1; else hi = mid;
    }
    r.u_mark[u] = m;
    r.u_cand[u] = cand;
    r.u_k[u] = k;
    r.u_lo[u] = lo;
    r.u_hi[u] = end;
}

__global__ __launch_bounds__(256) void sp_iota(uint32_t *out, uint32_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = (uint32_t)i;
}

// ---- the apply -------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t pred_of(const Plan &p, const uint8_t *pred, uint32_t c) { return c < p.C ? pred[c] : 0u; }

__global__ __launch_bounds__(256) void sa_records(const Plan p, const uint8_t *pred)
{
    const uint64_t j64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool live = j64 < p.N;
    const uint32_t j = live ? (uint32_t)j64 : 0u, lane = threadIdx.x & 63u;
    uint32_t f = 0, e = 0, n_h1 = 0, n_h2 = 0;
    if (live) {
        f = p.rec_first[j];
        e = p.rec_first[j + 1];
        e = e < p.R ? e : p.R;
        f = f < e ? f : e;
    }
    const bool heavy = e - f > kLight;
    if (!heavy)
        for (uint32_t i = f; i < e; ++i) {
            const uint2 run = p.runs[i];
            const uint32_t pr = pred_of(p, pred, run.x);
            n_h1 += pr == 1u ? run.y : 0u;
            n_h2 += pr == 2u ? run.y : 0u;
        }
    // the long records of this wavefront, one after the other by all its lanes (the ballot is the same in every lane)
    unsigned long long todo = __ballot(heavy);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        const uint32_t f0 = __shfl(f, src, 64), e0 = __shfl(e, src, 64);
        uint32_t h1 = 0, h2 = 0;
        for (uint64_t i = (uint64_t)f0 + lane; i < e0; i += 64) {
            const uint2 run = p.runs[i];
            const uint32_t pr = pred_of(p, pred, run.x);
            h1 += pr == 1u ? run.y : 0u;
            h2 += pr == 2u ? run.y : 0u;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            h1 += __shfl_xor(h1, o, 64);
            h2 += __shfl_xor(h2, o, 64);
        }
        if ((int)lane == src) {
            n_h1 = h1;
            n_h2 = h2;
        }
    }
    if (live) p.rec_h[j] = make_uint2(n_h1, n_h2);
}

__device__ __forceinline__ uint64_t abs_i64(long long d) { return d < 0 ? (uint64_t)0 - (uint64_t)d : (uint64_t)d; }

__global__ __launch_bounds__(256) void sa_marks(const Plan p, const uint8_t *pred, uint32_t min_votes, uint32_t pc_new, uint64_t *out_tag,
                                                 uint32_t *counts)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool live = i64 < p.U;
    bool given = false, own_only = false, bad = false;
    if (i64 < p.C) {                                             // candidate i: a call the plan cannot serve
        const uint32_t pr = pred[i64];
        bad = pr > 3u || ((pr == 1u || pr == 2u) && p.mask && !p.mask[i64]);
    }
    if (live) {
        const uint32_t u = (uint32_t)i64, m = p.u_mark[u], c = p.u_cand[u], k = p.u_k[u];
        uint32_t j = p.u_lo[u], hi = p.u_hi[u];
        hi = hi < p.N ? hi : p.N;
        uint32_t own_ps = 0, own_pred = 0;
        if (c < p.C) {                                           // the own contribution when the mark's candidate is a het call
            const uint32_t pr = pred[c];
            if (pr == 1u || pr == 2u) {
                own_pred = pr;
                own_ps = p.ps[c];
            }
        }
        // records ascend by PS inside a name: a strictly larger |d| replaces, so ties stay with the smaller PS
        uint64_t best = 0, best_in = 0;
        uint32_t best_ps = 0;
        bool best_h1 = false;
        for (; j < hi; ++j) {
            const uint32_t ps = p.rec_ps[j];
            const uint2 h = p.rec_h[j];
            const long long d_in = (long long)h.x - (long long)h.y;
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
        given = best >= min_votes;                               // (min_votes >= 1: a name without a record gives nothing)
        own_only = !given && best_in >= min_votes;
        uint64_t word = kUntagged;
        if (given) word = ((uint64_t)(best_h1 ? 1u : 2u) << 62) | ((uint64_t)pc_new << 32) | best_ps;
        if (m < p.M) out_tag[m] = word;
    }
    const unsigned long long b_un = __ballot(live), b_gv = __ballot(given), b_oo = __ballot(own_only), b_bad = __ballot(bad);
    if ((threadIdx.x & 63u) == 0) {
        if (b_un) atomicAdd(&counts[0], (uint32_t)__popcll(b_un));
        if (b_gv) atomicAdd(&counts[1], (uint32_t)__popcll(b_gv));
        if (b_oo) atomicAdd(&counts[2], (uint32_t)__popcll(b_oo));
        if (b_bad) atomicAdd(&counts[3], (uint32_t)__popcll(b_bad));
    }
}

uint32_t wave_grid(uint32_t n)      // workgroups of kWaves wavefronts for n wavefront-sized jobs (grid-stride beyond 2^18)
{
    const uint32_t nb = (n + kWaves - 1) / kWaves;
    return nb < (1u << 18) ? (nb ? nb : 1u) : (1u << 18);
}

int check_plan_args(duet_ctx *ctx, const duet_read_tags_problem *pr, uint32_t pc_cap, const uint64_t *out_tag, const uint32_t *out_index,
                    duet_sv_tags_plan_info *info)
{
    if (info) memset(info, 0, sizeof(*info));
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    ctx->svplan.valid = false;                                   // (a later plan replaces the one before it, accepted or not)
    if (pc_cap > kCapMax) return fail(ctx, DUET_ERR_INVALID, "pc_cap is above 2^30 - 3 (the tag word saturates pc at 2^30 - 2)");
    if (!pr || !info) return fail(ctx, DUET_ERR_INVALID, "null argument");
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
    if (!pr->cand_off || !pr->mark_read || !pr->mark_name || !pr->ps || (!pr->read_tag && pr->n_reads))
        return fail(ctx, DUET_ERR_INVALID, "null array");
    if (pr->n_names == 0) return fail(ctx, DUET_ERR_INVALID, "sv tags: marks without a single name (n_names is 0)");
    if (pr->cand_ctg_off && pr->n_contigs == 0) return fail(ctx, DUET_ERR_INVALID, "sv tags: no contig (n_contigs is 0)");
    return DUET_OK;
}

void empty_plan(duet_ctx *ctx, uint32_t C, uint32_t M)
{
    ctx->svplan = DuetSvPlan();
    ctx->svplan.C = C;
    ctx->svplan.M = M;
    ctx->svplan.valid = true;
}

// the plan of a device-resident problem, checked by the caller; mask device memory or null; out_tag and out_index are device
// memory, or with on_host host memory
int plan(duet_ctx *ctx, const duet_read_tags_problem *pr, const uint8_t *mask, uint64_t *out_tag, uint32_t *out_index,
         duet_sv_tags_plan_info *info, hipStream_t st, bool on_host)
{
    const uint32_t C = pr->n_cands, M = pr->n_marks, K = pr->cand_ctg_off ? pr->n_contigs : 0u;
    int rc;
    Prob a;
    memset(&a, 0, sizeof(a));
    a.C = C; a.M = M; a.K = K; a.n_reads = pr->n_reads; a.n_names = pr->n_names;
    a.cand_off = pr->cand_off; a.mark_order = pr->mark_order; a.mark_read = pr->mark_read; a.mark_name = pr->mark_name;
    a.ps = pr->ps; a.mask = mask; a.cand_contig = pr->cand_contig; a.read_tag = pr->read_tag;
    DevBuf *ws = ctx->svplan_ws.b;
    const uint32_t nb_m = (uint32_t)(((uint64_t)M + 255u) / 256u);

    // ---- the candidates: the masked ones and how many marks they hold; the marks: whose slot each is, which have no tag ----
    Arena a1;
    const size_t o_hdr = a1.take(kHdrWords * 4), o_ctg = a1.take(((size_t)K + 1) * 4), o_cnt = a1.take((size_t)C * 4),
                 o_start = a1.take((size_t)C * 4), o_part1 = a1.take(((size_t)(C + kScanTile - 1) / kScanTile + 1) * 4);
    if ((rc = duet_reserve(ctx, ws[0], a1.total))) return rc;
    Arena am;
    const size_t o_owner = am.take((size_t)M * 4), o_stage = am.take((size_t)M * 8), o_upos = am.take((size_t)M * 4),
                 o_partm = am.take(((size_t)(M + kScanTile - 1) / kScanTile + 1) * 4), o_iota = am.take(on_host ? (size_t)M * 4 : 0);
    if ((rc = duet_reserve(ctx, ws[1], am.total))) return rc;
    Arena ak;                                                    // kept: the plan's copies of ps and the mask
    const size_t o_ps = ak.take((size_t)C * 4), o_mask = ak.take(mask ? (size_t)C : 0);
    if ((rc = duet_reserve(ctx, ws[5], ak.total))) return rc;
    char *w1 = (char *)ws[0].ptr, *wm = (char *)ws[1].ptr, *wk = (char *)ws[5].ptr;
    uint32_t *d_hdr = (uint32_t *)(w1 + o_hdr), *d_ctg_off = (uint32_t *)(w1 + o_ctg), *cnt = (uint32_t *)(w1 + o_cnt),
             *start = (uint32_t *)(w1 + o_start), *part1 = (uint32_t *)(w1 + o_part1);
    uint32_t *owner = (uint32_t *)(wm + o_owner), *upos = (uint32_t *)(wm + o_upos), *partm = (uint32_t *)(wm + o_partm),
             *iota = (uint32_t *)(wm + o_iota);
    uint64_t *stage = (uint64_t *)(wm + o_stage);
    HIP_TRY(ctx, hipMemsetAsync(d_hdr, 0, kHdrWords * 4, st));
    HIP_TRY(ctx, hipMemsetAsync(owner, 0xFF, (size_t)M * 4, st));
    HIP_TRY(ctx, hipMemcpyAsync(wk + o_ps, pr->ps, (size_t)C * 4, hipMemcpyDeviceToDevice, st));
    if (mask) HIP_TRY(ctx, hipMemcpyAsync(wk + o_mask, mask, (size_t)C, hipMemcpyDeviceToDevice, st));
    if (K) {
        HIP_TRY(ctx, hipMemcpyAsync(d_ctg_off, pr->cand_ctg_off, ((size_t)K + 1) * 4, hipMemcpyHostToDevice, st));
        a.ctg_off = d_ctg_off;
    }
    hipLaunchKernelGGL(sp_count, dim3((C + 255u) / 256u), dim3(256), 0, st, a, cnt, d_hdr);
    hipLaunchKernelGGL(sp_owner, dim3(nb_m), dim3(256), 0, st, a, owner, d_hdr);
    if (a.mark_order) hipLaunchKernelGGL(sp_owner_check, dim3(nb_m), dim3(256), 0, st, a, (const uint32_t *)owner, d_hdr);
    launch_scan<0>(LoadPlain{cnt}, C, part1, StorePlain{start}, d_hdr + kHdrV, st);
    launch_scan<0>(LoadUntagged{a}, M, partm, StoreUpos{upos}, d_hdr + kHdrUntagged, st);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t hdr[kHdrWords];
    HIP_TRY(ctx, hipMemcpyAsync(hdr, d_hdr, sizeof(hdr), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                                   // round trip 1
    if (hdr[kBadOff]) return fail(ctx, DUET_ERR_INVALID, "sv tags: cand_off does not ascend within n_marks");
    if (hdr[kBadOrder]) return fail(ctx, DUET_ERR_INVALID, "sv tags: mark_order not below n_marks");
    if (hdr[kDupOrder]) return fail(ctx, DUET_ERR_INVALID, "sv tags: mark_order names a raw mark twice");
    if (hdr[kBadName]) return fail(ctx, DUET_ERR_INVALID, "sv tags: mark_name not below n_names");
    const uint32_t V = hdr[kHdrV], U = hdr[kHdrUntagged];
    if (V > M) return fail(ctx, DUET_ERR_INVALID, "sv tags: more contributing marks than marks (cand_off does not ascend)");
    if (U > M) return fail(ctx, DUET_ERR_HIP, "sv tags: the untagged count left its range");

    Arena au;                                                    // kept: the untagged marks
    const size_t o_um = au.take((size_t)U * 4), o_uc = au.take((size_t)U * 4), o_uk = au.take((size_t)U * 4), o_ul = au.take((size_t)U * 4),
                 o_uh = au.take((size_t)U * 4);
    if ((rc = duet_reserve(ctx, ws[4], au.total + 256))) return rc;
    char *wu = (char *)ws[4].ptr;
    MarkArgs d;
    memset(&d, 0, sizeof(d));
    DuetSvPlan np;
    uint32_t N = 0, R = 0;
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
        hipLaunchKernelGGL(sp_keys, dim3(wave_grid(C)), dim3(64 * kWaves), 0, st, a, (const uint32_t *)cnt, (const uint32_t *)start, V, keysA,
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
        N = hdr[kHdrRecs];
        R = hdr[kHdrRuns];
        if (N == 0 || N > V || R < N || R > V) return fail(ctx, DUET_ERR_HIP, "sv tags: the record or run count left its range");

        // ---- kept: the runs and the records ----
        Arena a3;
        const size_t o_runs = a3.take((size_t)R * 8), o_rf = a3.take(((size_t)N + 1) * 4), o_rn = a3.take((size_t)N * 4),
                     o_rp = a3.take((size_t)N * 4), o_rh = a3.take((size_t)N * 8);
        if ((rc = duet_reserve(ctx, ws[3], a3.total))) return rc;
        char *w3 = (char *)ws[3].ptr;
        RecordArgs r;
        memset(&r, 0, sizeof(r));
        r.a = a; r.keys = sk; r.perm = sv; r.cand_of = cand_of; r.start = start; r.rstart = rstart; r.run_id = run_id; r.n_recs = N;
        r.n_runs = R; r.V = V;
        r.rec_name = (uint32_t *)(w3 + o_rn); r.rec_ps = (uint32_t *)(w3 + o_rp); r.rec_first = (uint32_t *)(w3 + o_rf); r.hdr = d_hdr;
        hipLaunchKernelGGL(sp_runs, dim3((V + 255u) / 256u), dim3(256), 0, st, (const uint32_t *)sv, (const uint32_t *)run_id,
                           (const uint32_t *)run_start, (const uint32_t *)cand_of, R, V, kplace, (uint2 *)(w3 + o_runs));
        hipLaunchKernelGGL(sp_records, dim3(wave_grid(N)), dim3(64 * kWaves), 0, st, r);
        d.kplace = kplace; d.rec_name = r.rec_name;
        np.runs = w3 + o_runs; np.rec_first = r.rec_first; np.rec_ps = r.rec_ps; np.rec_h = w3 + o_rh;
    }

    // ---- the base words, into the staging block (a refusal found here leaves out_tag as it was), and the untagged marks ----
    d.a = a; d.owner = owner; d.cnt = cnt; d.start = start; d.upos = upos; d.n_recs = N; d.V = V; d.U = U; d.stage = stage;
    d.u_mark = (uint32_t *)(wu + o_um); d.u_cand = (uint32_t *)(wu + o_uc); d.u_k = (uint32_t *)(wu + o_uk);
    d.u_lo = (uint32_t *)(wu + o_ul); d.u_hi = (uint32_t *)(wu + o_uh);
    hipLaunchKernelGGL(sp_marks, dim3(nb_m), dim3(256), 0, st, d);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(hdr, d_hdr, sizeof(hdr), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                                   // round trip 3
    if (hdr[kTwoContigs]) return fail(ctx, DUET_ERR_INVALID, "sv tags: the marks of one name lie on two contigs");
    if (hdr[kTwoReads]) return fail(ctx, DUET_ERR_INVALID, "sv tags: the marks of one name carry two read indices");
    if (on_host) {
        hipLaunchKernelGGL(sp_iota, dim3(nb_m), dim3(256), 0, st, iota, M);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(out_tag, stage, (size_t)M * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(out_index, iota, (size_t)M * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
    } else {
        HIP_TRY(ctx, hipMemcpyAsync(out_tag, stage, (size_t)M * 8, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(sp_iota, dim3(nb_m), dim3(256), 0, st, out_index, M);
        HIP_TRY(ctx, hipGetLastError());
    }
    np.C = C; np.M = M; np.U = U; np.N = N; np.R = R; np.V = V;
    np.u_mark = d.u_mark; np.u_cand = d.u_cand; np.u_k = d.u_k; np.u_lo = d.u_lo; np.u_hi = d.u_hi;
    np.ps = wk + o_ps;
    np.mask = mask ? wk + o_mask : nullptr;
    np.valid = true;
    ctx->svplan = np;
    info->n_untagged = U; info->n_records = N; info->n_runs = R; info->n_contributing = V;
    return DUET_OK;
}

int check_apply_args(duet_ctx *ctx, const uint8_t *pred, uint32_t min_votes, uint32_t pc_new, const uint64_t *out_tag, const uint32_t *out_counts)
{
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    if (!ctx->svplan.valid) return fail(ctx, DUET_ERR_INVALID, "sv tags: apply without a plan (duet_sv_tags_plan_* comes first)");
    if (pc_new > kCapMax) return fail(ctx, DUET_ERR_INVALID, "sv tags: pc_new is above 2^30 - 3 (the tag word saturates pc at 2^30 - 2)");
    if (min_votes == 0) return fail(ctx, DUET_ERR_INVALID, "sv tags: min_votes is 0 (a tag needs at least one vote)");
    if (!out_counts) return fail(ctx, DUET_ERR_INVALID, "null argument");
    if (ctx->svplan.C && ctx->svplan.M && (!pred || !out_tag)) return fail(ctx, DUET_ERR_INVALID, "null argument");
    return DUET_OK;
}

// one vector on the context's plan: device arrays, nothing read back
int apply(duet_ctx *ctx, const uint8_t *pred, uint32_t min_votes, uint32_t pc_new, uint64_t *out_tag, uint32_t *out_counts, hipStream_t st)
{
    const DuetSvPlan &sp = ctx->svplan;
    HIP_TRY(ctx, hipMemsetAsync(out_counts, 0, 16, st));
    if (sp.C == 0 || sp.M == 0) return DUET_OK;
    Plan p;
    memset(&p, 0, sizeof(p));
    p.C = sp.C; p.M = sp.M; p.U = sp.U; p.N = sp.N; p.R = sp.R;
    p.runs = (const uint2 *)sp.runs; p.rec_first = sp.rec_first; p.rec_ps = sp.rec_ps; p.rec_h = (uint2 *)sp.rec_h;
    p.u_mark = sp.u_mark; p.u_cand = sp.u_cand; p.u_k = sp.u_k; p.u_lo = sp.u_lo; p.u_hi = sp.u_hi;
    p.ps = (const uint32_t *)sp.ps; p.mask = (const uint8_t *)sp.mask;
    if (p.N) hipLaunchKernelGGL(sa_records, dim3((p.N + 255u) / 256u), dim3(256), 0, st, p, pred);
    const uint32_t lanes = p.U > p.C ? p.U : p.C;
    hipLaunchKernelGGL(sa_marks, dim3((uint32_t)(((uint64_t)lanes + 255u) / 256u)), dim3(256), 0, st, p, pred, min_votes, pc_new, out_tag,
                       out_counts);
    HIP_TRY(ctx, hipGetLastError());
    return DUET_OK;
}

}  // namespace

extern "C" {

int duet_sv_tags_plan_device(duet_ctx *ctx, const duet_read_tags_problem *pr, const uint8_t *cand_mask, uint32_t pc_cap, uint64_t *out_tag,
                             uint32_t *out_index, duet_sv_tags_plan_info *info, void *stream_)
{
    int rc = check_plan_args(ctx, pr, pc_cap, out_tag, out_index, info);
    if (rc) return rc;
    if (pr->n_cands == 0 || pr->n_marks == 0) {
        empty_plan(ctx, pr->n_cands, pr->n_marks);
        return DUET_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return plan(ctx, pr, cand_mask, out_tag, out_index, info, (hipStream_t)stream_, false);
}

int duet_sv_tags_plan_host(duet_ctx *ctx, const duet_read_tags_problem *pr, const uint8_t *cand_mask, uint32_t pc_cap, uint64_t *out_tag,
                           uint32_t *out_index, duet_sv_tags_plan_info *info)
{
    int rc = check_plan_args(ctx, pr, pc_cap, out_tag, out_index, info);
    if (rc) return rc;
    const size_t C = pr->n_cands, M = pr->n_marks;
    if (C == 0 || M == 0) {
        empty_plan(ctx, pr->n_cands, pr->n_marks);
        return DUET_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->own_stream;
    // staging 0-7: cand_off, mark_order, mark_read, mark_name, the mask, ps, cand_contig, read_tag
    const void *src[8] = {pr->cand_off, pr->mark_order, pr->mark_read, pr->mark_name, cand_mask, pr->ps, pr->cand_contig, pr->read_tag};
    const size_t bytes[8] = {(C + 1) * 4, pr->mark_order ? M * 4 : 0, M * 4, M * 4, cand_mask ? C : 0, C * 4, pr->cand_contig ? C * 2 : 0,
                             (size_t)pr->n_reads * 8};
    void *dev[8];
    if ((rc = duet_stage_arrays(ctx, ctx->svplan_in.b, src, bytes, 8, s, dev))) return rc;
    duet_read_tags_problem d = *pr;
    d.cand_off = (const uint32_t *)dev[0];
    d.mark_order = pr->mark_order ? (const uint32_t *)dev[1] : nullptr;
    d.mark_read = (const uint32_t *)dev[2];
    d.mark_name = (const uint32_t *)dev[3];
    d.pred = nullptr;
    d.ps = (const uint32_t *)dev[5];
    d.cand_contig = pr->cand_contig ? (const uint16_t *)dev[6] : nullptr;
    d.read_tag = (const uint64_t *)dev[7];
    return plan(ctx, &d, cand_mask ? (const uint8_t *)dev[4] : nullptr, out_tag, out_index, info, s, true);
}

int duet_sv_tags_apply_device(duet_ctx *ctx, const uint8_t *pred, uint32_t min_votes, uint32_t pc_new, uint64_t *out_tag, uint32_t *out_counts,
                              void *stream_)
{
    int rc = check_apply_args(ctx, pred, min_votes, pc_new, out_tag, out_counts);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return apply(ctx, pred, min_votes, pc_new, out_tag, out_counts, (hipStream_t)stream_);
}

int duet_sv_tags_apply_host(duet_ctx *ctx, const uint8_t *pred, uint32_t min_votes, uint32_t pc_new, uint64_t *out_tag, uint32_t *out_counts)
{
    int rc = check_apply_args(ctx, pred, min_votes, pc_new, out_tag, out_counts);
    if (rc) return rc;                                           // (refused: nothing is written, the counters neither)
    const size_t C = ctx->svplan.C, M = ctx->svplan.M;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->own_stream;
    // staging 8-10: pred, the words, the counters
    const void *src[3] = {pred, out_tag, nullptr};
    const size_t bytes[3] = {C && M ? C : 0, C && M ? M * 8 : 0, 0};
    void *dev[3];
    if ((rc = duet_stage_arrays(ctx, ctx->svplan_in.b + 8, src, bytes, 3, s, dev))) return rc;
    if ((rc = apply(ctx, (const uint8_t *)dev[0], min_votes, pc_new, (uint64_t *)dev[1], (uint32_t *)dev[2], s))) return rc;
    if (bytes[1]) HIP_TRY(ctx, hipMemcpyAsync(out_tag, dev[1], bytes[1], hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(out_counts, dev[2], 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return DUET_OK;
}

}  // extern "C"
