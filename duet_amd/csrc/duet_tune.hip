// duet_tune.hip -- threshold sweep: per-candidate feature export and the T1-T5 tree of predict_hp
// (src/duet/sv_phasing_fn.py:142-183) applied with K threshold vectors at once, scored against a prepared truth set
// (the counts of src/scripts/evaluation.py:99-159).  ABI and conventions: include/duet_ef.h, "Threshold sweep".
//
//   tune_features   one wavefront per candidate: filter (:189-190), PS-class (:191-194), vote (:70-111) against the seed sets
//                   the E/F kernels of the same context left behind (duet_ef.hip; not changed by this file)
//   tune_decide     a tile of 256 candidates per workgroup, its features read once, then 32 vectors applied to it; the
//                   counts go out through integer atomics (wave-aggregated) and per-vector bit sets of truth ids and of
//                   (phase-set group, truth id) pairs
//   tune_groups     per (vector, group): the "same" / "flip" choice of :143-148 and the union of the chosen truth ids
//   tune_popcount   per vector: the sizes of the three truth-id sets
//   tune_strata_of, tune_decide_strata, tune_groups_strata, tune_popcount_strata
//                   strata (include/duet_ef.h: duet_tune_strata): every candidate's and group's stratum from its CHROM id, and
//                   the three scoring kernels with one count record per (vector, stratum)
#include "duet_internal.h"

#include <cmath>
#include <cstring>

namespace {

int fail(duet_ctx *ctx, int code, const char *msg) { return duet_fail(ctx, code, msg); }

#include "duet_tune_feat.hip.h"            // FeatArgs, features_body(): the feature record (shared with duet_tune_cap.hip)

// the seed source of tune_features: the reference's cap, and what the E/F kernels of the same context left in their workspace
struct EfSeeds {
    static constexpr bool kSeedPass = false;
    __device__ __forceinline__ uint32_t cap() const { return DUET_PC_MAX; }
    __device__ __forceinline__ uint32_t count(const FeatArgs &a, uint32_t k) const { return a.n_one[k]; }
    __device__ __forceinline__ const uint32_t *seeds(const FeatArgs &a, uint32_t k) const { return a.onebuf + a.ctg_off[k] + k + 1; }
    __device__ __forceinline__ void div_zero() const {}          // (E/F's own status word reports it: duet_ef_check)
};

__global__ __launch_bounds__(64) void tune_features(const FeatArgs a) { features_body(a, EfSeeds{}); }

#include "duet_tune_sweep.hip.h"           // decide_vec, stage_vectors, load_candidate, SweepWs, sweep_batch, stage_truth

struct SweepArgs {
    const duet_tune_feature *feat;
    uint32_t C, v0, nv;                  // this batch: vectors v0 .. v0 + nv
    const duet_tune_thresholds *vec;
    duet_tune_counts *counts;            // [K]
    uint8_t *out_pred;                   // [K * C] or null
    uint32_t *out_ps;                    // [C] or null (written by the first batch)
    // truth (has_truth)
    int has_truth;
    const uint16_t *flags;
    const uint32_t *group, *uid, *pair, *group_pair_off, *pair_uid;
    SweepWs ws;                          // of the batch
};

__device__ __forceinline__ void set_bit(uint32_t *w, uint32_t i)
{
    const uint32_t m = 1u << (i & 31);
    if (!(__atomic_load_n(&w[i >> 5], __ATOMIC_RELAXED) & m)) atomicOr(&w[i >> 5], m);
}

// lane 0 of the wave adds the wave's count of `pred` to *dst
__device__ __forceinline__ void wave_count(uint32_t *dst, bool pred)
{
    const uint64_t bal = __ballot(pred);
    if (bal && (threadIdx.x & 63) == __ffsll((unsigned long long)bal) - 1) atomicAdd(dst, (uint32_t)__popcll(bal));
}

__global__ __launch_bounds__(256) void tune_decide(const SweepArgs a)
{
    __shared__ duet_tune_thresholds s_t[kVecPerBlock];
    uint32_t vb0;
    const uint32_t nvb = stage_vectors(s_t, a.vec + a.v0, a.nv, &vb0);
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    const bool live = c < a.C;
    duet_tune_feature f;
    bool elig;
    const Derived d = load_candidate(a.feat, a.C, c, &f, &elig);
    if (a.out_ps && live && a.v0 == 0 && blockIdx.y == 0) a.out_ps[c] = elig ? f.ps : 0u;
    uint16_t fl = 0;
    uint32_t g = 0, u = 0, pr = 0;
    if (a.has_truth && elig) {
        fl = a.flags[c];
        if (fl & DUET_TUNE_IN_CALLS) g = a.group[c];
        if (fl & DUET_TUNE_MATCHED) { u = a.uid[c]; pr = a.pair[c]; }
    }
    for (uint32_t j = 0; j < nvb; ++j) {
        const uint32_t vb = vb0 + j, v = a.v0 + vb;
        const uint32_t pred = elig ? decide_vec(d, s_t[j]) : 0u;
        if (a.out_pred && live) a.out_pred[(size_t)v * a.C + c] = (uint8_t)pred;
        if (!a.counts) continue;
        duet_tune_counts *cnt = a.counts + v;
        if (!a.has_truth) {
            wave_count(&cnt->n_calls, pred != 0);
            continue;
        }
        const bool call = pred != 0 && (fl & DUET_TUNE_IN_CALLS);
        if (!__any(call)) continue;
        wave_count(&cnt->n_calls, call);
        wave_count(&cnt->n_raise, call && (fl & DUET_TUNE_RAISES));
        uint32_t *gcnt = a.ws.gcnt(vb), *tp = a.ws.tp(vb), *gt = a.ws.gt(vb), *same = a.ws.same(vb), *flip = a.ws.flip(vb);
        if (call) set_bit(gcnt + 3ull * g, 0);
        const bool hit = call && (fl & DUET_TUNE_MATCHED);
        wave_count(&cnt->call_tp, hit);
        const uint32_t hb = hit ? (uint32_t)(fl >> (3 * (pred - 1))) & 7u : 0u;
        wave_count(&cnt->call_gt, hb & 1u);
        if (hit) {
            set_bit(tp, u);
            if (hb & 1u) set_bit(gt, u);
            if (hb & 2u) { atomicAdd(gcnt + 3ull * g + 1, 1u); set_bit(same, pr); }
            if (hb & 4u) { atomicAdd(gcnt + 3ull * g + 2, 1u); set_bit(flip, pr); }
        }
    }
}

// per (vector, group): the labelling with more call ids plus truth ids, ties to "flip" (:143-148); its truth ids into the hp set
__global__ __launch_bounds__(256) void tune_groups(const SweepArgs a)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x, vb = blockIdx.y;
    const bool live = g < a.ws.n_groups;
    uint32_t *gcnt = a.ws.gcnt(vb), *hp = a.ws.hp(vb), *same = a.ws.same(vb), *flip = a.ws.flip(vb);
    duet_tune_counts *cnt = a.counts + a.v0 + vb;
    const bool present = live && gcnt[3ull * g] != 0;
    wave_count(&cnt->n_groups, present);
    uint32_t take_c = 0;
    if (present) {
        const uint32_t p0 = a.group_pair_off[g], p1 = a.group_pair_off[g + 1];
        uint32_t sb = 0, fb = 0;
        for (uint32_t p = p0; p < p1; ++p) {
            sb += (same[p >> 5] >> (p & 31)) & 1u;
            fb += (flip[p >> 5] >> (p & 31)) & 1u;
        }
        const uint32_t sc = gcnt[3ull * g + 1], fc = gcnt[3ull * g + 2];
        const bool take_same = (uint64_t)sc + sb > (uint64_t)fc + fb;
        const uint32_t *bits = take_same ? same : flip;
        take_c = take_same ? sc : fc;
        for (uint32_t p = p0; p < p1; ++p)
            if ((bits[p >> 5] >> (p & 31)) & 1u) set_bit(hp, a.pair_uid[p]);
    }
    take_c = wave_sum(take_c);
    if ((threadIdx.x & 63) == 0 && take_c) atomicAdd(&cnt->call_hp, take_c);
}

__global__ __launch_bounds__(256) void tune_popcount(const SweepArgs a)
{
    const uint32_t w = blockIdx.x * 256u + threadIdx.x, vb = blockIdx.y;
    const uint32_t *tp = a.ws.tp(vb);                            // (gt and hp follow it, uw words each)
    uint32_t n[3] = {0, 0, 0};
    if (w < a.ws.uw)
        for (int s = 0; s < 3; ++s) n[s] = (uint32_t)__popc(tp[(size_t)s * a.ws.uw + w]);
    duet_tune_counts *cnt = a.counts + a.v0 + vb;
    uint32_t *dst[3] = {&cnt->base_tp, &cnt->base_gt, &cnt->base_hp};
    for (int s = 0; s < 3; ++s) {
        const uint32_t t = wave_sum(n[s]);
        if ((threadIdx.x & 63) == 0 && t) atomicAdd(dst[s], t);
    }
}

// ---- strata (include/duet_ef.h: duet_tune_strata): the same three kernels with one count record per (vector, stratum) ----------
// A wavefront may hold calls (groups, id words) of several strata -- candidates are contig-major and a tile can cross a contig --
// so each kernel peels the distinct strata among its contributing lanes: the first such lane's stratum, the lanes that share it,
// one atomic per (wave, stratum, field), then those lanes are cleared.  A wave of one stratum goes through the loop once.

struct StrataArgs {
    uint32_t S;
    const uint8_t *cand_stratum, *group_stratum;
    uint32_t uid_off[DUET_TUNE_MAX_STRATA + 1];
};

// the lanes of `rem` that share the stratum of its first lane; *first = that lane, *s0 = its stratum
__device__ __forceinline__ uint64_t peel(uint64_t rem, bool in, uint32_t st, uint32_t *first, uint32_t *s0)
{
    *first = (uint32_t)__ffsll((unsigned long long)rem) - 1u;
    *s0 = __shfl(st, (int)*first);
    return __ballot(in && st == *s0);
}

__global__ __launch_bounds__(256) void tune_decide_strata(const SweepArgs a, const StrataArgs sa)
{
    __shared__ duet_tune_thresholds s_t[kVecPerBlock];
    uint32_t vb0;
    const uint32_t nvb = stage_vectors(s_t, a.vec + a.v0, a.nv, &vb0);
    const uint32_t c = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    duet_tune_feature f;
    bool elig;
    const Derived d = load_candidate(a.feat, a.C, c, &f, &elig);
    uint16_t fl = 0;
    uint32_t g = 0, u = 0, pr = 0, st = 0;
    if (elig) {
        fl = a.flags[c];
        if (fl & DUET_TUNE_IN_CALLS) { g = a.group[c]; st = sa.cand_stratum[c]; }
        if (fl & DUET_TUNE_MATCHED) { u = a.uid[c]; pr = a.pair[c]; }
    }
    if (!__any((fl & DUET_TUNE_IN_CALLS) != 0)) return;          // (after the only barrier) no vector can make a call of this wave
    for (uint32_t j = 0; j < nvb; ++j) {
        const uint32_t vb = vb0 + j;
        const uint32_t pred = elig ? decide_vec(d, s_t[j]) : 0u;
        const bool call = pred != 0 && (fl & DUET_TUNE_IN_CALLS);
        uint64_t rem = __ballot(call);
        if (!rem) continue;
        const bool hit = call && (fl & DUET_TUNE_MATCHED);
        const uint32_t hb = hit ? (uint32_t)(fl >> (3 * (pred - 1))) & 7u : 0u;
        const uint64_t b_raise = __ballot(call && (fl & DUET_TUNE_RAISES)), b_hit = __ballot(hit), b_gt = __ballot(hb & 1u);
        duet_tune_counts *row = a.counts + (size_t)(a.v0 + vb) * sa.S;
        while (rem) {
            uint32_t first, s0;
            const uint64_t m = peel(rem, call, st, &first, &s0);
            if (lane == first) {
                duet_tune_counts *cnt = row + s0;
                atomicAdd(&cnt->n_calls, (uint32_t)__popcll(m));
                if (m & b_raise) atomicAdd(&cnt->n_raise, (uint32_t)__popcll(m & b_raise));
                if (m & b_hit) atomicAdd(&cnt->call_tp, (uint32_t)__popcll(m & b_hit));
                if (m & b_gt) atomicAdd(&cnt->call_gt, (uint32_t)__popcll(m & b_gt));
            }
            rem &= ~m;
        }
        uint32_t *gcnt = a.ws.gcnt(vb), *tp = a.ws.tp(vb), *gt = a.ws.gt(vb), *same = a.ws.same(vb), *flip = a.ws.flip(vb);
        if (call) set_bit(gcnt + 3ull * g, 0);
        if (hit) {
            set_bit(tp, u);
            if (hb & 1u) set_bit(gt, u);
            if (hb & 2u) { atomicAdd(gcnt + 3ull * g + 1, 1u); set_bit(same, pr); }
            if (hb & 4u) { atomicAdd(gcnt + 3ull * g + 2, 1u); set_bit(flip, pr); }
        }
    }
}

__global__ __launch_bounds__(256) void tune_groups_strata(const SweepArgs a, const StrataArgs sa)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x, vb = blockIdx.y, lane = threadIdx.x & 63u;
    const bool live = g < a.ws.n_groups;
    uint32_t *gcnt = a.ws.gcnt(vb), *hp = a.ws.hp(vb), *same = a.ws.same(vb), *flip = a.ws.flip(vb);
    const bool present = live && gcnt[3ull * g] != 0;
    uint32_t take_c = 0, st = 0;
    if (present) {
        st = sa.group_stratum[g];
        const uint32_t p0 = a.group_pair_off[g], p1 = a.group_pair_off[g + 1];
        uint32_t sb = 0, fb = 0;
        for (uint32_t p = p0; p < p1; ++p) {
            sb += (same[p >> 5] >> (p & 31)) & 1u;
            fb += (flip[p >> 5] >> (p & 31)) & 1u;
        }
        const uint32_t sc = gcnt[3ull * g + 1], fc = gcnt[3ull * g + 2];
        const bool take_same = (uint64_t)sc + sb > (uint64_t)fc + fb;
        const uint32_t *bits = take_same ? same : flip;
        take_c = take_same ? sc : fc;
        for (uint32_t p = p0; p < p1; ++p)
            if ((bits[p >> 5] >> (p & 31)) & 1u) set_bit(hp, a.pair_uid[p]);
    }
    duet_tune_counts *row = a.counts + (size_t)(a.v0 + vb) * sa.S;
    uint64_t rem = __ballot(present);
    while (rem) {
        uint32_t first, s0;
        const uint64_t m = peel(rem, present, st, &first, &s0);
        const uint32_t t = wave_sum((m >> lane) & 1ull ? take_c : 0u);
        if (lane == first) {
            atomicAdd(&row[s0].n_groups, (uint32_t)__popcll(m));
            if (t) atomicAdd(&row[s0].call_hp, t);
        }
        rem &= ~m;
    }
}

// a 32-bit word of the id sets belongs to one stratum (uid_off is word-aligned): the one whose range holds the word's first id
__global__ __launch_bounds__(256) void tune_popcount_strata(const SweepArgs a, const StrataArgs sa)
{
    __shared__ uint32_t s_off[DUET_TUNE_MAX_STRATA + 1];
    if (threadIdx.x <= sa.S) s_off[threadIdx.x] = sa.uid_off[threadIdx.x];
    __syncthreads();
    const uint32_t w = blockIdx.x * 256u + threadIdx.x, vb = blockIdx.y, lane = threadIdx.x & 63u;
    const uint32_t *tp = a.ws.tp(vb);                            // (gt and hp follow it, uw words each)
    uint32_t n[3] = {0, 0, 0}, st = 0;
    if (w < a.ws.uw) {
        for (int s = 0; s < 3; ++s) n[s] = (uint32_t)__popc(tp[(size_t)s * a.ws.uw + w]);
        if (n[0] | n[1] | n[2]) {
            uint32_t lo = 0, hi = sa.S - 1;                      // the first stratum whose range ends behind id 32 w
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s_off[mid + 1] > 32u * w) hi = mid; else lo = mid + 1;
            }
            st = lo;
        }
    }
    const bool some = (n[0] | n[1] | n[2]) != 0;
    duet_tune_counts *row = a.counts + (size_t)(a.v0 + vb) * sa.S;
    uint64_t rem = __ballot(some);
    while (rem) {
        uint32_t first, s0;
        const uint64_t m = peel(rem, some, st, &first, &s0);
        const bool mine = (m >> lane) & 1ull;
        uint32_t *dst[3] = {&row[s0].base_tp, &row[s0].base_gt, &row[s0].base_hp};
        for (int s = 0; s < 3; ++s) {
            const uint32_t t = wave_sum(mine ? n[s] : 0u);
            if (lane == first && t) atomicAdd(dst[s], t);
        }
        rem &= ~m;
    }
}

// duet_tune_strata_build_*: the stratum of every candidate and, through the calls, of every phase-set group.  All calls of a
// group share a CHROM id, so the lanes that write one group_stratum entry write the same value.
struct StrataBuildArgs {
    uint32_t C, n_chrom, n_contigs, S;
    const uint32_t *cand_chrom;             // per-candidate form, else null and ...
    const uint16_t *cand_contig;            // ... the table form
    const uint32_t *chrom_id;
    const uint16_t *flags;
    const uint32_t *group;
    const uint8_t *chrom_stratum;
    uint8_t *cand_stratum, *group_stratum;
    uint32_t *status;                       // set to 1 by an id or a stratum out of range
};

__global__ __launch_bounds__(256) void tune_strata_of(const StrataBuildArgs a)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= a.C) return;
    const bool call = (a.flags[c] & DUET_TUNE_IN_CALLS) != 0;
    uint32_t id = 0, st = 0;
    bool ok = true;
    if (a.cand_chrom) {
        id = a.cand_chrom[c];
    } else {
        const uint32_t k = a.cand_contig[c];
        ok = k < a.n_contigs;               // (duet_tune_truth_build_* drops such a candidate: it is no call)
        if (ok) id = a.chrom_id[k];
    }
    bool bad = ok && id >= a.n_chrom;
    if (ok && !bad) {
        st = a.chrom_stratum[id];
        bad = st >= a.S;
    }
    if (bad) { st = 0; atomicOr(a.status, 1u); }
    a.cand_stratum[c] = (uint8_t)st;
    if (call) a.group_stratum[a.group[c]] = (uint8_t)st;
}

int check_strata_build(duet_ctx *ctx, const duet_tune_truth_problem *pr, const duet_tune_truth *t, const uint8_t *chrom_stratum,
                       uint32_t n_strata, const uint8_t *cand_stratum, const uint8_t *group_stratum, bool *table)
{
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    if (!pr || !t) return fail(ctx, DUET_ERR_INVALID, "null argument");
    if (n_strata == 0 || n_strata > DUET_TUNE_MAX_STRATA) return fail(ctx, DUET_ERR_INVALID, "n_strata is 0 or above DUET_TUNE_MAX_STRATA");
    *table = !pr->cand_key && !pr->cand_chrom;
    if (pr->n_cands == 0) return DUET_OK;
    if (!chrom_stratum || !cand_stratum || !group_stratum || !t->cand_flags || !t->cand_group) return fail(ctx, DUET_ERR_INVALID, "null array");
    if (*table ? (!pr->cand_contig || (pr->n_contigs && !pr->chrom_id)) : !pr->cand_chrom)
        return fail(ctx, DUET_ERR_INVALID, "null CHROM id array");
    return DUET_OK;
}

int check_sweep_args(duet_ctx *ctx, const duet_tune_feature *feat, uint32_t n_cands, const duet_tune_thresholds *vec, uint32_t n_vec,
                     const duet_tune_truth *truth)
{
    if (n_cands && !feat) return fail(ctx, DUET_ERR_INVALID, "null feature array");
    if (n_vec && !vec) return fail(ctx, DUET_ERR_INVALID, "null threshold vectors");
    return check_truth_arrays(ctx, truth, n_cands);
}

// the truth arrays and the workspace layout of a sweep against `truth`
int set_truth(duet_ctx *ctx, const duet_tune_truth *truth, SweepArgs *a)
{
    a->has_truth = 1;
    a->flags = truth->cand_flags; a->group = truth->cand_group; a->uid = truth->cand_uid; a->pair = truth->cand_pair;
    a->group_pair_off = truth->group_pair_off; a->pair_uid = truth->pair_uid;
    if (!sweep_ws_of(truth, &a->ws)) return fail(ctx, DUET_ERR_INVALID, "truth set too large");
    return DUET_OK;
}

int check_strata(duet_ctx *ctx, const duet_tune_truth *truth, const duet_tune_strata *st, uint32_t n_cands)
{
    if (!truth || !st) return fail(ctx, DUET_ERR_INVALID, "the stratified sweep needs a truth set and its strata");
    const uint32_t S = st->n_strata;
    if (S == 0 || S > DUET_TUNE_MAX_STRATA) return fail(ctx, DUET_ERR_INVALID, "n_strata is 0 or above DUET_TUNE_MAX_STRATA");
    if (!st->uid_off) return fail(ctx, DUET_ERR_INVALID, "null uid_off");
    if (n_cands && (!st->cand_stratum || (truth->n_groups && !st->group_stratum))) return fail(ctx, DUET_ERR_INVALID, "null strata array");
    bool ok = st->uid_off[0] == 0 && st->uid_off[S] == truth->n_uid;
    for (uint32_t s = 0; s < S && ok; ++s) ok = st->uid_off[s + 1] >= st->uid_off[s] && st->uid_off[s + 1] % 32u == 0;
    if (!ok) return fail(ctx, DUET_ERR_INVALID, "uid_off: not 0 .. n_uid in nondecreasing multiples of 32");
    return DUET_OK;
}

// the truth arrays of a host run -> staging buffers 9 .. 14 of tune_ws
int stage_sweep_truth(duet_ctx *ctx, const duet_tune_truth *truth, size_t C, hipStream_t s, duet_tune_truth *dt)
{
    return stage_truth(ctx, truth, C, ((size_t)truth->n_groups + 1) * 4, (size_t)truth->n_pairs * 4, ctx->tune_ws.b + 9, s, dt);
}

}  // namespace

extern "C" {

int duet_ef_features_device(duet_ctx *ctx, const duet_ef_problem *pr, duet_tune_feature *out, void *stream_)
{
    if (!ctx || !pr) return fail(ctx, DUET_ERR_INVALID, "null argument");
    int rc = duet_ef_validate(ctx, pr);
    if (rc) return rc;
    const uint32_t C = pr->n_cands;
    if (C == 0) return DUET_OK;
    if (!out) return fail(ctx, DUET_ERR_INVALID, "null feature array");
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf *bp = &ctx->tune_ws.b[0], *bs = &ctx->tune_ws.b[1];
    if ((rc = duet_reserve(ctx, *bp, C)) || (rc = duet_reserve(ctx, *bs, (size_t)C * 4))) return rc;
    // E/F itself: the seed sets, and the status the caller gets back
    if ((rc = duet_ef_run_device(ctx, pr, (uint8_t *)bp->ptr, (uint32_t *)bs->ptr, stream))) return rc;
    if ((rc = duet_ef_materialise_seeds(ctx))) return rc;
    FeatArgs a;
    memset(&a, 0, sizeof(a));
    a.C = C; a.K = pr->n_contigs; a.n_reads = pr->n_reads;
    a.svlen_thres = pr->svlen_thres; a.suppread_thres = pr->suppread_thres;
    a.read_tag = pr->read_tag;
    a.cand_pos = pr->cand_pos; a.cand_svlen = pr->cand_svlen; a.cand_svread = pr->cand_svread;
    a.cand_refread = pr->cand_refread; a.cand_off = pr->cand_off; a.mark_read = pr->mark_read; a.cand_gt_ok = pr->cand_gt_ok;
    a.ctg_off = ctx->d_ctg_off; a.n_one = ctx->d_n_one; a.onebuf = (const uint32_t *)ctx->ws_one.ptr;
    a.out = out;
    const uint32_t grid = C < (1u << 20) ? C : (1u << 20);
    hipLaunchKernelGGL(tune_features, dim3(grid), dim3(64), 0, stream, a);
    HIP_TRY(ctx, hipGetLastError());
    return duet_ef_check(ctx, stream);
}

int duet_ef_features_host(duet_ctx *ctx, const duet_ef_problem *pr, duet_tune_feature *out)
{
    if (!ctx || !pr) return fail(ctx, DUET_ERR_INVALID, "null argument");
    int rc = duet_ef_validate(ctx, pr);
    if (rc) return rc;
    const uint32_t C = pr->n_cands;
    if (C == 0) return DUET_OK;
    if (!out) return fail(ctx, DUET_ERR_INVALID, "null feature array");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->own_stream;
    duet_ef_problem d;
    if ((rc = duet_ef_upload(ctx, pr, &d, s))) return rc;
    DevBuf *bf = &ctx->tune_ws.b[2];
    if ((rc = duet_reserve(ctx, *bf, (size_t)C * sizeof(duet_tune_feature)))) return rc;
    rc = duet_ef_features_device(ctx, &d, (duet_tune_feature *)bf->ptr, s);
    if (rc && rc != DUET_ERR_DIV_ZERO) return rc;
    const std::string msg = ctx->err;
    HIP_TRY(ctx, hipMemcpy(out, bf->ptr, (size_t)C * sizeof(duet_tune_feature), hipMemcpyDeviceToHost));
    if (rc) ctx->err = msg;
    return rc;
}

int duet_tune_sweep_device(duet_ctx *ctx, const duet_tune_feature *feat, uint32_t n_cands, const duet_tune_thresholds *vec,
                           uint32_t n_vec, const duet_tune_truth *truth, duet_tune_counts *counts, uint8_t *out_pred,
                           uint32_t *out_ps, void *stream_)
{
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    if (truth && n_vec && !counts) return fail(ctx, DUET_ERR_INVALID, "a truth set needs the counts array");
    int rc = check_sweep_args(ctx, feat, n_cands, vec, n_vec, truth);
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (counts && n_vec) HIP_TRY(ctx, hipMemsetAsync(counts, 0, (size_t)n_vec * sizeof(duet_tune_counts), stream));
    if (n_cands == 0 || (n_vec == 0 && !out_ps)) return DUET_OK;
    SweepArgs a;
    memset(&a, 0, sizeof(a));
    if (n_vec == 0) {                            // no vector: out_ps is still owed (one row of tune_decide, whose vector loop is empty)
        a.feat = feat; a.C = n_cands; a.out_ps = out_ps;
        hipLaunchKernelGGL(tune_decide, dim3((n_cands + 255) / 256, 1), dim3(256), 0, stream, a);
        HIP_TRY(ctx, hipGetLastError());
        return DUET_OK;
    }
    a.feat = feat; a.C = n_cands; a.vec = vec; a.counts = counts; a.out_pred = out_pred; a.out_ps = out_ps;
    if (truth && (rc = set_truth(ctx, truth, &a))) return rc;
    const size_t per_vec = a.ws.words;                           // (0 without a truth set: no workspace, no tune_groups, no tune_popcount)
    const uint32_t batch = sweep_batch(n_vec, a.ws.words);
    if (per_vec && (rc = duet_reserve(ctx, ctx->tune_ws.b[3], (size_t)batch * per_vec * 4))) return rc;
    a.ws.base = (uint32_t *)ctx->tune_ws.b[3].ptr;
    const uint32_t tiles = (n_cands + 255) / 256;
    for (uint32_t v0 = 0; v0 < n_vec; v0 += batch) {
        const uint32_t nv = n_vec - v0 < batch ? n_vec - v0 : batch;
        a.v0 = v0; a.nv = nv;
        if (per_vec) HIP_TRY(ctx, hipMemsetAsync(a.ws.base, 0, (size_t)nv * per_vec * 4, stream));
        hipLaunchKernelGGL(tune_decide, dim3(tiles, (nv + kVecPerBlock - 1) / kVecPerBlock), dim3(256), 0, stream, a);
        if (per_vec) {
            if (a.ws.n_groups) hipLaunchKernelGGL(tune_groups, dim3((a.ws.n_groups + 255) / 256, nv), dim3(256), 0, stream, a);
            if (a.ws.uw) hipLaunchKernelGGL(tune_popcount, dim3((a.ws.uw + 255) / 256, nv), dim3(256), 0, stream, a);
        }
        HIP_TRY(ctx, hipGetLastError());
    }
    return DUET_OK;
}

int duet_tune_sweep_host(duet_ctx *ctx, const duet_tune_feature *feat, uint32_t n_cands, const duet_tune_thresholds *vec,
                         uint32_t n_vec, const duet_tune_truth *truth, duet_tune_counts *counts, uint8_t *out_pred, uint32_t *out_ps)
{
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    if (n_cands && !feat) return fail(ctx, DUET_ERR_INVALID, "null feature array");
    if (n_vec && !vec) return fail(ctx, DUET_ERR_INVALID, "null threshold vectors");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->own_stream;
    DevBuf *B = ctx->tune_ws.b;
    const size_t C = n_cands, K = n_vec;
    int rc;
    // staging: 4 features, 5 vectors, 6 counts, 7 pred, 8 ps, 9.. truth arrays
    auto up = [&](int i, const void *src, size_t bytes) -> int {
        int r = duet_reserve(ctx, B[i], bytes ? bytes : 16);
        if (r) return r;
        if (bytes && src) HIP_TRY(ctx, hipMemcpyAsync(B[i].ptr, src, bytes, hipMemcpyHostToDevice, s));
        return DUET_OK;
    };
    if ((rc = up(4, feat, C * sizeof(duet_tune_feature))) || (rc = up(5, vec, K * sizeof(duet_tune_thresholds)))) return rc;
    if (counts && (rc = up(6, nullptr, K * sizeof(duet_tune_counts)))) return rc;
    if (out_pred && (rc = up(7, nullptr, K * C))) return rc;
    if (out_ps && (rc = up(8, nullptr, C * 4))) return rc;
    duet_tune_truth dt;
    if (truth && (rc = stage_sweep_truth(ctx, truth, C, s, &dt))) return rc;
    rc = duet_tune_sweep_device(ctx, (const duet_tune_feature *)B[4].ptr, n_cands, (const duet_tune_thresholds *)B[5].ptr, n_vec,
                                truth ? &dt : nullptr, counts ? (duet_tune_counts *)B[6].ptr : nullptr,
                                out_pred ? (uint8_t *)B[7].ptr : nullptr, out_ps ? (uint32_t *)B[8].ptr : nullptr, s);
    if (rc) return rc;
    if (counts && K) HIP_TRY(ctx, hipMemcpyAsync(counts, B[6].ptr, K * sizeof(duet_tune_counts), hipMemcpyDeviceToHost, s));
    if (out_pred && K * C) HIP_TRY(ctx, hipMemcpyAsync(out_pred, B[7].ptr, K * C, hipMemcpyDeviceToHost, s));
    if (out_ps && C) HIP_TRY(ctx, hipMemcpyAsync(out_ps, B[8].ptr, C * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return DUET_OK;
}

int duet_tune_sweep_strata_device(duet_ctx *ctx, const duet_tune_feature *feat, uint32_t n_cands, const duet_tune_thresholds *vec,
                                  uint32_t n_vec, const duet_tune_truth *truth, const duet_tune_strata *strata,
                                  duet_tune_counts *counts, void *stream_)
{
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    int rc = check_strata(ctx, truth, strata, n_cands);
    if (rc || (rc = check_sweep_args(ctx, feat, n_cands, vec, n_vec, truth))) return rc;
    if (n_vec && !counts) return fail(ctx, DUET_ERR_INVALID, "null counts array");
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t S = strata->n_strata;
    if (n_vec) HIP_TRY(ctx, hipMemsetAsync(counts, 0, (size_t)n_vec * S * sizeof(duet_tune_counts), stream));
    if (n_cands == 0 || n_vec == 0) return DUET_OK;
    SweepArgs a;
    memset(&a, 0, sizeof(a));
    a.feat = feat; a.C = n_cands; a.vec = vec; a.counts = counts;
    if ((rc = set_truth(ctx, truth, &a))) return rc;     // (uid_off[S] == n_uid is a multiple of 32: the id sets have n_uid / 32 words)
    const size_t per_vec = a.ws.words;
    StrataArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.S = S; sa.cand_stratum = strata->cand_stratum; sa.group_stratum = strata->group_stratum;
    memcpy(sa.uid_off, strata->uid_off, ((size_t)S + 1) * 4);
    const uint32_t batch = sweep_batch(n_vec, a.ws.words);      // (the batches of duet_tune_sweep_device with a truth set)
    if ((rc = duet_reserve(ctx, ctx->tune_ws.b[3], (size_t)batch * per_vec * 4))) return rc;
    a.ws.base = (uint32_t *)ctx->tune_ws.b[3].ptr;
    const uint32_t tiles = (n_cands + 255) / 256;
    for (uint32_t v0 = 0; v0 < n_vec; v0 += batch) {
        const uint32_t nv = n_vec - v0 < batch ? n_vec - v0 : batch;
        a.v0 = v0; a.nv = nv;
        HIP_TRY(ctx, hipMemsetAsync(a.ws.base, 0, (size_t)nv * per_vec * 4, stream));
        hipLaunchKernelGGL(tune_decide_strata, dim3(tiles, (nv + kVecPerBlock - 1) / kVecPerBlock), dim3(256), 0, stream, a, sa);
        if (a.ws.n_groups) hipLaunchKernelGGL(tune_groups_strata, dim3((a.ws.n_groups + 255) / 256, nv), dim3(256), 0, stream, a, sa);
        if (a.ws.uw) hipLaunchKernelGGL(tune_popcount_strata, dim3((a.ws.uw + 255) / 256, nv), dim3(256), 0, stream, a, sa);
        HIP_TRY(ctx, hipGetLastError());
    }
    return DUET_OK;
}

int duet_tune_sweep_strata_host(duet_ctx *ctx, const duet_tune_feature *feat, uint32_t n_cands, const duet_tune_thresholds *vec,
                                uint32_t n_vec, const duet_tune_truth *truth, const duet_tune_strata *strata, duet_tune_counts *counts)
{
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    int rc = check_strata(ctx, truth, strata, n_cands);
    if (rc || (rc = check_sweep_args(ctx, feat, n_cands, vec, n_vec, truth))) return rc;
    if (n_vec && !counts) return fail(ctx, DUET_ERR_INVALID, "null counts array");
    const size_t C = n_cands, K = n_vec, S = strata->n_strata;
    for (size_t c = 0; c < C; ++c)                       // the host form can read them: no record index past the counts
        if ((truth->cand_flags[c] & DUET_TUNE_IN_CALLS) &&
            (strata->cand_stratum[c] >= S || truth->cand_group[c] >= truth->n_groups || strata->group_stratum[truth->cand_group[c]] >= S))
            return fail(ctx, DUET_ERR_INVALID, "a stratum of a call or of its group is not below n_strata");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->own_stream;
    DevBuf *B = ctx->tune_ws.b;
    // staging as in duet_tune_sweep_host: 4 features, 5 vectors, 6 counts, 9.. truth arrays; the strata arrays in tune_strata_ws 0, 1
    const void *src[3] = {feat, vec, nullptr};
    const size_t bytes[3] = {C * sizeof(duet_tune_feature), K * sizeof(duet_tune_thresholds), K * S * sizeof(duet_tune_counts)};
    void *dev[3];
    if ((rc = duet_stage_arrays(ctx, B + 4, src, bytes, 2, s, dev)) || (rc = duet_reserve(ctx, B[6], bytes[2] + 64))) return rc;
    duet_tune_truth dt;
    if ((rc = stage_sweep_truth(ctx, truth, C, s, &dt))) return rc;
    const void *ssrc[2] = {strata->cand_stratum, strata->group_stratum};
    const size_t sbytes[2] = {C, C ? (size_t)truth->n_groups : 0};
    void *sdev[2];
    if ((rc = duet_stage_arrays(ctx, ctx->tune_strata_ws.b, ssrc, sbytes, 2, s, sdev))) return rc;
    duet_tune_strata ds = *strata;
    ds.cand_stratum = (const uint8_t *)sdev[0]; ds.group_stratum = (const uint8_t *)sdev[1];
    if ((rc = duet_tune_sweep_strata_device(ctx, (const duet_tune_feature *)dev[0], n_cands, (const duet_tune_thresholds *)dev[1], n_vec,
                                            &dt, &ds, (duet_tune_counts *)B[6].ptr, s)))
        return rc;
    if (bytes[2]) HIP_TRY(ctx, hipMemcpyAsync(counts, B[6].ptr, bytes[2], hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return DUET_OK;
}

int duet_tune_strata_build_device(duet_ctx *ctx, const duet_tune_truth_problem *pr, const duet_tune_truth *t, const uint8_t *chrom_stratum,
                                  uint32_t n_strata, uint8_t *cand_stratum, uint8_t *group_stratum, void *stream_)
{
    bool table = false;
    int rc = check_strata_build(ctx, pr, t, chrom_stratum, n_strata, cand_stratum, group_stratum, &table);
    if (rc || pr->n_cands == 0) return rc;
    hipStream_t st = (hipStream_t)stream_;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf &sw = ctx->tune_strata_ws.b[2];
    if ((rc = duet_reserve(ctx, sw, 64))) return rc;
    StrataBuildArgs a;
    memset(&a, 0, sizeof(a));
    a.C = pr->n_cands; a.n_chrom = pr->n_chrom; a.n_contigs = pr->n_contigs; a.S = n_strata;
    a.cand_chrom = table ? nullptr : pr->cand_chrom; a.cand_contig = pr->cand_contig; a.chrom_id = pr->chrom_id;
    a.flags = t->cand_flags; a.group = t->cand_group;
    a.chrom_stratum = chrom_stratum; a.cand_stratum = cand_stratum; a.group_stratum = group_stratum;
    a.status = (uint32_t *)sw.ptr;
    HIP_TRY(ctx, hipMemsetAsync(a.status, 0, 4, st));
    hipLaunchKernelGGL(tune_strata_of, dim3((a.C + 255) / 256), dim3(256), 0, st, a);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t status = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&status, a.status, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (status) return fail(ctx, DUET_ERR_INVALID, "a chrom_stratum entry is not below n_strata, or a CHROM id not below n_chrom");
    return DUET_OK;
}

int duet_tune_strata_build_host(duet_ctx *ctx, const duet_tune_truth_problem *pr, const duet_tune_truth *t, const uint8_t *chrom_stratum,
                                uint32_t n_strata, uint8_t *cand_stratum, uint8_t *group_stratum)
{
    bool table = false;
    int rc = check_strata_build(ctx, pr, t, chrom_stratum, n_strata, cand_stratum, group_stratum, &table);
    if (rc || pr->n_cands == 0) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->own_stream;
    const size_t C = pr->n_cands, G = t->n_groups;
    if (G > C) return fail(ctx, DUET_ERR_INVALID, "more groups than candidates");
    for (size_t c = 0; c < C; ++c)                       // group_stratum has room for C entries: no group index past it
        if ((t->cand_flags[c] & DUET_TUNE_IN_CALLS) && t->cand_group[c] >= C) return fail(ctx, DUET_ERR_INVALID, "a group index is not below n_cands");
    const void *src[6] = {table ? nullptr : pr->cand_chrom, table ? pr->cand_contig : nullptr, table ? pr->chrom_id : nullptr,
                          t->cand_flags, t->cand_group, chrom_stratum};
    const size_t bytes[6] = {table ? 0 : C * 4, table ? C * 2 : 0, table ? (size_t)pr->n_contigs * 4 : 0, C * 2, C * 4, pr->n_chrom};
    void *dev[6];
    DevBuf *B = ctx->tune_strata_ws.b;
    if ((rc = duet_stage_arrays(ctx, B + 3, src, bytes, 6, s, dev)) || (rc = duet_reserve(ctx, B[0], C + 64)) || (rc = duet_reserve(ctx, B[1], C + 64)))
        return rc;
    duet_tune_truth_problem d = *pr;
    d.cand_chrom = table ? nullptr : (const uint32_t *)dev[0]; d.cand_key = d.cand_chrom;       // (only their being null or not is read)
    d.cand_contig = (const uint16_t *)dev[1]; d.chrom_id = (const uint32_t *)dev[2];
    duet_tune_truth dt = *t;
    dt.cand_flags = (const uint16_t *)dev[3]; dt.cand_group = (const uint32_t *)dev[4];
    if ((rc = duet_tune_strata_build_device(ctx, &d, &dt, (const uint8_t *)dev[5], n_strata, (uint8_t *)B[0].ptr, (uint8_t *)B[1].ptr, s))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(cand_stratum, B[0].ptr, C, hipMemcpyDeviceToHost, s));
    if (G) HIP_TRY(ctx, hipMemcpyAsync(group_stratum, B[1].ptr, G, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return DUET_OK;
}

}  // extern "C"
