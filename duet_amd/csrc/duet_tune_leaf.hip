// duet_tune_leaf.hip -- the leaf census of the threshold sweep: per (vector, stratum, leaf of the T1-T5 tree) how many eligible
// candidates end there, how many of them the evaluator lists and matches, and what the calls among them score
// (include/duet_ef.h, "Leaf census").  The tree is decide_vec's (duet_tune.hip), restated with its 18 exits numbered.
//
//   (duet_tune_sweep_device)   per batch of vectors the plain sweep runs into a scratch count array: it leaves the per-group
//                              counters and the same / flip pair bit sets of every vector of the batch in its workspace
//   tune_leaf_labels           per (vector, group): the labelling tune_groups takes (sc + sb > fc + fb, ties to flip), one bit
//   tune_leaf_census           a tile of 256 candidates per workgroup, its features read and derived once, then 32 vectors from
//                              LDS; per vector every lane's (stratum, leaf) key and verdict bits, the distinct keys of the wave
//                              peeled as the strata kernels peel strata: one integer atomic per (wave, key, non-zero field)
#include "duet_internal.h"

#include <cmath>
#include <cstring>

namespace {

constexpr int kVecPerBlock = 32;                  // tune_leaf_census: vectors applied to one tile of candidates
constexpr size_t kWsBudget = (size_t)256 << 20;   // the sweep's workspace budget per batch of vectors (duet_tune.hip)
constexpr uint32_t kLeaves = DUET_TUNE_N_LEAVES;

int fail(duet_ctx *ctx, int code, const char *msg) { return duet_fail(ctx, code, msg); }

#include "duet_tune_derive.hip.h"          // Derived, derive(): what the tree compares

// decide_vec (duet_tune.hip) with its exits numbered: a comparison that is false takes the else branch, for a nan constant too
__device__ __forceinline__ uint32_t leaf_of(const Derived &d, const duet_tune_thresholds &t, uint32_t *pred)
{
    uint32_t leaf, p = 0;
    if (d.cls == 0) {
        if (d.sv_ratio == 1.0 && d.svread >= t.c0_min_sv_num) { leaf = 0; p = 3; }
        else leaf = 1;
    } else if (d.cls == 2) {
        if (d.sv_ratio >= t.c2_min_sv_ratio) {
            if (d.diff <= t.c2_max_avgsc_diff) {
                if (d.svread >= t.c2_min_sv_num) { leaf = 3; p = 3; }
                else leaf = 4;
            } else {
                if (d.hap0 >= t.c2_min_hap0) { leaf = 5; p = 3; }
                else leaf = 6;
            }
        } else leaf = 2;
    } else {
        const bool gate = (d.hr <= t.c1_hapread_ratio && d.diff <= t.c1_max_avgsc_diff) || d.hr > t.c1_hapread_ratio;
        if (d.onehap) {
            if (d.sv_ratio <= t.c1_onehap_sv_ratio_lo) leaf = 7;
            else if (d.sv_ratio <= t.c1_onehap_sv_ratio_hi) {
                if (gate) { leaf = 8; p = d.a1pos ? 1 : 2; }
                else leaf = 9;
            } else {
                if (gate) { leaf = 10; p = 3; }
                else leaf = 11;
            }
        } else {
            if (d.sv_ratio <= t.c1_twohap_sv_ratio_1) leaf = 12;
            else if (d.sv_ratio <= t.c1_twohap_sv_ratio_2) {
                if (d.refread > t.c1_max_ref_num) leaf = 13;
                else { leaf = 14; p = d.t1gt ? 1 : 2; }
            } else if (d.sv_ratio <= t.c1_twohap_sv_ratio_3) {
                if (d.totsc <= t.c1_max_totsc_ratio) { leaf = 15; p = 3; }
                else { leaf = 16; p = d.t1gt ? 1 : 2; }
            } else { leaf = 17; p = 3; }
        }
    }
    *pred = p;
    return leaf;
}

// the sweep's workspace of one batch (duet_tune.hip, SweepArgs): per vector gcnt[3 * n_groups] (present, same calls, flip calls),
// three id sets of uw words, the same and the flip pair sets of pw words
struct LabelArgs {
    const uint32_t *ws;
    uint32_t ws_words, n_groups, uw, pw;
    const uint32_t *group_pair_off;
    uint32_t *label;                     // [nv * lw]: bit g of a vector's words = group g takes "same"
    uint32_t lw;                         // 2 * ceil(n_groups / 64)
};

// per (vector, group): tune_groups' choice.  A wave holds 64 consecutive groups: its ballot is two label words.
__global__ __launch_bounds__(256) void tune_leaf_labels(const LabelArgs a)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x, vb = blockIdx.y;
    const uint32_t *ws = a.ws + (size_t)vb * a.ws_words;
    const uint32_t *gcnt = ws, *same = ws + 3ull * a.n_groups + 3ull * a.uw, *flip = same + a.pw;
    bool take_same = false;
    if (g < a.n_groups && gcnt[3ull * g] != 0) {
        const uint32_t p0 = a.group_pair_off[g], p1 = a.group_pair_off[g + 1];
        uint32_t sb = 0, fb = 0;
        for (uint32_t p = p0; p < p1; ++p) {
            sb += (same[p >> 5] >> (p & 31)) & 1u;
            fb += (flip[p >> 5] >> (p & 31)) & 1u;
        }
        take_same = (uint64_t)gcnt[3ull * g + 1] + sb > (uint64_t)gcnt[3ull * g + 2] + fb;
    }
    const uint64_t bal = __ballot(take_same);
    const uint32_t g0 = g & ~63u;                                 // the wave's first group
    if ((threadIdx.x & 63u) == 0 && g0 < a.n_groups) {            // (then (g0 >> 5) + 1 < lw)
        uint32_t *dst = a.label + (size_t)vb * a.lw + (g0 >> 5);
        dst[0] = (uint32_t)bal;
        dst[1] = (uint32_t)(bal >> 32);
    }
}

struct LeafArgs {
    const duet_tune_feature *feat;
    uint32_t C, v0, nv;                  // this batch: vectors v0 .. v0 + nv
    const duet_tune_thresholds *vec;
    duet_tune_leaf_counts *out;          // [K * S * 18]
    uint32_t S;
    const uint8_t *cand_stratum;         // or null: S == 1
    int has_truth;
    const uint16_t *flags;
    const uint32_t *group;
    const uint32_t *label;               // of this batch
    uint32_t lw;
};

__device__ __forceinline__ void add_masked(uint32_t *dst, uint64_t m)
{
    if (m) atomicAdd(dst, (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(256) void tune_leaf_census(const LeafArgs a)
{
    __shared__ duet_tune_thresholds s_t[kVecPerBlock];
    const uint32_t vb0 = blockIdx.y * kVecPerBlock;
    const uint32_t nvb = a.nv - vb0 < (uint32_t)kVecPerBlock ? a.nv - vb0 : (uint32_t)kVecPerBlock;
    {
        const double *src = (const double *)(a.vec + a.v0 + vb0);
        double *dst = (double *)s_t;
        for (uint32_t i = threadIdx.x; i < nvb * 14u; i += 256u) dst[i] = src[i];
    }
    __syncthreads();
    const uint32_t c = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    duet_tune_feature f;
    if (c < a.C) f = a.feat[c];
    else memset(&f, 0, sizeof(f));
    const bool elig = c < a.C && f.eligible;
    if (!elig) f.deg = 1;                                        // (no division by zero in derive for the lanes that never decide)
    const Derived d = derive(f);
    uint32_t fl = 0, g = 0, st = 0;
    if (elig) {
        if (a.cand_stratum) {
            st = a.cand_stratum[c];
            if (st >= a.S) st = 0;                               // (never a record index past the array)
        }
        if (a.has_truth) {
            fl = a.flags[c];
            if (fl & DUET_TUNE_IN_CALLS) g = a.group[c];
        }
    }
    const uint64_t b_elig = __ballot(elig);
    if (!b_elig) return;                                         // (after the only barrier) only eligible candidates reach the tree
    const bool listed = (fl & DUET_TUNE_IN_CALLS) != 0, matched = listed && (fl & DUET_TUNE_MATCHED);
    const bool callable = a.has_truth ? listed : elig;           // without a truth set: every emitted candidate is a call
    const uint64_t b_listed = __ballot(listed), b_matched = __ballot(matched);
    for (uint32_t j = 0; j < nvb; ++j) {
        const uint32_t vb = vb0 + j;
        uint32_t pred;
        const uint32_t key = st * kLeaves + leaf_of(d, s_t[j], &pred);
        const bool call = callable && pred != 0;
        const bool hit = call && matched;
        const uint32_t hb = hit ? (fl >> (3 * (pred - 1))) & 7u : 0u;
        bool hp = false;
        if (hb & 6u) {                                           // same or flip: does it agree with the group's label
            const uint32_t w = a.label[(size_t)vb * a.lw + (g >> 5)];
            hp = (hb & ((w >> (g & 31)) & 1u ? 2u : 4u)) != 0;
        }
        const uint64_t b_call = __ballot(call), b_raise = __ballot(call && (fl & DUET_TUNE_RAISES)), b_tp = __ballot(hit),
                       b_gt = __ballot((hb & 1u) != 0), b_hp = __ballot(hp);
        duet_tune_leaf_counts *row = a.out + (size_t)(a.v0 + vb) * a.S * kLeaves;
        uint64_t rem = b_elig;
        while (rem) {                                            // the distinct keys among the wave's eligible lanes
            const uint32_t first = (uint32_t)__ffsll((unsigned long long)rem) - 1u;
            const uint32_t k0 = __shfl(key, (int)first);
            const uint64_t m = __ballot(elig && key == k0);
            if (lane == first) {
                duet_tune_leaf_counts *r = row + k0;
                atomicAdd(&r->n_cands, (uint32_t)__popcll(m));
                add_masked(&r->n_listed, m & b_listed);
                add_masked(&r->n_matched, m & b_matched);
                add_masked(&r->n_calls, m & b_call);
                add_masked(&r->call_tp, m & b_tp);
                add_masked(&r->call_gt, m & b_gt);
                add_masked(&r->call_hp, m & b_hp);
                add_masked(&r->n_raise, m & b_raise);
            }
            rem &= ~m;
        }
    }
}

int check_args(duet_ctx *ctx, const duet_tune_feature *feat, uint32_t n_cands, const duet_tune_thresholds *vec, uint32_t n_vec,
               const duet_tune_truth *truth, const duet_tune_strata *strata, const duet_tune_leaf_counts *out)
{
    if (strata && (strata->n_strata == 0 || strata->n_strata > DUET_TUNE_MAX_STRATA))
        return fail(ctx, DUET_ERR_INVALID, "n_strata is 0 or above DUET_TUNE_MAX_STRATA");
    if (n_vec && !out) return fail(ctx, DUET_ERR_INVALID, "null leaf record array");
    if (n_cands && !feat) return fail(ctx, DUET_ERR_INVALID, "null feature array");
    if (n_vec && !vec) return fail(ctx, DUET_ERR_INVALID, "null threshold vectors");
    if (truth && n_cands && (!truth->cand_flags || !truth->cand_group || !truth->cand_uid || !truth->cand_pair ||
                             !truth->group_pair_off || (truth->n_pairs && !truth->pair_uid)))
        return fail(ctx, DUET_ERR_INVALID, "null truth array");
    if (strata && n_cands && !strata->cand_stratum) return fail(ctx, DUET_ERR_INVALID, "null strata array");
    return DUET_OK;
}

}  // namespace

extern "C" {

int duet_tune_leaf_census_device(duet_ctx *ctx, const duet_tune_feature *feat, uint32_t n_cands, const duet_tune_thresholds *vec,
                                 uint32_t n_vec, const duet_tune_truth *truth, const duet_tune_strata *strata,
                                 duet_tune_leaf_counts *out, void *stream_)
{
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    int rc = check_args(ctx, feat, n_cands, vec, n_vec, truth, strata, out);
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t S = strata ? strata->n_strata : 1u;
    if (n_vec) HIP_TRY(ctx, hipMemsetAsync(out, 0, (size_t)n_vec * S * kLeaves * sizeof(duet_tune_leaf_counts), stream));
    if (n_cands == 0 || n_vec == 0) return DUET_OK;
    LeafArgs a;
    memset(&a, 0, sizeof(a));
    a.feat = feat; a.C = n_cands; a.vec = vec; a.out = out; a.S = S;
    a.cand_stratum = strata ? strata->cand_stratum : nullptr;
    LabelArgs la;
    memset(&la, 0, sizeof(la));
    // the batches of duet_tune_sweep_device: what the workspace budget holds (at least one vector) and, with a truth set, at most
    // 65,535 vectors -- a batch of that size is one batch of the sweep too, so its workspace holds every vector of it afterwards
    uint32_t batch = n_vec;
    if (truth) {
        a.has_truth = 1;
        a.flags = truth->cand_flags; a.group = truth->cand_group;
        la.n_groups = truth->n_groups;
        la.uw = (truth->n_uid + 31) / 32;
        la.pw = (truth->n_pairs + 31) / 32;
        la.group_pair_off = truth->group_pair_off;
        const size_t per_vec = 3ull * truth->n_groups + 3ull * la.uw + 2ull * la.pw + 1;
        if (per_vec > 0xFFFFFFFFull) return fail(ctx, DUET_ERR_INVALID, "truth set too large");
        la.ws_words = (uint32_t)per_vec;
        la.lw = 2u * ((truth->n_groups + 63u) / 64u);
        const size_t fit = kWsBudget / (per_vec * 4);
        if (fit < batch) batch = fit ? (uint32_t)fit : 1u;
        if (batch > 65535u) batch = 65535u;
        DevBuf *B = ctx->tune_leaf_ws.b;
        if ((rc = duet_reserve(ctx, B[0], (size_t)batch * sizeof(duet_tune_counts))) ||
            (rc = duet_reserve(ctx, B[1], (size_t)batch * la.lw * 4 + 16)))
            return rc;
        la.label = (uint32_t *)B[1].ptr;
        a.label = la.label; a.lw = la.lw;
    }
    if (batch > 65535u * kVecPerBlock) batch = 65535u * kVecPerBlock;
    const uint32_t tiles = (n_cands + 255) / 256;
    for (uint32_t v0 = 0; v0 < n_vec; v0 += batch) {
        const uint32_t nv = n_vec - v0 < batch ? n_vec - v0 : batch;
        a.v0 = v0; a.nv = nv;
        if (truth && truth->n_groups) {
            if ((rc = duet_tune_sweep_device(ctx, feat, n_cands, vec + v0, nv, truth, (duet_tune_counts *)ctx->tune_leaf_ws.b[0].ptr,
                                             nullptr, nullptr, stream_)))
                return rc;
            la.ws = (const uint32_t *)ctx->tune_ws.b[3].ptr;     // (reserved by the sweep for this batch)
            hipLaunchKernelGGL(tune_leaf_labels, dim3((la.n_groups + 255) / 256, nv), dim3(256), 0, stream, la);
        }
        hipLaunchKernelGGL(tune_leaf_census, dim3(tiles, (nv + kVecPerBlock - 1) / kVecPerBlock), dim3(256), 0, stream, a);
        HIP_TRY(ctx, hipGetLastError());
    }
    return DUET_OK;
}

int duet_tune_leaf_census_host(duet_ctx *ctx, const duet_tune_feature *feat, uint32_t n_cands, const duet_tune_thresholds *vec,
                               uint32_t n_vec, const duet_tune_truth *truth, const duet_tune_strata *strata, duet_tune_leaf_counts *out)
{
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    int rc = check_args(ctx, feat, n_cands, vec, n_vec, truth, strata, out);
    if (rc) return rc;
    const size_t C = n_cands, K = n_vec, S = strata ? strata->n_strata : 1;
    if (strata)
        for (size_t c = 0; c < C; ++c)                       // the host form can read them: no record index past the array
            if (strata->cand_stratum[c] >= S) return fail(ctx, DUET_ERR_INVALID, "a cand_stratum entry is not below n_strata");
    if (truth)
        for (size_t c = 0; c < C; ++c)                       // ... and no label bit past the label words
            if ((truth->cand_flags[c] & DUET_TUNE_IN_CALLS) && truth->cand_group[c] >= truth->n_groups)
                return fail(ctx, DUET_ERR_INVALID, "a group index is not below n_groups");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->own_stream;
    // staging in tune_leaf_ws: 2 features, 3 vectors, 4 cand_stratum, 5 the records, 6 .. 11 the truth arrays
    DevBuf *B = ctx->tune_leaf_ws.b;
    const size_t out_bytes = K * S * kLeaves * sizeof(duet_tune_leaf_counts);
    const void *src[3] = {feat, vec, strata ? strata->cand_stratum : nullptr};
    const size_t bytes[3] = {C * sizeof(duet_tune_feature), K * sizeof(duet_tune_thresholds), strata ? C : 0};
    void *dev[3];
    if ((rc = duet_stage_arrays(ctx, B + 2, src, bytes, 3, s, dev)) || (rc = duet_reserve(ctx, B[5], out_bytes + 64))) return rc;
    duet_tune_truth dt;
    if (truth) {
        const void *tsrc[6] = {truth->cand_flags, truth->cand_group, truth->cand_uid, truth->cand_pair, truth->group_pair_off, truth->pair_uid};
        const size_t tbytes[6] = {C * 2, C * 4, C * 4, C * 4, C ? ((size_t)truth->n_groups + 1) * 4 : 0, C ? (size_t)truth->n_pairs * 4 : 0};
        void *tdev[6];
        if ((rc = duet_stage_arrays(ctx, B + 6, tsrc, tbytes, 6, s, tdev))) return rc;
        dt = *truth;
        dt.cand_flags = (const uint16_t *)tdev[0]; dt.cand_group = (const uint32_t *)tdev[1];
        dt.cand_uid = (const uint32_t *)tdev[2]; dt.cand_pair = (const uint32_t *)tdev[3];
        dt.group_pair_off = (const uint32_t *)tdev[4]; dt.pair_uid = (const uint32_t *)tdev[5];
    }
    duet_tune_strata ds;
    if (strata) {
        ds = *strata;
        ds.cand_stratum = (const uint8_t *)dev[2];
    }
    if ((rc = duet_tune_leaf_census_device(ctx, (const duet_tune_feature *)dev[0], n_cands, (const duet_tune_thresholds *)dev[1], n_vec,
                                           truth ? &dt : nullptr, strata ? &ds : nullptr, (duet_tune_leaf_counts *)B[5].ptr, s)))
        return rc;
    if (out_bytes) HIP_TRY(ctx, hipMemcpyAsync(out, B[5].ptr, out_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return DUET_OK;
}

}  // extern "C"
