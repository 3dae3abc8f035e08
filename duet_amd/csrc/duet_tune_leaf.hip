// duet_tune_leaf.hip -- the leaf census of the threshold sweep: per (vector, stratum, leaf of the T1-T5 tree) how many eligible
// candidates end there, how many of them the evaluator lists and matches, and what the calls among them score
// (include/duet_ef.h, "Leaf census").  The tree is the sweep's: leaf_of (duet_tune_sweep.hip.h), whose verdict decide_vec is.
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

constexpr uint32_t kLeaves = DUET_TUNE_N_LEAVES;

int fail(duet_ctx *ctx, int code, const char *msg) { return duet_fail(ctx, code, msg); }

#include "duet_tune_sweep.hip.h"           // leaf_of, stage_vectors, load_candidate, SweepWs, sweep_batch, stage_truth

struct LabelArgs {
    SweepWs ws;                          // what the sweep left behind for this batch
    const uint32_t *group_pair_off;
    uint32_t *label;                     // [nv * lw]: bit g of a vector's words = group g takes "same"
    uint32_t lw;                         // 2 * ceil(n_groups / 64)
};

// per (vector, group): tune_groups' choice.  A wave holds 64 consecutive groups: its ballot is two label words.
__global__ __launch_bounds__(256) void tune_leaf_labels(const LabelArgs a)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x, vb = blockIdx.y;
    const uint32_t *gcnt = a.ws.gcnt(vb), *same = a.ws.same(vb), *flip = a.ws.flip(vb);
    bool take_same = false;
    if (g < a.ws.n_groups && gcnt[3ull * g] != 0) {
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
    if ((threadIdx.x & 63u) == 0 && g0 < a.ws.n_groups) {         // (then (g0 >> 5) + 1 < lw)
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
    uint32_t vb0;
    const uint32_t nvb = stage_vectors(s_t, a.vec + a.v0, a.nv, &vb0);
    const uint32_t c = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    duet_tune_feature f;
    bool elig;
    const Derived d = load_candidate(a.feat, a.C, c, &f, &elig);
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
    if (int rc = check_truth_arrays(ctx, truth, n_cands)) return rc;
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
    if (truth && !sweep_ws_of(truth, &la.ws)) return fail(ctx, DUET_ERR_INVALID, "truth set too large");
    // the sweep's own batches (sweep_batch): each is one batch of the sweep too, so its workspace holds every vector of it afterwards
    const uint32_t batch = sweep_batch(n_vec, la.ws.words);
    if (truth) {
        a.has_truth = 1;
        a.flags = truth->cand_flags; a.group = truth->cand_group;
        la.group_pair_off = truth->group_pair_off;
        la.lw = 2u * ((truth->n_groups + 63u) / 64u);
        DevBuf *B = ctx->tune_leaf_ws.b;
        if ((rc = duet_reserve(ctx, B[0], (size_t)batch * sizeof(duet_tune_counts))) ||
            (rc = duet_reserve(ctx, B[1], (size_t)batch * la.lw * 4 + 16)))
            return rc;
        la.label = (uint32_t *)B[1].ptr;
        a.label = la.label; a.lw = la.lw;
    }
    const uint32_t tiles = (n_cands + 255) / 256;
    for (uint32_t v0 = 0; v0 < n_vec; v0 += batch) {
        const uint32_t nv = n_vec - v0 < batch ? n_vec - v0 : batch;
        a.v0 = v0; a.nv = nv;
        if (truth && truth->n_groups) {
            if ((rc = duet_tune_sweep_device(ctx, feat, n_cands, vec + v0, nv, truth, (duet_tune_counts *)ctx->tune_leaf_ws.b[0].ptr,
                                             nullptr, nullptr, stream_)))
                return rc;
            la.ws.base = (uint32_t *)ctx->tune_ws.b[3].ptr;      // (reserved by the sweep for this batch)
            hipLaunchKernelGGL(tune_leaf_labels, dim3((la.ws.n_groups + 255) / 256, nv), dim3(256), 0, stream, la);
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
    if (truth && (rc = stage_truth(ctx, truth, C, C ? ((size_t)truth->n_groups + 1) * 4 : 0, C ? (size_t)truth->n_pairs * 4 : 0, B + 6, s, &dt)))
        return rc;
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
