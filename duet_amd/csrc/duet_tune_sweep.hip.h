// duet_tune_sweep.hip.h -- what the scoring kernels of the threshold sweep share: the T1-T5 tree of predict_hp
// (src/duet/sv_phasing_fn.py:142-183) with its 18 exits numbered, the opening of a tile of candidates, the workspace one batch
// of vectors leaves behind and the rule that sizes a batch.  The sweep (duet_tune.hip) writes that workspace and the leaf census
// (duet_tune_leaf.hip) reads it after running the sweep on its own batches, so both take layout and batches from here.
// Included inside each unit's anonymous namespace.
#ifndef DUET_TUNE_SWEEP_HIP_H
#define DUET_TUNE_SWEEP_HIP_H

#include "duet_tune_derive.hip.h"          // Derived, derive(): what the tree compares (shared with duet_tune_line.hip)

constexpr int kVecPerBlock = 32;                  // vectors applied to one tile of 256 candidates
constexpr size_t kWsBudget = (size_t)256 << 20;   // sweep workspace per batch of vectors

// predict_hp (:142-183) with the constants of vector t -> the exit taken (include/duet_ef.h, "Leaf census"), *pred = its verdict.
// A comparison that is false takes the else branch, for a nan constant too.
__device__ __forceinline__ uint32_t leaf_of(const Derived &d, const duet_tune_thresholds &t, uint32_t *pred)
{
    uint32_t leaf, p = 0;
    if (d.cls == 0) {                                                               // :145-147
        if (d.sv_ratio == 1.0 && d.svread >= t.c0_min_sv_num) { leaf = 0; p = 3; }
        else leaf = 1;
    } else if (d.cls == 2) {                                                        // :148-155
        if (d.sv_ratio >= t.c2_min_sv_ratio) {
            if (d.diff <= t.c2_max_avgsc_diff) {
                if (d.svread >= t.c2_min_sv_num) { leaf = 3; p = 3; }
                else leaf = 4;
            } else {
                if (d.hap0 >= t.c2_min_hap0) { leaf = 5; p = 3; }
                else leaf = 6;
            }
        } else leaf = 2;
    } else {                                                                        // :156-182
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

__device__ __forceinline__ uint32_t decide_vec(const Derived &d, const duet_tune_thresholds &t)
{
    uint32_t pred;
    leaf_of(d, t, &pred);
    return pred;
}

// The vectors of workgroup row blockIdx.y -- vb0 .. vb0 + (return value) of the batch's nv at vec -- into s_t[kVecPerBlock] (LDS),
// behind a barrier.  For the 256-thread kernels that apply kVecPerBlock vectors to one tile.
__device__ __forceinline__ uint32_t stage_vectors(duet_tune_thresholds *s_t, const duet_tune_thresholds *vec, uint32_t nv, uint32_t *vb0)
{
    *vb0 = blockIdx.y * kVecPerBlock;
    const uint32_t nvb = nv - *vb0 < (uint32_t)kVecPerBlock ? nv - *vb0 : (uint32_t)kVecPerBlock;
    const double *src = (const double *)(vec + *vb0);
    double *dst = (double *)s_t;
    for (uint32_t i = threadIdx.x; i < nvb * 14u; i += 256u) dst[i] = src[i];
    __syncthreads();
    return nvb;
}

// Candidate c of a tile: its record (zeroes past the end), whether it is eligible, and what the tree compares
__device__ __forceinline__ Derived load_candidate(const duet_tune_feature *feat, uint32_t C, uint32_t c, duet_tune_feature *f, bool *elig)
{
    if (c < C) *f = feat[c];
    else memset(f, 0, sizeof(*f));
    *elig = c < C && f->eligible;
    if (!*elig) f->deg = 1;                                      // (no division by zero in derive for the lanes that never decide)
    return derive(*f);
}

// The sweep's workspace of one batch.  Per vector `words` words: gcnt[3 * n_groups] (per group: present, same calls, flip calls),
// three bit sets of truth ids of uw words each (tp, gt, hp), two of (group, truth id) pairs of pw words each (same, flip), and
// one spare word.
struct SweepWs {
    uint32_t *base;
    uint32_t words, n_groups, uw, pw;
    __device__ __forceinline__ uint32_t *gcnt(uint32_t vb) const { return base + (size_t)vb * words; }
    __device__ __forceinline__ uint32_t *tp(uint32_t vb) const { return gcnt(vb) + 3ull * n_groups; }
    __device__ __forceinline__ uint32_t *gt(uint32_t vb) const { return tp(vb) + uw; }
    __device__ __forceinline__ uint32_t *hp(uint32_t vb) const { return gt(vb) + uw; }
    __device__ __forceinline__ uint32_t *same(uint32_t vb) const { return hp(vb) + uw; }
    __device__ __forceinline__ uint32_t *flip(uint32_t vb) const { return same(vb) + pw; }
};

// the layout for a truth set (base stays null); false: a vector's block does not fit 32 bits of words
inline bool sweep_ws_of(const duet_tune_truth *truth, SweepWs *w)
{
    memset(w, 0, sizeof(*w));
    w->n_groups = truth->n_groups;
    w->uw = (truth->n_uid + 31) / 32;
    w->pw = (truth->n_pairs + 31) / 32;
    const size_t words = 3ull * w->n_groups + 3ull * w->uw + 2ull * w->pw + 1;
    w->words = (uint32_t)words;
    return words <= 0xFFFFFFFFull;
}

// Vectors per batch: what the workspace budget holds (at least one), and what gridDim.y takes -- the tile kernels run one row of
// workgroups per kVecPerBlock vectors, the per-group and per-word kernels (truth set only: ws_words != 0) one row per vector
inline uint32_t sweep_batch(uint32_t n_vec, uint32_t ws_words)
{
    uint32_t batch = n_vec;
    if (ws_words) {
        const size_t fit = kWsBudget / ((size_t)ws_words * 4);
        if (fit < batch) batch = fit ? (uint32_t)fit : 1u;
        if (batch > 65535u) batch = 65535u;
    }
    if (batch > 65535u * kVecPerBlock) batch = 65535u * kVecPerBlock;
    return batch;
}

int check_truth_arrays(duet_ctx *ctx, const duet_tune_truth *truth, uint32_t n_cands)
{
    if (truth && n_cands && (!truth->cand_flags || !truth->cand_group || !truth->cand_uid || !truth->cand_pair ||
                             !truth->group_pair_off || (truth->n_pairs && !truth->pair_uid)))
        return duet_fail(ctx, DUET_ERR_INVALID, "null truth array");
    return DUET_OK;
}

// the truth arrays of a host run -> the staging buffers B[0 .. 6); *dt = *truth with device pointers.  The four per-candidate
// arrays have C entries; off_bytes, pair_bytes: what the caller stages of group_pair_off and pair_uid.
int stage_truth(duet_ctx *ctx, const duet_tune_truth *truth, size_t C, size_t off_bytes, size_t pair_bytes, DevBuf *B, hipStream_t s,
                duet_tune_truth *dt)
{
    const void *src[6] = {truth->cand_flags, truth->cand_group, truth->cand_uid, truth->cand_pair, truth->group_pair_off, truth->pair_uid};
    const size_t bytes[6] = {C * 2, C * 4, C * 4, C * 4, off_bytes, pair_bytes};
    for (int i = 0; i < 6; ++i) {
        int rc = duet_reserve(ctx, B[i], bytes[i] ? bytes[i] : 16);
        if (rc) return rc;
        if (bytes[i] && src[i]) HIP_TRY(ctx, hipMemcpyAsync(B[i].ptr, src[i], bytes[i], hipMemcpyHostToDevice, s));
    }
    *dt = *truth;
    dt->cand_flags = (const uint16_t *)B[0].ptr; dt->cand_group = (const uint32_t *)B[1].ptr;
    dt->cand_uid = (const uint32_t *)B[2].ptr; dt->cand_pair = (const uint32_t *)B[3].ptr;
    dt->group_pair_off = (const uint32_t *)B[4].ptr; dt->pair_uid = (const uint32_t *)B[5].ptr;
    return DUET_OK;
}

#endif
