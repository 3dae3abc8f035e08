// duet_eval_details.hip -- gfx950 kernels and C ABI for the evaluator's per-record outcome (duet_eval_details_host): what
// became of every call and of every truth record in the scoring of src/scripts/evaluation.py:99-159.
//
// The call side is the evaluator's own work with its findings kept (duet_eval.hip.h, DETAILS = true): eval_match stores the
// record a call was compared with, their distance and each test's result; eval_group_choose adds the labelling the call's
// phase-set group took and counts the call at its truth record -- n_calls, n_gt, n_hp, integer atomics on sums.  The six
// counts are made by the same statements as in duet_eval_run_host.
//
// The truth side is a nearest-neighbour search the other way round, which the evaluator never makes:
//   evd_keys     one lane per call: the key (list key << 32 | pos), the value the call's index
//   the shared stable radix sort over 32 + bits_for(n_keys) bits: the calls by (list key, pos, index) -- calls without a list
//                key sort behind every list
//   evd_truth    one lane per truth record: bisects the sorted keys for (its list key, its pos) -- which lands inside the key's
//                slice or at one of its ends -- and looks at both neighbours: the first call at or above its position, and the
//                first of the run of calls at the largest position below it (a second bisection; the sort is stable, so the
//                first of a run is the smallest index).  The nearer one is `nearest`, a tie goes to the lower position.  For a
//                record no call was counted at it says why, from the nearest call's distance and the length quotient; a nearest
//                call that passes both was compared with another record, or it would have been counted here.
// Nothing depends on the order of arrival.  Integers, apart from the binary64 length quotient; no LDS in the unit's own kernels.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>

#include "duet_ef.h"
#include "duet_internal.h"

#pragma clang fp contract(off)

namespace {

#include "duet_prims.hip.h"

#include "duet_eval.hip.h"

__global__ __launch_bounds__(256) void evd_keys(const uint32_t *call_key, const uint32_t *call_pos, uint32_t n_calls, uint32_t n_keys,
                                                uint64_t *keys, uint32_t *vals)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_calls) return;
    const uint32_t key = call_key[c];
    keys[c] = ((uint64_t)(key == kNone ? n_keys : key) << 32) | call_pos[c];
    vals[c] = c;
}

// first index in the ascending keys[0, n) whose key is not below `want`
__device__ __forceinline__ uint32_t first_at_or_above(const uint64_t *keys, uint32_t n, uint64_t want)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < want) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct TruthParams {
    uint32_t n_base, n_keys, n_calls, refdist;
    double ratio;
    const uint32_t *base_off, *base_pos, *base_len, *call_len;
    const uint64_t *keys;                         // the calls' keys, sorted
    const uint32_t *vals;                         // ... and their indices
    duet_eval_base_rec *base_rec;                 // n_calls, n_gt, n_hp are final
};

__global__ __launch_bounds__(256) void evd_truth(const TruthParams p)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= p.n_base) return;
    // the record's list key: the last list that starts at or before j (empty lists share their start with the next one)
    uint32_t lo = 0, hi = p.n_keys;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (p.base_off[mid] <= j) lo = mid; else hi = mid;
    }
    const uint32_t key = lo, bpos = p.base_pos[j];
    const uint64_t want = ((uint64_t)key << 32) | bpos;
    const uint32_t i = first_at_or_above(p.keys, p.n_calls, want);
    uint32_t at = kNone, dist = kNone;
    if (i < p.n_calls) {
        const uint64_t k = p.keys[i];
        if ((uint32_t)(k >> 32) == key) { at = i; dist = (uint32_t)k - bpos; }
    }
    if (i > 0u) {
        const uint64_t k = p.keys[i - 1u];
        // below the record: a tie with the call above goes to the lower position
        if ((uint32_t)(k >> 32) == key && (at == kNone || bpos - (uint32_t)k <= dist)) {
            at = first_at_or_above(p.keys, i, k);
            dist = bpos - (uint32_t)k;
        }
    }
    const uint32_t c = at == kNone ? kNone : p.vals[at];
    duet_eval_base_rec *out = p.base_rec + j;
    uint32_t reason = DUET_EVAL_HIT;
    if (out->n_calls == 0u) {
        if (c == kNone) reason = DUET_EVAL_NO_CALL;
        else if (dist > p.refdist) reason = DUET_EVAL_FAR;
        else if (!length_ratio_accepts(p.call_len[c], p.base_len[j], p.ratio)) reason = DUET_EVAL_WRONG_SIZE;
        else reason = DUET_EVAL_ELSEWHERE;          // (its own record is not j: it would have been counted here)
    }
    out->nearest = c;
    out->nearest_dist = dist;
    out->reason = (uint8_t)reason;
}

// what the device indexes with, looked at on the host first
int check_lists(duet_ctx *ctx, const duet_eval_problem *pr)
{
    const uint32_t nk = pr->n_keys;
    if (pr->base_off[0] != 0u || pr->base_off[nk] != pr->n_base) return duet_fail(ctx, DUET_ERR_INVALID, "base_off does not span the truth records");
    for (uint32_t k = 0; k < nk; ++k)
        if (pr->base_off[k] > pr->base_off[k + 1]) return duet_fail(ctx, DUET_ERR_INVALID, "base_off descends");
    for (uint32_t c = 0; c < pr->n_calls; ++c) {
        // (a call without a list key reads its group's counters too)
        if (pr->call_uid[c] >= pr->n_call_uid || pr->call_group[c] >= pr->n_groups) return duet_fail(ctx, DUET_ERR_INVALID, "a call's id or group is out of range");
        const uint32_t key = pr->call_key[c];
        if (key == kNone) continue;
        if (key >= nk || pr->base_off[key] == pr->base_off[key + 1]) return duet_fail(ctx, DUET_ERR_INVALID, "a call's list has no truth record");
    }
    for (uint32_t j = 0; j < pr->n_base; ++j)
        if (pr->base_uid[j] >= pr->n_base_uid) return duet_fail(ctx, DUET_ERR_INVALID, "a truth id is out of range");
    return DUET_OK;
}

}  // namespace

extern "C" {

int duet_eval_details_host(duet_ctx *ctx, const duet_eval_problem *pr, duet_eval_counts *counts, duet_eval_call_rec *calls,
                           duet_eval_base_rec *base_out)
{
    if (!ctx) return duet_fail(nullptr, DUET_ERR_INVALID, "null context");
    if (!pr || !counts || (pr->n_calls && !calls) || (pr->n_base && !base_out)) return duet_fail(ctx, DUET_ERR_INVALID, "null argument");
    memset(counts, 0, sizeof(*counts));
    const uint32_t nb = pr->n_base, nc = pr->n_calls, nk = pr->n_keys;
    if (nc == 0) {
        // no call anywhere: nothing to launch
        for (uint32_t j = 0; j < nb; ++j) {
            memset(base_out + j, 0, sizeof(*base_out));
            base_out[j].nearest = base_out[j].nearest_dist = kNone;
            base_out[j].reason = DUET_EVAL_NO_CALL;
        }
        return DUET_OK;
    }
    int rc;
    if ((rc = eval_check(ctx, pr))) return rc;
    if (nk == 0 || nk >= (1u << 24)) return duet_fail(ctx, DUET_ERR_INVALID, "n_keys outside 1 .. 2^24 - 1");
    if ((rc = check_lists(ctx, pr))) return rc;
    EvalRun run;
    if ((rc = eval_launch<true>(ctx, pr, &run))) return rc;
    hipStream_t st = ctx->own_stream;
    hipLaunchKernelGGL(evd_keys, dim3((nc + 255) / 256), dim3(256), 0, st, run.p.call_key, run.p.call_pos, nc, nk, run.keysA, run.valsA);
    uint64_t *sk = nullptr;
    uint32_t *sv = nullptr;
    radix_sort_pairs(run.keysA, run.keysB, run.valsA, run.valsB, nc, 32u + bits_for(nk), run.hist, run.spart, ctx->rx_dtot, st, &sk, &sv, nullptr);
    if (nb) {
        TruthParams t;
        t.n_base = nb; t.n_keys = nk; t.n_calls = nc; t.refdist = pr->refdist; t.ratio = pr->ratio;
        t.base_off = run.p.base_off; t.base_pos = run.p.base_pos; t.base_len = run.p.base_len; t.call_len = run.p.call_len;
        t.keys = sk; t.vals = sv; t.base_rec = run.p.base_rec;
        hipLaunchKernelGGL(evd_truth, dim3((nb + 255) / 256), dim3(256), 0, st, t);
    }
    HIP_TRY(ctx, hipGetLastError());
    uint32_t h[6];
    HIP_TRY(ctx, hipMemcpyAsync(h, run.d_out, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(calls, run.p.call_rec, (size_t)nc * sizeof(*calls), hipMemcpyDeviceToHost, st));
    if (nb) HIP_TRY(ctx, hipMemcpyAsync(base_out, run.p.base_rec, (size_t)nb * sizeof(*base_out), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    counts->call_tp = h[0]; counts->base_tp = h[1]; counts->call_gt = h[2]; counts->base_gt = h[3]; counts->call_hp = h[4]; counts->base_hp = h[5];
    return DUET_OK;
}

}  // extern "C"
