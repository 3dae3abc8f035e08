// duet_eval.hip -- gfx950 kernels and C ABI for the accuracy evaluator: a phased callset
// scored against a truth set, as src/scripts/evaluation.py:99-159 does it.
//
//   every call is matched to the NEAREST truth call of its contig and type (np.searchsorted; ties and the end-of-list
//   rule of :117-125), accepted within `refdist` and a length ratio of at least `ratio` (:126-127);
//   call_tp / base_tp / call_tp_gt / base_tp_gt are SETS of record ids (:128-133);
//   phasing is scored per (contig, phase set): the calls whose haplotype equals the truth's ("same") against those that
//   are its mirror image ("flip"), the labelling with more ids -- call ids plus truth ids -- wins, ties to "flip"
//   (:134-148); the winners are united over the phase sets.
//
// The host (duet_amd/evaluation.py) parses the two VCFs as upstream does and flattens them: truth calls per (contig, type)
// in position order, record ids and haplotype strings as small integers.  Sets become flag arrays indexed by id (a store of
// 1 is idempotent), the per-phase-set set sizes come from a hash set of (phase set, labelling, side, id) keys built with
// 64-bit compare-and-swap -- its CONTENT does not depend on the order of arrival.  The six counts come back; the ten numbers
// upstream prints are divisions of those counts in binary64 on the host, exactly as upstream divides them.
//
// Integer / index work, no floating point besides the one length-ratio division per call (binary64, as upstream).
//
// The kernels and the host code that uploads a problem and launches them are in duet_eval.hip.h, shared with
// duet_eval_details.hip (the per-record outcome of the same scoring).

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

}  // namespace

extern "C" {

int duet_eval_run_host(duet_ctx *ctx, const duet_eval_problem *pr, duet_eval_counts *out)
{
    if (!ctx) return duet_fail(nullptr, DUET_ERR_INVALID, "null context");
    if (!pr || !out) return duet_fail(ctx, DUET_ERR_INVALID, "null argument");
    memset(out, 0, sizeof(*out));
    if (pr->n_calls == 0) return DUET_OK;
    int rc;
    if ((rc = eval_check(ctx, pr))) return rc;
    EvalRun run;
    if ((rc = eval_launch<false>(ctx, pr, &run))) return rc;
    hipStream_t st = ctx->own_stream;
    uint32_t h[6];
    HIP_TRY(ctx, hipMemcpyAsync(h, run.d_out, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    out->call_tp = h[0]; out->base_tp = h[1]; out->call_gt = h[2]; out->base_gt = h[3]; out->call_hp = h[4]; out->base_hp = h[5];
    return DUET_OK;
}

}  // extern "C"
