// duet_tune_cap.hip -- the feature export (include/duet_ef.h: duet_tune_feature) with the PC cap as a run parameter: a mark votes
// iff its read is tagged and pc <= cap.  The cap decides who votes, which phase sets are seeds (sv_phasing_fn.py:197-203) and so
// which contigs are dropped (:209) and which PS a vote-less candidate takes (:106-111); the PS-class (:192-194) has no PC test.
// The E/F kernels keep the reference's cap as a compile-time constant, so these entries build the seed sets themselves and never
// run E/F, and they neither read nor write the E/F workspace of the context.
//
//   tc_keys      one wavefront per candidate, the seed pass of the shared body (duet_tune_feat.hip.h): kept, PS-class, the class's
//                first PS, "has a voter under the cap"; the 64-bit key contig | ps of a kept class-1 candidate with a voter (in
//                class 1 every tagged mark carries the one PS, so the first voter's PS is that PS), all-ones otherwise
//   a keys-only radix sort over the 32 + bits(K) bits in use (an all-ones key carries a contig field above every contig)
//   one scan over the head flags of the sorted keys: the distinct keys, compacted -- a contig's seeds come out ascending
//   tc_offsets   per contig: where its seeds start among the distinct keys
//   tc_features  the body of tune_features (duet_tune_feat.hip.h) with the cap and these seed arrays; sets the status word when
//                an eligible candidate has svread + refread == 0
// No float, no atomic, no host round trip between the stages: which seed lands where follows from the keys alone.
#include "duet_internal.h"

#include <cstring>

namespace {

#include "duet_prims.hip.h"
#include "duet_tune_feat.hip.h"

int fail(duet_ctx *ctx, int code, const char *msg) { return duet_fail(ctx, code, msg); }

constexpr uint32_t kCapMax = (1u << 30) - 3u;         // the tag word saturates pc at 2^30 - 2: a saturated value never votes
constexpr uint64_t kNoSeed = ~0ull;

// the seed source of tc_features
struct CapSeeds {
    static constexpr bool kSeedPass = false;
    uint32_t pc_cap;
    const uint32_t *seed_off;       // [K + 1] into seed_ps
    const uint32_t *seed_ps;        // the distinct seeds, contig-major, ascending inside a contig
    uint32_t *status;
    __device__ __forceinline__ uint32_t cap() const { return pc_cap; }
    __device__ __forceinline__ uint32_t count(const FeatArgs &, uint32_t k) const { return seed_off[k + 1] - seed_off[k]; }
    __device__ __forceinline__ const uint32_t *seeds(const FeatArgs &, uint32_t k) const { return seed_ps + seed_off[k]; }
    __device__ __forceinline__ void div_zero() const { if (threadIdx.x == 0) *status = 1u; }
};

// the seed pass: the key of a kept class-1 candidate with a voter (the other candidates' keys stay all-ones)
struct SeedKeys {
    static constexpr bool kSeedPass = true;
    uint32_t pc_cap;
    uint64_t *keys;                 // [C], all-ones on entry
    __device__ __forceinline__ uint32_t cap() const { return pc_cap; }
    __device__ __forceinline__ void seed(uint32_t c, uint32_t k, uint32_t ps) const { keys[c] = ((uint64_t)k << 32) | ps; }
    // (not reached by the seed pass)
    __device__ __forceinline__ uint32_t count(const FeatArgs &, uint32_t) const { return 0; }
    __device__ __forceinline__ const uint32_t *seeds(const FeatArgs &, uint32_t) const { return nullptr; }
    __device__ __forceinline__ void div_zero() const {}
};

__global__ __launch_bounds__(64) void tc_keys(const FeatArgs a, const SeedKeys sk) { features_body(a, sk); }

// the sorted keys: position i opens a run of one seed
struct LoadSeedHead {
    const uint64_t *keys;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const
    {
        const uint64_t k = keys[i];
        return (k != kNoSeed && (i == 0 || keys[i - 1] != k)) ? 1u : 0u;
    }
};
struct StoreSeed {
    const uint64_t *keys;
    uint64_t *seed_key;             // the distinct keys (for tc_offsets) ...
    uint32_t *seed_ps;              // ... and their PS fields (what the feature kernel searches)
    __device__ __forceinline__ void operator()(uint32_t i, uint32_t before, uint32_t head) const
    {
        if (!head) return;
        const uint64_t k = keys[i];
        seed_key[before] = k;
        seed_ps[before] = (uint32_t)k;
    }
};

// seed_off[k] = the distinct keys below contig k, k = 0 .. K
__global__ __launch_bounds__(256) void tc_offsets(const uint64_t *seed_key, const uint32_t *n_seeds, uint32_t K, uint32_t *seed_off)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k > K) return;
    const uint64_t want = (uint64_t)k << 32;
    uint32_t lo = 0, hi = *n_seeds;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (seed_key[mid] < want) lo = mid + 1; else hi = mid;
    }
    seed_off[k] = lo;
}

__global__ __launch_bounds__(64) void tc_features(const FeatArgs a, const CapSeeds sd) { features_body(a, sd); }

int check_cap(duet_ctx *ctx, const duet_ef_problem *pr, uint32_t pc_cap)
{
    if (!ctx || !pr) return fail(ctx, DUET_ERR_INVALID, "null argument");
    if (pc_cap > kCapMax) return fail(ctx, DUET_ERR_INVALID, "pc_cap is above 2^30 - 3 (the tag word saturates pc at 2^30 - 2)");
    return duet_ef_validate(ctx, pr);
}

}  // namespace

extern "C" {

int duet_ef_features_cap_device(duet_ctx *ctx, const duet_ef_problem *pr, uint32_t pc_cap, duet_tune_feature *out, void *stream_)
{
    int rc = check_cap(ctx, pr, pc_cap);
    if (rc) return rc;
    const uint32_t C = pr->n_cands, K = pr->n_contigs;
    if (C == 0) return DUET_OK;
    if (!out) return fail(ctx, DUET_ERR_INVALID, "null feature array");
    hipStream_t st = (hipStream_t)stream_;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t nb_rx = (C + kRxTile - 1) / kRxTile, nb_sc = (C + kScanTile - 1) / kScanTile;
    const uint32_t nb_hs = (256u * nb_rx + kScanTile - 1) / kScanTile;
    Arena ar;
    const size_t o_tot = ar.take(64), o_ka = ar.take((size_t)C * 8), o_kb = ar.take((size_t)C * 8), o_ps = ar.take((size_t)C * 4),
                 o_hist = ar.take((size_t)256 * nb_rx * 4), o_part = ar.take(((size_t)(nb_sc > nb_hs ? nb_sc : nb_hs) + 1) * 4),
                 o_ctg = ar.take(((size_t)K + 1) * 4), o_soff = ar.take(((size_t)K + 1) * 4);
    DevBuf &ws = ctx->tune_cap_ws.b[0];
    if ((rc = duet_reserve(ctx, ws, ar.total))) return rc;
    char *base = (char *)ws.ptr;
    uint32_t *d_tot = (uint32_t *)(base + o_tot), *d_status = d_tot + 1;
    uint64_t *keysA = (uint64_t *)(base + o_ka), *keysB = (uint64_t *)(base + o_kb);
    uint32_t *seed_ps = (uint32_t *)(base + o_ps), *hist = (uint32_t *)(base + o_hist), *spart = (uint32_t *)(base + o_part);
    uint32_t *d_ctg_off = (uint32_t *)(base + o_ctg), *seed_off = (uint32_t *)(base + o_soff);
    // cand_ctg_off is host memory: staged here, whatever an E/F run left in the context
    HIP_TRY(ctx, hipMemcpyAsync(d_ctg_off, pr->cand_ctg_off, ((size_t)K + 1) * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(d_tot, 0, 64, st));
    FeatArgs a;
    memset(&a, 0, sizeof(a));
    a.C = C; a.K = K; a.n_reads = pr->n_reads;
    a.svlen_thres = pr->svlen_thres; a.suppread_thres = pr->suppread_thres;
    a.read_tag = pr->read_tag;
    a.cand_pos = pr->cand_pos; a.cand_svlen = pr->cand_svlen; a.cand_svread = pr->cand_svread;
    a.cand_refread = pr->cand_refread; a.cand_off = pr->cand_off; a.mark_read = pr->mark_read; a.cand_gt_ok = pr->cand_gt_ok;
    a.ctg_off = d_ctg_off;
    a.out = out;
    const uint32_t grid = C < (1u << 20) ? C : (1u << 20);
    HIP_TRY(ctx, hipMemsetAsync(keysA, 0xFF, (size_t)C * 8, st));
    hipLaunchKernelGGL(tc_keys, dim3(grid), dim3(64), 0, st, a, SeedKeys{pc_cap, keysA});
    uint64_t *sorted = nullptr, *spare = nullptr;
    radix_sort_pairs(keysA, keysB, nullptr, nullptr, C, 32 + bits_for(K), hist, spart, ctx->rx_dtot, st, &sorted, nullptr, &spare);
    launch_scan<0>(LoadSeedHead{sorted}, C, spart, StoreSeed{sorted, spare, seed_ps}, d_tot, st);
    hipLaunchKernelGGL(tc_offsets, dim3((uint32_t)(((uint64_t)K + 256) / 256)), dim3(256), 0, st, (const uint64_t *)spare, (const uint32_t *)d_tot, K, seed_off);
    const CapSeeds sd{pc_cap, seed_off, seed_ps, d_status};
    hipLaunchKernelGGL(tc_features, dim3(grid), dim3(64), 0, st, a, sd);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t status = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&status, d_status, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (status) return fail(ctx, DUET_ERR_DIV_ZERO, "division by zero: svread + refread == 0 for a candidate that reaches the decision");
    return DUET_OK;
}

int duet_ef_features_cap_host(duet_ctx *ctx, const duet_ef_problem *pr, uint32_t pc_cap, duet_tune_feature *out)
{
    int rc = check_cap(ctx, pr, pc_cap);
    if (rc) return rc;
    const uint32_t C = pr->n_cands;
    if (C == 0) return DUET_OK;
    if (!out) return fail(ctx, DUET_ERR_INVALID, "null feature array");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->own_stream;
    duet_ef_problem d;
    if ((rc = duet_ef_upload(ctx, pr, &d, s))) return rc;
    DevBuf &bf = ctx->tune_cap_ws.b[1];
    if ((rc = duet_reserve(ctx, bf, (size_t)C * sizeof(duet_tune_feature)))) return rc;
    rc = duet_ef_features_cap_device(ctx, &d, pc_cap, (duet_tune_feature *)bf.ptr, s);
    if (rc && rc != DUET_ERR_DIV_ZERO) return rc;
    const std::string msg = ctx->err;
    HIP_TRY(ctx, hipMemcpy(out, bf.ptr, (size_t)C * sizeof(duet_tune_feature), hipMemcpyDeviceToHost));
    if (rc) ctx->err = msg;
    return rc;
}

}  // extern "C"
