// duet_tune_line.hip -- the line of one axis of the threshold vector (include/duet_ef.h: duet_tune_line_device), built on the
// device from the resident feature records, so that a fit (duet_amd/tune.py: fit) neither downloads the features nor uploads a
// block of vectors.  With the other 13 constants fixed the counts of a sweep change only where the axis crosses a feature value
// some candidate has: one vector per distinct value and one sentinel cover every behaviour of the axis.
//
//   tl_keys     one lane per candidate: the feature the axis is compared with (derive(), shared with duet_tune.hip) as its
//               binary64 bit pattern -- non-negative and finite, so the pattern orders like the value; all-ones for a candidate
//               that takes no part; a participant whose feature is not finite sets the status word and takes no part
//   one keys-only radix sort over the 64 key bits
//   one scan over the head flags of the sorted keys: the distinct values numbered, each head's key scattered to its rank
//   tl_vectors  one lane per output vector: *base with the axis field replaced by the sentinel or a distinct value
// Which rank a value gets follows from the keys alone: no atomic, nothing depends on the order of arrival.
#include "duet_internal.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

#include "duet_prims.hip.h"
#include "duet_tune_derive.hip.h"

constexpr uint64_t kNoKey = ~0ull;
constexpr uint32_t kAxes = 14;

int fail(duet_ctx *ctx, int code, const char *msg) { return duet_fail(ctx, code, msg); }

// the axes whose line starts with -inf (compared by <= or >); the others (>=) end with +inf
__host__ __device__ __forceinline__ bool axis_from_below(uint32_t axis) { return !(axis == 0u || axis == 1u || axis == 3u || axis == 4u); }

struct KeyArgs {
    const duet_tune_feature *feat;
    uint32_t C, axis;
    uint64_t *keys;
    uint32_t *status;
};

__global__ __launch_bounds__(256) void tl_keys(const KeyArgs a)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= a.C) return;
    const duet_tune_feature f = a.feat[c];
    const Derived d = derive(f);
    bool in = f.eligible != 0;
    double x = 0.0;
    switch (a.axis) {
    case 0: in = in && d.cls == 0; x = d.svread; break;
    case 1: in = in && d.cls == 2; x = d.sv_ratio; break;
    case 2: in = in && d.cls == 2; x = d.diff; break;
    case 3: in = in && d.cls == 2; x = d.svread; break;
    case 4: in = in && d.cls == 2; x = d.hap0; break;
    case 5: case 6: in = in && d.cls == 1 && d.onehap; x = d.sv_ratio; break;
    case 7: in = in && d.cls == 1 && d.onehap; x = d.hr; break;
    case 8: in = in && d.cls == 1 && d.onehap; x = d.diff; break;
    case 9: case 10: case 12: in = in && d.cls == 1 && !d.onehap; x = d.sv_ratio; break;
    case 11: in = in && d.cls == 1 && !d.onehap; x = d.refread; break;
    default: in = in && d.cls == 1 && !d.onehap; x = d.totsc; break;
    }
    uint64_t key = kNoKey;
    if (in) {
        if (isfinite(x)) key = (uint64_t)__double_as_longlong(x);
        else *a.status = 1u;                     // (every such lane stores the same word)
    }
    a.keys[c] = key;
}

struct LoadHead {
    const uint64_t *keys;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const
    {
        const uint64_t k = keys[i];
        return (k != kNoKey && (i == 0 || keys[i - 1] != k)) ? 1u : 0u;
    }
};
struct StoreDistinct {
    const uint64_t *keys;
    uint64_t *distinct;
    __device__ __forceinline__ void operator()(uint32_t i, uint32_t before, uint32_t head) const
    {
        if (head) distinct[before] = keys[i];
    }
};

struct VecArgs {
    duet_tune_thresholds base;
    const uint64_t *distinct;
    uint32_t D, n_vec, axis, sampled;            // sampled: n_vec < D + 1, entry i is line index floor(i * D / (n_vec - 1))
    duet_tune_thresholds *out;
};

__global__ __launch_bounds__(256) void tl_vectors(const VecArgs a)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n_vec) return;
    const uint32_t li = a.sampled ? (uint32_t)((uint64_t)i * a.D / (a.n_vec - 1u)) : i;
    double v;
    if (axis_from_below(a.axis)) v = li == 0 ? -INFINITY : __longlong_as_double((long long)a.distinct[li - 1u]);
    else v = li == a.D ? INFINITY : __longlong_as_double((long long)a.distinct[li]);
    const double *b = (const double *)&a.base;
    double *o = (double *)(a.out + i);
#pragma unroll
    for (uint32_t k = 0; k < kAxes; ++k) o[k] = k == a.axis ? v : b[k];
}

int check(duet_ctx *ctx, const duet_tune_feature *feat, uint32_t n_cands, const duet_tune_thresholds *base, uint32_t axis,
          uint32_t max_values, duet_tune_thresholds *out_vec, uint32_t *n_vec, uint32_t *n_distinct)
{
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    if (!base || !out_vec || !n_vec || !n_distinct) return fail(ctx, DUET_ERR_INVALID, "null argument");
    if (n_cands && !feat) return fail(ctx, DUET_ERR_INVALID, "null feature array");
    if (axis >= kAxes) return fail(ctx, DUET_ERR_INVALID, "axis is not one of the 14 fields");
    if (max_values == 1) return fail(ctx, DUET_ERR_INVALID, "max_values of 1: a line has at least its two ends (0 = all values)");
    if (n_cands == 0xFFFFFFFFu) return fail(ctx, DUET_ERR_INVALID, "n_cands + 1 vectors do not fit 32 bits");
    return DUET_OK;
}

}  // namespace

extern "C" {

int duet_tune_line_device(duet_ctx *ctx, const duet_tune_feature *feat, uint32_t n_cands, const duet_tune_thresholds *base,
                          uint32_t axis, uint32_t max_values, duet_tune_thresholds *out_vec, uint32_t *n_vec, uint32_t *n_distinct,
                          void *stream_)
{
    int rc = check(ctx, feat, n_cands, base, axis, max_values, out_vec, n_vec, n_distinct);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream_;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    *n_vec = 0;
    *n_distinct = 0;
    const uint32_t C = n_cands;
    uint32_t D = 0;
    const uint64_t *distinct = nullptr;
    if (C) {
        const uint32_t nb_rx = (C + kRxTile - 1) / kRxTile, nb_sc = (C + kScanTile - 1) / kScanTile;
        const uint32_t nb_hs = (256u * nb_rx + kScanTile - 1) / kScanTile;
        Arena ar;
        const size_t o_tot = ar.take(64), o_ka = ar.take((size_t)C * 8), o_kb = ar.take((size_t)C * 8),
                     o_hist = ar.take((size_t)256 * nb_rx * 4), o_part = ar.take(((size_t)(nb_sc > nb_hs ? nb_sc : nb_hs) + 1) * 4);
        DevBuf &ws = ctx->tune_line_ws.b[0];
        if ((rc = duet_reserve(ctx, ws, ar.total))) return rc;
        char *wb = (char *)ws.ptr;
        uint32_t *d_tot = (uint32_t *)(wb + o_tot);              // [0] the number of distinct values, [1] the status word
        uint64_t *keysA = (uint64_t *)(wb + o_ka), *keysB = (uint64_t *)(wb + o_kb);
        uint32_t *hist = (uint32_t *)(wb + o_hist), *spart = (uint32_t *)(wb + o_part);
        HIP_TRY(ctx, hipMemsetAsync(d_tot, 0, 64, st));
        KeyArgs k;
        k.feat = feat; k.C = C; k.axis = axis; k.keys = keysA; k.status = d_tot + 1;
        hipLaunchKernelGGL(tl_keys, dim3((C + 255) / 256), dim3(256), 0, st, k);
        uint64_t *kin = nullptr, *spare = nullptr;
        radix_sort_pairs(keysA, keysB, nullptr, nullptr, C, 64, hist, spart, ctx->rx_dtot, st, &kin, nullptr, &spare);
        launch_scan<0>(LoadHead{kin}, C, spart, StoreDistinct{kin, spare}, d_tot, st);      // the distinct values go to the sort's spare buffer
        HIP_TRY(ctx, hipGetLastError());
        uint32_t tot[2] = {0, 0};
        HIP_TRY(ctx, hipMemcpyAsync(tot, d_tot, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        D = tot[0];
        distinct = spare;
        *n_distinct = D;
        if (tot[1]) return fail(ctx, DUET_ERR_DIV_ZERO, "a candidate's compared feature is not finite (deg == 0 or svread + refread == 0)");
    }
    VecArgs v;
    memset(&v, 0, sizeof(v));
    v.base = *base;
    v.distinct = distinct; v.D = D; v.axis = axis; v.out = out_vec;
    v.sampled = (max_values >= 2 && D + 1 > max_values) ? 1u : 0u;
    v.n_vec = v.sampled ? max_values : D + 1;
    hipLaunchKernelGGL(tl_vectors, dim3((v.n_vec + 255) / 256), dim3(256), 0, st, v);
    HIP_TRY(ctx, hipGetLastError());
    *n_vec = v.n_vec;
    return DUET_OK;
}

int duet_tune_line_host(duet_ctx *ctx, const duet_tune_feature *feat, uint32_t n_cands, const duet_tune_thresholds *base, uint32_t axis,
                        uint32_t max_values, duet_tune_thresholds *out_vec, uint32_t *n_vec, uint32_t *n_distinct)
{
    int rc = check(ctx, feat, n_cands, base, axis, max_values, out_vec, n_vec, n_distinct);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->own_stream;
    DevBuf *B = ctx->tune_line_ws.b;
    const void *src[1] = {feat};
    const size_t bytes[1] = {(size_t)n_cands * sizeof(duet_tune_feature)};
    void *dev[1];
    if ((rc = duet_stage_arrays(ctx, B + 1, src, bytes, 1, s, dev)) ||
        (rc = duet_reserve(ctx, B[2], ((size_t)n_cands + 1) * sizeof(duet_tune_thresholds))))
        return rc;
    if ((rc = duet_tune_line_device(ctx, (const duet_tune_feature *)dev[0], n_cands, base, axis, max_values,
                                    (duet_tune_thresholds *)B[2].ptr, n_vec, n_distinct, s)))
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out_vec, B[2].ptr, (size_t)*n_vec * sizeof(duet_tune_thresholds), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return DUET_OK;
}

}  // extern "C"
