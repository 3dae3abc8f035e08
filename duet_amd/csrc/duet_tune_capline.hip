// duet_tune_capline.hip -- the line of the PC cap (include/duet_ef.h: duet_tune_cap_line_device, duet_svim_cap_line_device), built
// on the device from the resident problem, so that a fit (duet_amd/tune.py: fit, the pc_cap axis) neither downloads the marks nor
// guesses caps.  A mark votes iff its read is tagged and pc <= cap, so with the 14 constants fixed the feature records under a cap
// change only where the cap crosses the pc of a mark that can vote: the distinct pc values of those marks, with 0 in front, hold
// every behaviour of the cap.
//
//   cl_keys      (a duet_ef_problem) one wavefront per candidate, 64 marks at a time like features_body: the 64-bit key of a mark
//                is its pc when its candidate is kept and its read is tagged with pc <= 2^30 - 3, all-ones otherwise
//   cl_keys_raw  (a duet_svim_problem: no clustering) one lane per raw mark: the same without a kept test -- a superset of what
//                any -c / -r setting keeps; a value no kept mark carries costs one evaluation and scores like its neighbour
//   a keys-only radix sort over exactly 30 bits (an all-ones key has the field 2^30 - 1, above every participant)
//   one scan over the head flags of the sorted keys: the distinct values numbered and compacted into the sort's spare buffer;
//   D and x_1 end in the header words, which ONE host round trip reads
//   cl_pick      one lane per output value: the line (0 in front unless x_1 == 0), whole or sampled
// No float, and no atomic in the unit's own kernels (the shared sort's rx_hist accumulates its digit totals with integer atomics up
// to 1024 tiles, as for duet_tune_line.hip: sums, so nothing depends on the order of arrival); which rank a value gets follows from
// the keys alone.
#include "duet_internal.h"

#include <cstring>

namespace {

#include "duet_prims.hip.h"
#include "duet_seeds.hip.h"                // kEmpty, kUntagged, tag_pc

constexpr uint64_t kNoKey = ~0ull;
constexpr uint32_t kCapMax = (1u << 30) - 3u;         // the tag word saturates pc at 2^30 - 2: a saturated value never votes
constexpr uint32_t kKeyBits = 30;

int fail(duet_ctx *ctx, int code, const char *msg) { return duet_fail(ctx, code, msg); }

// the key of one mark: the tagged test is mark_tag's (duet_tune_feat.hip.h), the pc field tag_pc's
__device__ __forceinline__ uint64_t mark_key(const uint32_t *mark_read, const uint64_t *read_tag, uint32_t n_reads, uint32_t m)
{
    const uint32_t r = mark_read[m];
    if (r == kEmpty || r >= n_reads) return kNoKey;
    const uint64_t t = read_tag[r];
    if (t == kUntagged) return kNoKey;
    const uint32_t pc = tag_pc(t);
    return pc <= kCapMax ? (uint64_t)pc : kNoKey;
}

struct KeyArgs {
    uint32_t C, M, n_reads, svlen_thres, suppread_thres;
    const uint64_t *read_tag;
    const uint32_t *cand_svlen, *cand_svread, *cand_off, *mark_read;
    const uint8_t *cand_gt_ok;
    uint64_t *keys;                 // [M]
};

__global__ __launch_bounds__(64) void cl_keys(const KeyArgs a)
{
    const uint32_t lane = threadIdx.x;
    for (uint32_t c = blockIdx.x; c < a.C; c += gridDim.x) {
        uint32_t b = a.cand_off[c], e = a.cand_off[c + 1];
        e = e < a.M ? e : a.M;                                   // (nothing is written past the key array, whatever the offsets say)
        // the kept test as features_body states it (duet_tune_feat.hip.h: `const bool kept = ...`, sv_phasing_fn.py:189-190)
        const bool kept = a.cand_svlen[c] >= a.svlen_thres && a.cand_svread[c] >= a.suppread_thres && a.cand_gt_ok[c] != 0;
        for (uint32_t m0 = b; m0 < e; m0 += 64) {
            const uint32_t m = m0 + lane;
            if (m < e) a.keys[m] = kept ? mark_key(a.mark_read, a.read_tag, a.n_reads, m) : kNoKey;
        }
    }
}

__global__ __launch_bounds__(256) void cl_keys_raw(const uint32_t *mark_read, const uint64_t *read_tag, uint32_t n_reads, uint32_t M,
                                                   uint64_t *keys)
{
    const uint32_t m = blockIdx.x * 256u + threadIdx.x;
    if (m < M) keys[m] = mark_key(mark_read, read_tag, n_reads, m);
}

// the sorted keys: position i opens the run of one distinct value
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
    uint32_t *distinct;             // the sort's spare buffer, taken as words
    uint32_t *x1;                   // header word 1: the lowest distinct value
    __device__ __forceinline__ void operator()(uint32_t i, uint32_t before, uint32_t head) const
    {
        if (!head) return;
        const uint32_t v = (uint32_t)keys[i];
        distinct[before] = v;
        if (before == 0) *x1 = v;
    }
};

struct PickArgs {
    const uint32_t *distinct;
    uint32_t L, n_out, zero_front, sampled;     // sampled: n_out < L, entry i is line index floor(i * (L - 1) / (n_out - 1))
    uint32_t *out;
};

__global__ __launch_bounds__(256) void cl_pick(const PickArgs a)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n_out) return;
    const uint32_t li = a.sampled ? (uint32_t)((uint64_t)i * (a.L - 1u) / (a.n_out - 1u)) : i;
    a.out[i] = a.zero_front ? (li == 0 ? 0u : a.distinct[li - 1u]) : a.distinct[li];
}

int check_out(duet_ctx *ctx, const void *prob, uint32_t max_values, const uint32_t *out_caps, const uint32_t *n_caps, const uint32_t *n_distinct)
{
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    if (!prob || !out_caps || !n_caps || !n_distinct) return fail(ctx, DUET_ERR_INVALID, "null argument");
    if (max_values == 1) return fail(ctx, DUET_ERR_INVALID, "max_values of 1: a line has at least its two ends (0 = all values)");
    return DUET_OK;
}

// the values a call can write at most
uint32_t line_room(uint32_t M, uint32_t max_values)
{
    const uint32_t all = (M < kCapMax + 1u ? M : kCapMax + 1u) + 1u;
    return max_values && max_values < all ? max_values : all;
}

struct Keys {                       // what the keys kernel of either form needs
    bool raw;
    KeyArgs a;
};

// keys -> sort -> scan -> the round trip -> pick.  M == 0: the line [0], no workspace
int run_line(duet_ctx *ctx, const Keys &kk, uint32_t M, uint32_t max_values, uint32_t *out_caps, uint32_t *n_caps, uint32_t *n_distinct,
             hipStream_t st)
{
    *n_caps = 0;
    *n_distinct = 0;
    uint32_t D = 0, x1 = 0;
    const uint32_t *distinct = nullptr;
    if (M) {
        int rc;
        const uint32_t nb_rx = (M + kRxTile - 1) / kRxTile, nb_sc = (M + kScanTile - 1) / kScanTile;
        const uint32_t nb_hs = (256u * nb_rx + kScanTile - 1) / kScanTile;
        Arena ar;
        const size_t o_hdr = ar.take(64), o_ka = ar.take((size_t)M * 8), o_kb = ar.take((size_t)M * 8),
                     o_hist = ar.take((size_t)256 * nb_rx * 4), o_part = ar.take(((size_t)(nb_sc > nb_hs ? nb_sc : nb_hs) + 1) * 4);
        DevBuf &ws = ctx->tune_capline_ws.b[0];
        if ((rc = duet_reserve(ctx, ws, ar.total))) return rc;
        char *wb = (char *)ws.ptr;
        uint32_t *d_hdr = (uint32_t *)(wb + o_hdr);              // [0] the number of distinct values D, [1] the lowest of them x_1
        uint64_t *keysA = (uint64_t *)(wb + o_ka), *keysB = (uint64_t *)(wb + o_kb);
        uint32_t *hist = (uint32_t *)(wb + o_hist), *spart = (uint32_t *)(wb + o_part);
        HIP_TRY(ctx, hipMemsetAsync(d_hdr, 0, 64, st));
        if (kk.raw) {
            hipLaunchKernelGGL(cl_keys_raw, dim3((M + 255) / 256), dim3(256), 0, st, kk.a.mark_read, kk.a.read_tag, kk.a.n_reads, M, keysA);
        } else {
            KeyArgs a = kk.a;
            a.keys = keysA;
            HIP_TRY(ctx, hipMemsetAsync(keysA, 0xFF, (size_t)M * 8, st));      // (a mark no candidate's range holds takes no part)
            hipLaunchKernelGGL(cl_keys, dim3(a.C < (1u << 20) ? a.C : (1u << 20)), dim3(64), 0, st, a);
        }
        uint64_t *sorted = nullptr, *spare = nullptr;
        radix_sort_pairs(keysA, keysB, nullptr, nullptr, M, kKeyBits, hist, spart, ctx->rx_dtot, st, &sorted, nullptr, &spare);
        launch_scan<0>(LoadHead{sorted}, M, spart, StoreDistinct{sorted, (uint32_t *)spare, d_hdr + 1}, d_hdr, st);
        HIP_TRY(ctx, hipGetLastError());
        uint32_t hdr[2] = {0, 0};
        HIP_TRY(ctx, hipMemcpyAsync(hdr, d_hdr, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        D = hdr[0];
        x1 = hdr[1];
        distinct = (const uint32_t *)spare;
    }
    PickArgs p;
    memset(&p, 0, sizeof(p));
    p.distinct = distinct;
    p.zero_front = (D == 0 || x1 != 0) ? 1u : 0u;
    p.L = D + p.zero_front;
    p.sampled = (max_values >= 2 && p.L > max_values) ? 1u : 0u;
    p.n_out = p.sampled ? max_values : p.L;
    p.out = out_caps;
    hipLaunchKernelGGL(cl_pick, dim3((p.n_out + 255) / 256), dim3(256), 0, st, p);
    HIP_TRY(ctx, hipGetLastError());
    *n_distinct = D;
    *n_caps = p.n_out;
    return DUET_OK;
}

Keys ef_keys(const duet_ef_problem *pr)
{
    Keys k;
    memset(&k, 0, sizeof(k));
    k.raw = false;
    k.a.C = pr->n_cands; k.a.M = pr->n_marks; k.a.n_reads = pr->n_reads;
    k.a.svlen_thres = pr->svlen_thres; k.a.suppread_thres = pr->suppread_thres;
    k.a.read_tag = pr->read_tag;
    k.a.cand_svlen = pr->cand_svlen; k.a.cand_svread = pr->cand_svread; k.a.cand_off = pr->cand_off; k.a.mark_read = pr->mark_read;
    k.a.cand_gt_ok = pr->cand_gt_ok;
    return k;
}

// (candidates without a single mark: no array is read, the line is [0] whatever the arrays are)
int check_ef(duet_ctx *ctx, const duet_ef_problem *pr) { return pr->n_cands && !pr->n_marks ? DUET_OK : duet_ef_validate(ctx, pr); }

int check_svim(duet_ctx *ctx, const duet_svim_problem *pr)
{
    if (pr->marks.n_marks && !pr->mark_read) return fail(ctx, DUET_ERR_INVALID, "null array");
    if (pr->marks.n_marks && pr->n_reads && !pr->read_tag) return fail(ctx, DUET_ERR_INVALID, "read_tag is null");
    return DUET_OK;
}

Keys svim_keys(const duet_svim_problem *pr)
{
    Keys k;
    memset(&k, 0, sizeof(k));
    k.raw = true;
    k.a.M = pr->marks.n_marks; k.a.n_reads = pr->n_reads;
    k.a.read_tag = pr->read_tag; k.a.mark_read = pr->mark_read;
    return k;
}

// the device form on staged arrays, then the values back to the host
int run_line_host(duet_ctx *ctx, const Keys &kk, uint32_t M, uint32_t max_values, uint32_t *out_caps, uint32_t *n_caps, uint32_t *n_distinct,
                  hipStream_t s)
{
    int rc;
    DevBuf &bo = ctx->tune_capline_ws.b[1];
    if ((rc = duet_reserve(ctx, bo, (size_t)line_room(M, max_values) * 4))) return rc;
    if ((rc = run_line(ctx, kk, M, max_values, (uint32_t *)bo.ptr, n_caps, n_distinct, s))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out_caps, bo.ptr, (size_t)*n_caps * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return DUET_OK;
}

}  // namespace

extern "C" {

int duet_tune_cap_line_device(duet_ctx *ctx, const duet_ef_problem *pr, uint32_t max_values, uint32_t *out_caps, uint32_t *n_caps,
                              uint32_t *n_distinct, void *stream_)
{
    int rc = check_out(ctx, pr, max_values, out_caps, n_caps, n_distinct);
    if (rc || (rc = check_ef(ctx, pr))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return run_line(ctx, ef_keys(pr), pr->n_cands ? pr->n_marks : 0u, max_values, out_caps, n_caps, n_distinct, (hipStream_t)stream_);
}

int duet_tune_cap_line_host(duet_ctx *ctx, const duet_ef_problem *pr, uint32_t max_values, uint32_t *out_caps, uint32_t *n_caps,
                            uint32_t *n_distinct)
{
    int rc = check_out(ctx, pr, max_values, out_caps, n_caps, n_distinct);
    if (rc || (rc = check_ef(ctx, pr))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->own_stream;
    duet_ef_problem d = *pr;
    if (pr->n_cands && pr->n_marks && (rc = duet_ef_upload(ctx, pr, &d, s))) return rc;
    return run_line_host(ctx, ef_keys(&d), pr->n_cands ? pr->n_marks : 0u, max_values, out_caps, n_caps, n_distinct, s);
}

int duet_svim_cap_line_device(duet_ctx *ctx, const duet_svim_problem *pr, uint32_t max_values, uint32_t *out_caps, uint32_t *n_caps,
                              uint32_t *n_distinct, void *stream_)
{
    int rc = check_out(ctx, pr, max_values, out_caps, n_caps, n_distinct);
    if (rc || (rc = check_svim(ctx, pr))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return run_line(ctx, svim_keys(pr), pr->marks.n_marks, max_values, out_caps, n_caps, n_distinct, (hipStream_t)stream_);
}

int duet_svim_cap_line_host(duet_ctx *ctx, const duet_svim_problem *pr, uint32_t max_values, uint32_t *out_caps, uint32_t *n_caps,
                            uint32_t *n_distinct)
{
    int rc = check_out(ctx, pr, max_values, out_caps, n_caps, n_distinct);
    if (rc || (rc = check_svim(ctx, pr))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->own_stream;
    const uint32_t M = pr->marks.n_marks;
    duet_svim_problem d = *pr;
    if (M) {
        const void *src[2] = {pr->mark_read, pr->read_tag};
        const size_t bytes[2] = {(size_t)M * 4, (size_t)pr->n_reads * 8};
        void *dev[2];
        if ((rc = duet_stage_arrays(ctx, ctx->tune_capline_ws.b + 2, src, bytes, 2, s, dev))) return rc;
        d.mark_read = (const uint32_t *)dev[0];
        d.read_tag = (const uint64_t *)dev[1];
    }
    return run_line_host(ctx, svim_keys(&d), M, max_values, out_caps, n_caps, n_distinct, s);
}

}  // extern "C"
