// duet_prims_check.hip -- diagnostics (include/duet_ef.h, "Diagnostics"): the shared device primitives of duet_prims.hip.h on host
// arrays, so that tests/test_gpu_prims.py can compare each of them with numpy at its plan boundaries -- the sort's 1024-tile and
// kDtotCopies edges, the scan's kSelfSpine / kSelfSpineDyn switches and its device-side count, the local sort's two compare modes,
// its halo and rx_big's three paths.  Every entry uploads its arrays, sizes the workspace as the comments above the primitive
// prescribe, runs the primitive UNCHANGED on the context's own stream with the context's digit totals, and copies the results
// back.  No product path calls these.
#include "duet_internal.h"

namespace {

#include "duet_prims.hip.h"

int fail(duet_ctx *ctx, int code, const char *msg) { return duet_fail(ctx, code, msg); }

// the sort key of an 8-byte element: its low key_bits (whatever sits above them is payload), as KeyOfU64 of duet_recsort.hip.h
struct KeyOfLow {
    uint64_t km;
    __device__ __forceinline__ uint64_t operator()(const uint64_t &e) const { return e & km; }
};

inline uint64_t low_mask(uint32_t key_bits) { return key_bits >= 64u ? ~0ull : (1ull << key_bits) - 1ull; }

// the tile arithmetic of the sort kernels is 32-bit (a tile's base + kRxTile)
constexpr uint32_t kMaxKeys = 1u << 31;

// what radix_sort_pairs asks for n keys: hist and spart in words
struct SortSizes {
    uint32_t nb_rx;
    size_t hist, spart;
    explicit SortSizes(uint32_t n) : nb_rx((n + kRxTile - 1) / kRxTile), hist((size_t)256 * nb_rx), spart((256 * (size_t)nb_rx + kScanTile - 1) / kScanTile + 1) {}
};

}  // namespace

extern "C" {

int duet_prims_sort_host(duet_ctx *ctx, const uint64_t *keys, const uint32_t *vals, uint32_t n, uint32_t key_bits, uint32_t first_shift,
                         int force_scan, uint64_t *out_keys, uint32_t *out_vals)
{
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    if (key_bits < 1u || key_bits > 64u) return fail(ctx, DUET_ERR_INVALID, "key_bits is not in 1..64");
    if (first_shift >= key_bits) return fail(ctx, DUET_ERR_INVALID, "first_shift is not below key_bits");
    if ((vals == nullptr) != (out_vals == nullptr)) return fail(ctx, DUET_ERR_INVALID, "vals and out_vals: both or neither");
    if (n > kMaxKeys) return fail(ctx, DUET_ERR_INVALID, "more than 2^31 keys");
    if (n == 0) return DUET_OK;
    if (!keys || !out_keys) return fail(ctx, DUET_ERR_INVALID, "null array");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->own_stream;
    const SortSizes sz(n);
    Arena ar;
    const size_t o_ka = ar.take((size_t)n * 8), o_kb = ar.take((size_t)n * 8), o_va = ar.take(vals ? (size_t)n * 4 : 0),
                 o_vb = ar.take(vals ? (size_t)n * 4 : 0), o_hist = ar.take(sz.hist * 4), o_part = ar.take(sz.spart * 4);
    DevBuf &ws = ctx->prims_ws.b[0];
    int rc = duet_reserve(ctx, ws, ar.total);
    if (rc) return rc;
    char *wb = (char *)ws.ptr;
    uint64_t *keysA = (uint64_t *)(wb + o_ka), *keysB = (uint64_t *)(wb + o_kb);
    uint32_t *valsA = vals ? (uint32_t *)(wb + o_va) : nullptr, *valsB = vals ? (uint32_t *)(wb + o_vb) : nullptr;
    uint32_t *hist = (uint32_t *)(wb + o_hist), *spart = (uint32_t *)(wb + o_part);
    HIP_TRY(ctx, hipMemcpyAsync(keysA, keys, (size_t)n * 8, hipMemcpyHostToDevice, st));
    if (vals) HIP_TRY(ctx, hipMemcpyAsync(valsA, vals, (size_t)n * 4, hipMemcpyHostToDevice, st));
    uint64_t *kin = nullptr;
    uint32_t *vin = nullptr;
    radix_sort_pairs(keysA, keysB, valsA, valsB, n, key_bits, hist, spart, ctx->rx_dtot, st, &kin, vals ? &vin : nullptr, nullptr, force_scan != 0,
                     false, first_shift);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out_keys, kin, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    if (vals) HIP_TRY(ctx, hipMemcpyAsync(out_vals, vin, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return DUET_OK;
}

int duet_prims_scan_host(duet_ctx *ctx, const uint32_t *in, uint32_t n, int op, uint32_t n_dyn, int force_spine, uint32_t *out,
                         uint32_t *total, uint32_t *zero14)
{
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    if (op != 0 && op != 1) return fail(ctx, DUET_ERR_INVALID, "op is neither 0 (sum) nor 1 (max)");
    if (n > kMaxKeys) return fail(ctx, DUET_ERR_INVALID, "more than 2^31 elements");
    if (n == 0) return DUET_OK;
    if (!in || !out || !total) return fail(ctx, DUET_ERR_INVALID, "null array");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->own_stream;
    const bool dyn = n_dyn != 0xFFFFFFFFu;
    const uint32_t nb = (n + kScanTile - 1) / kScanTile;
    Arena ar;
    const size_t o_in = ar.take((size_t)n * 4), o_out = ar.take((size_t)n * 4), o_part = ar.take(((size_t)nb + 1) * 4), o_small = ar.take(256);
    DevBuf &ws = ctx->prims_ws.b[0];
    int rc = duet_reserve(ctx, ws, ar.total);
    if (rc) return rc;
    char *wb = (char *)ws.ptr;
    uint32_t *d_in = (uint32_t *)(wb + o_in), *d_out = (uint32_t *)(wb + o_out), *part = (uint32_t *)(wb + o_part);
    uint32_t *small = (uint32_t *)(wb + o_small);                // [0] total, [1] the real count, [16..30) zero14
    uint32_t *d_total = small, *d_dyn = small + 1, *d_zero = small + 16;
    const uint32_t head[2] = {0xA5A5A5A5u, n_dyn};
    HIP_TRY(ctx, hipMemcpyAsync(d_in, in, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_out, out, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(small, head, 8, hipMemcpyHostToDevice, st));
    if (zero14) HIP_TRY(ctx, hipMemcpyAsync(d_zero, zero14, 14 * 4, hipMemcpyHostToDevice, st));
    uint32_t *z = zero14 ? d_zero : (uint32_t *)nullptr;
    const uint32_t *nd = dyn ? d_dyn : (const uint32_t *)nullptr;
    if (op == 0) launch_scan<0>(LoadPlain{d_in}, n, part, StorePlain{d_out}, d_total, st, z, force_spine != 0, nd);
    else launch_scan<1>(LoadPlain{d_in}, n, part, StorePlain{d_out}, d_total, st, z, force_spine != 0, nd);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out, d_out, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(total, d_total, 4, hipMemcpyDeviceToHost, st));
    if (zero14) HIP_TRY(ctx, hipMemcpyAsync(zero14, d_zero, 14 * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return DUET_OK;
}

int duet_prims_local_sort_host(duet_ctx *ctx, const uint64_t *keys, uint32_t n, uint32_t key_bits, uint32_t lo, uint32_t cap,
                               uint32_t threads, uint64_t *out_keys)
{
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    if (key_bits < 1u || key_bits > 64u) return fail(ctx, DUET_ERR_INVALID, "key_bits is not in 1..64");
    if (lo < 1u || lo >= 32u) return fail(ctx, DUET_ERR_INVALID, "lo is not in 1..31 (the local stage holds the low bits in 32-bit words)");
    if (lo >= key_bits) return fail(ctx, DUET_ERR_INVALID, "lo is not below key_bits");
    if (cap < 1u || cap > (uint32_t)kLocHalo) return fail(ctx, DUET_ERR_INVALID, "cap is not in 1..kLocHalo (a group of cap keys must end inside the window)");
    if (threads != 256u && threads != 1024u) return fail(ctx, DUET_ERR_INVALID, "threads is neither 256 nor 1024");
    if (n > kMaxKeys) return fail(ctx, DUET_ERR_INVALID, "more than 2^31 keys");
    if (n == 0) return DUET_OK;
    if (!keys || !out_keys) return fail(ctx, DUET_ERR_INVALID, "null array");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->own_stream;
    const SortSizes sz(n);
    Arena ar;
    const size_t o_ka = ar.take((size_t)n * 8), o_kb = ar.take((size_t)n * 8), o_hist = ar.take(sz.hist * 4), o_part = ar.take(sz.spart * 4),
                 o_list = ar.take((size_t)n * 4), o_count = ar.take(64);
    DevBuf &ws = ctx->prims_ws.b[0];
    int rc = duet_reserve(ctx, ws, ar.total);
    if (rc) return rc;
    char *wb = (char *)ws.ptr;
    uint64_t *keysA = (uint64_t *)(wb + o_ka), *keysB = (uint64_t *)(wb + o_kb);
    uint32_t *hist = (uint32_t *)(wb + o_hist), *spart = (uint32_t *)(wb + o_part);
    uint32_t *big_list = (uint32_t *)(wb + o_list), *big_count = (uint32_t *)(wb + o_count);     // (a group on the list has its first key's position there: n words hold any)
    HIP_TRY(ctx, hipMemcpyAsync(keysA, keys, (size_t)n * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(big_count, 0, 64, st));
    // as the key-only branch of stage A0's host driver: the global passes over the bits [lo, key_bits), the groups of up to cap keys
    // ranked from the sort's result into its spare buffer, the larger ones by rx_big between the two; the result is the spare buffer
    uint64_t *kin = nullptr, *kout = nullptr;
    radix_sort_pairs(keysA, keysB, nullptr, nullptr, n, key_bits, hist, spart, ctx->rx_dtot, st, &kin, nullptr, &kout, false, false, lo);
    const KeyOfLow keyof{low_mask(key_bits)};
    const dim3 grid((n + kLocTile - 1) / kLocTile);
    if (threads == 1024u)
        hipLaunchKernelGGL((rx_local<1024, uint64_t, KeyOfLow>), grid, dim3(1024), 0, st, (const uint64_t *)kin, kout, n, lo, keyof, cap, big_list, big_count);
    else
        hipLaunchKernelGGL((rx_local<256, uint64_t, KeyOfLow>), grid, dim3(256), 0, st, (const uint64_t *)kin, kout, n, lo, keyof, cap, big_list, big_count);
    hipLaunchKernelGGL((rx_big<uint64_t, KeyOfLow>), dim3(256), dim3(256), 0, st, kin, kout, n, lo, keyof, (const uint32_t *)big_list, (const uint32_t *)big_count);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out_keys, kout, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return DUET_OK;
}

}  // extern "C"
