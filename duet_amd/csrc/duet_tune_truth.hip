// duet_tune_truth.hip -- the threshold sweep's truth arrays (include/duet_ef.h: duet_tune_truth) built on the device, so that a sweep
// over -s, -r and -c keeps features and truth arrays in HBM.  The normative text is prepare_truth of duet_amd/tune.py.
//
//   tt_expand   table form only: (contig, type, pos) -> the candidate's list key and CHROM id, the BED ranges folded in
//   tt_match    one lane per candidate: the evaluator's nearest truth record (src/scripts/evaluation.py:117-127), the flag word,
//               the truth id, and the candidate's sort key  [not a call : 1 | CHROM id | ps : 32 | uid, n_uid when unmatched]
//   one stable radix sort of the (key, candidate) pairs: the calls come first, group by group, a group's matched calls truth id
//   by truth id
//   two scans over the sorted keys: group heads -> cand_group; pair heads -> cand_pair, pair_uid, group_pair_off
//   tt_close    group_pair_off[n_groups] = n_pairs
// Which number a group or a pair gets follows from the keys alone: no atomic, nothing depends on the order of arrival.
#include "duet_internal.h"

#pragma clang fp contract(off)

namespace {

#include "duet_prims.hip.h"

int fail(duet_ctx *ctx, int code, const char *msg) { return duet_fail(ctx, code, msg); }

struct TruthArgs {
    uint32_t C, n_keys, n_uid, refdist;
    double ratio;
    const duet_tune_feature *feat;
    const uint32_t *cand_pos, *cand_len, *cand_key, *cand_chrom;
    const uint32_t *base_off, *base_pos, *base_len, *base_uid;
    const uint8_t *base_hp;
    uint32_t ubits, cmask, call_bits;       // bits of the uid field; mask of the CHROM id; bits below the "not a call" bit
    uint16_t *flags;
    uint32_t *group, *uid, *pair;
    uint64_t *keys;
    uint32_t *vals;
};

struct ExpandArgs {
    uint32_t C, n_contigs;
    const uint16_t *cand_contig;
    const uint8_t *cand_type;
    const uint32_t *cand_pos, *key_table, *chrom_id, *bed_off, *bed_lo, *bed_hi;
    uint32_t *out_key, *out_chrom;
};

__global__ __launch_bounds__(256) void tt_expand(const ExpandArgs a)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= a.C) return;
    const uint32_t k = a.cand_contig[c], t = a.cand_type[c];
    uint32_t key = DUET_TUNE_KEY_SKIP, chrom = 0;
    if (k < a.n_contigs && t < 4u) {
        key = a.key_table[4u * k + t];
        chrom = a.chrom_id[k];
        if (a.bed_off && key != DUET_TUNE_KEY_SKIP) {
            // the last range that starts at or before pos (the ranges are merged: no other one can hold it)
            const uint32_t pos = a.cand_pos[c], b = a.bed_off[k];
            uint32_t lo = 0, hi = a.bed_off[k + 1] - b;
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (a.bed_lo[b + mid] <= pos) lo = mid + 1; else hi = mid;
            }
            if (lo == 0 || pos > a.bed_hi[b + lo - 1]) key = DUET_TUNE_KEY_SKIP;
        }
    }
    a.out_key[c] = key;
    a.out_chrom[c] = chrom;
}

__global__ __launch_bounds__(256) void tt_match(const TruthArgs a)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= a.C) return;
    uint32_t key = a.cand_key[c];
    const bool call = a.feat[c].eligible != 0 && key != DUET_TUNE_KEY_SKIP && a.cand_len[c] >= 50u;
    uint32_t fl = 0, uid = 0;
    uint64_t sk = 1ull << a.call_bits;
    if (call) {
        fl = DUET_TUNE_IN_CALLS;
        uint32_t field = a.n_uid;
        if (key < a.n_keys) {
            const uint32_t lo0 = a.base_off[key], n = a.base_off[key + 1] - lo0;
            if (n == 0) {
                fl |= DUET_TUNE_RAISES;
            } else {
                const uint32_t pos = a.cand_pos[c];
                const uint32_t b = lo0 + nearest_truth(a.base_pos + lo0, n, pos);
                if (truth_accepts(pos, a.base_pos[b], a.cand_len[c], a.base_len[b], a.refdist, a.ratio)) {
                    const uint32_t h = a.base_hp[b];
                    uid = field = a.base_uid[b];
                    fl |= DUET_TUNE_MATCHED;
                    // bits 3 (p - 1) + {gt, same, flip} for pred p = 1 '1|0', 2 '0|1', 3 '1|1' (evaluation.py:130-141)
                    if (h < 2u) fl |= 1u | 8u | (h == 0u ? 2u | 32u : 4u | 16u);
                    else if (h == 2u) fl |= 7u << 6;
                }
            }
        }
        sk = ((((uint64_t)(a.cand_chrom[c] & a.cmask) << 32) | a.feat[c].ps) << a.ubits) | field;
    }
    a.flags[c] = (uint16_t)fl;
    a.uid[c] = uid;
    a.group[c] = 0;
    a.pair[c] = 0;
    a.keys[c] = sk;
    a.vals[c] = c;
}

// the sorted keys: is position i a call, the first of its group, the first of its (group, uid) pair
struct Sorted {
    const uint64_t *keys;
    uint32_t ubits, call_bits, n_uid;
    __device__ __forceinline__ bool call(uint64_t k) const { return (k >> call_bits) == 0; }
    __device__ __forceinline__ uint32_t field(uint64_t k) const { return (uint32_t)(k & ((1ull << ubits) - 1ull)); }
    __device__ __forceinline__ bool group_head(uint32_t i) const
    {
        const uint64_t k = keys[i];
        return call(k) && (i == 0 || (keys[i - 1] >> ubits) != (k >> ubits));
    }
    __device__ __forceinline__ bool pair_head(uint32_t i) const
    {
        const uint64_t k = keys[i];
        return call(k) && field(k) != n_uid && (i == 0 || keys[i - 1] != k);
    }
};
struct LoadGroupHead {
    Sorted s;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return s.group_head(i) ? 1u : 0u; }
};
struct StoreGroup {
    Sorted s;
    const uint32_t *vals;
    uint32_t *group;
    __device__ __forceinline__ void operator()(uint32_t i, uint32_t before, uint32_t head) const
    {
        if (s.call(s.keys[i])) group[vals[i]] = before + head - 1u;
    }
};
struct LoadPairHead {
    Sorted s;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return s.pair_head(i) ? 1u : 0u; }
};
struct StorePair {
    Sorted s;
    const uint32_t *vals, *group;
    uint32_t *pair, *pair_uid, *group_pair_off;
    __device__ __forceinline__ void operator()(uint32_t i, uint32_t before, uint32_t head) const
    {
        const uint64_t k = s.keys[i];
        if (!s.call(k)) return;
        const uint32_t c = vals[i];
        if (s.group_head(i)) group_pair_off[group[c]] = before;      // pairs are numbered in sorted order: group-major
        if (s.field(k) == s.n_uid) return;
        pair[c] = before + head - 1u;
        if (head) pair_uid[before] = s.field(k);
    }
};

__global__ void tt_close(const uint32_t *tot, uint32_t *group_pair_off) { group_pair_off[tot[0]] = tot[1]; }

int check(duet_ctx *ctx, const duet_tune_truth_problem *pr, const duet_tune_truth *t, bool *table)
{
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    if (!pr || !t) return fail(ctx, DUET_ERR_INVALID, "null argument");
    *table = !pr->cand_key && !pr->cand_chrom;
    if (!t->group_pair_off) return fail(ctx, DUET_ERR_INVALID, "null truth array");
    if (pr->n_cands == 0) return DUET_OK;
    if (!t->cand_flags || !t->cand_group || !t->cand_uid || !t->cand_pair || !t->pair_uid) return fail(ctx, DUET_ERR_INVALID, "null truth array");
    if (!pr->feat || !pr->cand_pos || !pr->cand_len || !pr->base_off) return fail(ctx, DUET_ERR_INVALID, "null array");
    if (pr->n_base && (!pr->base_pos || !pr->base_len || !pr->base_uid || !pr->base_hp)) return fail(ctx, DUET_ERR_INVALID, "null truth-set array");
    if (*table) {
        if (!pr->cand_contig || !pr->cand_type || (pr->n_contigs && (!pr->key_table || !pr->chrom_id)))
            return fail(ctx, DUET_ERR_INVALID, "null array of the table form");
    } else if (!pr->cand_key || !pr->cand_chrom) {
        return fail(ctx, DUET_ERR_INVALID, "cand_key and cand_chrom go together");
    }
    const uint32_t bits = (pr->n_chrom > 1 ? bits_for(pr->n_chrom - 1) : 0) + 32 + bits_for(pr->n_base_uid) + 1;
    if (bits > 64) return fail(ctx, DUET_ERR_INVALID, "CHROM ids and truth ids need more than 64 key bits");
    return DUET_OK;
}

}  // namespace

extern "C" {

int duet_tune_truth_build_device(duet_ctx *ctx, const duet_tune_truth_problem *pr, duet_tune_truth *t, void *stream_)
{
    bool table = false;
    int rc = check(ctx, pr, t, &table);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream_;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t C = pr->n_cands;
    t->n_uid = pr->n_base_uid; t->n_groups = 0; t->n_pairs = 0; t->reserved = 0;
    uint32_t *gpo = const_cast<uint32_t *>(t->group_pair_off);
    if (C == 0) {
        HIP_TRY(ctx, hipMemsetAsync(gpo, 0, 4, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        return DUET_OK;
    }
    const uint32_t nb_rx = (C + kRxTile - 1) / kRxTile, nb_sc = (C + kScanTile - 1) / kScanTile;
    const uint32_t nb_hs = (256u * nb_rx + kScanTile - 1) / kScanTile;
    Arena ar;
    const size_t o_tot = ar.take(64), o_ka = ar.take((size_t)C * 8), o_kb = ar.take((size_t)C * 8), o_va = ar.take((size_t)C * 4),
                 o_vb = ar.take((size_t)C * 4), o_hist = ar.take((size_t)256 * nb_rx * 4),
                 o_part = ar.take(((size_t)(nb_sc > nb_hs ? nb_sc : nb_hs) + 1) * 4), o_key = ar.take(table ? (size_t)C * 4 : 0),
                 o_chrom = ar.take(table ? (size_t)C * 4 : 0);
    DevBuf &ws = ctx->tune_ws.b[15];
    if ((rc = duet_reserve(ctx, ws, ar.total))) return rc;
    char *base = (char *)ws.ptr;
    uint32_t *d_tot = (uint32_t *)(base + o_tot);
    uint64_t *keysA = (uint64_t *)(base + o_ka), *keysB = (uint64_t *)(base + o_kb);
    uint32_t *valsA = (uint32_t *)(base + o_va), *valsB = (uint32_t *)(base + o_vb);
    uint32_t *hist = (uint32_t *)(base + o_hist), *spart = (uint32_t *)(base + o_part);
    const dim3 grid((C + 255) / 256), block(256);

    TruthArgs a;
    memset(&a, 0, sizeof(a));
    a.cand_key = pr->cand_key; a.cand_chrom = pr->cand_chrom;
    if (table) {
        ExpandArgs e;
        memset(&e, 0, sizeof(e));
        e.C = C; e.n_contigs = pr->n_contigs;
        e.cand_contig = pr->cand_contig; e.cand_type = pr->cand_type; e.cand_pos = pr->cand_pos;
        e.key_table = pr->key_table; e.chrom_id = pr->chrom_id;
        e.bed_off = pr->bed_off; e.bed_lo = pr->bed_lo; e.bed_hi = pr->bed_hi;
        e.out_key = (uint32_t *)(base + o_key); e.out_chrom = (uint32_t *)(base + o_chrom);
        hipLaunchKernelGGL(tt_expand, grid, block, 0, st, e);
        a.cand_key = e.out_key; a.cand_chrom = e.out_chrom;
    }
    const uint32_t cbits = pr->n_chrom > 1 ? bits_for(pr->n_chrom - 1) : 0;
    a.C = C; a.n_keys = pr->n_keys; a.n_uid = pr->n_base_uid; a.refdist = pr->refdist; a.ratio = pr->ratio;
    a.feat = pr->feat; a.cand_pos = pr->cand_pos; a.cand_len = pr->cand_len;
    a.base_off = pr->base_off; a.base_pos = pr->base_pos; a.base_len = pr->base_len; a.base_uid = pr->base_uid; a.base_hp = pr->base_hp;
    a.ubits = bits_for(pr->n_base_uid);
    a.cmask = cbits ? (uint32_t)((1ull << cbits) - 1ull) : 0u;
    a.call_bits = cbits + 32 + a.ubits;
    a.flags = const_cast<uint16_t *>(t->cand_flags); a.group = const_cast<uint32_t *>(t->cand_group);
    a.uid = const_cast<uint32_t *>(t->cand_uid); a.pair = const_cast<uint32_t *>(t->cand_pair);
    a.keys = keysA; a.vals = valsA;
    HIP_TRY(ctx, hipMemsetAsync(d_tot, 0, 64, st));
    hipLaunchKernelGGL(tt_match, grid, block, 0, st, a);
    uint64_t *kin = nullptr;
    uint32_t *vin = nullptr;
    radix_sort_pairs(keysA, keysB, valsA, valsB, C, a.call_bits + 1, hist, spart, ctx->rx_dtot, st, &kin, &vin, nullptr);
    const Sorted s{kin, a.ubits, a.call_bits, a.n_uid};
    launch_scan<0>(LoadGroupHead{s}, C, spart, StoreGroup{s, vin, a.group}, d_tot, st);
    launch_scan<0>(LoadPairHead{s}, C, spart, StorePair{s, vin, a.group, a.pair, const_cast<uint32_t *>(t->pair_uid), gpo}, d_tot + 1, st);
    hipLaunchKernelGGL(tt_close, dim3(1), dim3(1), 0, st, (const uint32_t *)d_tot, gpo);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t tot[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(tot, d_tot, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    t->n_groups = tot[0];
    t->n_pairs = tot[1];
    return DUET_OK;
}

int duet_tune_truth_build_host(duet_ctx *ctx, const duet_tune_truth_problem *pr, duet_tune_truth *t)
{
    bool table = false;
    int rc = check(ctx, pr, t, &table);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->own_stream;
    const size_t C = pr->n_cands, K = pr->n_contigs, nb = pr->n_base;
    // the BED ranges' count is the last offset
    const size_t n_bed = (table && pr->bed_off && K) ? pr->bed_off[K] : 0;
    const void *src[16] = {pr->feat, pr->cand_pos, pr->cand_len, pr->cand_key, pr->cand_chrom, pr->cand_contig, pr->cand_type,
                           pr->key_table, pr->chrom_id, pr->bed_off, pr->bed_lo, pr->bed_hi, pr->base_off, pr->base_pos,
                           pr->base_len, pr->base_uid};
    size_t bytes[16] = {C * sizeof(duet_tune_feature), C * 4, C * 4, table ? 0 : C * 4, table ? 0 : C * 4, table ? C * 2 : 0,
                        table ? C : 0, table ? K * 16 : 0, table ? K * 4 : 0, (table && pr->bed_off) ? (K + 1) * 4 : 0,
                        n_bed * 4, n_bed * 4, ((size_t)pr->n_keys + 1) * 4, nb * 4, nb * 4, nb * 4};
    for (int i = 0; i < 16; ++i)
        if (!src[i]) bytes[i] = 0;
    void *dev[16];
    if ((rc = duet_stage_arrays(ctx, ctx->tune_truth_in.b, src, bytes, 16, s, dev))) return rc;
    // base_hp, and the six outputs
    DevBuf *O = ctx->tune_truth_out.b;
    const size_t ob[7] = {nb, C * 2, C * 4, C * 4, C * 4, (C + 1) * 4, C * 4};
    for (int i = 0; i < 7; ++i)
        if ((rc = duet_reserve(ctx, O[i], ob[i] + 64))) return rc;
    if (nb) HIP_TRY(ctx, hipMemcpyAsync(O[0].ptr, pr->base_hp, nb, hipMemcpyHostToDevice, s));
    duet_tune_truth_problem d = *pr;
    d.feat = (const duet_tune_feature *)dev[0]; d.cand_pos = (const uint32_t *)dev[1]; d.cand_len = (const uint32_t *)dev[2];
    d.cand_key = table ? nullptr : (const uint32_t *)dev[3]; d.cand_chrom = table ? nullptr : (const uint32_t *)dev[4];
    d.cand_contig = (const uint16_t *)dev[5]; d.cand_type = (const uint8_t *)dev[6];
    d.key_table = (const uint32_t *)dev[7]; d.chrom_id = (const uint32_t *)dev[8];
    d.bed_off = (table && pr->bed_off) ? (const uint32_t *)dev[9] : nullptr;
    d.bed_lo = (const uint32_t *)dev[10]; d.bed_hi = (const uint32_t *)dev[11];
    d.base_off = (const uint32_t *)dev[12]; d.base_pos = (const uint32_t *)dev[13]; d.base_len = (const uint32_t *)dev[14];
    d.base_uid = (const uint32_t *)dev[15]; d.base_hp = (const uint8_t *)O[0].ptr;
    duet_tune_truth dt = *t;
    dt.cand_flags = (const uint16_t *)O[1].ptr; dt.cand_group = (const uint32_t *)O[2].ptr; dt.cand_uid = (const uint32_t *)O[3].ptr;
    dt.cand_pair = (const uint32_t *)O[4].ptr; dt.group_pair_off = (const uint32_t *)O[5].ptr; dt.pair_uid = (const uint32_t *)O[6].ptr;
    if ((rc = duet_tune_truth_build_device(ctx, &d, &dt, s))) return rc;
    t->n_uid = dt.n_uid; t->n_groups = dt.n_groups; t->n_pairs = dt.n_pairs; t->reserved = 0;
    const void *from[6] = {O[1].ptr, O[2].ptr, O[3].ptr, O[4].ptr, O[5].ptr, O[6].ptr};
    const void *to[6] = {t->cand_flags, t->cand_group, t->cand_uid, t->cand_pair, t->group_pair_off, t->pair_uid};
    const size_t nbytes[6] = {C * 2, C * 4, C * 4, C * 4, ((size_t)dt.n_groups + 1) * 4, (size_t)dt.n_pairs * 4};
    for (int i = 0; i < 6; ++i)
        if (nbytes[i]) HIP_TRY(ctx, hipMemcpyAsync(const_cast<void *>(to[i]), from[i], nbytes[i], hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return DUET_OK;
}

}  // extern "C"
