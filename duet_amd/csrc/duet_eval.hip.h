// duet_eval.hip.h -- what the two units of the accuracy evaluator share: the four kernels of src/scripts/evaluation.py:99-159
// (duet_eval.hip has their description) and the host code that lays out the arena, uploads a problem and launches them.
// duet_eval.hip (duet_eval_run_host) instantiates everything with DETAILS = false: the kernels keep the six id sets and nothing
// else.  duet_eval_details.hip (duet_eval_details_host) instantiates it with DETAILS = true: eval_match also stores what it
// found for every call -- the record it compared the call with, their distance and the tests one by one --, eval_group_choose
// also stores the labelling the call's phase-set group took and counts the call at its truth record.  The id sets, and with
// them the six counts, are made by the same statements in either form.
// Included inside the unit's anonymous namespace, behind duet_prims.hip.h.
#ifndef DUET_EVAL_HIP_H
#define DUET_EVAL_HIP_H

constexpr uint32_t kNone = 0xFFFFFFFFu;

struct EvalParams {
    uint32_t n_calls, refdist;
    double ratio;
    const uint32_t *base_off, *base_pos, *base_len, *base_uid;
    const uint8_t *base_hp;
    const uint32_t *call_key, *call_pos, *call_len, *call_uid, *call_group;
    const uint8_t *call_hp;
    // per call: matched truth record (global index) or kNone; bit 0 tp (always set with a match), 1 gt, 2 same, 3 flip
    uint32_t *match;
    uint8_t *bits;
    uint8_t *f_call_tp, *f_base_tp, *f_call_gt, *f_base_gt, *f_call_hp, *f_base_hp;      // flag arrays, indexed by id
    unsigned long long *table;                    // hash set, `mask` + 1 slots, 0 = empty
    uint32_t mask;
    uint32_t *cnt_same, *cnt_flip;                // [n_groups]: ids (call side + truth side) per labelling
    // DETAILS only: the records (the truth side's zero on entry)
    duet_eval_call_rec *call_rec;
    duet_eval_base_rec *base_rec;
};

// haplotype codes fixed by the host: 0 '1|0', 1 '0|1', 2 '1|1', anything else >= 3 (compared for equality only)
template <bool DETAILS>
__global__ __launch_bounds__(256) void eval_match(const EvalParams p)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= p.n_calls) return;
    const uint32_t key = p.call_key[c];
    uint32_t m = kNone;
    uint8_t bits = 0;
    duet_eval_call_rec rec = {kNone, kNone, 0u};
    if (key != kNone) {
        const uint32_t lo0 = p.base_off[key], n = p.base_off[key + 1] - lo0;
        const uint32_t *bp = p.base_pos + lo0;
        const uint32_t pos = p.call_pos[c];
        const uint32_t j = nearest_truth(bp, n, pos);                  // :117-125
        const uint32_t b = lo0 + j;
        bool ok;                                                                                        // :126-127
        if (DETAILS) {
            // the two halves of truth_accepts, each kept: MATCHED is NEAR and SIZE by construction
            const uint32_t bpos = bp[j], dist = pos < bpos ? bpos - pos : pos - bpos;
            const bool near = dist <= p.refdist, size = length_ratio_accepts(p.call_len[c], p.base_len[b], p.ratio);
            ok = near && size;
            rec.base = b;
            rec.dist = dist;
            rec.bits = (near ? DUET_EVAL_NEAR : 0u) | (size ? DUET_EVAL_SIZE : 0u);
        } else {
            ok = truth_accepts(pos, bp[j], p.call_len[c], p.base_len[b], p.refdist, p.ratio);
        }
        if (ok) {
            m = b;
            const uint8_t ch = p.call_hp[c], bh = p.base_hp[b];
            const bool gt = (ch < 2 && bh < 2) || (ch == 2 && bh == 2);                                  // :130-133
            const bool same = ch == bh;                                                                 // :134-136
            const bool flip = (ch == 2 && bh == 2) || (ch == 1 && bh == 0) || (ch == 0 && bh == 1);      // :137-141
            bits = (uint8_t)(1u | (gt ? 2u : 0u) | (same ? 4u : 0u) | (flip ? 8u : 0u));
            p.f_call_tp[p.call_uid[c]] = 1;
            p.f_base_tp[p.base_uid[b]] = 1;
            if (gt) { p.f_call_gt[p.call_uid[c]] = 1; p.f_base_gt[p.base_uid[b]] = 1; }
            if (DETAILS) rec.bits |= DUET_EVAL_MATCHED | (gt ? DUET_EVAL_GT : 0u) | (same ? DUET_EVAL_SAME : 0u) | (flip ? DUET_EVAL_FLIP : 0u);
        }
    }
    p.match[c] = m;
    p.bits[c] = bits;
    if (DETAILS) p.call_rec[c] = rec;
}

// true when `key` was not in the set yet
__device__ __forceinline__ bool set_insert(unsigned long long *table, uint32_t mask, unsigned long long key)
{
    const unsigned long long stored = key + 1ull;                       // 0 marks an empty slot
    unsigned long long h = key * 0x9E3779B97F4A7C15ull;
    uint32_t slot = (uint32_t)(h >> 32) & mask;
    for (;;) {
        const unsigned long long old = atomicCAS(&table[slot], 0ull, stored);
        if (old == 0ull) return true;
        if (old == stored) return false;
        slot = (slot + 1u) & mask;
    }
}

// key = labelling (1 bit) | phase-set group (30 bits) | side (1 bit: 0 call, 1 truth) | id (32 bits)
__device__ __forceinline__ unsigned long long set_key(uint32_t labelling, uint32_t group, uint32_t side, uint32_t id)
{
    return ((unsigned long long)labelling << 63) | ((unsigned long long)group << 33) | ((unsigned long long)side << 32) | id;
}

__global__ __launch_bounds__(256) void eval_group_sets(const EvalParams p)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= p.n_calls) return;
    const uint8_t bits = p.bits[c];
    if (!(bits & 12u)) return;
    const uint32_t g = p.call_group[c], cu = p.call_uid[c], bu = p.base_uid[p.match[c]];
    if (bits & 4u) {
        uint32_t add = set_insert(p.table, p.mask, set_key(0, g, 0, cu)) ? 1u : 0u;
        add += set_insert(p.table, p.mask, set_key(0, g, 1, bu)) ? 1u : 0u;
        if (add) atomicAdd(&p.cnt_same[g], add);
    }
    if (bits & 8u) {
        uint32_t add = set_insert(p.table, p.mask, set_key(1, g, 0, cu)) ? 1u : 0u;
        add += set_insert(p.table, p.mask, set_key(1, g, 1, bu)) ? 1u : 0u;
        if (add) atomicAdd(&p.cnt_flip[g], add);
    }
}

template <bool DETAILS>
__global__ __launch_bounds__(256) void eval_group_choose(const EvalParams p)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= p.n_calls) return;
    const uint8_t bits = p.bits[c];
    if (!DETAILS && !(bits & 12u)) return;
    const uint32_t g = p.call_group[c];
    const bool use_same = p.cnt_same[g] > p.cnt_flip[g];                // :143-148, ties to the mirrored labelling
    const bool hp = (bits & (use_same ? 4u : 8u)) != 0;
    if (hp) {
        p.f_call_hp[p.call_uid[c]] = 1;
        p.f_base_hp[p.base_uid[p.match[c]]] = 1;
    }
    if (DETAILS) {
        // every call carries its group's labelling, matched or not; a matched one is counted at its truth record -- integer sums,
        // whatever the order of arrival
        p.call_rec[c].bits |= (use_same ? 0u : DUET_EVAL_LABEL) | (hp ? DUET_EVAL_HP : 0u);
        if (bits & 1u) {
            duet_eval_base_rec *b = p.base_rec + p.match[c];
            atomicAdd(&b->n_calls, 1u);
            if (bits & 2u) atomicAdd(&b->n_gt, 1u);
            if (hp) atomicAdd(&b->n_hp, 1u);
        }
    }
}

// out[which] += number of set flags
__global__ __launch_bounds__(256) void eval_count(const uint8_t *flags, uint32_t n, uint32_t *out)
{
    uint32_t acc = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) acc += flags[i] ? 1u : 0u;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if ((threadIdx.x & 63u) == 0 && acc) atomicAdd(out, acc);
}

// where a launched run left its results, and (DETAILS) the workspace of the truth side
struct EvalRun {
    EvalParams p;
    uint32_t *d_out;                              // the six counts
    uint64_t *keysA, *keysB;                      // [n_calls] each
    uint32_t *valsA, *valsB, *hist, *spart;
};

// The arguments both entries check; nc > 0 behind it.
inline int eval_check(duet_ctx *ctx, const duet_eval_problem *pr)
{
    if (pr->n_groups >= (1u << 30)) return duet_fail(ctx, DUET_ERR_INVALID, "too many phase sets");
    if (!pr->base_off || !pr->call_key || !pr->call_pos || !pr->call_len || !pr->call_hp || !pr->call_uid || !pr->call_group ||
        (pr->n_base && (!pr->base_pos || !pr->base_len || !pr->base_hp || !pr->base_uid)))
        return duet_fail(ctx, DUET_ERR_INVALID, "null array");
    return DUET_OK;
}

// Uploads *pr (host arrays, checked, n_calls > 0) into the context's arena and launches the four kernels on the context's
// stream; nothing is read back and nothing waited for.
template <bool DETAILS>
int eval_launch(duet_ctx *ctx, const duet_eval_problem *pr, EvalRun *run)
{
    const uint32_t nb = pr->n_base, nc = pr->n_calls, ng = pr->n_groups, nk = pr->n_keys;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->own_stream;
    // one arena: inputs, then the scratch that has to start at zero
    uint32_t slots = 64;
    while (slots < 8u * nc && slots < (1u << 31)) slots <<= 1;
    const size_t in_bytes[11] = {((size_t)nk + 1) * 4, (size_t)nb * 4, (size_t)nb * 4, (size_t)nb * 4, (size_t)nb,
                                 (size_t)nc * 4, (size_t)nc * 4, (size_t)nc * 4, (size_t)nc * 4, (size_t)nc * 4, (size_t)nc};
    const void *in_src[11] = {pr->base_off, pr->base_pos, pr->base_len, pr->base_uid, pr->base_hp, pr->call_key, pr->call_pos,
                              pr->call_len, pr->call_uid, pr->call_group, pr->call_hp};
    size_t off[11], total = 0;
    for (int i = 0; i < 11; ++i) { off[i] = total; total += (in_bytes[i] + 255) & ~(size_t)255; }
    const size_t o_match = total;  total += ((size_t)nc * 4 + 255) & ~(size_t)255;
    const size_t o_bits = total;   total += ((size_t)nc + 255) & ~(size_t)255;
    // (DETAILS) the call records, every one written whole by eval_match, and the sort of the truth side
    const uint32_t nb_rx = (nc + kRxTile - 1) / kRxTile, nb_hs = (256u * nb_rx + kScanTile - 1) / kScanTile;
    Arena d;
    d.total = total;
    const size_t o_crec = d.take(DETAILS ? (size_t)nc * sizeof(duet_eval_call_rec) : 0), o_ka = d.take(DETAILS ? (size_t)nc * 8 : 0),
                 o_kb = d.take(DETAILS ? (size_t)nc * 8 : 0), o_va = d.take(DETAILS ? (size_t)nc * 4 : 0), o_vb = d.take(DETAILS ? (size_t)nc * 4 : 0),
                 o_hist = d.take(DETAILS ? (size_t)256 * nb_rx * 4 : 0), o_part = d.take(DETAILS ? ((size_t)nb_hs + 1) * 4 : 0);
    total = d.total;
    const size_t zero_from = total;
    const uint32_t ncu = pr->n_call_uid, nbu = pr->n_base_uid;
    const size_t o_flags[6] = {total, total + ncu, total + 2 * (size_t)ncu, total + 3 * (size_t)ncu, total + 3 * (size_t)ncu + nbu,
                               total + 3 * (size_t)ncu + 2 * (size_t)nbu};      // call tp/gt/hp, truth tp/gt/hp
    total += (3 * ((size_t)ncu + nbu) + 255) & ~(size_t)255;
    const size_t o_cnt = total;    total += ((size_t)ng * 8 + 255) & ~(size_t)255;
    const size_t o_out = total;    total += 256;
    const size_t o_brec = total;   total += DETAILS ? ((size_t)nb * sizeof(duet_eval_base_rec) + 255) & ~(size_t)255 : 0;
    const size_t o_table = total;  total += (size_t)slots * 8;
    int rc;
    if ((rc = duet_reserve(ctx, ctx->eval_ws, total))) return rc;
    char *base = (char *)ctx->eval_ws.ptr;
    for (int i = 0; i < 11; ++i)
        if (in_bytes[i]) HIP_TRY(ctx, hipMemcpyAsync(base + off[i], in_src[i], in_bytes[i], hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(base + zero_from, 0, total - zero_from, st));
    EvalParams &p = run->p;
    p.n_calls = nc; p.refdist = pr->refdist; p.ratio = pr->ratio;
    p.base_off = (const uint32_t *)(base + off[0]); p.base_pos = (const uint32_t *)(base + off[1]);
    p.base_len = (const uint32_t *)(base + off[2]); p.base_uid = (const uint32_t *)(base + off[3]);
    p.base_hp = (const uint8_t *)(base + off[4]); p.call_key = (const uint32_t *)(base + off[5]);
    p.call_pos = (const uint32_t *)(base + off[6]); p.call_len = (const uint32_t *)(base + off[7]);
    p.call_uid = (const uint32_t *)(base + off[8]); p.call_group = (const uint32_t *)(base + off[9]);
    p.call_hp = (const uint8_t *)(base + off[10]);
    p.match = (uint32_t *)(base + o_match); p.bits = (uint8_t *)(base + o_bits);
    p.f_call_tp = (uint8_t *)(base + o_flags[0]); p.f_call_gt = (uint8_t *)(base + o_flags[1]); p.f_call_hp = (uint8_t *)(base + o_flags[2]);
    p.f_base_tp = (uint8_t *)(base + o_flags[3]); p.f_base_gt = (uint8_t *)(base + o_flags[4]); p.f_base_hp = (uint8_t *)(base + o_flags[5]);
    p.cnt_same = (uint32_t *)(base + o_cnt); p.cnt_flip = p.cnt_same + ng;
    p.table = (unsigned long long *)(base + o_table); p.mask = slots - 1u;
    p.call_rec = DETAILS ? (duet_eval_call_rec *)(base + o_crec) : nullptr;
    p.base_rec = DETAILS ? (duet_eval_base_rec *)(base + o_brec) : nullptr;
    run->keysA = DETAILS ? (uint64_t *)(base + o_ka) : nullptr; run->keysB = DETAILS ? (uint64_t *)(base + o_kb) : nullptr;
    run->valsA = DETAILS ? (uint32_t *)(base + o_va) : nullptr; run->valsB = DETAILS ? (uint32_t *)(base + o_vb) : nullptr;
    run->hist = DETAILS ? (uint32_t *)(base + o_hist) : nullptr; run->spart = DETAILS ? (uint32_t *)(base + o_part) : nullptr;
    const dim3 grid((nc + 255) / 256), block(256);
    hipLaunchKernelGGL(eval_match<DETAILS>, grid, block, 0, st, p);
    hipLaunchKernelGGL(eval_group_sets, grid, block, 0, st, p);
    hipLaunchKernelGGL(eval_group_choose<DETAILS>, grid, block, 0, st, p);
    run->d_out = (uint32_t *)(base + o_out);
    const uint8_t *fl[6] = {p.f_call_tp, p.f_base_tp, p.f_call_gt, p.f_base_gt, p.f_call_hp, p.f_base_hp};
    const uint32_t fn[6] = {ncu, nbu, ncu, nbu, ncu, nbu};
    for (int i = 0; i < 6; ++i)
        if (fn[i]) hipLaunchKernelGGL(eval_count, dim3((fn[i] + 2047) / 2048 < 1024u ? (fn[i] + 2047) / 2048 : 1024u), block, 0, st, fl[i], fn[i], run->d_out + i);
    HIP_TRY(ctx, hipGetLastError());
    return DUET_OK;
}

#endif
