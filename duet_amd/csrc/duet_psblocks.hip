// duet_psblocks.hip -- the blocks of the phase-set links, built on the device (include/duet_ef.h: duet_ps_blocks_device,
// duet_ps_join_links_device): the table (contig, PS) -> (BLOCK, FLIP) of duet_amd/ps_links.py: blocks -- a
// maximum spanning forest with parity over the trusted links, taken in the strict order (-n_win, -w_win, row index) -- from the
// resident records, and that table applied to the read tags without visiting the host.
//
//   pb_keys      one lane per record: the refusals (a word of the call's own), both ends as node keys contig << 32 | ps, the first
//                ranking key ~w_win, the trusted records counted by ballot
//   the node keys sorted (32 + bits_for(K - 1) bits), head flags scanned: the nodes numbered ascending by (contig, ps)
//   the ranks: two stable sorts with the record index as the value, by ~w_win (64 bits), then by untrusted << 32 | ~n_win (33 bits);
//   rank r is the r-th link Kruskal would take, the untrusted records behind all trusted ones
//   pb_ends      one lane per rank: the two node numbers by bisection, the sense and the trusted bit
//   rounds (Boruvka; their number and the jumps of each are fixed on the host from the bound 2 * n_links on the nodes: no round trip)
//     pb_best    one lane per rank: a trusted link between two components offers its rank to both roots (integer atomicMin: the
//                minimum is the same whatever the order of arrival)
//     pb_hook    one lane per node: a root with an offer hangs itself under the root at the link's other end, with the parity the
//                link implies; two roots that chose the same link: the smaller index stays the root.  Written to a second array.
//     pb_jump    par[x] ^= par[parent[x]]; parent[x] = parent[parent[x]], parent and parity in one word, from one array into the
//                other; the first jump of a round also clears the offers
//   pb_min       the smallest node index of every component (atomicMin): its smallest PS, because the nodes ascend
//   pb_rows      one lane per node: BLOCK and FLIP relative to that node; the rows, and the table in the layout pj_tags reads
//   the conflicts: a trusted link outside the forest whose ends' parities differ from its sense, flagged per rank and compacted
//   by a scan: rank order
//   pb_slices    (join) the table's slice per contig by bisection over the node keys; an empty table after a refusal
// Why rounds select Kruskal's links: the order is strict, so the maximum spanning forest is unique, and the best-ranked link that
// leaves a component belongs to it (the cut property).  Components are paths, so labels are not propagated: pointers are jumped.
// Integers only, no kernel waits on a word another workgroup writes; the atomics are minima and sums.
#include "duet_internal.h"

#include <cstring>

namespace {

#include "duet_prims.hip.h"

constexpr uint32_t kThreads = 256;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kMaxLinks = 1u << 30;              // a node index and its parity share a 32-bit word
// header words of a call; the second half is the header of pj_tags (its word 0: the changed tag words)
constexpr uint32_t kBad = 0, kRows = 1, kTrusted = 2, kConf = 3, kComp = 4, kPjHdr = 16, kHdrWords = 32;
constexpr uint32_t kBadOrder = 1, kBadContig = 2, kBadAscend = 4;

int fail(duet_ctx *ctx, int code, const char *msg) { return duet_fail(ctx, code, msg); }

// the verdict of a record: (n_same, w_same) against (n_flip, w_flip), lexicographically
struct Win {
    uint32_t n;
    uint64_t w;
    uint32_t sense;                 // 0 same, 1 flip
    bool trusted;                   // a verdict, and n >= min_sv
};
__device__ __forceinline__ Win win_of(const duet_ps_link *l, uint32_t min_sv)
{
    const uint32_t ns = l->n_same, nf = l->n_flip;
    const uint64_t ws = l->w_same, wf = l->w_flip;
    const bool same = ns > nf || (ns == nf && ws > wf), flip = nf > ns || (ns == nf && wf > ws);
    Win v;
    v.sense = flip ? 1u : 0u;
    v.n = flip ? nf : ns;
    v.w = flip ? wf : ws;
    v.trusted = (same || flip) && v.n >= min_sv;
    return v;
}

__global__ __launch_bounds__(kThreads) void pb_keys(const duet_ps_link *links, uint32_t n, uint32_t K, uint32_t min_sv, uint64_t *node_keys,
                                                     uint64_t *rank_keys, uint32_t *rank_vals, uint32_t *hdr)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t i = (uint32_t)i64;
    bool trusted = false;
    if (i64 < n) {
        const duet_ps_link *l = links + i;
        const uint32_t k = l->contig, a = l->ps_a, b = l->ps_b;
        uint32_t bad = 0;
        if (a >= b) bad |= kBadOrder;
        if (k >= K) bad |= kBadContig;
        if (i) {
            const duet_ps_link *p = l - 1;
            const uint32_t pk = p->contig, pa = p->ps_a, pb = p->ps_b;
            if (!(pk < k || (pk == k && (pa < a || (pa == a && pb < b))))) bad |= kBadAscend;
        }
        if (bad) atomicOr(hdr + kBad, bad);
        const uint64_t kk = (uint64_t)(k < K ? k : 0u) << 32;                // (a refused call still runs: every key stays in range)
        node_keys[2 * (size_t)i] = kk | a;
        node_keys[2 * (size_t)i + 1] = kk | b;
        const Win v = win_of(l, min_sv);
        trusted = v.trusted;
        rank_keys[i] = ~v.w;
        rank_vals[i] = i;
    }
    const unsigned long long m = __ballot(trusted);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(hdr + kTrusted, (uint32_t)__popcll(m));
}

// the sorted node keys: position i opens a node
struct LoadNodeHead {
    const uint64_t *keys;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return (i == 0 || keys[i - 1] != keys[i]) ? 1u : 0u; }
};
struct StoreNode {                  // node[number] = key, for the heads
    const uint64_t *keys;
    uint64_t *node;
    __device__ __forceinline__ void operator()(uint32_t i, uint32_t before, uint32_t head) const
    {
        if (head) node[before] = keys[i];
    }
};

// second ranking pass: untrusted << 32 | ~n_win of the records as the first pass left them (the permutation stays the value)
__global__ __launch_bounds__(kThreads) void pb_key_n(const duet_ps_link *links, const uint32_t *perm, uint32_t n, uint32_t min_sv, uint64_t *keys)
{
    const uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= n) return;
    const uint32_t i = perm[r];
    uint64_t key = 1ull << 32;
    if (i < n) {
        const Win v = win_of(links + i, min_sv);
        if (v.trusted) key = (uint32_t)~v.n;
    }
    keys[r] = key;
}

// the first index with a[i] >= key
__device__ __forceinline__ uint32_t lower_bound_u64(const uint64_t *a, uint32_t n, uint64_t key)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t rows_of(const uint32_t *hdr, uint32_t V)
{
    const uint32_t r = hdr[kRows];
    return r < V ? r : V;
}

struct Forest {                     // rank r: the link perm[r], between the nodes ea[r] and eb[r] (kNone: none), es[r] = sense | trusted << 1
    uint32_t n, V;                  // links; the bound on the nodes
    const uint32_t *hdr;
    uint32_t *ea, *eb, *es, *in_forest, *best, *minnode;
};

__global__ __launch_bounds__(kThreads) void pb_ends(const duet_ps_link *links, const uint32_t *perm, uint32_t K, uint32_t min_sv,
                                                     const uint64_t *node, const Forest f)
{
    const uint64_t r64 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r64 >= f.n) return;
    const uint32_t r = (uint32_t)r64, i = perm[r], N = rows_of(f.hdr, f.V);
    uint32_t a = kNone, b = kNone, s = 0;
    if (i < f.n) {
        const duet_ps_link *l = links + i;
        const uint32_t k = l->contig;
        const uint64_t kk = (uint64_t)(k < K ? k : 0u) << 32, ka = kk | l->ps_a, kb = kk | l->ps_b;
        const uint32_t ia = lower_bound_u64(node, N, ka), ib = lower_bound_u64(node, N, kb);
        if (ia < N && ib < N && node[ia] == ka && node[ib] == kb) {
            const Win v = win_of(l, min_sv);
            a = ia; b = ib;
            s = v.sense | (v.trusted ? 2u : 0u);
        }
    }
    f.ea[r] = a; f.eb[r] = b; f.es[r] = s;
    f.in_forest[r] = 0;
}

// every node its own root, parity 0; no offer, no smallest node yet
__global__ __launch_bounds__(kThreads) void pb_init(uint32_t *P, const Forest f)
{
    const uint64_t x = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (x >= f.V) return;
    P[x] = (uint32_t)x << 1;
    f.best[x] = kNone;
    f.minnode[x] = kNone;
}

// P is flat here: P[x] >> 1 is the root of x, P[x] & 1 the sense of x relative to it
__global__ __launch_bounds__(kThreads) void pb_best(const uint32_t *P, const Forest f)
{
    const uint64_t r64 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r64 >= f.n) return;
    const uint32_t r = (uint32_t)r64, a = f.ea[r], b = f.eb[r];
    if (!(f.es[r] & 2u) || a >= f.V || b >= f.V) return;
    const uint32_t ra = P[a] >> 1, rb = P[b] >> 1;
    if (ra == rb || ra >= f.V || rb >= f.V) return;
    atomicMin(f.best + ra, r);
    atomicMin(f.best + rb, r);
}

__global__ __launch_bounds__(kThreads) void pb_hook(const uint32_t *P, uint32_t *Pn, const Forest f)
{
    const uint64_t v64 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v64 >= rows_of(f.hdr, f.V)) return;
    const uint32_t v = (uint32_t)v64, p = P[v];
    uint32_t out = p;
    const uint32_t r = (p >> 1) == v ? f.best[v] : kNone;
    if (r < f.n) {
        const uint32_t a = f.ea[r], b = f.eb[r];
        if (a < f.V && b < f.V) {
            const uint32_t pa = P[a], pb = P[b], ra = pa >> 1, rb = pb >> 1;
            const uint32_t other = ra == v ? rb : ra;
            // (two roots that chose one link: the smaller index stays the root; longer cycles cannot form under a strict order)
            if (other < f.V && other != v && !(f.best[other] == r && v < other)) {
                out = (other << 1) | ((pa ^ pb ^ f.es[r]) & 1u);
                f.in_forest[r] = 1u;
            }
        }
    }
    Pn[v] = out;
}

__global__ __launch_bounds__(kThreads) void pb_jump(const uint32_t *P, uint32_t *Pn, const Forest f, uint32_t clear_best)
{
    const uint64_t x64 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (x64 >= rows_of(f.hdr, f.V)) return;
    const uint32_t x = (uint32_t)x64, p = P[x];
    uint32_t out = p;
    if ((p >> 1) < f.V) {
        const uint32_t q = P[p >> 1];
        out = (q & ~1u) | ((p ^ q) & 1u);
    }
    Pn[x] = out;
    if (clear_best) f.best[x] = kNone;
}

__global__ __launch_bounds__(kThreads) void pb_min(const uint32_t *P, const Forest f)
{
    const uint64_t x64 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (x64 >= rows_of(f.hdr, f.V)) return;
    const uint32_t root = P[x64] >> 1;
    if (root < f.V) atomicMin(f.minnode + root, (uint32_t)x64);
}

// rows: the table of blocks(); key / val: the same table as pj_tags reads it (PS; flip << 32 | block).  Either may be null.
__global__ __launch_bounds__(kThreads) void pb_rows(const uint32_t *P, const uint64_t *node, const Forest f, duet_ps_block *rows, uint32_t *key,
                                                     uint64_t *val, uint32_t *hdr)
{
    const uint64_t x64 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    bool first = false;
    if (x64 < rows_of(f.hdr, f.V)) {
        const uint32_t x = (uint32_t)x64, p = P[x], root = p >> 1;
        uint32_t m = root < f.V ? f.minnode[root] : x;
        if (m >= f.V) m = x;
        const uint64_t kx = node[x];
        const uint32_t block = (uint32_t)node[m], flip = (p ^ P[m]) & 1u;
        first = m == x;
        if (rows) {
            duet_ps_block b;
            b.contig = (uint32_t)(kx >> 32); b.ps = (uint32_t)kx; b.block = block; b.flip = flip;
            rows[x] = b;
        }
        if (key) {
            key[x] = (uint32_t)kx;
            val[x] = ((uint64_t)flip << 32) | block;
        }
    }
    const unsigned long long m = __ballot(first);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(hdr + kComp, (uint32_t)__popcll(m));
}

// rank r is a conflict: trusted, not a link of the forest, and the parities of its ends differ from its sense
struct LoadConflict {
    Forest f;
    const uint32_t *P;
    __device__ __forceinline__ uint32_t operator()(uint32_t r) const
    {
        const uint32_t a = f.ea[r], b = f.eb[r], s = f.es[r];
        if (!(s & 2u) || f.in_forest[r] || a >= f.V || b >= f.V) return 0u;
        return (P[a] ^ P[b] ^ s) & 1u;
    }
};
struct StoreConflict {              // conflicts[number] = the record's row index
    const uint32_t *perm;
    uint32_t *conf, n;
    __device__ __forceinline__ void operator()(uint32_t r, uint32_t before, uint32_t is) const
    {
        if (is && before < n) conf[before] = perm[r];
    }
};

// slice_off[k] = the first node of contig k, slice_off[K] = the nodes; all zero (an empty table) after a refusal
__global__ __launch_bounds__(kThreads) void pb_slices(const uint64_t *node, uint32_t K, uint32_t V, const uint32_t *hdr, uint32_t *slice_off)
{
    const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k > K) return;
    const uint32_t N = rows_of(hdr, V);
    slice_off[k] = hdr[kBad] ? 0u : (k == K ? N : lower_bound_u64(node, N, k << 32));
}

uint32_t grid(uint64_t n) { return (uint32_t)((n + kThreads - 1) / kThreads); }

struct Built {                      // what a build leaves in the workspace
    uint32_t *hdr;                  // [kHdrWords]
    duet_ps_block *rows;            // [2 n] (with want_rows)
    uint32_t *conf;                 // [n]
    uint32_t *slice_off, *key;      // [K + 1], [2 n] (with want_table)
    uint64_t *val;                  // [2 n]
    uint32_t *read_off;             // [K + 1] room for the caller's offsets (with want_table)
};

// links: device memory, n >= 1 records, K >= 1.  Everything is enqueued on st; nothing is read back.
int build(duet_ctx *ctx, const duet_ps_link *links, uint32_t n, uint32_t K, uint32_t min_sv, bool want_rows, bool want_table, hipStream_t st,
          Built &o)
{
    const uint32_t V = 2u * n;
    const uint32_t nb_rx = (V + kRxTile - 1) / kRxTile, nb_sc = (V + kScanTile - 1) / kScanTile;
    const uint32_t nb_hs = (256u * nb_rx + kScanTile - 1) / kScanTile;
    Arena a;
    const size_t o_hdr = a.take(kHdrWords * 4), o_ka = a.take((size_t)V * 8), o_kb = a.take((size_t)V * 8), o_node = a.take((size_t)V * 8),
                 o_rka = a.take((size_t)n * 8), o_rkb = a.take((size_t)n * 8), o_rva = a.take((size_t)n * 4), o_rvb = a.take((size_t)n * 4),
                 o_ea = a.take((size_t)n * 4), o_eb = a.take((size_t)n * 4), o_es = a.take((size_t)n * 4), o_if = a.take((size_t)n * 4),
                 o_p0 = a.take((size_t)V * 4), o_p1 = a.take((size_t)V * 4), o_best = a.take((size_t)V * 4), o_min = a.take((size_t)V * 4),
                 o_hist = a.take((size_t)256 * nb_rx * 4), o_part = a.take(((size_t)(nb_sc > nb_hs ? nb_sc : nb_hs) + 1) * 4),
                 o_conf = a.take((size_t)n * 4), o_rows = a.take(want_rows ? (size_t)V * sizeof(duet_ps_block) : 0),
                 o_sl = a.take(want_table ? ((size_t)K + 1) * 4 : 0), o_ro = a.take(want_table ? ((size_t)K + 1) * 4 : 0),
                 o_val = a.take(want_table ? (size_t)V * 8 : 0), o_key = a.take(want_table ? (size_t)V * 4 : 0);
    DevBuf &ws = ctx->psblocks_ws.b[0];
    int rc;
    if ((rc = duet_reserve(ctx, ws, a.total))) return rc;
    char *w = (char *)ws.ptr;
    uint32_t *hdr = (uint32_t *)(w + o_hdr), *rvA = (uint32_t *)(w + o_rva), *rvB = (uint32_t *)(w + o_rvb), *P0 = (uint32_t *)(w + o_p0),
             *P1 = (uint32_t *)(w + o_p1), *hist = (uint32_t *)(w + o_hist), *spart = (uint32_t *)(w + o_part);
    uint64_t *kA = (uint64_t *)(w + o_ka), *kB = (uint64_t *)(w + o_kb), *node = (uint64_t *)(w + o_node), *rkA = (uint64_t *)(w + o_rka),
             *rkB = (uint64_t *)(w + o_rkb);
    Forest f;
    f.n = n; f.V = V; f.hdr = hdr;
    f.ea = (uint32_t *)(w + o_ea); f.eb = (uint32_t *)(w + o_eb); f.es = (uint32_t *)(w + o_es); f.in_forest = (uint32_t *)(w + o_if);
    f.best = (uint32_t *)(w + o_best); f.minnode = (uint32_t *)(w + o_min);
    o.hdr = hdr;
    o.conf = (uint32_t *)(w + o_conf);
    o.rows = want_rows ? (duet_ps_block *)(w + o_rows) : nullptr;
    o.slice_off = want_table ? (uint32_t *)(w + o_sl) : nullptr;
    o.read_off = want_table ? (uint32_t *)(w + o_ro) : nullptr;
    o.key = want_table ? (uint32_t *)(w + o_key) : nullptr;
    o.val = want_table ? (uint64_t *)(w + o_val) : nullptr;

    HIP_TRY(ctx, hipMemsetAsync(hdr, 0, kHdrWords * 4, st));
    hipLaunchKernelGGL(pb_keys, dim3(grid(n)), dim3(kThreads), 0, st, links, n, K, min_sv, kA, rkA, rvA, hdr);
    // ---- the nodes ----
    const uint32_t node_bits = 32u + bits_for((uint64_t)K - 1u);
    uint64_t *sk = nullptr;
    radix_sort_pairs(kA, kB, nullptr, nullptr, V, node_bits, hist, spart, ctx->rx_dtot, st, &sk, nullptr, nullptr);
    launch_scan<0>(LoadNodeHead{sk}, V, spart, StoreNode{sk, node}, hdr + kRows, st);
    // ---- the ranks ----
    uint64_t *k1 = nullptr, *k1_spare = nullptr, *k2 = nullptr;
    uint32_t *perm1 = nullptr, *perm = nullptr;
    radix_sort_pairs(rkA, rkB, rvA, rvB, n, 64u, hist, spart, ctx->rx_dtot, st, &k1, &perm1, &k1_spare);
    uint32_t *perm1_spare = perm1 == rvA ? rvB : rvA;
    hipLaunchKernelGGL(pb_key_n, dim3(grid(n)), dim3(kThreads), 0, st, links, (const uint32_t *)perm1, n, min_sv, k1_spare);
    radix_sort_pairs(k1_spare, k1, perm1, perm1_spare, n, 33u, hist, spart, ctx->rx_dtot, st, &k2, &perm, nullptr);
    hipLaunchKernelGGL(pb_ends, dim3(grid(n)), dim3(kThreads), 0, st, links, (const uint32_t *)perm, K, min_sv, (const uint64_t *)node, f);
    hipLaunchKernelGGL(pb_init, dim3(grid(V)), dim3(kThreads), 0, st, P0, f);
    // ---- the forest.  A component that still has a link to another one at round r has merged in every round before: it holds
    // at least 2^r nodes, so there are at most V >> r of them (none when that is below 2); the roots they hook into chains of at
    // most that many, which bits_for(V >> r) jumps flatten ----
    uint32_t *P = P0, *Pn = P1;
    for (uint32_t r = 0; (V >> r) >= 2u; ++r) {
        hipLaunchKernelGGL(pb_best, dim3(grid(n)), dim3(kThreads), 0, st, (const uint32_t *)P, f);
        hipLaunchKernelGGL(pb_hook, dim3(grid(V)), dim3(kThreads), 0, st, (const uint32_t *)P, Pn, f);
        std::swap(P, Pn);
        const uint32_t jumps = bits_for(V >> r);
        for (uint32_t j = 0; j < jumps; ++j) {
            hipLaunchKernelGGL(pb_jump, dim3(grid(V)), dim3(kThreads), 0, st, (const uint32_t *)P, Pn, f, j == 0 ? 1u : 0u);
            std::swap(P, Pn);
        }
    }
    // ---- the rows, the conflicts, the slices ----
    hipLaunchKernelGGL(pb_min, dim3(grid(V)), dim3(kThreads), 0, st, (const uint32_t *)P, f);
    hipLaunchKernelGGL(pb_rows, dim3(grid(V)), dim3(kThreads), 0, st, (const uint32_t *)P, (const uint64_t *)node, f, o.rows, o.key, o.val, hdr);
    launch_scan<0>(LoadConflict{f, P}, n, spart, StoreConflict{perm, o.conf, n}, hdr + kConf, st);
    if (want_table)
        hipLaunchKernelGGL(pb_slices, dim3(grid((uint64_t)K + 1)), dim3(kThreads), 0, st, (const uint64_t *)node, K, V, (const uint32_t *)hdr,
                           o.slice_off);
    HIP_TRY(ctx, hipGetLastError());
    return DUET_OK;
}

int refusal(duet_ctx *ctx, uint32_t bad)
{
    if (bad & kBadOrder) return fail(ctx, DUET_ERR_INVALID, "ps blocks: a record's ps_a is not below its ps_b");
    if (bad & kBadContig) return fail(ctx, DUET_ERR_INVALID, "ps blocks: a record's contig is not below the contig count");
    return fail(ctx, DUET_ERR_INVALID, "ps blocks: the records do not strictly ascend by (contig, ps_a, ps_b)");
}

int check_args(duet_ctx *ctx, const duet_ps_link *links, uint32_t n_links, uint32_t K, uint32_t min_sv, duet_ps_blocks_counts *counts)
{
    if (counts) memset(counts, 0, sizeof(*counts));
    if (!ctx) return fail(nullptr, DUET_ERR_INVALID, "null context");
    if (!counts || (n_links && !links)) return fail(ctx, DUET_ERR_INVALID, "null argument");
    if (min_sv < 1) return fail(ctx, DUET_ERR_INVALID, "ps blocks: min_sv below 1");
    if (n_links >= kMaxLinks) return fail(ctx, DUET_ERR_INVALID, "ps blocks: 2^30 records or more");
    if (n_links && K == 0) return fail(ctx, DUET_ERR_INVALID, "ps blocks: a record's contig is not below the contig count");
    return DUET_OK;
}

// links: device memory; the outputs device memory, or with out_on_host host memory
int blocks_run(duet_ctx *ctx, const duet_ps_link *links, uint32_t n, uint32_t K, uint32_t min_sv, duet_ps_block *out_rows, uint32_t rows_cap,
               uint32_t *out_conflicts, uint32_t conflicts_cap, duet_ps_blocks_counts *counts, hipStream_t st, bool out_on_host)
{
    Built b;
    int rc;
    if ((rc = build(ctx, links, n, K, min_sv, true, false, st, b))) return rc;
    uint32_t hdr[kHdrWords];
    HIP_TRY(ctx, hipMemcpyAsync(hdr, b.hdr, sizeof(hdr), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                      // the one round trip: the counts and the refusals
    if (hdr[kBad]) return refusal(ctx, hdr[kBad]);
    if (hdr[kRows] > 2u * n || hdr[kConf] > n) return fail(ctx, DUET_ERR_HIP, "ps blocks: more rows than ends, or more conflicts than records");
    if (hdr[kRows] > rows_cap) return fail(ctx, DUET_ERR_INVALID, "ps blocks: the row buffer is too small (rows_cap below n_rows)");
    if (out_conflicts && hdr[kConf] > conflicts_cap)             // (no conflict buffer: the count alone is wanted)
        return fail(ctx, DUET_ERR_INVALID, "ps blocks: the conflict buffer is too small (conflicts_cap below n_conflicts)");
    const hipMemcpyKind kind = out_on_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (hdr[kRows]) HIP_TRY(ctx, hipMemcpyAsync(out_rows, b.rows, (size_t)hdr[kRows] * sizeof(duet_ps_block), kind, st));
    if (out_conflicts && hdr[kConf]) HIP_TRY(ctx, hipMemcpyAsync(out_conflicts, b.conf, (size_t)hdr[kConf] * 4, kind, st));
    if (out_on_host) HIP_TRY(ctx, hipStreamSynchronize(st));
    counts->n_rows = hdr[kRows]; counts->n_trusted = hdr[kTrusted]; counts->n_conflicts = hdr[kConf]; counts->n_components = hdr[kComp];
    return DUET_OK;
}

}  // namespace

extern "C" {

int duet_ps_blocks_device(duet_ctx *ctx, const duet_ps_link *links, uint32_t n_links, uint32_t n_contigs, uint32_t min_sv,
                          duet_ps_block *out_rows, uint32_t rows_cap, uint32_t *out_conflicts, uint32_t conflicts_cap,
                          duet_ps_blocks_counts *counts, void *stream_)
{
    int rc = check_args(ctx, links, n_links, n_contigs, min_sv, counts);
    if (rc) return rc;
    if ((rows_cap && !out_rows) || (conflicts_cap && !out_conflicts)) return fail(ctx, DUET_ERR_INVALID, "null argument");
    if (n_links == 0) return DUET_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return blocks_run(ctx, links, n_links, n_contigs, min_sv, out_rows, rows_cap, out_conflicts, conflicts_cap, counts, (hipStream_t)stream_,
                      false);
}

int duet_ps_blocks_host(duet_ctx *ctx, const duet_ps_link *links, uint32_t n_links, uint32_t n_contigs, uint32_t min_sv,
                        duet_ps_block *out_rows, uint32_t rows_cap, uint32_t *out_conflicts, uint32_t conflicts_cap,
                        duet_ps_blocks_counts *counts)
{
    int rc = check_args(ctx, links, n_links, n_contigs, min_sv, counts);
    if (rc) return rc;
    if ((rows_cap && !out_rows) || (conflicts_cap && !out_conflicts)) return fail(ctx, DUET_ERR_INVALID, "null argument");
    if (n_links == 0) return DUET_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->own_stream;
    // staging 1: the records
    const void *src[1] = {links};
    const size_t bytes[1] = {(size_t)n_links * sizeof(duet_ps_link)};
    void *dev[1];
    if ((rc = duet_stage_arrays(ctx, ctx->psblocks_ws.b + 1, src, bytes, 1, s, dev))) return rc;
    return blocks_run(ctx, (const duet_ps_link *)dev[0], n_links, n_contigs, min_sv, out_rows, rows_cap, out_conflicts, conflicts_cap, counts,
                      s, true);
}

int duet_ps_join_links_device(duet_ctx *ctx, const duet_ps_link *links, uint32_t n_links, uint32_t min_sv, const uint64_t *read_tag,
                              const uint32_t *read_off, uint32_t n_contigs, uint32_t n_reads, uint64_t *out_tag,
                              duet_ps_blocks_counts *counts, uint32_t *n_changed, void *stream_)
{
    if (n_changed) *n_changed = 0;
    int rc = check_args(ctx, links, n_links, n_contigs, min_sv, counts);
    if (rc) return rc;
    const uint32_t K = n_contigs, R = n_reads;
    if (!n_changed || !read_off || (R && (!read_tag || !out_tag))) return fail(ctx, DUET_ERR_INVALID, "null argument");
    if (K == 0 && R) return fail(ctx, DUET_ERR_INVALID, "ps join: no contig (n_contigs is 0)");
    bool ok = read_off[0] == 0 && read_off[K] == R;
    for (uint32_t k = 0; ok && k < K; ++k) ok = read_off[k] <= read_off[k + 1];
    if (!ok) return fail(ctx, DUET_ERR_INVALID, "ps join: read_off does not ascend from 0 to n_reads");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream_;
    if (n_links == 0) {
        if (R && out_tag != read_tag) HIP_TRY(ctx, hipMemcpyAsync(out_tag, read_tag, (size_t)R * 8, hipMemcpyDeviceToDevice, st));
        return DUET_OK;
    }
    Built b;
    if ((rc = build(ctx, links, n_links, K, min_sv, false, true, st, b))) return rc;
    if (R) {
        HIP_TRY(ctx, hipMemcpyAsync(b.read_off, read_off, ((size_t)K + 1) * 4, hipMemcpyHostToDevice, st));
        // (the table's row count stays on the device: its bound stands for it, as the "no such row" index)
        if ((rc = duet_ps_join_tags_staged(ctx, read_tag, b.read_off, K, R, b.slice_off, b.key, b.val, 2u * n_links, out_tag, b.hdr + kPjHdr, st)))
            return rc;
    }
    uint32_t hdr[kHdrWords];
    HIP_TRY(ctx, hipMemcpyAsync(hdr, b.hdr, sizeof(hdr), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                      // the one round trip: the counts, the refusals, the changed words
    if (hdr[kBad]) return refusal(ctx, hdr[kBad]);
    counts->n_rows = hdr[kRows]; counts->n_trusted = hdr[kTrusted]; counts->n_conflicts = hdr[kConf]; counts->n_components = hdr[kComp];
    *n_changed = hdr[kPjHdr];
    return DUET_OK;
}

}  // extern "C"
