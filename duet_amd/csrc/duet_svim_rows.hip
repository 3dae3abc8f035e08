// duet_svim_rows.hip -- gfx950 kernels and C ABI for the last step of the svim-gpu mode on the device: from a cluster result and
// its (pred, ps) to the data rows of phased_sv.vcf, as text.
//
// What it restates: duet_amd/svim_mode.py rows_text -- the rows of src/duet/write_file.py:6-17 with symbolic alleles, the SVLEN
// sign rule of src/duet/sv_phasing_fn.py:225 (positive for INS and DUP), the stable sort of :229 (CHROM as text, POS as int; ties
// keep candidate order).
//
// Pipeline (one stream):
//   scan + compaction     kept = pred != 0; the scan's store writes the kept candidates' indices
//   sr_check_len          per kept candidate: pred <= 3 and contig < K (status word), the row's length without its row number,
//                         summed in 64 bits; the largest POS (the sort covers exactly the bits in use)
//   (ONE host round trip: the row count, the status word, the sum, the largest POS.  The digits of the row numbers 1..n_rows
//   add up to a number the host knows from n_rows alone, so the text's exact size is known here, before the sort.)
//   sr_keys               key = rank(CHROM text) << pos_bits | POS, value = the candidate
//   radix sort            stable LSD over exactly the bits in use
//   sr_tile_len           bytes of every tile of 64 consecutive rows -> scan_spine_u64 (one workgroup, 64-bit) -> tile offsets
//   sr_write              one workgroup per tile; see there
//
// CHROM's byte-order rank among the distinct texts is computed by the host once per call (equal texts share a rank).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "duet_ef.h"
#include "duet_internal.h"

namespace {

#include "duet_prims.hip.h"
#include "duet_text.hip.h"

constexpr uint32_t kSrRows = 64;                // rows per tile of sr_write: one wavefront stages them, a lane each
constexpr uint32_t kSrThreads = 256;
constexpr uint32_t kSrMaxChrom = 1u << 20;      // a tile's bytes are counted in 32 bits: 64 * (2^20 + 95) fits

struct SrParams {
    uint32_t C, K, N, pos_bits;
    const uint16_t *cand_contig;
    const uint8_t *cand_type;
    const uint32_t *cand_pos, *cand_span;
    const uint8_t *pred;
    const uint32_t *ps;
    const uint32_t *chrom_off;                  // [K + 1] into chrom_pool
    const uint16_t *chrom_rank;                 // [K]
    const char *chrom_pool;
    const uint32_t *sorted;                     // candidate of each row
    uint64_t *tile_off;                         // [tiles] bytes of each tile, then (scan_spine_u64) its offset in the text
    uint64_t *sum;                              // status block: [0] the rows' bytes without their row numbers
    uint32_t *flag, *max_pos;                   //               bit 0 pred > 3, bit 1 contig >= K, bit 2 a tile past out_cap
    char *out;
    uint64_t cap;
};

// The row behind CHROM, every number at its full ten digits and the sign present: 95 bytes.
//     \t PPPPPPPPPP \tDuet. NNNNNNNNNN \tN\t< TTT >\t.\tPASS\tSVLEN= - SSSSSSSSSS ;SVTYPE=< TTT >\tHP:PS\t h|h : QQQQQQQQQQ \n
//     0  1..10      11..16  17..26     27..30 31..33 34..48           49 50..59    60..68    69..71 72..79  80..82 83 84..93 94
// A real row leaves out the leading digit slots of each number and, where SVLEN is not negative, the sign: byte o of the row maps
// to a template position by adding, field after field, what the row left out in front of it (sr_byte).  The template holds a
// literal byte (< 0x80) or a code: 0x80 | field << 4 | k = digit 10^k of number `field` (0 POS, 1 row number, 2 span, 3 ps);
// 0xC0 | i = letter i of the type name; 0xE0 / 0xE1 = the two haplotype digits.
constexpr uint32_t kTplLen = 95, kTplP = 1, kTplN = 17, kTplSign = 49, kTplS = 50, kTplQ = 84;

struct SrTables {
    uint8_t tpl[96];
    uint8_t typ[12];
    uint32_t p10[10], magic[10];
};

constexpr SrTables sr_tables()
{
    SrTables t = {};
    // '#': a digit slot, '@': a letter of the type name, 'h': a haplotype digit
    const char lit[] = "\t##########\tDuet.##########\tN\t<@@@>\t.\tPASS\tSVLEN=-##########;SVTYPE=<@@@>\tHP:PS\th|h:##########\n";
    static_assert(sizeof(lit) == kTplLen + 1, "the template has 95 bytes");
    uint32_t field = 0, slot = 0, letter = 0, hap = 0;
    for (uint32_t i = 0; i < kTplLen; ++i) {
        const char c = lit[i];
        if (c == '#') {
            t.tpl[i] = (uint8_t)(0x80u | (field << 4) | (9u - slot));
            if (++slot == 10) { slot = 0; ++field; }
        } else if (c == '@') {
            t.tpl[i] = (uint8_t)(0xC0u | (letter++ % 3u));
        } else if (c == 'h') {
            t.tpl[i] = (uint8_t)(0xE0u | hap++);
        } else {
            t.tpl[i] = (uint8_t)c;
        }
    }
    const char names[] = "DELINSINVDUP";
    for (uint32_t i = 0; i < 12; ++i) t.typ[i] = (uint8_t)names[i];
    uint32_t p = 1;
    for (uint32_t k = 0; k < 10; ++k) {
        t.p10[k] = p;
        t.magic[k] = k ? (uint32_t)((1ull << 32) / p) : 0xFFFFFFFFu;      // v / 10^k = umulhi(v, magic), or one more (sr_byte)
        if (k < 9) p *= 10u;
    }
    return t;
}

constexpr SrTables kSrHostTab = sr_tables();
static_assert(kSrHostTab.tpl[kTplP] == 0x89 && kSrHostTab.tpl[kTplN] == 0x99 && kSrHostTab.tpl[kTplSign] == '-' &&
              kSrHostTab.tpl[kTplS] == 0xA9 && kSrHostTab.tpl[kTplQ] == 0xB9 && kSrHostTab.tpl[kTplQ + 9] == 0xB0 &&
              kSrHostTab.tpl[31] == 0xC0 && kSrHostTab.tpl[71] == 0xC2 && kSrHostTab.tpl[80] == 0xE0 && kSrHostTab.tpl[82] == 0xE1 &&
              kSrHostTab.tpl[94] == '\n', "template positions");
__device__ __constant__ const SrTables kSrTab = sr_tables();

// what a row leaves out of the template, and its two small fields
//   bits 0-3 POS slots, 4-7 row-number slots, 8 the sign, 9-12 span slots, 13-16 ps slots, 17-18 type, 19-20 pred
__device__ __forceinline__ uint32_t sr_pack(uint32_t pos, uint32_t n, uint32_t span, uint32_t ps, uint32_t type, uint32_t pred)
{
    const uint32_t neg = ((type & 1u) == 0u && span != 0u) ? 1u : 0u;          // INS (1) and DUP (3) are written positive
    return (10u - digits_u32(pos)) | (10u - digits_u32(n)) << 4 | (1u - neg) << 8 | (10u - digits_u32(span)) << 9 |
           (10u - digits_u32(ps)) << 13 | (type & 3u) << 17 | (pred & 3u) << 19;
}

__device__ __forceinline__ uint32_t sr_left_out(uint32_t pk)
{
    return (pk & 15u) + ((pk >> 4) & 15u) + ((pk >> 8) & 1u) + ((pk >> 9) & 15u) + ((pk >> 13) & 15u);
}

struct SrRow {
    uint32_t len, L, choff, pos, span, ps, pk;
};

// row j (0-based) of the sorted order
__device__ __forceinline__ SrRow sr_row(const SrParams &p, uint32_t j)
{
    SrRow r;
    const uint32_t c = p.sorted[j];
    const uint32_t k = p.cand_contig[c];
    r.choff = p.chrom_off[k];
    r.L = p.chrom_off[k + 1] - r.choff;
    r.pos = p.cand_pos[c];
    r.span = p.cand_span[c];
    r.ps = p.ps[c];
    r.pk = sr_pack(r.pos, j + 1u, r.span, r.ps, p.cand_type[c], p.pred[c]);
    r.len = r.L + kTplLen - sr_left_out(r.pk);
    return r;
}

__global__ __launch_bounds__(256) void sr_check_len(const SrParams p)
{
    __shared__ uint64_t s_sum[4];
    __shared__ uint32_t s_max[4], s_bad[4];
    const uint32_t c = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t len = 0;
    uint32_t mx = 0, bad = 0;
    if (c < p.C) {
        const uint32_t pr = p.pred[c];
        if (pr) {
            const uint32_t k = p.cand_contig[c];
            bad = (pr > 3u ? 1u : 0u) | (k >= p.K ? 2u : 0u);
            if (!bad) {
                mx = p.cand_pos[c];
                // (row number 0: one digit, taken off again -- the host adds the digits of 1..n_rows)
                const uint32_t pk = sr_pack(mx, 0u, p.cand_span[c], p.ps[c], p.cand_type[c], pr);
                len = (uint64_t)(p.chrom_off[k + 1] - p.chrom_off[k]) + (kTplLen - 1u - sr_left_out(pk));
            }
        }
    }
#pragma unroll
    for (uint32_t d = 32; d > 0; d >>= 1) {
        len += shfl_xor_u64(len, d);
        const uint32_t m2 = __shfl_xor(mx, d, 64), b2 = __shfl_xor(bad, d, 64);
        mx = mx > m2 ? mx : m2;
        bad |= b2;
    }
    if (lane == 0) { s_sum[wave] = len; s_max[wave] = mx; s_bad[wave] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint64_t t = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        const uint32_t m = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3])), b = s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3];
        if (t) atomicAdd((unsigned long long *)p.sum, (unsigned long long)t);
        if (m) atomicMax(p.max_pos, m);
        if (b) atomicOr(p.flag, b);
    }
}

__global__ __launch_bounds__(256) void sr_keys(const SrParams p, const uint32_t *idx, uint64_t *keys, uint32_t *vals)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= p.N) return;
    const uint32_t c = idx[j];
    keys[j] = ((uint64_t)p.chrom_rank[p.cand_contig[c]] << p.pos_bits) | p.cand_pos[c];
    vals[j] = c;
}

// a wavefront per tile: tile_off[t] <- the bytes of rows [64 t, 64 t + 64)
__global__ __launch_bounds__(256) void sr_tile_len(const SrParams p, uint32_t n_tiles)
{
    const uint32_t lane = threadIdx.x & 63u, tile = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    const uint32_t j = tile * kSrRows + lane;
    const uint32_t len = wave_sum(j < p.N ? sr_row(p, j).len : 0u);
    if (lane == 0) p.tile_off[tile] = len;
}

// what sr_write keeps in LDS: the tile's rows (a field per array: lanes on neighbouring rows read neighbouring words) and the tables
struct SrShared {
    uint32_t start[kSrRows + 1];                // byte offset of each row within the tile; [64] = the tile's bytes
    uint32_t L[kSrRows], choff[kSrRows], pos[kSrRows], span[kSrRows], ps[kSrRows], pk[kSrRows];
    uint32_t p10[10], magic[10];
    uint8_t tpl[96], typ[12];
};

// the row's fields in registers
struct SrCur {
    uint32_t start, end, L, choff, pos, n, span, ps, pk;
};

__device__ __forceinline__ SrCur sr_load(const SrShared &s, uint32_t i, uint32_t n)
{
    SrCur r;
    r.start = s.start[i]; r.end = s.start[i + 1];
    r.L = s.L[i]; r.choff = s.choff[i]; r.pos = s.pos[i]; r.span = s.span[i]; r.ps = s.ps[i]; r.pk = s.pk[i];
    r.n = n;
    return r;
}

// byte o of the row
__device__ __forceinline__ uint32_t sr_byte(const SrShared &s, const SrCur &r, uint32_t o, const char *pool)
{
    if (o < r.L) return (uint8_t)pool[r.choff + o];
    uint32_t t = o - r.L;
    t += t >= kTplP ? (r.pk & 15u) : 0u;
    t += t >= kTplN ? ((r.pk >> 4) & 15u) : 0u;
    t += t >= kTplSign ? ((r.pk >> 8) & 1u) : 0u;
    t += t >= kTplS ? ((r.pk >> 9) & 15u) : 0u;
    t += t >= kTplQ ? ((r.pk >> 13) & 15u) : 0u;
    const uint32_t code = s.tpl[t];
    if (code < 0x80u) return code;
    if (code & 0x40u) {
        const uint32_t hp = (r.pk >> 19) & 3u;                                  // 1: 1|0, 2: 0|1, 3: 1|1
        if (code & 0x20u) return (code & 1u) ? (hp == 1u ? '0' : '1') : (hp == 2u ? '0' : '1');
        return s.typ[3u * ((r.pk >> 17) & 3u) + (code & 3u)];
    }
    const uint32_t f = (code >> 4) & 3u, k = code & 15u;
    const uint32_t v = f == 0u ? r.pos : (f == 1u ? r.n : (f == 2u ? r.span : r.ps));
    const uint32_t pw = s.p10[k];
    uint32_t q = __umulhi(v, s.magic[k]);                                       // floor(v / 10^k) or one less
    q += (v - q * pw >= pw) ? 1u : 0u;
    return '0' + q % 10u;
}

// the last row of the tile's first nr that starts at or before byte b
__device__ __forceinline__ uint32_t sr_find(const SrShared &s, uint32_t nr, uint32_t b)
{
    uint32_t i = 0;
#pragma unroll
    for (uint32_t step = kSrRows / 2; step > 0; step >>= 1)
        if (i + step < nr && s.start[i + step] <= b) i += step;
    return i;
}

// One workgroup per tile of 64 consecutive rows -- a contiguous piece of the text, 5.4 KB at 84 bytes a row.  The first wavefront
// stages the rows' numbers and lengths in LDS (a lane per row) and scans the lengths; then EVERY lane works out bytes of its own:
// thread t takes the aligned dwords t, t + 256, ... of the piece, finds the row of the dword's first byte (six compares in LDS),
// derives each of its four bytes from the row's numbers (sr_byte: a template position by five compares, a digit by one multiply
// with a table entry) and stores the dword.  A dword spans at most two rows (a row has 30 bytes or more).  The piece's up to
// three bytes in front of the first aligned address and behind the last go out as bytes, so no workgroup touches a neighbour's.
__global__ __launch_bounds__(kSrThreads) void sr_write(const SrParams p)
{
    __shared__ SrShared s;
    const uint32_t tid = threadIdx.x;
    const uint32_t j0 = blockIdx.x * kSrRows, nr = min(kSrRows, p.N - j0);
    if (tid >= 64u && tid < 64u + 96u) s.tpl[tid - 64u] = kSrTab.tpl[tid - 64u];
    if (tid >= 160u && tid < 172u) s.typ[tid - 160u] = kSrTab.typ[tid - 160u];
    if (tid >= 192u && tid < 202u) { s.p10[tid - 192u] = kSrTab.p10[tid - 192u]; s.magic[tid - 192u] = kSrTab.magic[tid - 192u]; }
    if (tid < kSrRows) {
        SrRow r;
        r.len = r.L = r.choff = r.pos = r.span = r.ps = r.pk = 0u;
        if (tid < nr) r = sr_row(p, j0 + tid);
        const uint32_t x = wave_scan(r.len, tid);
        s.start[tid] = x - r.len;
        if (tid == kSrRows - 1u) s.start[kSrRows] = x;
        s.L[tid] = r.L; s.choff[tid] = r.choff; s.pos[tid] = r.pos; s.span[tid] = r.span; s.ps[tid] = r.ps; s.pk[tid] = r.pk;
    }
    __syncthreads();
    const uint32_t bytes = s.start[kSrRows];
    const uint64_t base = p.tile_off[blockIdx.x];
    if (base + bytes > p.cap) {                                                 // (the host checked the total: not reached)
        if (tid == 0) atomicOr(p.flag, 4u);
        return;
    }
    char *dst = p.out + base;
    const uint32_t mis = (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u), head = mis < bytes ? mis : bytes;
    const uint32_t nd = (bytes - head) >> 2, tail = bytes - head - 4u * nd;
    for (uint32_t d = tid; d < nd; d += kSrThreads) {
        const uint32_t b = head + 4u * d;
        uint32_t i = sr_find(s, nr, b);
        SrCur r = sr_load(s, i, j0 + i + 1u);
        uint32_t word = 0;
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            if (b + q >= r.end) {
                ++i;
                r = sr_load(s, i, j0 + i + 1u);
            }
            word |= sr_byte(s, r, b + q - r.start, p.chrom_pool) << (8u * q);
        }
        *reinterpret_cast<uint32_t *>(dst + b) = word;
    }
    if (tid < head + tail) {
        const uint32_t b = tid < head ? tid : 4u * nd + tid;                    // (head + 4 nd + (tid - head))
        const uint32_t i = sr_find(s, nr, b);
        const SrCur r = sr_load(s, i, j0 + i + 1u);
        dst[b] = (char)sr_byte(s, r, b - r.start, p.chrom_pool);
    }
}

// digits of 1..n written in decimal, all together
uint64_t digits_of_row_numbers(uint32_t n)
{
    uint64_t total = 0, lo = 1;
    for (uint32_t d = 1; d <= 10 && lo <= n; ++d, lo *= 10) {
        const uint64_t hi = std::min<uint64_t>(n, lo * 10 - 1);
        total += (hi - lo + 1) * d;
    }
    return total;
}

// the arrays of one call: device pointers, except the CHROM texts (HOST)
struct SrInputs {
    uint32_t C, K;
    const uint16_t *cand_contig;
    const uint8_t *cand_type;
    const uint32_t *cand_pos, *cand_span;
    const uint8_t *pred;
    const uint32_t *ps;
    const char *const *chrom;
};

int sr_check_args(duet_ctx *ctx, const duet_cluster_result *res, uint32_t n_cands, const uint8_t *pred, const uint32_t *ps,
                  uint32_t n_contigs, const char *const *chrom, uint64_t *out_len, uint32_t *n_rows)
{
    if (!ctx) return duet_fail(nullptr, DUET_ERR_INVALID, "null context");
    if (!res || !out_len || !n_rows) return duet_fail(ctx, DUET_ERR_INVALID, "null argument");
    *out_len = 0;
    *n_rows = 0;
    if (n_contigs == 0 || n_contigs > 65535) return duet_fail(ctx, DUET_ERR_INVALID, "bad contig count (1 to 65535)");
    if (!chrom) return duet_fail(ctx, DUET_ERR_INVALID, "null CHROM text array");
    for (uint32_t k = 0; k < n_contigs; ++k) {
        if (!chrom[k]) return duet_fail(ctx, DUET_ERR_INVALID, "null CHROM text");
        if (strlen(chrom[k]) > kSrMaxChrom) return duet_fail(ctx, DUET_ERR_INVALID, "CHROM text longer than 1 MiB");
    }
    if (n_cands && (!res->cand_contig || !res->cand_type || !res->cand_pos || !res->cand_span || !pred || !ps))
        return duet_fail(ctx, DUET_ERR_INVALID, "null array");
    return DUET_OK;
}

// to_host: out_text is HOST memory -- the rows are written to the context's text buffer, copied, and the stream synchronised
int sr_run(duet_ctx *ctx, const SrInputs &in, char *out_text, uint64_t out_cap, uint64_t *out_len, uint32_t *n_rows, hipStream_t st,
           bool to_host)
{
    const uint32_t C = in.C, K = in.K;
    // CHROM: the texts in one pool, and each contig's rank among the distinct texts in unsigned byte order
    const DuetChromTable ct = duet_chrom_table(in.chrom, K, true);
    const uint32_t n_texts = ct.n_texts;
    const size_t off_bytes = ((size_t)K + 1) * 4, rank_bytes = ((size_t)K * 2 + 3) & ~(size_t)3;
    std::vector<char> small(off_bytes + rank_bytes + ct.pool.size());                 // one upload: offsets | ranks | pool
    memcpy(small.data(), ct.off.data(), off_bytes);
    memcpy(small.data() + off_bytes, ct.rank.data(), (size_t)K * 2);
    memcpy(small.data() + off_bytes + rank_bytes, ct.pool.data(), ct.pool.size());

    const uint32_t nb_rx = (C + kRxTile - 1) / kRxTile, nb_sc = (C + kScanTile - 1) / kScanTile;
    const uint32_t nb_hs = (256u * nb_rx + kScanTile - 1) / kScanTile;
    const uint32_t tiles_max = (C + kSrRows - 1) / kSrRows;
    const size_t sizes[9] = {(size_t)C * 4, (size_t)C * 8, (size_t)C * 8, (size_t)C * 4, (size_t)C * 4, (size_t)256 * nb_rx * 4,
                             ((size_t)(nb_sc > nb_hs ? nb_sc : nb_hs) + 1) * 4, 64 + small.size() + 64, (size_t)tiles_max * 8};
    DevBuf *ws = ctx->svim_rows_ws.b;
    int rc;
    for (int i = 0; i < 9; ++i)
        if ((rc = duet_reserve(ctx, ws[i], sizes[i]))) return rc;
    uint32_t *idx = (uint32_t *)ws[0].ptr;
    uint64_t *keysA = (uint64_t *)ws[1].ptr, *keysB = (uint64_t *)ws[2].ptr;
    uint32_t *valsA = (uint32_t *)ws[3].ptr, *valsB = (uint32_t *)ws[4].ptr;
    uint32_t *hist = (uint32_t *)ws[5].ptr, *spart = (uint32_t *)ws[6].ptr;
    char *sm = (char *)ws[7].ptr;                              // status: u64 sum | flag | max_pos | rows ; then the contig tables
    uint32_t *d_scal = (uint32_t *)sm;

    HIP_TRY(ctx, hipMemsetAsync(sm, 0, 32, st));
    HIP_TRY(ctx, hipMemcpyAsync(sm + 64, small.data(), small.size(), hipMemcpyHostToDevice, st));
    SrParams p;
    memset(&p, 0, sizeof(p));
    p.C = C; p.K = K;
    p.cand_contig = in.cand_contig; p.cand_type = in.cand_type; p.cand_pos = in.cand_pos; p.cand_span = in.cand_span;
    p.pred = in.pred; p.ps = in.ps;
    p.chrom_off = (const uint32_t *)(sm + 64);
    p.chrom_rank = (const uint16_t *)(sm + 64 + off_bytes);
    p.chrom_pool = sm + 64 + off_bytes + rank_bytes;
    p.tile_off = (uint64_t *)ws[8].ptr;
    p.sum = (uint64_t *)sm; p.flag = d_scal + 2; p.max_pos = d_scal + 3;
    // kept candidates, in candidate order; their checks and the bytes they take
    launch_scan<0>(LoadKeep{in.pred}, C, spart, StoreCompact{idx}, d_scal + 4, st);
    hipLaunchKernelGGL(sr_check_len, dim3((C + 255) / 256), dim3(256), 0, st, p);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t fin[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(fin, sm, 32, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (fin[2] & 1u) return duet_fail(ctx, DUET_ERR_INVALID, "a kept candidate's pred is not 1, 2 or 3");
    if (fin[2] & 2u) return duet_fail(ctx, DUET_ERR_INVALID, "a kept candidate's contig is not below n_contigs");
    const uint32_t N = fin[4];
    if (N == 0) return DUET_OK;
    const uint64_t need = (((uint64_t)fin[1] << 32) | fin[0]) + digits_of_row_numbers(N);
    *n_rows = N;
    *out_len = need;
    if (need > out_cap)
        return duet_fail(ctx, DUET_ERR_INVALID, "output buffer too small for the rows of phased_sv.vcf (*out_len = size needed)");
    if (!out_text) return duet_fail(ctx, DUET_ERR_INVALID, "null output buffer");
    char *d_out = out_text;
    if (to_host) {
        if ((rc = duet_reserve(ctx, ws[15], need + 64))) return rc;
        d_out = (char *)ws[15].ptr;
    }

    p.N = N;
    p.pos_bits = bits_for(fin[3]);
    const uint32_t key_bits = p.pos_bits + bits_for(n_texts - 1);
    hipLaunchKernelGGL(sr_keys, dim3((N + 255) / 256), dim3(256), 0, st, p, (const uint32_t *)idx, keysA, valsA);
    uint64_t *kin = nullptr;
    uint32_t *vin = nullptr;
    radix_sort_pairs(keysA, keysB, valsA, valsB, N, key_bits, hist, spart, ctx->rx_dtot, st, &kin, &vin, nullptr);
    p.sorted = vin;
    p.out = d_out;
    p.cap = need;
    const uint32_t n_tiles = (N + kSrRows - 1) / kSrRows;
    hipLaunchKernelGGL(sr_tile_len, dim3((n_tiles + 3) / 4), dim3(256), 0, st, p, n_tiles);
    hipLaunchKernelGGL(scan_spine_u64, dim3(1), dim3(1024), 0, st, p.tile_off, n_tiles, (uint64_t *)nullptr);
    hipLaunchKernelGGL(sr_write, dim3(n_tiles), dim3(kSrThreads), 0, st, p);
    HIP_TRY(ctx, hipGetLastError());
    if (!to_host) return DUET_OK;
    uint32_t flag = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&flag, p.flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out_text, d_out, need, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (flag & 4u) return duet_fail(ctx, DUET_ERR_INVALID, "the rows of phased_sv.vcf overran their offsets");
    return DUET_OK;
}

}  // namespace

extern "C" {

int duet_svim_phased_rows_device(duet_ctx *ctx, const duet_cluster_result *res, uint32_t n_cands, const uint8_t *pred,
                                 const uint32_t *ps, uint32_t n_contigs, const char *const *chrom, char *out_text, uint64_t out_cap,
                                 uint64_t *out_len, uint32_t *n_rows, void *stream)
{
    int rc;
    if ((rc = sr_check_args(ctx, res, n_cands, pred, ps, n_contigs, chrom, out_len, n_rows))) return rc;
    if (n_cands == 0) return DUET_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const SrInputs in = {n_cands, n_contigs, res->cand_contig, res->cand_type, res->cand_pos, res->cand_span, pred, ps, chrom};
    return sr_run(ctx, in, out_text, out_cap, out_len, n_rows, (hipStream_t)stream, false);
}

int duet_svim_phased_rows_host(duet_ctx *ctx, const duet_cluster_result *res, uint32_t n_cands, const uint8_t *pred,
                               const uint32_t *ps, uint32_t n_contigs, const char *const *chrom, char *out_text, uint64_t out_cap,
                               uint64_t *out_len, uint32_t *n_rows)
{
    int rc;
    if ((rc = sr_check_args(ctx, res, n_cands, pred, ps, n_contigs, chrom, out_len, n_rows))) return rc;
    if (n_cands == 0) return DUET_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->own_stream;
    const size_t N = n_cands;
    const void *src[6] = {res->cand_contig, res->cand_type, res->cand_pos, res->cand_span, pred, ps};
    const size_t bytes[6] = {N * 2, N, N * 4, N * 4, N, N * 4};
    void *dev[6];
    if ((rc = duet_stage_arrays(ctx, ctx->svim_rows_ws.b + 9, src, bytes, 6, s, dev))) return rc;
    const SrInputs in = {n_cands, n_contigs, (const uint16_t *)dev[0], (const uint8_t *)dev[1], (const uint32_t *)dev[2],
                         (const uint32_t *)dev[3], (const uint8_t *)dev[4], (const uint32_t *)dev[5], chrom};
    return sr_run(ctx, in, out_text, out_cap, out_len, n_rows, s, true);
}

}  // extern "C"
