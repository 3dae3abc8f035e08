// duet_text.hip.h -- device parts shared by the units that write rows as text (duet_rows.hip, duet_callset.hip,
// duet_svim_rows.hip, duet_evidence.hip): decimal digits, 64-bit shuffles, wave scans and sums, the 64-bit spine scan and the
// tile scans around it, the kept-candidate functors of the compaction scan, and the two steps of a row that one wavefront writes
// piece by piece.  Included inside each unit's
// anonymous namespace (after duet_prims.hip.h where the unit uses that too); nothing here needs it.

// decimal digits of v.  The compare chain is on rows_write's and sr_write's path, the loop on cs_write's: both stay.
__device__ __forceinline__ uint32_t digits_u32(uint32_t v)
{
    uint32_t d = 1;
    d += v >= 10u; d += v >= 100u; d += v >= 1000u; d += v >= 10000u; d += v >= 100000u;
    d += v >= 1000000u; d += v >= 10000000u; d += v >= 100000000u; d += v >= 1000000000u;
    return d;
}

__device__ __forceinline__ uint32_t digits_u64(uint64_t v)
{
    uint32_t d = 1;
    while (v >= 10u) { v /= 10u; ++d; }
    return d;
}

// v in decimal at dst -> the number of bytes
__device__ __forceinline__ uint32_t put_u32(char *dst, uint32_t v)
{
    const uint32_t n = digits_u32(v);
    for (uint32_t i = n; i-- > 0;) {
        dst[i] = (char)('0' + v % 10u);
        v /= 10u;
    }
    return n;
}

__device__ __forceinline__ uint32_t put_u64(char *dst, uint64_t v)
{
    const uint32_t n = digits_u64(v);
    for (uint32_t i = n; i-- > 0;) {
        dst[i] = (char)('0' + (uint32_t)(v % 10u));
        v /= 10u;
    }
    return n;
}

__device__ __forceinline__ uint32_t put_str(char *dst, const char *s)
{
    uint32_t n = 0;
    while (s[n]) { dst[n] = s[n]; ++n; }
    return n;
}

__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, uint32_t d)
{
    const uint32_t lo = __shfl_up((uint32_t)v, d, 64), hi = __shfl_up((uint32_t)(v >> 32), d, 64);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, uint32_t d)
{
    const uint32_t lo = __shfl_xor((uint32_t)v, d, 64), hi = __shfl_xor((uint32_t)(v >> 32), d, 64);
    return ((uint64_t)hi << 32) | lo;
}

// inclusive sum over the wavefront's lanes 0..lane (T: uint32_t or uint64_t), six steps
template <class T>
__device__ __forceinline__ T wave_scan(T x, uint32_t lane)
{
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        T y;
        if constexpr (sizeof(T) == 8) y = shfl_up_u64(x, d); else y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

// sum over the wavefront's 64 lanes, in every lane
template <class T>
__device__ __forceinline__ T wave_sum(T x)
{
#pragma unroll
    for (uint32_t d = 32; d > 0; d >>= 1) {
        if constexpr (sizeof(T) == 8) x += shfl_xor_u64(x, d); else x += __shfl_xor(x, d, 64);
    }
    return x;
}

// one workgroup: part[0..nb) <- exclusive sums (each thread a contiguous run); *total (may be null) <- the sum of everything
__global__ __launch_bounds__(1024) void scan_spine_u64(uint64_t *part, uint32_t nb, uint64_t *total)
{
    __shared__ uint64_t s_w[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t per = (nb + 1023u) / 1024u, lo = min(nb, tid * per), hi = min(nb, lo + per);
    uint64_t acc = 0;
    for (uint32_t i = lo; i < hi; ++i) acc += part[i];
    const uint64_t x = wave_scan(acc, lane);
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    uint64_t run = x - acc;
    for (uint32_t w = 0; w < wave; ++w) run += s_w[w];
    if (total && tid == 1023) *total = run + acc;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint64_t v = part[i];
        part[i] = run;
        run += v;
    }
}

// 64-bit exclusive scan of 32-bit row lengths, around scan_spine_u64 (row lengths are 32-bit, their sums are not): tiles of
// kThreads * kItems rows, one workgroup of kThreads (a multiple of 64, at most 1024) each.  Templates: only a unit that launches
// them compiles them.  (duet_callset.hip keeps the pair it had before these: cs_scan_reduce, cs_scan_apply.)
//   rows_scan_reduce    part[tile] <- the tile's sum
//   scan_spine_u64      part[] <- exclusive sums, *total
//   rows_scan_apply     row_off[i] <- part[tile] + the sum of the tile's rows before i
template <uint32_t kThreads, uint32_t kItems>
__global__ __launch_bounds__(kThreads) void rows_scan_reduce(const uint32_t *len, uint32_t n, uint64_t *part)
{
    __shared__ uint64_t s_w[kThreads / 64];
    const uint32_t tid = threadIdx.x, base = blockIdx.x * (kThreads * kItems) + tid * kItems;
    uint64_t acc = 0;
#pragma unroll
    for (uint32_t j = 0; j < kItems; ++j)
        if (base + j < n) acc += len[base + j];
    acc = wave_sum(acc);
    if ((tid & 63u) == 0) s_w[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        uint64_t sum = 0;
        for (uint32_t w = 0; w < kThreads / 64; ++w) sum += s_w[w];
        part[blockIdx.x] = sum;
    }
}

template <uint32_t kThreads, uint32_t kItems>
__global__ __launch_bounds__(kThreads) void rows_scan_apply(const uint32_t *len, uint32_t n, const uint64_t *part, uint64_t *row_off)
{
    __shared__ uint64_t s_w[kThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t base = blockIdx.x * (kThreads * kItems) + tid * kItems;
    uint32_t v[kItems];
    uint64_t acc = 0;
#pragma unroll
    for (uint32_t j = 0; j < kItems; ++j) {
        v[j] = base + j < n ? len[base + j] : 0u;
        acc += v[j];
    }
    const uint64_t x = wave_scan(acc, lane);
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    uint64_t run = part[blockIdx.x] + x - acc;
    for (uint32_t w = 0; w < wave; ++w) run += s_w[w];
#pragma unroll
    for (uint32_t j = 0; j < kItems; ++j) {
        if (base + j < n) row_off[base + j] = run;
        run += v[j];
    }
}

// the compaction scan's functors: kept = pred != 0; the store writes the kept candidates' indices
struct LoadKeep {
    const uint8_t *pred;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return pred[i] != 0 ? 1u : 0u; }
};
struct StoreCompact {
    uint32_t *idx;
    __device__ __forceinline__ void operator()(uint32_t i, uint32_t v, uint32_t in) const { if (in) idx[v] = i; }
};

// Lane 0 has written pieces of a row into its wavefront's part of LDS; behind this the other lanes of that wavefront read them.
// The release fence orders lane 0's LDS stores before the barrier, the acquire fence the other lanes' loads behind it; the
// wavefront's lanes run in lockstep, so wave_barrier costs no instruction: it keeps the compiler from moving either across.
__device__ __forceinline__ void wave_publish()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the wavefront copies n bytes, consecutive lanes on consecutive bytes (src: LDS or global memory)
__device__ __forceinline__ void wave_copy(char *dst, const char *src, uint32_t n, uint32_t lane)
{
    for (uint32_t i = lane; i < n; i += 64) dst[i] = src[i];
}
