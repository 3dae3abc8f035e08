// duet_seeds.hip.h -- the read tag's fields and the ascending seed array of a contig (sv_phasing_fn.py:107: np.sort(list(oneps_set))),
// stated once for the units that read them on the device: duet_ef.hip (the product's step E/F), duet_tune_feat.hip.h (the feature
// record) and duet_tune_capline.hip (the PC field only).  Included inside the unit's anonymous namespace, like duet_prims.hip.h.
#ifndef DUET_SEEDS_HIP_H
#define DUET_SEEDS_HIP_H

constexpr uint32_t kEmpty = 0xFFFFFFFFu;          // "no seed" / "no PS yet"; in mark_read: the mark has no read
constexpr uint64_t kUntagged = ~0ull;             // tag word of a mark whose read has no tag

// the tag word's fields (include/duet_ef.h: DUET_TAG)
__device__ __forceinline__ uint32_t tag_ps(uint64_t t) { return (uint32_t)t; }
__device__ __forceinline__ uint32_t tag_pc(uint64_t t) { return (uint32_t)(t >> 32) & 0x3FFFFFFFu; }
__device__ __forceinline__ uint32_t tag_hap(uint64_t t) { return (uint32_t)(t >> 62); }

// first index of a[0 .. n), ascending, whose value is not below key
__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t *a, uint32_t n, uint32_t key)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// sv_phasing_fn.py:107-111 -- the nearest seed, ties to the larger one (n >= 1)
__device__ __forceinline__ uint32_t nearest_seed(const uint32_t *a, uint32_t n, uint32_t pos)
{
    const uint32_t i = lower_bound_u32(a, n, pos);
    const uint32_t lo = i > 0 ? i - 1 : 0;
    const uint32_t hi = i < n - 1 ? i : n - 1;
    const int64_t dl = llabs((int64_t)pos - (int64_t)a[lo]);
    const int64_t dh = llabs((int64_t)pos - (int64_t)a[hi]);
    return dl < dh ? a[lo] : a[hi];
}

#endif
