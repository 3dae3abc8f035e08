// duet_tune_feat.hip.h -- the per-candidate feature record (include/duet_ef.h: duet_tune_feature): filter (sv_phasing_fn.py:189-190),
// PS-class (:191-194) and vote (:70-111), stated once for the two kernels that write it.  Included inside the anonymous namespace
// of duet_tune.hip (tune_features: the reference's PC cap, the seed sets an E/F run of the same context left behind) and of
// duet_tune_cap.hip (tc_features: the cap and the seed arrays are arguments).  What differs between the two is the seed source S:
//   cap()             a mark votes iff its read is tagged and pc <= cap()
//   count(a, k)       seeds of contig k
//   seeds(a, k)       contig k's seed PS values, ascending
//   div_zero()        an eligible candidate has svread + refread == 0
//   kSeedPass         true: the pass that finds the seeds -- filter, PS-class and contig as below, then seed(c, k, ps) for a kept
//                     class-1 candidate of contig k with a voter, and no record is written
#ifndef DUET_TUNE_FEAT_HIP_H
#define DUET_TUNE_FEAT_HIP_H

#include "duet_seeds.hip.h"                // kEmpty, kUntagged, tag_ps / tag_pc / tag_hap, lower_bound_u32, nearest_seed

constexpr int kStage = 1024;                  // features_body: voter words staged in LDS per pass over a candidate's marks (8 KiB)

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint64_t wave_max64(uint64_t v)
{
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}

struct FeatArgs {
    uint32_t C, K, n_reads, svlen_thres, suppread_thres;
    const uint64_t *read_tag;
    const uint32_t *cand_pos, *cand_svlen, *cand_svread, *cand_refread, *cand_off, *mark_read;
    const uint8_t *cand_gt_ok;
    const uint32_t *ctg_off, *n_one, *onebuf;     // contig offsets; the E/F workspace's seed counts and ascending seed arrays (EfSeeds)
    duet_tune_feature *out;
};

// the tag of mark m, kUntagged for a mark whose read has no tag
__device__ __forceinline__ uint64_t mark_tag(const FeatArgs &a, uint32_t m)
{
    const uint32_t r = a.mark_read[m];
    return (r == kEmpty || r >= a.n_reads) ? kUntagged : a.read_tag[r];
}
__device__ __forceinline__ bool is_voter(uint64_t t, uint32_t cap) { return t != kUntagged && tag_pc(t) <= cap; }

// One candidate per workgroup of one wavefront: every walk over the marks goes 64 at a time, so a candidate of any degree and any
// number of phase sets takes the same code.  The multi-PS winner (:85-105): among voters whose PS is a seed, the PS with the most
// voters, ties to the one seen first -- i.e. the largest (count, -first index) over the first occurrences.
template <class S>
__device__ __forceinline__ void features_body(const FeatArgs &a, const S &sd)
{
    __shared__ uint64_t s_w[kStage];
    const uint32_t lane = threadIdx.x;
    const uint32_t cap = sd.cap();
    for (uint32_t c = blockIdx.x; c < a.C; c += gridDim.x) {
        const uint32_t b = a.cand_off[c], e = a.cand_off[c + 1];
        const uint32_t svread = a.cand_svread[c], refread = a.cand_refread[c];
        duet_tune_feature f;
        memset(&f, 0, sizeof(f));
        f.deg = e - b;
        f.svread = svread;
        f.refread = refread;
        const bool kept = a.cand_svlen[c] >= a.svlen_thres && svread >= a.suppread_thres && a.cand_gt_ok[c] != 0;
        f.kept = kept ? 1 : 0;
        if (kept) {
            // PS-class: distinct PS among ALL tagged marks (no PC test, :192-194)
            uint32_t p0 = 0;
            bool have = false, multi = false;
            for (uint32_t m0 = b; m0 < e && !multi; m0 += 64) {
                const uint32_t m = m0 + lane;
                const uint64_t t = m < e ? mark_tag(a, m) : kUntagged;
                const bool tagged = t != kUntagged;
                const uint64_t bal = __ballot(tagged);
                if (!have && bal) {
                    p0 = __shfl(tag_ps(t), __ffsll((unsigned long long)bal) - 1);
                    have = true;
                }
                if (have) multi = __any(tagged && tag_ps(t) != p0);
            }
            f.cls = multi ? 2 : (have ? 1 : 0);
            // the contig and its seed set
            uint32_t lo = 0, hi = a.K;
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (a.ctg_off[mid] <= c) lo = mid; else hi = mid;
            }
            if constexpr (S::kSeedPass) {
                // (:197-203) a kept class-1 candidate with a voter makes its PS a seed of its contig: in class 1 every tagged mark
                // carries the one PS, so the first voter's PS is p0
                bool voter = false;
                for (uint32_t m0 = b; m0 < e && !voter && f.cls == 1; m0 += 64) {
                    const uint32_t m = m0 + lane;
                    voter = __any(is_voter(m < e ? mark_tag(a, m) : kUntagged, cap));
                }
                if (voter && lane == 0) sd.seed(c, lo, p0);
                continue;
            }
            const uint32_t n_seed = sd.count(a, lo);
            const uint32_t *seeds = sd.seeds(a, lo);
            if (n_seed) {
                f.eligible = 1;
                if ((uint64_t)svread + (uint64_t)refread == 0) sd.div_zero();
                uint32_t hap1 = 0, hap2 = 0, allhap = 0, ps = 0;
                uint64_t t1 = 0, t2 = 0;
                if (f.cls == 1) {                                   // :74-84
                    for (uint32_t m0 = b; m0 < e; m0 += 64) {
                        const uint32_t m = m0 + lane;
                        const uint64_t t = m < e ? mark_tag(a, m) : kUntagged;
                        if (is_voter(t, cap)) {
                            if (tag_hap(t) == 1) { ++hap1; t1 += tag_pc(t); }
                            else if (tag_hap(t) == 2) { ++hap2; t2 += tag_pc(t); }
                        }
                    }
                    hap1 = wave_sum(hap1); hap2 = wave_sum(hap2);
                    t1 = wave_sum64(t1); t2 = wave_sum64(t2);
                    allhap = hap1 + hap2;
                    ps = p0;                                        // every voter carries the one PS
                } else if (f.cls == 2) {                            // :85-105
                    uint64_t best = 0;                              // (count << 32) | ~(index of the first occurrence)
                    for (uint32_t i0 = b; i0 < e; i0 += 64) {
                        const uint32_t i = i0 + lane;
                        const uint64_t t = i < e ? mark_tag(a, i) : kUntagged;
                        const bool voter = is_voter(t, cap);
                        allhap += voter ? 1u : 0u;
                        const uint64_t my = voter ? ((1ull << 32) | tag_ps(t)) : 0ull;
                        const uint32_t ni = n_seed;
                        bool cand = false;
                        if (voter) {
                            const uint32_t at = lower_bound_u32(seeds, ni, tag_ps(t));
                            cand = at < ni && seeds[at] == tag_ps(t);     // :91
                        }
                        if (!__any(cand)) continue;
                        uint32_t n = 0;
                        bool first = cand;
                        for (uint32_t j0 = b; j0 < e; j0 += kStage) {
                            const uint32_t cnt = e - j0 < (uint32_t)kStage ? e - j0 : (uint32_t)kStage;
                            __syncthreads();
                            for (uint32_t jj = lane; jj < cnt; jj += 64) {
                                const uint64_t u = mark_tag(a, j0 + jj);
                                s_w[jj] = is_voter(u, cap) ? ((1ull << 32) | tag_ps(u)) : 0ull;
                            }
                            __syncthreads();
                            if (cand)
                                for (uint32_t jj = 0; jj < cnt; ++jj)
                                    if (s_w[jj] == my) {
                                        ++n;
                                        if (j0 + jj < i) first = false;
                                    }
                        }
                        const uint64_t key = (cand && first) ? (((uint64_t)n << 32) | (uint64_t)(~(i - b))) : 0ull;
                        const uint64_t w = wave_max64(key);
                        best = w > best ? w : best;
                    }
                    allhap = wave_sum(allhap);
                    if (best) {
                        const uint32_t at = b + ~(uint32_t)best;
                        const uint32_t win = tag_ps(mark_tag(a, at));
                        for (uint32_t m0 = b; m0 < e; m0 += 64) {
                            const uint32_t m = m0 + lane;
                            const uint64_t t = m < e ? mark_tag(a, m) : kUntagged;
                            if (is_voter(t, cap) && tag_ps(t) == win) {
                                if (tag_hap(t) == 1) { ++hap1; t1 += tag_pc(t); }
                                else if (tag_hap(t) == 2) { ++hap2; t2 += tag_pc(t); }
                            }
                        }
                        hap1 = wave_sum(hap1); hap2 = wave_sum(hap2);
                        t1 = wave_sum64(t1); t2 = wave_sum64(t2);
                        f.hap0 = allhap - hap1 - hap2;              // only with a winner (:105)
                        ps = win;
                    }
                }
                if (f.cls == 0 || (hap1 == 0 && hap2 == 0)) ps = nearest_seed(seeds, n_seed, a.cand_pos[c]);   // :106-111
                f.hap1 = hap1; f.hap2 = hap2; f.allhap = allhap; f.t1 = t1; f.t2 = t2; f.ps = ps;
            }
        }
        if constexpr (S::kSeedPass) continue;
        if (lane == 0) a.out[c] = f;
    }
}

#endif
