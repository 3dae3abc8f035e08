// duet_cluster_plan.h -- what stage A0's host driver (duet_cluster_run, duet_cluster.hip) DECIDES for an input: every switch, the
// record sort's digits and the grids, each condition once.  Plain C++, no HIP call; included behind include/duet_ef.h (the debug
// bits), duet_prims.hip.h and duet_recsort.hip.h (the tile constants).  tools/cluster_plan_check.hip prints it, and
// tests/test_cluster_plan_host.py holds the numpy model of tests/cluster_model.py to it.
#ifndef DUET_CLUSTER_PLAN_H
#define DUET_CLUSTER_PLAN_H

constexpr int kClasses = 5;                            // the work lists by partition size and their pieces (duet_cluster.hip: WorkList)
constexpr int kShards = 64;

struct ClPlan {
    uint32_t M, key_bits, idx_bits;
    bool idx_packed, rec_mode, big_sort, small_in;
    uint32_t rs_top, rs_lo, rs_np, rs_w[8];            // the record sort: rs_np passes of rs_w[] bits over the key's top rs_top bits, rs_lo bits locally
    uint32_t nb_sc, nb_rx, nb_hs, nb_rs, rs_chunks, tps;
    bool rs_small, rx_totals, hybrid, use_spine, box_applies, tiers, wide, cap100, gate_forks, join_in_sums;
    uint32_t top_bits, top_shift, loc_cap;
    uint32_t g_loc, g_lists, g_waves, g_find_big, g_big, g_link, g_sums, g_emit;       // grids, from M alone
};

// Small inputs: the sort's hybrid and record variants order their groups with 1024 threads a tile, the partitions of more than 64 marks
// fork to a side stream (through gate kernels, once the context has seen them work) and one launch takes all the others
inline bool cl_small_in(uint32_t M, uint32_t dbg) { return M <= (4u << 20) && !(dbg & DUET_DBG_CLUSTER_LARGE); }
static_assert((4u << 20) == kSelfSpine * (uint32_t)kScanTile, "small_in's bound is the spine-less scan's reach: box_applies needs part_spine's carries");

// M >= 1 marks whose keys are contig | type | centre of these widths (key_bits > 64: nothing behind key_bits is set, the driver rejects
// it); gates_open: cl_gate kernels have been seen to work on this context
inline ClPlan cl_plan(uint32_t M, uint32_t centre_bits, uint32_t type_bits, uint32_t contig_bits, uint32_t dbg, uint32_t part_max, bool gates_open)
{
    ClPlan pl = {};
    pl.M = M;
    const uint32_t key_bits = pl.key_bits = centre_bits + type_bits + contig_bits;
    if (key_bits > 64) return pl;
    pl.nb_sc = (M + kScanTile - 1) / kScanTile;
    pl.nb_rx = (M + kRxTile - 1) / kRxTile;
    pl.nb_hs = (256u * pl.nb_rx + kScanTile - 1) / kScanTile;      // scan tiles of the radix histogram
    pl.tps = (pl.nb_sc + kShards - 1) / kShards;
    // The record travels with the key (duet_recsort.hip.h) when contig, type and mark index fit one word of it
    pl.idx_bits = bits_for(M - 1);
    pl.idx_packed = key_bits + pl.idx_bits <= 64 && !(dbg & DUET_DBG_CLUSTER_PAIRS);
    // ... from 1.25 M marks on: below, every pass is launch-latency bound and 8-byte keys are the cheaper thing to move (measured
    // on the fused pipeline, round 4: 1.0 M marks, one contig 0.277 ms with the key sort against 0.287; 2 M marks over 24 contigs 0.369
    // against 0.316, 4 M 0.483 / 0.455, 8 M 0.946 / 0.869, 2e7 2.35 / 2.22; round 6, 24 contigs, key sort / record sort: 0.9 M 0.252 / 0.259,
    // 1.1 M 0.253 / 0.253, 1.2 M 0.229 / 0.227, 1.3 M 0.283 / 0.249, 1.5 M 0.276 / 0.240 -- rounds 4-5 drew the line at 1.5 M);
    // DUET_DBG_CLUSTER_RECSORT takes it at any size
    pl.rec_mode = contig_bits + type_bits + pl.idx_bits <= 32u &&
                  (M >= 1250000u || (dbg & (DUET_DBG_CLUSTER_RECSORT | DUET_DBG_CLUSTER_LARGE))) &&
                  !(dbg & (DUET_DBG_CLUSTER_PAIRS | DUET_DBG_CLUSTER_LSD | DUET_DBG_CLUSTER_KEYSORT));
    // the digits of the record sort: LSD passes of up to kRsMaxW bits over the key's top bits, so many of them that the marks
    // that agree in them (a GROUP: one type within 2^lo centres) are a few dozen; the low bits are ordered group by group
    if (pl.rec_mode) {
        // (measured at 2e7 marks, 34-bit keys: 20 top bits in two 10-bit passes leave groups of 53 marks on average and the local
        // stage takes 285 + 33 us; 21 bits 235 us; 22 bits, two 11-bit passes, 212 us but 33 us more in the second scatter and
        // its offsets: 21 it is.  1.0 M marks: 16 bits in two 8-bit passes, groups of 32)
        uint32_t T = std::max(bits_for(M >> 4), 8u);
        T = std::min(T, key_bits);
        if (key_bits - T > 31u) T = key_bits - 31u;            // (the local stage holds the low bits in 32-bit words)
        pl.rs_top = T;
        pl.rs_lo = key_bits - T;
        pl.rs_np = (T + kRsMaxW - 1u) / kRsMaxW;
        for (uint32_t i = 0; i < pl.rs_np; ++i) pl.rs_w[i] = T / pl.rs_np + (i < T % pl.rs_np ? 1u : 0u);
    }
    pl.nb_rs = (M + kRsTile - 1) / kRsTile;
    pl.rs_chunks = (pl.nb_rs + kRsChunk - 1) / kRsChunk;
    pl.big_sort = (dbg & DUET_DBG_CLUSTER_LARGE) != 0;     // (tests: the tile-offset path of > 4 M keys)
    pl.rs_small = pl.nb_rs <= kRsSmallTiles && !pl.big_sort;
    pl.rx_totals = pl.nb_rx <= kRxTotalsTiles && !pl.big_sort;
    // Small inputs whose keys would take four passes or more: global passes over the top 16 bits only, then the groups of keys
    // that agree in them -- the marks of one type within 2^(key_bits - 16) centres, a few dozen -- are put in order by their low
    // bits locally (rx_local: a rank count in LDS; rx_big for a group of more than 256 keys).  8 launches instead of 13.
    // (The first attempt at this, earlier in round 3, ordered the groups with three ballot-ranked LDS radix passes and cost
    // what the global passes it replaced did: 91 against 88 us at 1 M marks; on the uneven groups of 2e7 marks over a whole
    // genome it was slower, 1010 against 745 us, and large inputs keep the plain LSD passes.)
    pl.small_in = cl_small_in(M, dbg);
    // (the global passes take the top 16 bits of a small input's keys, the top 24 of a large one's: groups of a few keys to a
    // few dozen either way on a genome; used where that saves two passes or more)
    pl.top_bits = M <= (2u << 20) ? 16u : 24u;     // (16 bits leave groups of a hundred keys and more beyond 2 M marks)
    // (rx_local and rx_big hold the low bits in 32-bit words: wider keys than top_bits + 31 take plain LSD passes)
    pl.hybrid = !pl.rec_mode && pl.idx_packed && (key_bits + 7u) / 8u >= pl.top_bits / 8u + 2u && key_bits - pl.top_bits < 32u && !(dbg & DUET_DBG_CLUSTER_LSD);
    pl.top_shift = pl.hybrid ? key_bits - pl.top_bits : 0u;
    pl.loc_cap = (dbg & DUET_DBG_CLUSTER_SMALLCAP) ? 3u : (uint32_t)kLocHalo;
    pl.g_loc = (M + kLocTile - 1) / kLocTile;
    // large inputs, record sort: cl_box is also the partition scan's last stage (no part_apply launch)
    // (small inputs keep part_apply: there the chain of the partitions of more than 64 marks is the critical path and has to start
    // beside the box test, not behind it -- measured: 315 us against 287 at 1.0 M marks)
    // (cl_box<.., true> reads tiles[tile] as the EXCLUSIVE carry part_spine leaves: it applies exactly where the spine launch runs,
    // i.e. never together with the spine-less part_apply<true> of `nb_sc <= kSelfSpine && !big_sort`)
    pl.use_spine = pl.nb_sc > kSelfSpine || pl.big_sort;
    pl.box_applies = pl.rec_mode && (!pl.small_in || pl.big_sort) && pl.use_spine;
    pl.g_lists = M < 16384u ? M : 16384u;               // partitions <= marks; kernels stride over them
    pl.g_waves = std::min(32768u, std::max(1024u, M / 256u));     // (a wavefront per virtual block, striding)
    pl.cap100 = part_max <= 100u;          // no unit has more rows than part_max
    pl.gate_forks = pl.small_in && gates_open && !(dbg & DUET_DBG_CLUSTER_EVENT_FORKS);
    pl.tiers = !pl.small_in || (dbg & DUET_DBG_CLUSTER_TIERS);
    // small inputs: every partition of more than 64 marks on its own workgroup of eight wavefronts (wide_unit), on the side stream beside cl_box and
    // cl_fast_all
    // (up to 2 M marks: a wide unit holds 143 KB of LDS, i.e. a CU, for 50 us -- at 4 M marks the 80-odd of them take a third of the chip from
    // cl_fast_all for that long and the pipeline is 1 % slower with them, 0.423 against 0.419 ms; level at 2 M)
    // (measured, profiles/history/r06_wide_units.txt: for the listed partitions of up to 64 marks four-wavefront units LOSE -- cl_fast_all is
    // bound by the chip's throughput there, not by a chain -- so only the partitions of more than 64 marks take wide units)
    pl.wide = !pl.tiers && M <= (2u << 20) && !(dbg & DUET_DBG_CLUSTER_WIDE_OFF);
    pl.g_find_big = std::max(1u, std::min(512u, (M / 8u + 255u) / 256u));
    pl.g_big = std::min(4096u, std::max(256u, (M / 64u + 63u) / 64u));      // (partitions <= marks; 64 of them per wavefront and step)
    pl.g_link = std::min(pl.g_big, 1024u);
    // (the join inside cl_pc_sums: its waiting workgroups hold wave slots -- up to M / 2048 workgroups of four wavefronts when every mark is a partition of its
    // own -- so only up to 2 M marks, where they cannot take more than half of the chip's from the side stream's kernels; beyond, a one-lane gate kernel)
    pl.join_in_sums = pl.gate_forks && M <= (2u << 20);
    pl.g_sums = (M + 2047u) / 2048u;
    pl.g_emit = std::min((M + 16383u) / 16384u * 8u, 4096u);        // (a wave per 64 partitions, striding)
    return pl;
}

#endif
