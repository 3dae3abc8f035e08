// cluster_plan_check.hip -- stage A0's plan function (duet_amd/csrc/duet_cluster_plan.h: cl_plan, the one duet_cluster_run calls) as a
// stand-alone program: no HIP call, no GPU.  tests/test_cluster_plan_host.py builds it and holds tests/cluster_model.py to it.
//     hipcc --offload-arch=gfx950 -std=c++17 -Iinclude -Iduet_amd/csrc tools/cluster_plan_check.hip -o cluster_plan_check
// Standard input: lines of `M centre_bits type_bits contig_bits dbg part_max gates_open`; standard output: one line of name=value per
// input line, every field of ClPlan (rs_w as the widths of its rs_np passes, comma-separated; T is rs_top, as the model calls it).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>

#include "duet_ef.h"

namespace {
#include "duet_prims.hip.h"
#include "duet_recsort.hip.h"
#include "duet_cluster_plan.h"
}  // namespace

int main()
{
    unsigned M, centre_bits, type_bits, contig_bits, dbg, part_max, gates_open;
    while (scanf("%u %u %u %u %u %u %u", &M, &centre_bits, &type_bits, &contig_bits, &dbg, &part_max, &gates_open) == 7) {
        const ClPlan pl = cl_plan(M, centre_bits, type_bits, contig_bits, dbg, part_max, gates_open != 0);
        printf("M=%u centre_bits=%u type_bits=%u contig_bits=%u key_bits=%u", pl.M, centre_bits, type_bits, contig_bits, pl.key_bits);
        if (pl.key_bits > 64) {                                   // (the driver rejects it: nothing else is set)
            printf("\n");
            continue;
        }
        printf(" idx_bits=%u idx_packed=%d rec_mode=%d big_sort=%d small_in=%d T=%u rs_lo=%u rs_np=%u rs_w=", pl.idx_bits, pl.idx_packed, pl.rec_mode,
               pl.big_sort, pl.small_in, pl.rs_top, pl.rs_lo, pl.rs_np);
        for (uint32_t i = 0; i < pl.rs_np; ++i) printf(i ? ",%u" : "%u", pl.rs_w[i]);
        printf(" nb_sc=%u nb_rx=%u nb_hs=%u nb_rs=%u rs_chunks=%u tps=%u rs_small=%d rx_totals=%d hybrid=%d use_spine=%d box_applies=%d tiers=%d wide=%d"
               " cap100=%d gate_forks=%d join_in_sums=%d top_bits=%u top_shift=%u loc_cap=%u",
               pl.nb_sc, pl.nb_rx, pl.nb_hs, pl.nb_rs, pl.rs_chunks, pl.tps, pl.rs_small, pl.rx_totals, pl.hybrid, pl.use_spine, pl.box_applies, pl.tiers,
               pl.wide, pl.cap100, pl.gate_forks, pl.join_in_sums, pl.top_bits, pl.top_shift, pl.loc_cap);
        printf(" g_loc=%u g_lists=%u g_waves=%u g_find_big=%u g_big=%u g_link=%u g_sums=%u g_emit=%u\n", pl.g_loc, pl.g_lists, pl.g_waves, pl.g_find_big,
               pl.g_big, pl.g_link, pl.g_sums, pl.g_emit);
    }
    return 0;
}
