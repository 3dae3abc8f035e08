#!/usr/bin/env python3
"""GPU-side: step E/F as two launches (ef_classify + ef_finalize_own: every finalize tile builds its contig's seed set itself) against the
three launches of rounds 1-5, over problem sizes -- where the two launches stop paying sets kOwnMaxTiles (duet_ef.hip) -- and, on the
two launches, ef_classify_split (two lanes per candidate, round 9) against ef_classify: where the wide kernel stops paying sets
kSplitMaxTiles; and ef_finalize_own_wide (two tiles per workgroup, round 10: the default where a contig spans more than 256 tiles)
against ef_finalize_own (column "two, narrow"): where the narrow kernel is ahead by more than the run-to-run range the rule must not
select the wide one.  (Beyond kSplitMaxTiles the library takes ef_classify whatever the debug word: for the sizes above it the column
"two" is measured on a build with the constant raised.)

    python3 tools/own_sweep.py [steps=200] [largest genome in marks=2e7] [one]
        one: instead of the genomes, ONE contig of config 2's kind at 196 .. 1,563 tiles, then two to four such contigs of 300 .. 600
        tiles each -- every one of them has the long contig that the wide kernel is meant for, so the columns "two, narrow" and
        "two, wide" show at which sizes it pays (duet_ef_run_device's rule)
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from duet_amd import _lib, engine, synth
from duet_amd.devmem import DeviceProblem

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
largest = int(float(sys.argv[2])) if len(sys.argv) > 2 else 20000000
OWN_OFF, OWN_ALL, SPLIT_OFF, WIDE, NARROW = 0x800000, 0x1000000, 0x200000, 0x1, 0x2
ctx = _lib.Context(0)
cases = [('config2 1 contig 1.0e6', [synth.bench_contig('1', 200000, 100000, 1, spelled='chr1')])]
if 'one' in sys.argv[1:]:
    largest = 0
    for tiles in (196, 300, 450, 512, 513, 576, 640, 768, 782, 1024, 1100, 1280, 1536, 1563):
        cases.append(('one contig', [synth.bench_contig('1', 512 * tiles, 256 * tiles, 1, spelled='chr1')]))
    for n, tiles in ((2, 256), (4, 300), (2, 450), (3, 400), (2, 600)):
        cases.append(('%d contigs of %d tiles' % (n, tiles), [synth.bench_contig(str(i + 1), 512 * tiles, 256 * tiles, 1 + i) for i in range(n)]))
for m in (250000, 1000000, 2000000, 4000000, 8000000, 20000000):
    if m > largest:
        break
    cases.append(('genome 24 contigs %.1e' % m, synth.bench_genome(m, 3)))
for name, contigs in cases:
    soa = engine.soa_from_synth(contigs)
    del contigs
    dp = DeviceProblem(soa, 50, 2)
    line = '%-28s %8d cand %5d tiles:' % (name, soa.n_cands, (soa.n_cands + 255) // 256)
    with torch.cuda.stream(torch.cuda.Stream()):
        st = torch.cuda.current_stream().cuda_stream
        ref = None
        for label, dbg in (('three', OWN_OFF), ('two, one lane', OWN_ALL | SPLIT_OFF), ('two', OWN_ALL), ('two, narrow', OWN_ALL | NARROW),
                           ('two, wide', OWN_ALL | WIDE)):
            ctx.set_debug(dbg)
            for _ in range(5):
                dp.run(ctx, st)
            ctx.check(st)
            torch.cuda.synchronize()
            best = 1e9
            for rep in range(3):
                t0 = time.perf_counter()
                for _ in range(steps):
                    dp.run(ctx, st)
                torch.cuda.synchronize()
                best = min(best, (time.perf_counter() - t0) / steps)
            ctx.set_profiling(2)
            for _ in range(50):
                dp.run(ctx, st)
            torch.cuda.synchronize()
            iso = ctx.profile_collect()
            ctx.set_profiling(0)
            pred, ps = dp.results(0)
            if ref is None:
                ref = (pred.copy(), ps.copy())
            same = bool(np.array_equal(pred, ref[0]) and np.array_equal(ps, ref[1]))
            line += '  %s %.2f us (kernels %s)%s' % (label, best * 1e6, ' / '.join('%.1f' % (x * 1e3) for x in iso.kernel_ms), '' if same else ' RESULTS DIFFER')
        ctx.set_debug(0)
    print(line, flush=True)
    del dp
    torch.cuda.empty_cache()
