#!/usr/bin/env python3
"""GPU-side diagnostic: per-block phase timeline of the three kernels (libduet_ef_stamps.so, -DDUET_STAMPS).
Not part of the product; run its numbers as SHARES, the stamped build is slower.

    python3 tools/stamps.py [cfg2 | genome | fused] [3k] [wide | narrow]
        3k: the three launches; wide / narrow: ef_finalize_own_wide / ef_finalize_own whatever the size (DUET_DBG_EF_OWN_WIDE / _NARROW)"""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from duet_amd import _lib, engine, synth
_lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), 'libduet_ef_stamps.so')
from duet_amd.devmem import DeviceProblem

ctx = _lib.Context(0)
if '3k' in sys.argv:
    ctx.set_debug(0x800000)        # DUET_DBG_EF_OWN_OFF: the three launches of rounds 1-5
elif 'wide' in sys.argv:
    ctx.set_debug(0x1)             # DUET_DBG_EF_OWN_WIDE
elif 'narrow' in sys.argv:
    ctx.set_debug(0x2)             # DUET_DBG_EF_OWN_NARROW
lib = _lib.load()
lib.duet_dbg_stamps.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
which = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] not in ('3k', 'wide', 'narrow') else 'cfg2'
if which == 'fused':
    # the E/F problem that stage A0 hands over in the fused pipeline (candidates ordered by type, then centre)
    from oracle import c_oracle
    contigs = [synth.bench_contig('1', 200000, 100000, 1)]
    base = engine.soa_from_synth(contigs)
    marks = synth.raw_marks(contigs, 1, reads_of=base)
    depth, depth_off = synth.depth_bins(contigs, 1000, 1)
    cl = c_oracle.cluster(marks['contig'], marks['type'], marks['pos'], marks['span'])
    N = len(cl['cand_pos'])
    support = np.diff(cl['cand_off'].astype(np.int64))
    k = cl['cand_contig'].astype(np.int64)
    d = depth[depth_off[k] + np.minimum(cl['cand_pos'].astype(np.int64) // 1000, np.diff(depth_off)[k] - 1)].astype(np.int64)
    soa = engine.EfSoA(cand_ctg_off=np.searchsorted(k, np.arange(2)), read_tag=base.read_tag, cand_pos=cl['cand_pos'],
                       cand_svlen=cl['cand_span'], cand_svread=support, cand_refread=np.maximum(d - support, 0),
                       cand_gt_ok=np.ones(N, dtype=np.uint8), cand_off=cl['cand_off'], mark_read=marks['read'][cl['order']])
else:
    soa = engine.soa_from_synth([synth.bench_contig('1', 200000, 100000, 1)]) if which == 'cfg2' else \
        engine.soa_from_synth(synth.bench_genome(20000000, 3))
dp = DeviceProblem(soa, 50, 2)
stream = torch.cuda.current_stream().cuda_stream
for _ in range(5):
    dp.run(ctx, stream)
torch.cuda.synchronize()
lib.duet_dbg_stamps(ctx.handle, 1, None)
dp.run(ctx, stream)
torch.cuda.synchronize()
buf = np.zeros(6 * 65536 * 8, dtype=np.uint64)          # (areas 3..5: stage A0's chains, tools/stamps_cl.py)
lib.duet_dbg_stamps(ctx.handle, 0, buf.ctypes.data)
st = buf[:3 * 65536 * 8].reshape(3, 65536, 8).astype(np.int64)
t0 = st[0][st[0][:, 0] > 0][:, 0].min()
names = [['start', 'offsets', 'staged', 'consumed', 'loop_end', 'decided', 'end'],
         ['start', 'gathered', 'sorted', 'end', 'recs', 'counted', 'written', 'runs'],
         ['start', 'meta', 'staged'] if '3k' in sys.argv else ['start', 'cleared', 'inserted', 'records', 'columns', 'ranked', 'end']]
# stamp indices in program order, for the phase durations (ef_finalize_own: `records` -- the seed records have arrived, behind the
# wait in front of the insert phase -- lies between `cleared` and `inserted`; `columns` -- the columns and summaries have arrived,
# behind the first trip's one wait -- splits start -> cleared into the trip and the clear + barrier)
order_of = [list(range(7)), None, [0, 1, 2] if '3k' in sys.argv else [0, 4, 1, 3, 2, 5, 6]]
for k in range(3):
    blk = st[k][st[k][:, 0] > 0]
    nb = len(blk)
    print('kernel', k, 'blocks stamped', nb)
    rel = (blk - t0) * 10.0 / 1000.0   # 100 MHz ticks -> us
    for i, nm in enumerate(names[k]):
        col = rel[:, i]
        col = col[blk[:, i] > 0]
        if len(col):
            print('  %-9s first %.2f  median %.2f  p90 %.2f  last %.2f us' % (nm, col.min(), np.median(col), np.percentile(col, 90), col.max()))
    if k == 1:
        order = [0, 4, 5, 6, 1, 7, 2, 3]          # stamp indices in program order
        for b in range(nb):
            print('  contig block %d:' % b, ' '.join('%s@%.2f' % (names[1][i], rel[b, i]) for i in order if blk[b, i] > 0))
        continue
    cols = [i for i in order_of[k] if (blk[:, i] > 0).all()]
    d = np.diff(rel[:, cols], axis=1)
    print('  phase durations (median us):', ' '.join('%s=%.2f' % (names[k][cols[i + 1]], np.median(d[:, i])) for i in range(d.shape[1])))
if st[1][1][0] > 0:                         # (a diagnostic build may leave (n << 32 | distinct) of contig 0's seed list there)
    print('seed list of contig 0: n %d distinct %d' % (int(st[1][1][0]) >> 32, int(st[1][1][0]) & 0xFFFFFFFF))
