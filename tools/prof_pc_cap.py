#!/usr/bin/env python3
"""GPU-side: what the PC cap as a run parameter costs at the tools/prof_sweep.py configs[1] workload (synth.bench_genome(1e6):
~1 M marks, ~1e5 candidates), in one process, interleaved, medians over seven rounds, host clock around work that ends in a
synchronise:

  features      duet_ef_features_cap_device at cap 8100 (seed pass, keys-only sort, scan, offsets, feature kernel, one status
                word back) beside duet_ef_features_device (an E/F run for its seed sets, then the feature kernel) on the same
                resident problem -- after a byte comparison of the two outputs.  The existing entry is left alone by the cap, so
                its figure is also the figure of before.
  sweep         tune.sweep_settings with five caps in one call beside five calls with one cap each, on the same candidates (the
                ingest is replaced by the synthetic problem and a synthetic truth file, so the figures hold the uploads, the
                features calls, the truth builds and the sweeps)

One JSON line each, appended to profiles/prof_pc_cap.jsonl when a path is given.

    python3 tools/prof_pc_cap.py [out.jsonl]
"""
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from duet_amd import _lib, engine, synth, tune
from duet_amd.devmem import DeviceProblem

ROUNDS = 7
CAPS = (972, 2400, 4000, 8100, 9720)
out_path = sys.argv[1] if len(sys.argv) > 1 else ''
soa = engine.soa_from_synth(synth.bench_genome(1000000, 2))
ctx = _lib.Context(0)
C = soa.n_cands
dp = DeviceProblem(soa, 50, 2, device='cuda:0')
nbytes = C * _lib.FEATURE_DTYPE.itemsize
bufs = [torch.zeros(nbytes + 64, dtype=torch.uint8, device='cuda:0') for _ in range(2)]
stream = torch.cuda.current_stream().cuda_stream


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        with open(out_path, 'a') as f:
            f.write(line + '\n')


def plain():
    ctx.features_device(dp.problem, bufs[0].data_ptr(), stream)
    torch.cuda.synchronize()


def capped():
    ctx.features_device(dp.problem, bufs[1].data_ptr(), stream, pc_cap=8100)
    torch.cuda.synchronize()


plain()
capped()
same = bool(torch.equal(bufs[0][:nbytes], bufs[1][:nbytes]))
assert same, 'duet_ef_features_cap_device at 8100 differs from duet_ef_features_device'
times = dict(plain=[], capped=[])
for rnd in range(ROUNDS + 1):                               # (round 0 warms both up)
    for name, fn in (('plain', plain), ('capped', capped)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if rnd:
            times[name].append((time.perf_counter() - t0) * 1e3)
p, c = statistics.median(times['plain']), statistics.median(times['capped'])
emit(dict(what='features', C=C, M=soa.n_marks, rounds=ROUNDS, outputs_equal=same, features_device_ms=round(p, 4),
          features_cap_device_8100_ms=round(c, 4), ratio=round(c / p, 3)))

# the sweep: the synthetic candidates in place of a work directory's, a truth file written from them
ctg = np.searchsorted(soa.cand_ctg_off, np.arange(C), side='right') - 1
labels = [str(i) for i in range(1, 23)] + ['X', 'Y']
txt = dict(chrom=['chr' + labels[k % 24] for k in ctg], ref=['N'] * C, alt=['<%s>' % ('INS', 'DEL')[c & 1] for c in range(C)],
           svtype=[('INS', 'DEL')[c & 1] for c in range(C)])
tune._candidates = lambda *a: (soa, txt)
fd, truth = tempfile.mkstemp(suffix='.vcf')
with os.fdopen(fd, 'w') as f:
    f.write('#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n')
    for c in range(0, C, 2):
        t = txt['svtype'][c]
        ln = max(int(soa.cand_svlen[c]), 50)
        f.write('%s\t%d\tt%d\tN\t<%s>\t.\tPASS\tSVTYPE=%s;SVLEN=%d\tGT:PS\t%s:1\n' % (txt['chrom'][c], int(soa.cand_pos[c]), c, t, t,
                                                                                 ln if t == 'INS' else -ln, ('1|0', '0|1', '1|1')[c % 3]))
vecs = tune.vector()[None, :]


def sweep_five():
    rows = tune.sweep_settings('unused', truth, vecs, ctx=ctx, pc_cap=CAPS)
    torch.cuda.synchronize()
    return rows


def sweep_singly():
    rows = []
    for cap in CAPS:
        rows += tune.sweep_settings('unused', truth, vecs, ctx=ctx, pc_cap=(cap,))
    torch.cuda.synchronize()
    return rows


try:
    a, b = sweep_five(), sweep_singly()
    assert [[repr(r[n]) for n in r] for r in a] == [[repr(r[n]) for n in r] for r in b], 'the two ways give different rows'
    times = dict(five=[], singly=[])
    for rnd in range(ROUNDS):
        for name, fn in (('five', sweep_five), ('singly', sweep_singly)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    f5, s5 = statistics.median(times['five']), statistics.median(times['singly'])
    emit(dict(what='sweep', C=C, caps=list(CAPS), rounds=ROUNDS, one_call_of_five_caps_ms=round(f5, 2), five_calls_of_one_cap_ms=round(s5, 2),
              hp_f1=[r['hp_f1'] for r in a], eligible_differs=len({repr(r['hp_f1']) for r in a}) > 1))
finally:
    os.remove(truth)
ctx.close()
