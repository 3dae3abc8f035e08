#!/usr/bin/env python3
"""GPU-side: time of the threshold sweep (duet_tune_sweep_device, duet_amd/csrc/duet_tune.hip) at BASELINE configs[1] size
(synth.bench_genome(1e6): ~1 M marks, ~1e5 candidates) for K = 1, 256 and 4096 vectors, without scoring (decisions and the
emitted-call count only) and with scoring against a synthetic prepared truth set (every eligible candidate a call, three in
four matched, two candidates per truth id, the phase-set groups of the candidates' own (contig, PS)).  Everything is resident
in HBM; the time is HIP events around `steps` sweeps after one warm-up.  Prints one JSON line per configuration.

    python3 tools/prof_sweep.py [steps=5]
"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from duet_amd import _lib, engine, synth, tune

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
soa = engine.soa_from_synth(synth.bench_genome(1000000, 2))
ctx = _lib.Context(0)
feat = ctx.features_host(soa, 50, 2)
C = len(feat)
rng = np.random.default_rng(1)
elig = feat['eligible'] != 0
ctg = np.searchsorted(soa.cand_ctg_off, np.arange(C), side='right') - 1
gkey = ctg.astype(np.int64) * (1 << 32) + feat['ps']
_, group = np.unique(gkey, return_inverse=True)
matched = elig & (rng.random(C) < 0.75)
uid = (np.arange(C) // 2).astype(np.uint32)
bits = rng.integers(0, 1 << 9, C).astype(np.uint16)
flags = np.where(elig, _lib.TUNE_IN_CALLS, 0) | np.where(matched, _lib.TUNE_MATCHED, 0) | np.where(matched, bits, 0)
pairs = {}
pair = np.zeros(C, dtype=np.uint32)
for c in np.lexsort((uid, group)):
    if matched[c]:
        pair[c] = pairs.setdefault((int(group[c]), int(uid[c])), len(pairs))
G = int(group.max()) + 1
gpo = np.zeros(G + 1, dtype=np.int64)
pair_uid = np.zeros(len(pairs), dtype=np.uint32)
for (g, u), p in pairs.items():
    gpo[g + 1] += 1
    pair_uid[p] = u
np.cumsum(gpo, out=gpo)
dev = torch.device('cuda', 0)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
d_feat = t(feat.view(np.uint8))
d = dict(cand_flags=t(flags.astype(np.uint16).view(np.int16)), cand_group=t(group.astype(np.uint32).view(np.int32)),
         cand_uid=t(uid.view(np.int32)), cand_pair=t(pair.view(np.int32)), group_pair_off=t(gpo.astype(np.uint32).view(np.int32)),
         pair_uid=t(pair_uid.view(np.int32)))
tr = _lib.TuneTruth()
tr.n_uid, tr.n_groups, tr.n_pairs = int(uid.max()) + 1, G, len(pairs)
for k, v in d.items():
    setattr(tr, k, v.data_ptr())
stream = torch.cuda.current_stream(dev)
for K in (1, 256, 4096):
    vecs = np.repeat(tune.vector()[None, :], K, axis=0)
    vecs[:, 1] = np.linspace(0.5, 0.9, K)
    vecs[:, 12] = np.linspace(0.6, 0.9, K)[::-1]
    d_vec = t(vecs)
    d_counts = torch.zeros(K * _lib.COUNTS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    for scoring in (False, True):
        def run():
            rc = ctx.lib.duet_tune_sweep_device(ctx.handle, ctypes.c_void_p(d_feat.data_ptr()), C, ctypes.c_void_p(d_vec.data_ptr()), K,
                                                ctypes.byref(tr) if scoring else None, ctypes.c_void_p(d_counts.data_ptr()), None, None,
                                                ctypes.c_void_p(stream.cuda_stream))
            assert rc == 0, ctx.last_error()
        run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(steps):
            run()
        e1.record(stream)
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / steps
        print(json.dumps(dict(K=K, C=C, marks=soa.n_marks, eligible=int(elig.sum()), scoring=scoring, steps=steps, ms=round(ms, 4),
                              decisions_per_s=float('%.4g' % (K * C / (ms * 1e-3))), groups=G, truth_ids=int(tr.n_uid),
                              pairs=len(pairs))), flush=True)
ctx.close()
