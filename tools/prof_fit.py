#!/usr/bin/env python3
"""GPU-side: what the fit's inner loop costs at the tools/prof_sweep.py configs[1] workload (synth.bench_genome(1e6): ~1 M marks,
~1e5 candidates, the same synthetic prepared truth set), in one process, interleaved, medians over seven rounds:

  line_device   duet_tune_line_device per axis on the resident features (keys, sort, scan, one host round trip, vectors), host clock
                around the call and a stream synchronise
  line_host_way the way without these kernels, beside it: download the features, numpy.unique of the same expressions, build
                the block of vectors, upload it
  round         one whole round of 14 axes of the fit (tune._fit_setting: line, sweep with scoring, counts back, tune.scores per
                vector on the host) with max_values 0 and 4096

One JSON line each, appended to profiles/prof_fit.jsonl when a path is given.

    python3 tools/prof_fit.py [out.jsonl]
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from duet_amd import _lib, engine, synth, tune
from duet_amd.devmem import DeviceTune

ROUNDS = 7
out_path = sys.argv[1] if len(sys.argv) > 1 else ''
soa = engine.soa_from_synth(synth.bench_genome(1000000, 2))
ctx = _lib.Context(0)
feat = ctx.features_host(soa, 50, 2)
C = len(feat)
# the prepared truth set of tools/prof_sweep.py
rng = np.random.default_rng(1)
elig = feat['eligible'] != 0
ctg = np.searchsorted(soa.cand_ctg_off, np.arange(C), side='right') - 1
_, group = np.unique(ctg.astype(np.int64) * (1 << 32) + feat['ps'], return_inverse=True)
matched = elig & (rng.random(C) < 0.75)
uid = (np.arange(C) // 2).astype(np.uint32)
bits = rng.integers(0, 1 << 9, C).astype(np.uint16)
flags = np.where(elig, _lib.TUNE_IN_CALLS, 0) | np.where(matched, _lib.TUNE_MATCHED, 0) | np.where(matched, bits, 0)
pairs, pair = {}, np.zeros(C, dtype=np.uint32)
for c in np.lexsort((uid, group)):
    if matched[c]:
        pair[c] = pairs.setdefault((int(group[c]), int(uid[c])), len(pairs))
G = int(group.max()) + 1
gpo, pair_uid = np.zeros(G + 1, dtype=np.int64), np.zeros(len(pairs), dtype=np.uint32)
for (g, u), p in pairs.items():
    gpo[g + 1] += 1
    pair_uid[p] = u
np.cumsum(gpo, out=gpo)
n_base = int(uid.max()) + 1

dev = torch.device('cuda', 0)
empty = dict(base_off=np.zeros(1, np.uint32), base_pos=np.zeros(0, np.uint32), base_len=np.zeros(0, np.uint32),
             base_uid=np.zeros(0, np.uint32), base_hp=np.zeros(0, np.uint8), n_base_uid=0)
dt = DeviceTune(C, empty, 1000, 0.0, tune.vector()[None, :], device='cuda:0')       # (only its residency: features, truth arrays, line block)
dt.feat[:feat.nbytes] = torch.from_numpy(feat.view(np.uint8).copy()).to(dev)
for name, a, kind in (('cand_flags', flags, np.uint16), ('cand_group', group, np.uint32), ('cand_uid', uid, np.uint32),
                      ('cand_pair', pair, np.uint32), ('group_pair_off', gpo, np.uint32), ('pair_uid', pair_uid, np.uint32)):
    a = np.ascontiguousarray(a, dtype=kind)
    dt.keep[name][:a.nbytes] = torch.from_numpy(a.view(np.uint8).copy()).to(dev)
dt.truth.n_uid, dt.truth.n_groups, dt.truth.n_pairs = n_base, G, len(pairs)
base = tune.vector()
GE = (0, 1, 3, 4)


def host_way(axis):
    """Download, numpy.unique of derive()'s expression for the axis, the block of vectors, upload -> n_vec"""
    f = dt.features_host(C)
    e = f['eligible'] != 0
    lo, hi = np.minimum(f['t1'], f['t2']), np.maximum(f['t1'], f['t2'])
    one = (lo == 0) & (hi != 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        sv = f['svread'] / (f['svread'].astype(np.float64) + f['refread'])
        a1 = np.where(f['hap1'] > 0, f['t1'] / np.maximum(f['hap1'], 1).astype(np.float64), 0.0)
        a2 = np.where(f['hap2'] > 0, f['t2'] / np.maximum(f['hap2'], 1).astype(np.float64), 0.0)
        x = (f['svread'], sv, np.abs(a2 - a1), f['svread'], f['hap0'], sv, sv, f['allhap'] / f['deg'].astype(np.float64), np.abs(a2 - a1), sv, sv,
             f['refread'], sv, np.where(lo > 0, hi / np.maximum(lo, 1).astype(np.float64), 0.0))[axis].astype(np.float64)
    part = e & ((f['cls'] == 0) if axis == 0 else (f['cls'] == 2) if axis < 5 else (f['cls'] == 1) & (one if axis < 9 else ~one))
    xs = np.unique(x[part])
    line = np.concatenate([xs, [np.inf]]) if axis in GE else np.concatenate([[-np.inf], xs])
    vecs = np.tile(base, (len(line), 1))
    vecs[:, axis] = line
    dt.line_vec[:vecs.nbytes] = torch.from_numpy(vecs.view(np.uint8).reshape(-1)).to(dev)
    torch.cuda.synchronize()
    return len(line)


def device_way(axis):
    n_vec, _ = dt.line(ctx, C, base, axis, 0)
    torch.cuda.synchronize()
    return n_vec


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        with open(out_path, 'a') as f:
            f.write(line + '\n')


times = {(way, axis): [] for way in ('device', 'host') for axis in range(14)}
n_vec = {}
for rnd in range(ROUNDS + 1):                               # (round 0 warms both ways up)
    for axis in range(14):
        for way, fn in (('device', device_way), ('host', host_way)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = fn(axis)
            dt_ms = (time.perf_counter() - t0) * 1e3
            assert n_vec.setdefault(axis, n) == n, (axis, way, n, n_vec[axis])          # the two ways make lines of one length
            if rnd:
                times[(way, axis)].append(dt_ms)
for axis in range(14):
    d, h = statistics.median(times[('device', axis)]), statistics.median(times[('host', axis)])
    emit(dict(what='line', axis=tune.NAMES[axis], C=C, n_vec=n_vec[axis], rounds=ROUNDS, line_device_ms=round(d, 4), line_host_way_ms=round(h, 4),
              device_is_faster=d < h))
tot_d = sum(statistics.median(times[('device', a)]) for a in range(14))
tot_h = sum(statistics.median(times[('host', a)]) for a in range(14))
emit(dict(what='line_all_axes', C=C, rounds=ROUNDS, line_device_ms=round(tot_d, 4), line_host_way_ms=round(tot_h, 4), device_is_faster=tot_d < tot_h))
for max_values in (0, 4096):
    ts, vectors = [], 0
    for rnd in range(ROUNDS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, trace, _, _ = tune._fit_setting(ctx, dt, C, base, list(range(14)), 1, max_values, tune.SCORES.index('hp_f1'), n_base)
        torch.cuda.synchronize()
        if rnd:
            ts.append((time.perf_counter() - t0) * 1e3)
        vectors = sum(r['n_vec'] + 1 for r in trace)
    emit(dict(what='round', max_values=max_values, C=C, vectors_scored=vectors, rounds=ROUNDS, round_ms=round(statistics.median(ts), 3),
              moves=sum(r['old'] != r['new'] for r in trace), objective_after=trace[-1]['objective_after']))
ctx.close()
