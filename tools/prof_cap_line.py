#!/usr/bin/env python3
"""GPU-side: what the PC cap's line and the fit's cap axis cost at the tools/prof_sweep.py configs[1] workload
(synth.bench_genome(1e6): ~1 M marks, ~1e5 candidates; a synthetic truth side written from the candidates), in one process,
interleaved, medians over seven rounds, host clock around work that ends in a synchronise:

  line          (a) duet_tune_cap_line_device and duet_svim_cap_line_device on the resident problem, the values brought to the host,
                against the way without them: download the mark / tag / candidate arrays, numpy.unique of the same selection.  The
                two ways' outputs are compared word for word first.  (b) D and L of the workload.
  value         (c) the cost of one line value, split: the features call under the cap, the truth build, the sweep at K = 1 with
                its counts brought back, the host scoring
  step          (d) one whole step of the fit on the cap axis (tune._cap_step) with max_values 0, 4096 and 256, and the objective
                each reaches

One JSON line each, appended to profiles/prof_cap_line.jsonl when a path is given.

    python3 tools/prof_cap_line.py [out.jsonl]
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
CAP_MAX = _lib.PC_CAP_MAX
out_path = sys.argv[1] if len(sys.argv) > 1 else ''
soa = engine.soa_from_synth(synth.bench_genome(1000000, 2))
ctx = _lib.Context(0)
C, M, K = soa.n_cands, soa.n_marks, soa.n_contigs
S_THRES, R_THRES = 50, 2

# a truth side from the candidates: three in four have a record at their position, on the list 2 * contig + (c & 1)
rng = np.random.default_rng(1)
ctg = (np.searchsorted(soa.cand_ctg_off, np.arange(C), side='right') - 1).astype(np.uint32)
cand_key = (2 * ctg + (np.arange(C) & 1)).astype(np.uint32)
has = rng.random(C) < 0.75
order = np.lexsort((soa.cand_pos[has], cand_key[has]))
base_key = cand_key[has][order]
n_keys = 2 * K
base = dict(base_off=np.searchsorted(base_key, np.arange(n_keys + 1)).astype(np.uint32), base_pos=soa.cand_pos[has][order],
            base_len=np.maximum(soa.cand_svlen[has][order], 50), base_uid=np.arange(int(has.sum()), dtype=np.uint32),
            base_hp=rng.integers(0, 3, int(has.sum())).astype(np.uint8), n_base_uid=int(has.sum()))
n_base = int(has.sum())

dev = torch.device('cuda', 0)
# the resident problem: the fit's own candidate source over the synthetic candidates in place of a work directory's
tune._candidates = lambda *a: (soa, dict(chrom=[], ref=[], alt=[], svtype=[]))
src = tune._Callset(ctx, 'unused', [S_THRES], [R_THRES], [None], '', False, False, 1)
next(src.ingests())
dp = src.dp
SETTING = dict(svlen_thres=S_THRES, suppread_thres=R_THRES)
dt = DeviceTune(C, base, 1000, 0.0, tune.vector()[None, :], device='cuda:0')
dt.set_candidates(soa.cand_pos, np.maximum(soa.cand_svlen, 50), cand_key, ctg, K)
sp = _lib.SvimProblem()
sp.marks.n_marks, sp.n_reads = M, soa.n_reads
sp.mark_read, sp.read_tag = dp.problem.mark_read, dp.problem.read_tag
vec = tune.vector()
score_of = tune.SCORES.index('hp_f1')


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        with open(out_path, 'a') as f:
            f.write(line + '\n')


def down(name, kind, n):
    return dp.buffers[name][:n * np.dtype(kind).itemsize].cpu().numpy().view(kind)


def host_way(raw):
    """Download the arrays, select the marks that can vote, numpy.unique -> the line on the host"""
    mark_read, tag = down('mark_read', np.uint32, M), down('read_tag', np.uint64, soa.n_reads)
    ok = (mark_read != _lib.MARK_ABSENT) & (mark_read < len(tag))
    if not raw:
        off = down('cand_off', np.uint32, C + 1)
        kept = (down('cand_svlen', np.uint32, C) >= S_THRES) & (down('cand_svread', np.uint32, C) >= R_THRES) & (down('cand_gt_ok', np.uint8, C) != 0)
        ok &= np.repeat(kept, np.diff(off.astype(np.int64)))
    t = tag[mark_read[ok]]
    pc = ((t >> np.uint64(32)) & np.uint64(0x3FFFFFFF)).astype(np.uint32)
    xs = np.unique(pc[(t != np.uint64(0xFFFFFFFFFFFFFFFF)) & (pc <= CAP_MAX)])
    return (xs if len(xs) and xs[0] == 0 else np.concatenate([np.zeros(1, dtype=np.uint32), xs])), len(xs)


def device_way(raw):
    caps, D, whole = dt.cap_line(ctx, sp if raw else dp.problem, 0)
    assert whole
    return caps, D


# (a), (b)
for raw in (False, True):
    got, want = device_way(raw), host_way(raw)
    assert got[1] == want[1] and np.array_equal(got[0], want[0]), (raw, got[1], want[1])        # word for word, first
times = {(way, raw): [] for way in ('device', 'host') for raw in (False, True)}
shape = {}
for rnd in range(ROUNDS + 1):                               # (round 0 warms both ways up)
    for raw in (False, True):
        for way, fn in (('device', device_way), ('host', host_way)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            caps, D = fn(raw)
            torch.cuda.synchronize()
            if rnd:
                times[(way, raw)].append((time.perf_counter() - t0) * 1e3)
            shape[raw] = (D, len(caps))
for raw in (False, True):
    d, h = statistics.median(times[('device', raw)]), statistics.median(times[('host', raw)])
    emit(dict(what='line', form='svim' if raw else 'candidate', C=C, M=M, D=shape[raw][0], L=shape[raw][1], rounds=ROUNDS,
              line_device_ms=round(d, 4), line_host_way_ms=round(h, 4), device_is_faster=d < h))

# (c): one line value, piece by piece
dt.set_line_vector(vec)
line = device_way(False)[0]
pieces = dict(features=[], truth_build=[], sweep_k1=[], host_scoring=[])
for rnd in range(ROUNDS + 1):
    cap = int(line[(rnd * 977) % len(line)])

    def clock(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        if rnd:
            pieces[name].append((time.perf_counter() - t0) * 1e3)
        return r

    clock('features', lambda: ctx.features_device(dp.problem, dt.feat.data_ptr(), dt.stream(), pc_cap=cap))
    clock('truth_build', lambda: dt.build(ctx, C))
    rec = clock('sweep_k1', lambda: dt.sweep_line(ctx, C, 0, 1)[0])
    clock('host_scoring', lambda: tune.scores(rec, n_base))
med = {k: round(statistics.median(v), 4) for k, v in pieces.items()}
emit(dict(what='value', C=C, M=M, rounds=ROUNDS, dominant=max(med, key=med.get), total_ms=round(sum(med.values()), 4), **{k + '_ms': v for k, v in med.items()}))

# (d): one whole step on the cap axis
for max_values in (256, 4096, 0):
    ts, row = [], None
    for rnd in range(ROUNDS + (1 if max_values else 0)):    # (the smaller steps have warmed everything up for the whole line)
        memo = {}
        src.features(dt, SETTING, _lib.PC_MAX)
        dt.build(ctx, C)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        row, _, _ = tune._cap_step(src, dt, SETTING, _lib.PC_MAX, vec, max_values, score_of, n_base, None, None,
                                   lambda rec, nb: memo.setdefault((rec.tobytes(), nb), tune.scores(rec, nb)))
        torch.cuda.synchronize()
        if rnd or not max_values:
            ts.append((time.perf_counter() - t0) * 1e3)
    emit(dict(what='step', max_values=max_values, C=C, M=M, n_distinct=row['n_distinct'], values_scored=row['n_vec'] + 1, exact=row['exact'],
              rounds=len(ts), step_ms=round(statistics.median(ts), 3), ms_per_value=round(statistics.median(ts) / (row['n_vec'] + 1), 4),
              old=row['old'], new=row['new'], objective_before=row['objective_before'], objective_after=row['objective_after']))
ctx.close()
