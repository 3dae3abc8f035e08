#!/usr/bin/env python3
"""GPU-side: what a step of the fit on the cap axis costs with and without --join_ps, at the tools/prof_cap_line.py workload
(synth.bench_genome(1e6): ~1 M marks, ~1e5 candidates; the same synthetic truth side), in one process, interleaved, medians over
seven rounds after a warm-up round, host clock around work that ends in a synchronise:

  step          one whole step of the fit on the cap axis (tune._cap_step) with max_values 256, for the setting without a join and
                for join_min_sv 2: per line value the joined setting also builds the links under the value, their blocks and the
                remapped tags (DeviceProblem.joined_tags: duet_ps_links_device, duet_ps_join_links_device)
  value         the joined setting's extra work for one line value, split: the links, the blocks and the remap

One JSON line each, appended to the file given.

    python3 tools/prof_cap_step_join.py [out.jsonl]
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


MAX_VALUES, MIN_SV = 256, 2
settings = (('plain', SETTING), ('joined', dict(SETTING, join_min_sv=MIN_SV)))
ts, rows = {name: [] for name, _ in settings}, {}
for rnd in range(ROUNDS + 1):
    for name, setting in settings:
        memo = {}
        src.features(dt, setting, _lib.PC_MAX)
        dt.build(ctx, C)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows[name], _, _ = tune._cap_step(src, dt, setting, _lib.PC_MAX, vec, MAX_VALUES, score_of, n_base, None, None,
                                          lambda rec, nb: memo.setdefault((rec.tobytes(), nb), tune.scores(rec, nb)))
        torch.cuda.synchronize()
        if rnd:
            ts[name].append((time.perf_counter() - t0) * 1e3)
for name, _ in settings:
    row, med = rows[name], statistics.median(ts[name])
    emit(dict(what='step', setting=name, min_sv=MIN_SV if name == 'joined' else 0, max_values=MAX_VALUES, C=C, M=M,
              n_distinct=row['n_distinct'], values_scored=row['n_vec'] + 1, rounds=ROUNDS, step_ms=round(med, 3), step_ms_min=round(min(ts[name]), 3),
              step_ms_max=round(max(ts[name]), 3), ms_per_value=round(med / (row['n_vec'] + 1), 4), old=row['old'], new=row['new'],
              objective_after=row['objective_after']))

# the joined setting's extra work for one value
line = dt.cap_line(ctx, dp.problem, 0)[0]
room = _lib.ps_links_room(M)
links = torch.empty(max(room, 1) * _lib.PS_LINK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
tags = dp.buffers['read_tag'].clone()
pieces = dict(links=[], blocks_and_remap=[], joined_tags=[])
for rnd in range(ROUNDS + 1):
    cap = int(line[(rnd * 977) % len(line)])
    got = {}

    def clock(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        if rnd:
            pieces[name].append((time.perf_counter() - t0) * 1e3)
        return r

    n = clock('links', lambda: ctx.ps_links_device(dp.problem, links.data_ptr(), room, dt.stream(), pc_cap=cap))
    clock('blocks_and_remap', lambda: ctx.ps_join_links_device(links.data_ptr(), n, MIN_SV, dp.problem.read_tag, soa.read_off, soa.n_reads,
                                                               tags.data_ptr(), dt.stream()))
    clock('joined_tags', lambda: dp.joined_tags(ctx, MIN_SV, pc_cap=cap, stream=dt.stream()))
emit(dict(what='value', C=C, M=M, rounds=ROUNDS, **{k + '_ms': round(statistics.median(v), 4) for k, v in pieces.items()}))
ctx.close()
