#!/usr/bin/env python3
"""GPU-side: what one setting of a sweep over -s, -r and -c costs (duet_amd/tune.py: sweep_settings), on the workload of
tools/prof_sweep.py -- BASELINE configs[1] size, synth.bench_genome(1e6): ~1 M marks, ~1e5 candidates, a truth set with one id
per two candidates.  The candidates get the text a callset would give them (CHROM chr<label>, symbolic ALT, INS and DEL in turn)
and the truth set is a VCF, so that tune.prepare_truth -- the host truth match the device build replaces -- runs on the same
candidates and the same truth set.  One JSON line per measurement, appended to profiles/prof_tune_grid.jsonl:

    truth_build       duet_tune_truth_build_device alone, everything resident; wall clock around the call (it ends with the one
                      host round trip that learns n_groups and n_pairs), mean of `steps` after one warm-up
    prepare_truth     tune.prepare_truth on the same candidates, once (host; seconds), and the ratio of the two
    setting           a whole setting: duet_ef_features_device + the truth build + duet_tune_sweep_device at K = 256 and the copy
                      of the 256 count records
    from_bams_grid    (unless marks is 0) a 3 x 3 x 3 grid of -c, -s, -r over the BAMs of synth.bench_genome(marks) at K = 256:
                      wall clock of sweep_settings, ingest included, and per setting

    python3 tools/prof_tune_grid.py [steps=5] [marks of the from_bams grid=1000000]
"""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from duet_amd import _lib, engine, synth, tune
from duet_amd.devmem import DeviceProblem, DeviceTune

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
grid_marks = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'prof_tune_grid.jsonl')


def emit(**rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, 'a') as f:
        f.write(line + '\n')


contigs = synth.bench_genome(1000000, 2)
soa = engine.soa_from_synth(contigs)
ctx = _lib.Context(0)
feat = ctx.features_host(soa, 50, 2)
C = len(feat)
rng = np.random.default_rng(1)
ctg = np.searchsorted(soa.cand_ctg_off, np.arange(C), side='right') - 1
svtype = [('INS', 'DEL')[c & 1] for c in range(C)]
cands = dict(feat=feat, chrom=['chr' + contigs[int(k)].label for k in ctg], pos=soa.cand_pos, svlen=np.maximum(soa.cand_svlen, 50),
             ref=['N'] * C, alt=['<%s>' % t for t in svtype], svtype=svtype)
tmp = tempfile.mkdtemp()
truth_vcf = os.path.join(tmp, 'truth.vcf')
with open(truth_vcf, 'w') as f:
    f.write('#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n')
    for c in range(0, C, 2):                                # one truth id per two candidates
        t, ln = svtype[c], int(cands['svlen'][c])
        f.write('%s\t%d\ttruth%d\tN\t<%s>\t.\tPASS\tSVTYPE=%s;SVLEN=%d\tGT:PS\t%s:%d\n' % (
            cands['chrom'][c], int(soa.cand_pos[c]), c // 2, t, t, ln if t == 'INS' else -ln, ('1|0', '0|1', '1|1')[int(rng.integers(3))],
            int(rng.integers(1, 6))))

t0 = time.perf_counter()
ref = tune.prepare_truth(cands, truth_vcf)
host_s = time.perf_counter() - t0

base = tune.truth_side(truth_vcf)
t0 = time.perf_counter()
key, chrom, n_chrom = tune.candidate_keys(cands)
keys_s = time.perf_counter() - t0
K = 256
vecs = np.repeat(tune.vector()[None, :], K, axis=0)
vecs[:, 1] = np.linspace(0.5, 0.9, K)
vecs[:, 12] = np.linspace(0.6, 0.9, K)[::-1]
dt = DeviceTune(C, base, 1000, 0.0, vecs)
dt.set_candidates(soa.cand_pos, cands['svlen'], key, chrom, n_chrom)
dp = DeviceProblem(soa, 50, 2)
dt.feat[:feat.nbytes] = torch.from_numpy(feat.view(np.uint8).copy()).to(dt.device)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


build_ms = timed(lambda: dt.build(ctx, C))
assert (dt.truth.n_groups, dt.truth.n_pairs) == (ref['n_groups'], ref['n_pairs'])
common = dict(C=C, marks=soa.n_marks, eligible=int((feat['eligible'] != 0).sum()), truth_ids=base['n_base_uid'],
              groups=int(dt.truth.n_groups), pairs=int(dt.truth.n_pairs), steps=steps)
emit(what='truth_build', ms=round(build_ms, 4), **common)
emit(what='prepare_truth', ms=round(host_s * 1e3, 1), ratio_to_truth_build=float('%.4g' % (host_s * 1e3 / build_ms)),
     candidate_keys_once_per_workdir_ms=round(keys_s * 1e3, 1), **common)


def setting():
    ctx.features_device(dp.problem, dt.feat.data_ptr(), dt.stream())
    dt.build(ctx, C)
    dt.sweep(ctx, C)


emit(what='setting', K=K, ms=round(timed(setting), 4), **common)

if grid_marks:
    home = os.path.join(tmp, 'w')
    t0 = time.perf_counter()
    synth.write_svim_workdir(home, synth.bench_genome(grid_marks, 2), 2, write_sam=False)
    write_s = time.perf_counter() - t0
    cs, ss, rs = (0.7, 0.9, 1.1), (40, 50, 60), (2, 3, 4)
    t0 = time.perf_counter()
    rows = tune.sweep_settings(home, truth_vcf, vecs, ss, rs, cs, from_bams=True, ctx=ctx)
    grid_s = time.perf_counter() - t0
    assert len(rows) == 27 * K
    emit(what='from_bams_grid', marks_target=grid_marks, K=K, settings=27, ingests=3, ms=round(grid_s * 1e3, 1),
         ms_per_setting=round(grid_s * 1e3 / 27, 2), write_workdir_s=round(write_s, 1))
ctx.close()
