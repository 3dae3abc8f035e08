#!/usr/bin/env python3
"""GPU-side: cost of sv_calling/variants.vcf in the svim-gpu mode (--write_sv_calls, duet_amd/csrc/duet_callset.hip).

Default mode, on M synthetic raw marks held in HBM (24 hg19-sized contigs, M / 5 reads with 36-byte ONT-style names, binned
depth): one fused run (duet_svim_phase_device), then `steps` times each of
  rows     duet_svim_vcf_rows_device (the kernels plus its one host round trip), HIP events on the stream
  d2h      the text's copy to host memory (torch .cpu() of the used bytes)
  write    header + text to a file under the system's temporary directory (page cache; no fsync)
and one JSON line with the medians.  --kernels-only: the rows call `steps` times and nothing else, for a
`rocprofv3 --kernel-trace --stats` run of its own.  --stage: also the whole svim-gpu stage (svim_mode.sv_phasing_from_bams:
extraction from BAMs, fused pipeline, files) on a synthetic work directory of synth.bench_genome(M), with and without the flag,
wall clock after one warm-up run each.

    python3 tools/prof_callset.py M [steps=5] [--kernels-only] [--stage]
"""
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from duet_amd import _lib, svim_mode, synth
from duet_amd.devmem import DeviceSvim

args = [a for a in sys.argv[1:] if not a.startswith('--')]
M = int(float(args[0])) if args else 1000000
steps = int(args[1]) if len(args) > 1 else 5
K = 24
rng = np.random.default_rng(3)
lengths = np.array([synth.HG19_LENGTHS[l] for l in synth.DEFAULT_CONTIGS[:K]], dtype=np.float64)
contig = np.sort(rng.choice(K, M, p=lengths / lengths.sum())).astype(np.uint16)
pos = (rng.random(M) * lengths[contig]).astype(np.uint32) + 1
marks = dict(contig=contig, type=rng.integers(0, 4, M).astype(np.uint8), pos=pos,
             span=rng.integers(50, 3000, M).astype(np.uint32), read=np.full(M, 0xFFFFFFFF, np.uint32))
R = max(M // 5, 1)
hexd = np.frombuffer(b'0123456789abcdef', dtype=np.uint8)
pool = hexd[rng.integers(0, 16, (R, 36))]
pool[:, [8, 13, 18, 23]] = ord('-')
names = dict(mark_name=rng.integers(0, R, M).astype(np.uint32), name_off=np.arange(R + 1, dtype=np.uint64) * 36,
             name_pool=pool.reshape(-1).copy())
bins = (lengths // 1000).astype(np.int64) + 1
depth_off = np.concatenate([[0], np.cumsum(bins)]).astype(np.uint32)
depth = rng.integers(5, 60, int(depth_off[-1])).astype(np.uint32)
texts = ['chr' + l for l in synth.DEFAULT_CONTIGS[:K]]

ctx = _lib.Context(0)
ds = DeviceSvim(marks, np.zeros(0, np.uint64), depth, depth_off, 1000, 50, 2, device='cuda:0')
ds.run_fused(ctx)
N = ds.n_found
dev = ds.device
stream = torch.cuda.current_stream(dev)
up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
keep = [up(names['mark_name']), up(names['name_off']), up(names['name_pool'])]
hold = []
nm = _lib.callset_names(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), texts, hold)
nm.n_names = R
cap = _lib.callset_bound(N, M, names['name_off'], texts)
out = torch.empty(cap, dtype=torch.uint8, device=dev)
call = lambda: ctx.svim_vcf_rows_device(ds.sv_problem, ds.result, N, nm, out.data_ptr(), cap, stream.cuda_stream)
n = call()
torch.cuda.synchronize(dev)
if '--kernels-only' in sys.argv:
    for _ in range(steps):
        call()
    torch.cuda.synchronize(dev)
    print(json.dumps(dict(tool='prof_callset', mode='kernels-only', marks=M, cands=N, bytes=n, steps=steps)))
    sys.exit(0)
t_rows, t_d2h, t_write = [], [], []
path = os.path.join(tempfile.mkdtemp(prefix='prof_callset_'), 'variants.vcf')
head = ''.join('##contig=<ID=%s,length=%d>\n' % (t, int(l)) for t, l in zip(texts, lengths))
for _ in range(steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    call()
    b.record(stream)
    b.synchronize()
    t_rows.append(a.elapsed_time(b))
    t0 = time.perf_counter()
    host = out[:n].cpu().numpy()
    t_d2h.append(1e3 * (time.perf_counter() - t0))
    t0 = time.perf_counter()
    with open(path, 'wb') as f:
        f.write(('##fileformat=VCFv4.2\n##source=duet_amd svim-gpu\n' + head + svim_mode.CALLSET_INFO + svim_mode.CALLSET_COLS).encode())
        f.write(host)
    t_write.append(1e3 * (time.perf_counter() - t0))
shutil.rmtree(os.path.dirname(path))
med = lambda v: round(float(np.median(v)), 3)
line = dict(tool='prof_callset', marks=M, cands=N, text_bytes=n, steps=steps, rows_ms=med(t_rows), d2h_ms=med(t_d2h),
            write_ms=med(t_write), d2h_GBps=round(n / med(t_d2h) / 1e6, 2), write_GBps=round(n / med(t_write) / 1e6, 2))
if '--stage' in sys.argv:
    home = tempfile.mkdtemp(prefix='prof_callset_stage_')
    try:
        t0 = time.perf_counter()
        synth.write_svim_workdir(home, synth.bench_genome(M, 2), 2, write_sam=False)
        line['workdir_build_s'] = round(time.perf_counter() - t0, 1)
        for flag in (False, True):
            svim_mode.sv_phasing_from_bams(home, 50, 2, 16, False, 0.9, 0, write_sv_calls=flag)
            t0 = time.perf_counter()
            svim_mode.sv_phasing_from_bams(home, 50, 2, 16, False, 0.9, 0, write_sv_calls=flag)
            line['stage_%s_s' % ('with_flag' if flag else 'without_flag')] = round(time.perf_counter() - t0, 3)
        line['stage_callset_bytes'] = os.path.getsize(svim_mode.callset_path(home))
    finally:
        shutil.rmtree(home, ignore_errors=True)
print(json.dumps(line))
