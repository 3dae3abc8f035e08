#!/usr/bin/env python3
"""GPU-side: cost of the data rows of phased_sv.vcf in the svim-gpu mode (duet_amd/csrc/duet_svim_rows.hip).

Default mode, on the raw marks of synth.bench_genome(M) held in HBM (24 hg19-sized contigs, the reads' tags as the BAMs would
give them, so a realistic share of the candidates is phased): one fused run (duet_svim_phase_device), then after a warm-up
`steps` times each of
  rows     duet_svim_phased_rows_device (the kernels plus its one host round trip), HIP events on the stream
  d2h      the text's copy to host memory (torch .cpu() of the used bytes)
  host     what the call replaces: DeviceSvim.fetch() plus svim_mode.rows_text on the same results, wall clock
and one JSON line with the medians (and whether the two texts are the same bytes).
--kernels-only: the rows call `steps` times and nothing else, for a `rocprofv3 --kernel-trace --stats` run of its own.
--vcf-rows: instead, the VCF mode's rows (duet_rows_run_device: rows_write) on BASELINE configs[2]'s contig `steps` times, for the
same kind of run -- the rate sr_write is set beside.
--stage: only the whole svim-gpu stage (svim_mode.sv_phasing_from_bams: extraction from BAMs, fused pipeline, file) on a synthetic
work directory of synth.bench_genome(M), wall clock of one run after a warm-up run.

    python3 tools/prof_svim_rows.py M [steps=5] [--kernels-only | --vcf-rows | --stage]
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
from duet_amd import _lib, engine, svim_mode, synth
from duet_amd.devmem import DeviceSvim

args = [a for a in sys.argv[1:] if not a.startswith('--')]
M = int(float(args[0])) if args else 1000000
steps = int(args[1]) if len(args) > 1 else 5
med = lambda v: round(float(np.median(v)), 3)

if '--stage' in sys.argv:
    home = tempfile.mkdtemp(prefix='prof_svim_rows_stage_')
    try:
        synth.write_svim_workdir(home, synth.bench_genome(M, 2), 2, write_sam=False)
        svim_mode.sv_phasing_from_bams(home, 50, 2, 16, False, 0.9, 0)
        t0 = time.perf_counter()
        svim_mode.sv_phasing_from_bams(home, 50, 2, 16, False, 0.9, 0)
        t = time.perf_counter() - t0
        import hashlib
        text = open(home + '/phased_sv.vcf', 'rb').read()
        print(json.dumps(dict(tool='prof_svim_rows', mode='stage', marks=M, stage_s=round(t, 3), phased_sv_vcf_bytes=len(text),
                              rows=text.count(b'\n') - text.count(b'\n#') - 1, sha256=hashlib.sha256(text).hexdigest())))
    finally:
        shutil.rmtree(home, ignore_errors=True)
    sys.exit(0)

ctx = _lib.Context(0)

if '--vcf-rows' in sys.argv:
    from duet_amd.devmem import DeviceProblem, device_rows
    from duet_amd.native import NativeIngest
    from duet_amd.read_file import init_chrom_list
    home = tempfile.mkdtemp(prefix='prof_svim_rows_vcf_')
    try:
        synth.write_workdir(home, [synth.bench_contig('1', 200000, 100000, 1)], dialect='cutesv', seed=1, write_sam=False)
        ing = NativeIngest.load(os.path.join(home, 'sv_calling', 'variants.vcf'), home + '/snp_phasing/', init_chrom_list(False, home), 4)
        rows = ing.rows()
        dp = DeviceProblem(ing.soa, 50, 2)
        st = dp.run(ctx)
        ctx.check(st)
        for _ in range(steps + 1):
            body, n_rows = device_rows(ctx, dp, rows, stream=st)
        print(json.dumps(dict(tool='prof_svim_rows', mode='vcf-rows', cands=int(ing.soa.n_cands), rows=int(n_rows), text_bytes=len(body),
                              steps=steps + 1)))
        ing.close()
    finally:
        shutil.rmtree(home, ignore_errors=True)
    sys.exit(0)

contigs = synth.bench_genome(M, 3)
soa = engine.soa_from_synth(contigs)
marks = synth.raw_marks(contigs, 1, reads_of=soa)
depth, depth_off = synth.depth_bins(contigs, 1000, 1)
n_marks = len(marks['pos'])
ds = DeviceSvim(marks, soa.read_tag, depth, depth_off, 1000, 50, 2, device='cuda:0')
del contigs
ds.run_fused(ctx)
N = ds.n_found
dev = ds.device
stream = torch.cuda.current_stream(dev)
# a work directory that spells the 24 contigs chr<c>, for the host formatter's lookup
home = tempfile.mkdtemp(prefix='prof_svim_rows_')
os.makedirs(os.path.join(home, 'snp_phasing'))
chroms = list(synth.DEFAULT_CONTIGS[:24])
for c in chroms:
    open(os.path.join(home, 'snp_phasing', 'chr' + c + '.bam'), 'wb').close()
texts = svim_mode.spelled_contigs(home, chroms)
cap = _lib.phased_rows_bound(N, texts)
out = torch.empty(cap, dtype=torch.uint8, device=dev)
call = lambda: ctx.svim_phased_rows_device(ds.result, N, ds.out_pred.data_ptr(), ds.out_ps.data_ptr(), texts, out.data_ptr(), cap,
                                           stream.cuda_stream)
try:
    n, n_rows = call()
    torch.cuda.synchronize(dev)
    if '--kernels-only' in sys.argv:
        for _ in range(steps):
            call()
        torch.cuda.synchronize(dev)
        print(json.dumps(dict(tool='prof_svim_rows', mode='kernels-only', marks=n_marks, cands=N, rows=n_rows, text_bytes=n, steps=steps + 1)))
        sys.exit(0)
    t_rows, t_d2h, t_host = [], [], []
    host = out[:n].cpu().numpy()
    want = svim_mode.rows_text(home, dict(ds.fetch(), chroms=chroms))                  # (the warm-up of both)
    same = host.tobytes() == want.encode()
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
        want = svim_mode.rows_text(home, dict(ds.fetch(), chroms=chroms))
        t_host.append(1e3 * (time.perf_counter() - t0))
    print(json.dumps(dict(tool='prof_svim_rows', marks=n_marks, cands=N, rows=n_rows, text_bytes=n, steps=steps, rows_ms=med(t_rows),
                          d2h_ms=med(t_d2h), device_plus_copy_ms=round(med(t_rows) + med(t_d2h), 3), host_fetch_rows_text_ms=med(t_host),
                          identical=bool(same))))
finally:
    shutil.rmtree(home, ignore_errors=True)
