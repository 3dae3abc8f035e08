#!/usr/bin/env python3
"""GPU-side: what the evidence table costs (duet_tune_leaves_device + duet_evidence_rows_device, duet_amd/csrc/duet_evidence.hip)
against writing it on the host, at two sizes: tools/prof_sweep.py's workload (synth.bench_genome(1e6): ~1 M marks, 100,002
candidates on 24 contigs) and the 2e7-mark genome (synth.bench_genome(2e7): ~2 M candidates).  The table form: CHROM by contig,
SVTYPE by type code, the candidates' own positions and lengths.

    device      the leaves call and the rows call on resident arrays, to the synchronise behind the writer
    plan        the rows call with out_cap = 0: the length kernel, the scan and the round trip, refused before the writer --
                device minus plan minus leaves is the writer alone, whose bytes/s stand beside cs_write's
    leaves      the leaves call alone
    copy        the text from HBM to the host
    host_way    without the new kernels: the features and the sweep's pred brought to the host, the leaves there (numpy, derived
                once), the rows by the reference formatter (tests/evidence_ref.py: % formatting, a row at a time)

Everything is resident in HBM and every variant runs in this one process, interleaved: per round each variant once, the host
clock around work that ends in a device synchronise (the host way ends on the host); the figure is the median over the rounds
after one warm-up round.  The device's text is compared with the host way's byte for byte before anything is timed.  Appends one
JSON line per (size, variant) to the file given and prints a table.

    python3 tools/prof_evidence.py [rounds=7] [out=profiles/prof_evidence.jsonl] [host_rounds_at_2e7=3]
"""
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
from duet_amd import _lib, engine, synth, tune
from tests import evidence_ref

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, 'profiles', 'prof_evidence.jsonl')
host_rounds_big = int(sys.argv[3]) if len(sys.argv) > 3 else 3
ctx = _lib.Context(0)
dev = torch.device('cuda', 0)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
stream = torch.cuda.current_stream(dev)
vec = tune.vector()


def host_leaves(f, v):
    """The leaf of every candidate under v (include/duet_ef.h, "Leaf census" and "Evidence table"), in binary64 as the tree compares."""
    with np.errstate(divide='ignore', invalid='ignore'):
        t1, t2 = f['t1'].astype(np.float64), f['t2'].astype(np.float64)
        a1 = np.where(f['hap1'] > 0, t1 / f['hap1'], 0.0)
        a2 = np.where(f['hap2'] > 0, t2 / f['hap2'], 0.0)
        lo, hi = np.minimum(f['t1'], f['t2']), np.maximum(f['t1'], f['t2'])
        hr = f['allhap'] / f['deg'].astype(np.float64)
        sv = f['svread'] / (f['svread'].astype(np.float64) + f['refread'])
        totsc = np.where(lo > 0, hi / np.maximum(lo, 1).astype(np.float64), 0.0)
    onehap, diff = (lo == 0) & (hi != 0), np.abs(a2 - a1)
    gate = ((hr <= v[7]) & (diff <= v[8])) | (hr > v[7])
    c0 = np.where((sv == 1.0) & (f['svread'] >= v[0]), 0, 1)
    c2 = np.where(~(sv >= v[1]), 2, np.where(diff <= v[2], np.where(f['svread'] >= v[3], 3, 4), np.where(f['hap0'] >= v[4], 5, 6)))
    one = np.where(sv <= v[5], 7, np.where(sv <= v[6], np.where(gate, 8, 9), np.where(gate, 10, 11)))
    two = np.where(sv <= v[9], 12, np.where(sv <= v[10], np.where(f['refread'] > v[11], 13, 14),
                                            np.where(sv <= v[12], np.where(totsc <= v[13], 15, 16), 17)))
    leaf = np.where(f['cls'] == 0, c0, np.where(f['cls'] == 2, c2, np.where(onehap, one, two)))
    return np.where(f['eligible'] != 0, leaf, np.where(f['kept'] != 0, _lib.LEAF_NO_SEED, _lib.LEAF_FILTERED)).astype(np.uint8)


lines = []
for marks, seed in ((1000000, 2), (20000000, 3)):
    soa = engine.soa_from_synth(synth.bench_genome(marks, seed))
    feat = ctx.features_host(soa, 50, 2)
    C, K = len(feat), soa.n_contigs
    contig = (np.searchsorted(soa.cand_ctg_off, np.arange(C), side='right') - 1).astype(np.uint16)
    ctype = (np.random.default_rng(seed).random(C) < 0.5).astype(np.uint8)
    chroms = ['chr%d' % (k + 1) for k in range(K)]
    keep = dict(feat=t(feat.view(np.uint8)), pos=t(soa.cand_pos.view(np.int32)), svlen=t(soa.cand_svlen.view(np.int32)),
                contig=t(contig.view(np.int16)), ctype=t(ctype), vec=t(vec))
    leaf, pred = torch.zeros(C + 64, dtype=torch.uint8, device=dev), torch.zeros(C + 64, dtype=torch.uint8, device=dev)
    ps = torch.zeros(C + 16, dtype=torch.int32, device=dev)
    texts = (ctypes.c_char_p * K)(*[c.encode() for c in chroms])
    p = _lib.EvidenceProblem()
    p.n_cands, p.n_contigs = C, K
    p.feat, p.leaf, p.pred = keep['feat'].data_ptr(), leaf.data_ptr(), pred.data_ptr()
    p.cand_pos, p.cand_svlen, p.cand_contig, p.cand_type = (keep[n].data_ptr() for n in ('pos', 'svlen', 'contig', 'ctype'))
    p.chrom = texts
    cap = _lib.evidence_bound(C, max(len(c) for c in chroms))
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    got = {}

    def run_leaves():
        ctx.leaves_device(keep['feat'].data_ptr(), C, vec, leaf.data_ptr(), pred.data_ptr(), stream.cuda_stream)
        torch.cuda.synchronize()

    def device():
        ctx.leaves_device(keep['feat'].data_ptr(), C, vec, leaf.data_ptr(), pred.data_ptr(), stream.cuda_stream)
        got['n'] = ctx.evidence_rows_device(p, out.data_ptr(), cap, stream.cuda_stream)
        torch.cuda.synchronize()

    def plan():
        n = ctypes.c_uint64(0)
        rc = ctx.lib.duet_evidence_rows_device(ctx.handle, ctypes.byref(p), ctypes.c_void_p(out.data_ptr()), ctypes.c_uint64(0), ctypes.byref(n),
                                               ctypes.c_void_p(stream.cuda_stream))
        assert rc == _lib.DUET_ERR_INVALID and n.value == got['n']
        torch.cuda.synchronize()

    def copy():
        got['text'] = out[:got['n']].cpu().numpy()

    def host_way():
        ctx.apply_device(keep['feat'].data_ptr(), C, keep['vec'].data_ptr(), pred.data_ptr(), ps.data_ptr(), stream.cuda_stream)
        h_feat = keep['feat'].cpu().numpy().view(_lib.FEATURE_DTYPE)
        h_pred = pred[:C].cpu().numpy()
        got['host'] = evidence_ref.table_text(contig, ctype, soa.cand_pos, soa.cand_svlen, chroms, h_feat, host_leaves(h_feat, vec), h_pred)

    big = marks > 1000000
    variants = [('device', device, rounds), ('plan', plan, rounds), ('leaves', run_leaves, rounds), ('copy', copy, rounds),
                ('host_way', host_way, min(rounds, host_rounds_big) if big else rounds)]
    for _, run, _ in variants:                                                 # warm-up, and the two texts against each other
        run()
    assert got['text'].tobytes() == got['host'].encode(), 'the device text differs from the host way'
    rules = set(r.split('\t')[7] for r in got['host'].splitlines()[:200000])
    ms = {i: [] for i in range(len(variants))}
    for r in range(rounds):
        for i, (_, run, n) in enumerate(variants):
            if r >= n:
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            ms[i].append((time.perf_counter() - t0) * 1e3)
    med = {what: float(np.median(ms[i])) for i, (what, _, _) in enumerate(variants)}
    writer_ms = med['device'] - med['plan'] - med['leaves']
    for i, (what, _, n) in enumerate(variants):
        lines.append(dict(marks=soa.n_marks, C=C, bytes=got['n'], variant=what, rounds=n, ms_median=round(med[what], 4),
                          ms_min=round(min(ms[i]), 4), ms_max=round(max(ms[i]), 4), rules_seen=len(rules),
                          writer_ms=round(writer_ms, 4), writer_GBps=round(got['n'] / max(writer_ms, 1e-6) / 1e6, 2)))
        print(json.dumps(lines[-1]), flush=True)
    del keep, out, leaf, pred, ps
ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'a') as f:
    for ln in lines:
        f.write(json.dumps(ln) + '\n')
print('| candidates | text MB | device ms | copy ms | host way ms | host way / (device + copy) | writer ms | writer GB/s |')
print('|---|---|---|---|---|---|---|---|')
for C in sorted(set(ln['C'] for ln in lines)):
    m = {ln['variant']: ln for ln in lines if ln['C'] == C}
    d, c, h = m['device']['ms_median'], m['copy']['ms_median'], m['host_way']['ms_median']
    print('| %d | %.1f | %.3f | %.3f | %.1f | %.1f | %.3f | %.1f |' % (C, m['device']['bytes'] / 1e6, d, c, h, h / (d + c), m['device']['writer_ms'],
                                                                m['device']['writer_GBps']))
