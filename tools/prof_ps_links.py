#!/usr/bin/env python3
"""GPU-side: what the phase-set links cost (duet_ps_links_device, duet_amd/csrc/duet_pslinks.hip) against building them on the
host, at two sizes: BASELINE configs[1] (bench.py's flagship: synth.bench_contig('1', 200000, 100000, 1), ~1 M marks on one
contig) and the 2e7-mark genome (synth.bench_genome(2e7, 3): 24 contigs).

    device      duet_ps_links_device on the resident problem, to the synchronise behind the record kernel (its three host round
                trips included)
    copy        the records from HBM to the host
    host_way    without the new kernels: the rule restated in numpy on the host arrays (host_links below: masks, one np.unique
                over the voters' (candidate, ps) keys, bincounts, one lexsort of the observations, reduceat)

Everything is resident in HBM and every variant runs in this one process, interleaved: per round each variant once, the host
clock around work that ends in a device synchronise (the host way ends on the host); the figure is the median over the rounds
after one warm-up round.  The device's records are compared with the host way's byte for byte before anything is timed.  Also
reported: how many candidates have voters in two or more phase sets, how many observations and how many links there are -- a
workload without any would time nothing.  Appends one JSON line per (size, variant) to the file given and prints a table.

    python3 tools/prof_ps_links.py [rounds=7] [out=profiles/prof_ps_links.jsonl] [host_rounds_at_2e7=3]
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
from duet_amd import _lib, engine, synth
from duet_amd.devmem import DeviceProblem

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, 'profiles', 'prof_ps_links.jsonl')
host_rounds_big = int(sys.argv[3]) if len(sys.argv) > 3 else 3
DT = _lib.PS_LINK_DTYPE


def host_links(soa, svlen_thres, suppread_thres, cap, info):
    """The rule of include/duet_ef.h ("Phase-set links") in numpy -> PS_LINK_DTYPE records; info: n_multi, n_obs."""
    C, R = soa.n_cands, soa.n_reads
    out = np.zeros(0, dtype=DT)
    info['n_multi'], info['n_obs'] = 0, 0
    if C == 0 or soa.n_marks == 0:
        return out
    kept = (soa.cand_svlen >= svlen_thres) & (soa.cand_svread >= suppread_thres) & (soa.cand_gt_ok != 0)
    cand = np.repeat(np.arange(C, dtype=np.uint64), np.diff(soa.cand_off.astype(np.int64)))
    mr = soa.mark_read
    ok = (mr != _lib.MARK_ABSENT) & (mr < R) & kept[cand.astype(np.int64)]
    tag = soa.read_tag[np.where(ok, mr, 0)] if R else np.zeros(len(mr), dtype=np.uint64)
    hap, pc = tag >> np.uint64(62), (tag >> np.uint64(32)) & np.uint64(0x3FFFFFFF)
    vote = ok & (tag != np.uint64(0xFFFFFFFFFFFFFFFF)) & (pc <= cap) & ((hap == 1) | (hap == 2))
    key = (cand[vote] << np.uint64(32)) | (tag[vote] & np.uint64(0xFFFFFFFF))
    groups, inv = np.unique(key, return_inverse=True)
    if len(groups) < 2:
        return out
    h2 = np.bincount(inv[hap[vote] == 2], minlength=len(groups)).astype(np.int64)
    d = np.bincount(inv, minlength=len(groups)).astype(np.int64) - 2 * h2
    gc, gp = groups >> np.uint64(32), groups & np.uint64(0xFFFFFFFF)
    pair = gc[1:] == gc[:-1]
    info['n_obs'] = int(pair.sum())
    info['n_multi'] = len(np.unique(gc[1:][pair]))
    if not info['n_obs']:
        return out
    c, a, b, da, db = gc[1:][pair].astype(np.int64), gp[:-1][pair], gp[1:][pair], d[:-1][pair], d[1:][pair]
    contig = np.searchsorted(soa.cand_ctg_off, c, side='right') - 1
    opened = (da == 0) | (db == 0)
    same = ~opened & ((da > 0) == (db > 0))
    flip = ~opened & ~same
    w = np.minimum(np.abs(da), np.abs(db)).astype(np.uint64)
    pos = soa.cand_pos[c]
    order = np.lexsort((b, a, contig))
    contig, a, b = contig[order], a[order], b[order]
    head = np.ones(len(order), dtype=bool)
    head[1:] = (contig[1:] != contig[:-1]) | (a[1:] != a[:-1]) | (b[1:] != b[:-1])
    at = np.flatnonzero(head)
    out = np.zeros(len(at), dtype=DT)
    out['contig'], out['ps_a'], out['ps_b'] = contig[at], a[at], b[at]
    for name, v in (('n_same', same), ('n_flip', flip), ('n_open', opened)):
        out[name] = np.add.reduceat(v[order].astype(np.int64), at)
    out['n_sv'] = out['n_same'] + out['n_flip'] + out['n_open']
    out['w_same'] = np.add.reduceat(np.where(same, w, 0).astype(np.uint64)[order], at)
    out['w_flip'] = np.add.reduceat(np.where(flip, w, 0).astype(np.uint64)[order], at)
    out['pos_min'], out['pos_max'] = np.minimum.reduceat(pos[order], at), np.maximum.reduceat(pos[order], at)
    return out


def main():
    ctx = _lib.Context(0)
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev)
    lines = []
    for label, make in (('configs[1]', lambda: [synth.bench_contig('1', 200000, 100000, 1, spelled='chr1')]),
                        ('2e7 marks', lambda: synth.bench_genome(20000000, 3))):
        soa = engine.soa_from_synth(make())
        dp = DeviceProblem(soa, 50, 2)
        room = _lib.ps_links_room(soa.n_marks)
        out = torch.zeros(max(room, 1) * DT.itemsize, dtype=torch.uint8, device=dev)
        got, info = {}, {}

        def device():
            got['n'] = ctx.ps_links_device(dp.problem, out.data_ptr(), room, stream.cuda_stream)
            torch.cuda.synchronize()

        def copy():
            got['records'] = out[:got['n'] * DT.itemsize].cpu().numpy().view(DT)

        def host_way():
            got['host'] = host_links(soa, 50, 2, _lib.PC_MAX, info)

        big = soa.n_marks > 2000000
        variants = [('device', device, rounds), ('copy', copy, rounds), ('host_way', host_way, min(rounds, host_rounds_big) if big else rounds)]
        for _, run, _ in variants:                                                 # warm-up, and the two results against each other
            run()
        assert got['records'].tobytes() == got['host'].tobytes(), 'the device records differ from the host way'
        ms = {i: [] for i in range(len(variants))}
        for r in range(rounds):
            for i, (_, run, n) in enumerate(variants):
                if r >= n:
                    continue
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                ms[i].append((time.perf_counter() - t0) * 1e3)
        assert got['records'].tobytes() == got['host'].tobytes()
        med = {what: float(np.median(ms[i])) for i, (what, _, _) in enumerate(variants)}
        for i, (what, _, n) in enumerate(variants):
            lines.append(dict(workload=label, marks=soa.n_marks, C=soa.n_cands, contigs=soa.n_contigs, n_multi=info['n_multi'], n_obs=info['n_obs'],
                              links=int(got['n']), variant=what, rounds=n, ms_median=round(med[what], 4), ms_min=round(min(ms[i]), 4),
                              ms_max=round(max(ms[i]), 4)))
            print(json.dumps(lines[-1]), flush=True)
        del dp, out, got
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'a') as f:
        for ln in lines:
            f.write(json.dumps(ln) + '\n')
    print('| workload | marks | candidates | multi-PS candidates | observations | links | device ms | copy ms | host way ms | host way / (device + copy) |')
    print('|---|---|---|---|---|---|---|---|---|---|')
    for label in ('configs[1]', '2e7 marks'):
        m = {ln['variant']: ln for ln in lines if ln['workload'] == label}
        d, c, h = m['device']['ms_median'], m['copy']['ms_median'], m['host_way']['ms_median']
        x = m['device']
        print('| %s | %d | %d | %d | %d | %d | %.3f | %.3f | %.1f | %.1f |' % (label, x['marks'], x['C'], x['n_multi'], x['n_obs'], x['links'], d, c, h,
                                                                            h / (d + c)))


if __name__ == '__main__':
    main()
