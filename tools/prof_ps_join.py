#!/usr/bin/env python3
"""GPU-side: what the joined phase sets cost (duet_ps_join_tags_device and duet_ps_join_diff_device,
duet_amd/csrc/duet_psjoin.hip) against the same rule on the host, at two sizes: BASELINE configs[1] (bench.py's flagship:
synth.bench_contig('1', 200000, 100000, 1), ~1 M marks on one contig) and the 2e7-mark genome (synth.bench_genome(2e7, 3): 24
contigs).  The table is the one `duet --join_ps` would use: the links of duet_ps_links_device on the resident problem, joined by
duet_amd/ps_links.py: blocks with min_sv 2.  The calls before and after are those of duet_ef_run_device on the resident problem
and on the same problem over the remapped tags (not timed: the ordinary run).

    device      duet_ps_join_tags_device into a second resident table, then duet_ps_join_diff_device on the resident calls, to the
                synchronise behind the copy of the codes out of the workspace (one host round trip each; the staging of the table
                included)
    host_way    without the new kernels: the rule restated in numpy on the host arrays (host_remap and host_diff below: one
                searchsorted per contig and masks)

Everything is resident in HBM and both variants run in this one process, interleaved: per round each variant once, the host clock
around work that ends in a device synchronise (the host way ends on the host); the figure is the median over the rounds after one
warm-up round.  The device's tag words, codes and counts are compared with the host way's byte for byte before anything is timed.
Appends one JSON line per (size, variant) to the file given and prints a table.

    python3 tools/prof_ps_join.py [rounds=7] [out=profiles/prof_ps_join.jsonl]
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
from duet_amd import _lib, engine, ps_join, ps_links, synth
from duet_amd.devmem import DEVICE_FIELDS, DeviceProblem

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, 'profiles', 'prof_ps_join.jsonl')
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
U32 = np.uint64(0xFFFFFFFF)


def lookup(table, k, ps):
    """The rows of contig k for the PS values ps -> (hit mask, block, flip)."""
    rows = table[table['contig'] == k]
    if not len(rows):
        return np.zeros(len(ps), dtype=bool), ps, np.zeros(len(ps), dtype=np.uint32)
    at = np.minimum(np.searchsorted(rows['ps'], ps), len(rows) - 1)
    hit = rows['ps'][at] == ps
    return hit, np.where(hit, rows['block'][at], ps), np.where(hit, rows['flip'][at], 0).astype(np.uint32)


def host_remap(read_tag, read_off, table):
    """The rule of include/duet_ef.h ("Joined phase sets", Tag word) in numpy -> (words, n_changed)."""
    out = read_tag.copy()
    for k in range(len(read_off) - 1):
        w = read_tag[read_off[k]:read_off[k + 1]]
        hit, block, flip = lookup(table, k, (w & U32).astype(np.uint32))
        hit &= w != ONES
        hap = w >> np.uint64(62)
        turn = hit & (flip == 1) & ((hap == 1) | (hap == 2))
        new = (w & ~U32) | block.astype(np.uint64)
        new = np.where(turn, new ^ (np.uint64(3) << np.uint64(62)), new)
        out[read_off[k]:read_off[k + 1]] = np.where(hit, new, w)
    return out, int((out != read_tag).sum())


def host_diff(ctg_off, p0, s0, p1, s1, table):
    """... (Change) in numpy -> (codes u8[C], counts u32[8])."""
    C = len(p0)
    pe, se = p0.copy(), s0.copy()
    for k in range(len(ctg_off) - 1):
        a, b = int(ctg_off[k]), int(ctg_off[k + 1])
        hit, block, flip = lookup(table, k, s0[a:b])
        het = (p0[a:b] == 1) | (p0[a:b] == 2)
        pe[a:b] = np.where(hit & (flip == 1) & het, 3 - p0[a:b], p0[a:b])
        se[a:b] = block
    het0, het1 = (p0 == 1) | (p0 == 2), (p1 == 1) | (p1 == 2)
    conds = [(p0 == 0) & (p1 == 0), p0 == 0, p1 == 0, (p1 == p0) & (s1 == s0), (p1 == pe) & (s1 == se), (p0 == 3) & het1, het0 & (p1 == 3)]
    codes = np.select(conds, list(range(7)), default=7).astype(np.uint8)
    return codes, np.bincount(codes, minlength=8).astype(np.uint32)[:8] if C else np.zeros(8, dtype=np.uint32)


def main():
    ctx = _lib.Context(0)
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev)
    lines = []
    for label, make in (('configs[1]', lambda: [synth.bench_contig('1', 200000, 100000, 1, spelled='chr1')]),
                        ('2e7 marks', lambda: synth.bench_genome(20000000, 3))):
        soa = engine.soa_from_synth(make())
        C, R, K = soa.n_cands, soa.n_reads, soa.n_contigs
        dp = DeviceProblem(soa, 50, 2)
        dp.run(ctx)
        torch.cuda.synchronize()
        room = _lib.ps_links_room(soa.n_marks)
        links = torch.zeros(max(room, 1) * _lib.PS_LINK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        n_links = ctx.ps_links_device(dp.problem, links.data_ptr(), room, stream.cuda_stream)
        recs = links[:n_links * _lib.PS_LINK_DTYPE.itemsize].cpu().numpy().view(_lib.PS_LINK_DTYPE).copy()
        del links
        rows, conflicts = ps_links.blocks(recs, min_sv=2)
        table = ps_join.table(rows)
        ef = dp.problem
        tags1 = torch.zeros(R * 8 + 64, dtype=torch.uint8, device=dev)
        ptrs = {name: dp.buffers[name].data_ptr() for name in DEVICE_FIELDS}
        ptrs['read_tag'] = tags1.data_ptr()
        joined = _lib.problem_from_device(soa, ptrs, 50, 2)
        calls1 = torch.zeros(C * 5 + 64, dtype=torch.uint8, device=dev)
        change = torch.zeros(C + 64, dtype=torch.uint8, device=dev)
        pred0_ptr, ps0_ptr = dp.out_block.data_ptr() + 4 * dp.n_max, dp.out_block.data_ptr()
        pred1_ptr, ps1_ptr = calls1.data_ptr() + 4 * C, calls1.data_ptr()
        got = {}

        def remap():
            got['n_changed'] = ctx.ps_join_tags_device(ef.read_tag, soa.read_off, R, table, tags1.data_ptr(), stream.cuda_stream)
            torch.cuda.synchronize()

        def diff():
            got['counts'] = ctx.ps_join_diff_device(C, pred0_ptr, ps0_ptr, pred1_ptr, ps1_ptr, table, K, change.data_ptr(),
                                                    cand_ctg_off=soa.cand_ctg_off, stream=stream.cuda_stream)
            torch.cuda.synchronize()

        def device():
            remap()
            diff()

        remap()
        ctx.run_device(joined, pred1_ptr, ps1_ptr, stream.cuda_stream)          # the joined run: the ordinary run on the remapped table
        ctx.check(stream.cuda_stream)
        p0, s0 = dp.results()
        raw = calls1.cpu().numpy()
        s1, p1 = raw[:4 * C].view(np.uint32).copy(), raw[4 * C:5 * C].copy()

        def host_way():
            got['host_tags'], got['host_changed'] = host_remap(soa.read_tag, soa.read_off, table)
            got['host_codes'], got['host_counts'] = host_diff(soa.cand_ctg_off, p0, s0, p1, s1, table)

        def same():
            assert tags1[:R * 8].cpu().numpy().view(np.uint64).tobytes() == got['host_tags'].tobytes(), 'the remapped words differ'
            assert got['n_changed'] == got['host_changed']
            assert change[:C].cpu().numpy().tobytes() == got['host_codes'].tobytes(), 'the change codes differ'
            assert got['counts'].tolist() == got['host_counts'].tolist()

        variants = [('device', device), ('host_way', host_way)]
        for _, run in variants:                                                    # warm-up, and the two results against each other
            run()
        same()
        ms = {i: [] for i in range(len(variants))}
        for r in range(rounds):
            for i, (_, run) in enumerate(variants):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                ms[i].append((time.perf_counter() - t0) * 1e3)
        same()
        for i, (what, _) in enumerate(variants):
            lines.append(dict(workload=label, marks=soa.n_marks, C=C, reads=R, contigs=K, links=int(n_links), table_rows=len(rows),
                              contradicted=len(conflicts), n_changed=int(got['n_changed']),
                              counts={n: int(v) for n, v in zip(_lib.JOIN_CHANGE_NAMES, got['counts'])}, variant=what, rounds=rounds,
                              ms_median=round(float(np.median(ms[i])), 4), ms_min=round(min(ms[i]), 4), ms_max=round(max(ms[i]), 4)))
            print(json.dumps(lines[-1]), flush=True)
        del dp, tags1, calls1, change, got
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'a') as f:
        for ln in lines:
            f.write(json.dumps(ln) + '\n')
    print('| workload | marks | candidates | reads | table rows | reads remapped | device ms | host way ms | host way / device |')
    print('|---|---|---|---|---|---|---|---|---|')
    for label in ('configs[1]', '2e7 marks'):
        m = {ln['variant']: ln for ln in lines if ln['workload'] == label}
        d, h, x = m['device']['ms_median'], m['host_way']['ms_median'], m['device']
        print('| %s | %d | %d | %d | %d | %d | %.3f | %.2f | %.1f |' % (label, x['marks'], x['C'], x['reads'], x['table_rows'], x['n_changed'],
                                                                    d, h, h / d))


if __name__ == '__main__':
    main()
