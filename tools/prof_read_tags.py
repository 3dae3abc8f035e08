#!/usr/bin/env python3
"""GPU-side: what the read tags cost (duet_read_tags_device and duet_read_tags_rows_device, duet_amd/csrc/duet_readtags.hip)
against building the records on the host, at two sizes: BASELINE configs[1] (bench.py's flagship:
synth.bench_contig('1', 200000, 100000, 1), ~1 M marks on one contig) and the 2e7-mark genome (synth.bench_genome(2e7, 3): 24
contigs).  The calls (pred, ps) are those of duet_ef_run_device on the same resident problem; a read's name is its index in the
tag table, a mark without a read has a name of its own behind them; the name texts are ten bytes each.

    device      duet_read_tags_device on the resident problem, to the synchronise behind the copy of the records out of the
                workspace (its three host round trips included)
    copy        the records from HBM to the host
    host_way    without the new kernels: the rule restated in numpy on the host arrays (host_read_tags below: masks, one stable
                sort of the (name, ps) keys, reduceat)
    rows        duet_read_tags_rows_device on the resident records, to the synchronise behind the writer; GB/s = text bytes / time

Everything is resident in HBM and every variant runs in this one process, interleaved: per round each variant once, the host
clock around work that ends in a device synchronise (the host way ends on the host); the figure is the median over the rounds
after one warm-up round.  The device's records are compared with the host way's byte for byte before anything is timed.
Appends one JSON line per (size, variant) to the file given and prints a table.

    python3 tools/prof_read_tags.py [rounds=7] [out=profiles/prof_read_tags.jsonl] [host_rounds_at_2e7=3]
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
from duet_amd.devmem import DeviceProblem, upload

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, 'profiles', 'prof_read_tags.jsonl')
host_rounds_big = int(sys.argv[3]) if len(sys.argv) > 3 else 3
DT = _lib.READ_TAG_DTYPE
ABSENT = _lib.MARK_ABSENT
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def host_read_tags(soa, mark_name, pred, ps, cap):
    """The rule of include/duet_ef.h ("Read tags from phased SVs") in numpy -> READ_TAG_DTYPE records."""
    C, R = soa.n_cands, soa.n_reads
    if C == 0 or soa.n_marks == 0:
        return np.zeros(0, dtype=DT)
    cand = np.repeat(np.arange(C, dtype=np.int64), np.diff(soa.cand_off.astype(np.int64)))
    het = ((pred == 1) | (pred == 2))[cand]
    c = cand[het]
    if not len(c):
        return np.zeros(0, dtype=DT)
    key = (mark_name[het].astype(np.uint64) << np.uint64(32)) | ps[c].astype(np.uint64)
    order = np.argsort(key, kind='stable')
    key, c, rd = key[order], c[order], soa.mark_read[het][order]
    head = np.ones(len(key), dtype=bool)
    head[1:] = key[1:] != key[:-1]
    at = np.flatnonzero(head)
    contig = (np.searchsorted(soa.cand_ctg_off, c, side='right') - 1).astype(np.uint32)
    out = np.zeros(len(at), dtype=DT)
    out['name'], out['ps'] = (key[at] >> np.uint64(32)).astype(np.uint32), (key[at] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    out['n_h1'] = np.add.reduceat((pred[c] == 1).astype(np.int64), at)
    out['n_h2'] = np.add.reduceat((pred[c] == 2).astype(np.int64), at)
    pos = soa.cand_pos[c]
    out['pos_min'], out['pos_max'] = np.minimum.reduceat(pos, at), np.maximum.reduceat(pos, at)
    out['contig'], out['read'] = np.minimum.reduceat(contig, at), np.minimum.reduceat(rd, at)
    # one name, one contig, one read index: inside a record and from one record of a name to the next
    same = out['name'][1:] == out['name'][:-1]
    if np.any(np.maximum.reduceat(contig, at) != out['contig']) or np.any(np.maximum.reduceat(rd, at) != out['read']) or \
            np.any(same & ((out['contig'][1:] != out['contig'][:-1]) | (out['read'][1:] != out['read'][:-1]))):
        raise ValueError('a name on two contigs or with two read indices')
    present = (out['read'] != ABSENT) & (out['read'] < R)
    t = soa.read_tag[np.where(present, out['read'], 0)] if R else np.zeros(len(at), dtype=np.uint64)
    hap, pc = (t >> np.uint64(62)).astype(np.int64), (t >> np.uint64(32)) & np.uint64(0x3FFFFFFF)
    usable = present & (t != ONES) & ((hap == 1) | (hap == 2)) & (pc <= np.uint64(cap))
    sv = np.where(out['n_h1'] > out['n_h2'], 1, np.where(out['n_h2'] > out['n_h1'], 2, 0))
    other = usable & ((t & np.uint64(0xFFFFFFFF)).astype(np.uint32) != out['ps'])
    out['status'] = np.where(other, 4, np.where(sv == 0, 2, np.where(usable, np.where(hap == sv, 0, 1), 3)))
    return out


def synthetic_names(soa):
    """-> (mark_name u32[M], n_names, name_off u64[n_names + 1], name_pool u8[10 * n_names]): r_ and eight hex digits."""
    mr = soa.mark_read
    absent = mr == ABSENT
    mark_name = np.where(absent, soa.n_reads + np.cumsum(absent) - 1, mr).astype(np.uint32)
    n = soa.n_reads + int(absent.sum())
    idx = np.arange(n, dtype=np.uint32)
    pool = np.empty((n, 10), dtype=np.uint8)
    pool[:, 0], pool[:, 1] = ord('r'), ord('_')
    digits = np.frombuffer(b'0123456789abcdef', dtype=np.uint8)
    for j in range(8):
        pool[:, 2 + j] = digits[(idx >> np.uint32(4 * (7 - j))) & np.uint32(15)]
    return mark_name, n, np.arange(n + 1, dtype=np.uint64) * np.uint64(10), pool.reshape(-1)


def main():
    ctx = _lib.Context(0)
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev)
    lines = []
    for label, make in (('configs[1]', lambda: [synth.bench_contig('1', 200000, 100000, 1, spelled='chr1')]),
                        ('2e7 marks', lambda: synth.bench_genome(20000000, 3))):
        soa = engine.soa_from_synth(make())
        dp = DeviceProblem(soa, 50, 2)
        dp.run(ctx)
        torch.cuda.synchronize()
        pred, ps = dp.results()
        mark_name, n_names, name_off, name_pool = synthetic_names(soa)
        chroms = ['chr%d' % (k + 1) for k in range(soa.n_contigs)]
        keep = [upload(torch, dev, mark_name, np.uint32), upload(torch, dev, name_off, np.uint64), upload(torch, dev, name_pool, np.uint8)]
        ctg_off = np.ascontiguousarray(soa.cand_ctg_off, dtype=np.uint32)
        p = _lib.ReadTagsProblem()
        p.n_cands, p.n_marks, p.n_reads, p.n_names, p.n_contigs = soa.n_cands, soa.n_marks, soa.n_reads, n_names, soa.n_contigs
        ef = dp.problem
        p.cand_off, p.mark_read, p.read_tag, p.cand_pos = ef.cand_off, ef.mark_read, ef.read_tag, ef.cand_pos
        p.mark_name, p.cand_ctg_off = keep[0].data_ptr(), ctg_off.ctypes.data
        p.pred, p.ps = dp.out_block.data_ptr() + 4 * dp.n_max, dp.out_block.data_ptr()
        room = soa.n_marks
        out = torch.zeros(max(room, 1) * DT.itemsize, dtype=torch.uint8, device=dev)
        hold = []
        nm = _lib.callset_names(0, keep[1].data_ptr(), keep[2].data_ptr(), chroms, hold)
        nm.n_names = n_names
        got = {}

        def device():
            got['n'] = ctx.read_tags_device(p, out.data_ptr(), room, stream.cuda_stream)
            torch.cuda.synchronize()

        def copy():
            got['records'] = out[:got['n'] * DT.itemsize].cpu().numpy().view(DT)

        def host_way():
            got['host'] = host_read_tags(soa, mark_name, pred, ps, _lib.PC_MAX)

        device()
        cap = _lib.read_tags_bound(got['n'], name_off[:2], chroms)            # (every name has ten bytes)
        text = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)

        def rows():
            got['bytes'] = ctx.read_tags_rows_device(out.data_ptr(), got['n'], nm, ef.read_tag, soa.n_reads, text.data_ptr(), cap,
                                                     stream.cuda_stream)
            torch.cuda.synchronize()

        big = soa.n_marks > 2000000
        variants = [('device', device, rounds), ('copy', copy, rounds), ('host_way', host_way, min(rounds, host_rounds_big) if big else rounds),
                    ('rows', rows, rounds)]
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
        counts = np.bincount(got['records']['status'].astype(np.int64), minlength=5)
        med = {what: float(np.median(ms[i])) for i, (what, _, _) in enumerate(variants)}
        for i, (what, _, n) in enumerate(variants):
            lines.append(dict(workload=label, marks=soa.n_marks, C=soa.n_cands, contigs=soa.n_contigs, n_names=n_names,
                              het=int(((pred == 1) | (pred == 2)).sum()), records=int(got['n']),
                              status={s: int(counts[j]) for j, s in enumerate(_lib.READ_TAG_STATUS_NAMES)}, text_bytes=int(got['bytes']),
                              variant=what, rounds=n, ms_median=round(med[what], 4), ms_min=round(min(ms[i]), 4), ms_max=round(max(ms[i]), 4)))
            print(json.dumps(lines[-1]), flush=True)
        del dp, out, text, keep, got
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'a') as f:
        for ln in lines:
            f.write(json.dumps(ln) + '\n')
    print('| workload | marks | candidates | het calls | records | device ms | copy ms | host way ms | host way / (device + copy) | rows ms | rows GB/s |')
    print('|---|---|---|---|---|---|---|---|---|---|---|')
    for label in ('configs[1]', '2e7 marks'):
        m = {ln['variant']: ln for ln in lines if ln['workload'] == label}
        d, c, h, w = m['device']['ms_median'], m['copy']['ms_median'], m['host_way']['ms_median'], m['rows']['ms_median']
        x = m['device']
        print('| %s | %d | %d | %d | %d | %.3f | %.3f | %.1f | %.1f | %.3f | %.1f |' % (
            label, x['marks'], x['C'], x['het'], x['records'], d, c, h, h / (d + c), w, x['text_bytes'] / (w * 1e6)))


if __name__ == '__main__':
    main()
