#!/usr/bin/env python3
"""GPU-side: what the tags from other SVs cost (duet_sv_tags_device, duet_amd/csrc/duet_svtags.hip) against the same rule on the
host, at two sizes: BASELINE configs[1] (bench.py's flagship: synth.bench_contig('1', 200000, 100000, 1), ~1 M marks on one
contig) and the 2e7-mark genome (synth.bench_genome(2e7, 3): 24 contigs).  Every third tag word of each contig is turned to
all-ones, as in tests/sv_tags_cases.py; the calls (pred, ps) are those of duet_ef_run_device on the same resident problem; a
read's name is its index in the tag table, a mark without a read has a name of its own behind them.

    device      duet_sv_tags_device on the resident problem, to the synchronise behind the copy of the words out of the workspace
                and the identity index (its three host round trips included)
    copy        out_tag from HBM to the host (the second run on the device does not need it; the host way ends on the host)
    host_way    without the new kernels: the rule restated in numpy on the host arrays (host_sv_tags below: masks, one stable
                sort of the (name, ps) keys, reduceat, run lengths, a loop over the records of a name)

Everything is resident in HBM and every variant runs in this one process, interleaved: per round each variant once, the host
clock around work that ends in a device synchronise (the host way ends on the host); the figure is the median over the rounds
after one warm-up round.  The device's words and counters are compared with the host way's byte for byte before anything is
timed.  The change counts are those of one more duet_ef_run_device on the expanded problem (not timed).
Appends one JSON line per (size, variant) to the file given and prints a table.

    python3 tools/prof_sv_tags.py [rounds=7] [out=profiles/prof_sv_tags.jsonl] [host_rounds_at_2e7=3]
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
from duet_amd import _lib, engine, sv_tags, synth
from duet_amd.devmem import DeviceProblem, upload

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, 'profiles', 'prof_sv_tags.jsonl')
host_rounds_big = int(sys.argv[3]) if len(sys.argv) > 3 else 3
ABSENT = _lib.MARK_ABSENT
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
SHARE = 3


def host_sv_tags(soa, mark_name, pred, ps, min_votes=1, pc_new=0):
    """The rule of include/duet_ef.h ("Tags from other SVs") in numpy, identity mark order -> (out_tag u64[M], counts)."""
    C, M, R = soa.n_cands, soa.n_marks, soa.n_reads
    cand = np.repeat(np.arange(C, dtype=np.int64), np.diff(soa.cand_off.astype(np.int64)))
    rd = soa.mark_read
    present = (rd != ABSENT) & (rd < R)
    word = np.where(present, soa.read_tag[np.where(present, rd, 0)], ONES) if R else np.full(M, ONES, dtype=np.uint64)
    het = ((pred == 1) | (pred == 2))[cand]
    idx = np.flatnonzero(het)
    k_mark = np.zeros(M, dtype=np.int64)
    rec_name, rec_ps = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    h1 = h2 = np.zeros(0, dtype=np.int64)
    if len(idx):
        c = cand[idx]
        key = (mark_name[idx].astype(np.uint64) << np.uint64(32)) | ps[c].astype(np.uint64)
        order = np.argsort(key, kind='stable')
        key, c, r = key[order], c[order], rd[idx][order]
        head = np.ones(len(key), dtype=bool)
        head[1:] = key[1:] != key[:-1]
        at = np.flatnonzero(head)
        rec_name, rec_ps = (key[at] >> np.uint64(32)).astype(np.int64), (key[at] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        h1 = np.add.reduceat((pred[c] == 1).astype(np.int64), at)
        h2 = np.add.reduceat((pred[c] == 2).astype(np.int64), at)
        contig = np.searchsorted(soa.cand_ctg_off, c, side='right') - 1
        k_lo, r_lo = np.minimum.reduceat(contig, at), np.minimum.reduceat(r, at)
        same = rec_name[1:] == rec_name[:-1]
        if np.any(np.maximum.reduceat(contig, at) != k_lo) or np.any(np.maximum.reduceat(r, at) != r_lo) or \
                np.any(same & ((k_lo[1:] != k_lo[:-1]) | (r_lo[1:] != r_lo[:-1]))):
            raise ValueError('a name on two contigs or with two read indices')
        # a candidate's members of one record are adjacent (stable sort, marks in candidate order): a run's length is k
        rhead = head.copy()
        rhead[1:] |= c[1:] != c[:-1]
        rat = np.flatnonzero(rhead)
        rlen = np.diff(np.append(rat, len(key)))
        k_mark[idx[order]] = np.repeat(rlen, rlen)
    u = np.flatnonzero(word == ONES)
    nm, cu = mark_name[u].astype(np.int64), cand[u]
    lo, hi = np.searchsorted(rec_name, nm, side='left'), np.searchsorted(rec_name, nm, side='right')
    own_pred = np.where(het[u], pred[cu].astype(np.int64), 0)
    own_ps, k = ps[cu].astype(np.int64), k_mark[u]
    best = np.zeros(len(u), dtype=np.int64)
    best_in = np.zeros(len(u), dtype=np.int64)
    best_ps = np.zeros(len(u), dtype=np.int64)
    best_h1 = np.zeros(len(u), dtype=bool)
    for j in range(int((hi - lo).max()) if len(u) else 0):         # the records of a name ascend by PS: a strictly larger |d| replaces
        live = lo + j < hi
        r = np.where(live, lo + j, 0)
        d_in = np.where(live, h1[r] - h2[r], 0)
        own = live & (own_pred != 0) & (rec_ps[r] == own_ps)
        d = d_in + np.where(own, np.where(own_pred == 1, -k, k), 0)
        best_in = np.maximum(best_in, np.abs(d_in))
        better = live & (np.abs(d) > best)
        best, best_ps, best_h1 = np.where(better, np.abs(d), best), np.where(better, rec_ps[r], best_ps), np.where(better, d > 0, best_h1)
    given = best >= min_votes
    out = word.copy()
    out[u[given]] = (np.where(best_h1[given], 1, 2).astype(np.uint64) << np.uint64(62)) | (np.uint64(pc_new) << np.uint64(32)) | \
        best_ps[given].astype(np.uint64)
    return out, (len(u), int(given.sum()), int((~given & (best_in >= min_votes)).sum()))


def synthetic_names(soa):
    mr = soa.mark_read
    absent = mr == ABSENT
    return np.where(absent, soa.n_reads + np.cumsum(absent) - 1, mr).astype(np.uint32), soa.n_reads + int(absent.sum())


def untagged(soa):
    tags = soa.read_tag.copy()
    for k in range(len(soa.read_off) - 1):
        tags[int(soa.read_off[k]):int(soa.read_off[k + 1]):SHARE] = ONES
    kw = {name: getattr(soa, name) for name, _ in engine.EfSoA.FIELDS}
    kw['read_tag'] = tags
    return engine.EfSoA(read_off=soa.read_off, **kw)


def main():
    ctx = _lib.Context(0)
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev)
    lines = []
    for label, make in (('configs[1]', lambda: [synth.bench_contig('1', 200000, 100000, 1, spelled='chr1')]),
                        ('2e7 marks', lambda: synth.bench_genome(20000000, 3))):
        soa = untagged(engine.soa_from_synth(make()))
        M = soa.n_marks
        dp = DeviceProblem(soa, 50, 2, n_out=2)
        dp.run(ctx)
        torch.cuda.synchronize()
        pred, ps = dp.results()
        mark_name, n_names = synthetic_names(soa)
        d_names = upload(torch, dev, mark_name, np.uint32)
        ctg_off = np.ascontiguousarray(soa.cand_ctg_off, dtype=np.uint32)
        p = _lib.ReadTagsProblem()
        p.n_cands, p.n_marks, p.n_reads, p.n_names, p.n_contigs = soa.n_cands, M, soa.n_reads, n_names, soa.n_contigs
        ef = dp.problem
        p.cand_off, p.mark_read, p.read_tag = ef.cand_off, ef.mark_read, ef.read_tag
        p.mark_name, p.cand_ctg_off = d_names.data_ptr(), ctg_off.ctypes.data
        p.pred, p.ps = dp.out_block.data_ptr() + 4 * dp.n_max, dp.out_block.data_ptr()
        out = torch.zeros(M * 8 + 64, dtype=torch.uint8, device=dev)
        index = torch.zeros(M * 4 + 64, dtype=torch.uint8, device=dev)
        got = {}

        def device():
            got['counts'] = ctx.sv_tags_device(p, out.data_ptr(), index.data_ptr(), stream=stream.cuda_stream)
            torch.cuda.synchronize()

        def copy():
            got['words'] = out[:M * 8].cpu().numpy().view(np.uint64)

        def host_way():
            got['host'] = host_sv_tags(soa, mark_name, pred, ps)

        big = M > 2000000
        variants = [('device', device, rounds), ('copy', copy, rounds), ('host_way', host_way, min(rounds, host_rounds_big) if big else rounds)]
        for _, run, _ in variants:                                                 # warm-up, and the two results against each other
            run()
        assert got['words'].tobytes() == got['host'][0].tobytes(), 'the device words differ from the host way'
        assert got['counts'] == got['host'][1], (got['counts'], got['host'][1])
        assert index[:M * 4].cpu().numpy().view(np.uint32).tobytes() == np.arange(M, dtype=np.uint32).tobytes()
        # the second run, once: the same resident problem pointed at the words and the identity index
        second = _lib.EfProblem.from_buffer_copy(ef)
        second.read_tag, second.mark_read, second.n_reads = out.data_ptr(), index.data_ptr(), M
        blk = dp.out_blocks[1]
        ctx.run_device(second, blk.data_ptr() + 4 * dp.n_max, blk.data_ptr(), stream.cuda_stream)
        ctx.check(stream.cuda_stream)
        pred1, ps1 = dp.results(1)
        _, changes = sv_tags.change_codes(pred, ps, pred1, ps1)
        ms = {i: [] for i in range(len(variants))}
        for r in range(rounds):
            for i, (_, run, n) in enumerate(variants):
                if r >= n:
                    continue
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                ms[i].append((time.perf_counter() - t0) * 1e3)
        assert got['words'].tobytes() == got['host'][0].tobytes()
        med = {what: float(np.median(ms[i])) for i, (what, _, _) in enumerate(variants)}
        for i, (what, _, n) in enumerate(variants):
            lines.append(dict(workload=label, marks=M, C=soa.n_cands, contigs=soa.n_contigs, n_names=n_names, share='1/%d' % SHARE,
                              het=int(((pred == 1) | (pred == 2)).sum()), untagged=got['counts'][0], given=got['counts'][1],
                              own_only=got['counts'][2], changes={n_: int(v) for n_, v in zip(_lib.JOIN_CHANGE_NAMES, changes)},
                              variant=what, rounds=n, ms_median=round(med[what], 4), ms_min=round(min(ms[i]), 4), ms_max=round(max(ms[i]), 4)))
            print(json.dumps(lines[-1]), flush=True)
        del dp, out, index, d_names, got
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'a') as f:
        for ln in lines:
            f.write(json.dumps(ln) + '\n')
    print('| workload | marks | candidates | het calls | untagged | given | own-only | gained | lost | device ms | copy ms | host way ms | host way / (device + copy) |')
    print('|---|---|---|---|---|---|---|---|---|---|---|---|---|')
    for label in ('configs[1]', '2e7 marks'):
        m = {ln['variant']: ln for ln in lines if ln['workload'] == label}
        d, c, h = m['device']['ms_median'], m['copy']['ms_median'], m['host_way']['ms_median']
        x = m['device']
        print('| %s | %d | %d | %d | %d | %d | %d | %d | %d | %.3f | %.3f | %.1f | %.1f |' % (
            label, x['marks'], x['C'], x['het'], x['untagged'], x['given'], x['own_only'], x['changes']['gained'], x['changes']['lost'],
            d, c, h, h / (d + c)))


if __name__ == '__main__':
    main()
