#!/usr/bin/env python3
"""GPU-side: what the planned tags from other SVs cost (duet_sv_tags_plan_device / duet_sv_tags_apply_device,
duet_amd/csrc/duet_svtags_plan.hip) against duet_sv_tags_device per vector, at the two sizes of tools/prof_sv_tags.py: BASELINE
configs[1] (~1 M marks on one contig) and the 2e7-mark genome (24 contigs), every third tag word of each contig all-ones, the calls
(pred, ps) those of duet_ef_run_device on the same resident problem, the mask = pred != 0.

    sv_tags     duet_sv_tags_device on the resident problem, to the synchronise behind it: the parent's way, per vector
    plan        duet_sv_tags_plan_device, once per setting, to the synchronise behind it
    apply       one duet_sv_tags_apply_device: VECTORS (>= 32) applies queued between two synchronisations, the time divided by
                their number -- every other one with a pred whose het calls are thinned, so that the words do move

One process, the variants interleaved: per round each once, the host clock around work that ends in a device synchronise; the
figure is the median over the rounds after one warm-up round, with minimum and maximum.  Before anything is timed the words and
the counters of plan + apply are compared with duet_sv_tags_device's byte for byte, for both preds.
Appends one JSON line per (size, variant) to the file given and prints a table.

    python3 tools/prof_sv_tags_plan.py [rounds=7] [out=profiles/prof_sv_tags_plan.jsonl]
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
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, 'profiles', 'prof_sv_tags_plan.jsonl')
ABSENT = _lib.MARK_ABSENT
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
SHARE = 3
VECTORS = 32


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
    st = stream.cuda_stream
    lines = []
    for label, make in (('configs[1]', lambda: [synth.bench_contig('1', 200000, 100000, 1, spelled='chr1')]),
                        ('2e7 marks', lambda: synth.bench_genome(20000000, 3))):
        soa = untagged(engine.soa_from_synth(make()))
        M, C = soa.n_marks, soa.n_cands
        dp = DeviceProblem(soa, 50, 2)
        dp.run(ctx)
        torch.cuda.synchronize()
        pred, ps = dp.results()
        thin = pred.copy()
        het = np.flatnonzero((pred == 1) | (pred == 2))
        thin[het[::2]] = 0
        preds = [upload(torch, dev, a, np.uint8) for a in (pred, thin)]
        mask = upload(torch, dev, (pred != 0).astype(np.uint8), np.uint8)
        mark_name, n_names = synthetic_names(soa)
        d_names = upload(torch, dev, mark_name, np.uint32)
        ctg_off = np.ascontiguousarray(soa.cand_ctg_off, dtype=np.uint32)
        p = _lib.ReadTagsProblem()
        p.n_cands, p.n_marks, p.n_reads, p.n_names, p.n_contigs = C, M, soa.n_reads, n_names, soa.n_contigs
        ef = dp.problem
        p.cand_off, p.mark_read, p.read_tag = ef.cand_off, ef.mark_read, ef.read_tag
        p.mark_name, p.cand_ctg_off = d_names.data_ptr(), ctg_off.ctypes.data
        p.pred, p.ps = preds[0].data_ptr(), dp.out_block.data_ptr()
        out = torch.zeros(M * 8 + 64, dtype=torch.uint8, device=dev)
        out2 = torch.zeros(M * 8 + 64, dtype=torch.uint8, device=dev)
        index = torch.zeros(M * 4 + 64, dtype=torch.uint8, device=dev)
        four = torch.zeros(4 * VECTORS, dtype=torch.int32, device=dev)
        got = {}

        def sv_tags():
            got['counts'] = ctx.sv_tags_device(p, out.data_ptr(), index.data_ptr(), stream=st)
            torch.cuda.synchronize()

        def plan():
            got['info'] = ctx.sv_tags_plan_device(p, out2.data_ptr(), index.data_ptr(), cand_mask_ptr=mask.data_ptr(), stream=st)
            torch.cuda.synchronize()

        def applies():
            for v in range(VECTORS):
                ctx.sv_tags_apply_device(preds[v & 1].data_ptr(), out2.data_ptr(), four.data_ptr() + 16 * v, stream=st)
            torch.cuda.synchronize()

        # the two ways against each other, byte for byte, for both preds
        plan()
        for i in (0, 1):
            p.pred = preds[i].data_ptr()
            sv_tags()
            ctx.sv_tags_apply_device(preds[i].data_ptr(), out2.data_ptr(), four.data_ptr(), stream=st)
            torch.cuda.synchronize()
            assert out[:M * 8].cpu().numpy().tobytes() == out2[:M * 8].cpu().numpy().tobytes(), 'the applied words differ from duet_sv_tags_device'
            assert tuple(four[:4].cpu().numpy().tolist()) == got['counts'] + (0,), (four[:4].cpu().numpy().tolist(), got['counts'])
            got['counts%d' % i] = got['counts']
        p.pred = preds[0].data_ptr()
        variants = [('sv_tags', sv_tags, 1), ('plan', plan, 1), ('apply', applies, VECTORS)]
        for _, run, _ in variants:
            run()
        ms = {i: [] for i in range(len(variants))}
        for r in range(rounds):
            for i, (_, run, n) in enumerate(variants):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                ms[i].append((time.perf_counter() - t0) * 1e3 / n)
        for i, (what, _, n) in enumerate(variants):
            lines.append(dict(workload=label, marks=M, C=C, contigs=soa.n_contigs, n_names=n_names, share='1/%d' % SHARE,
                              het=int(len(het)), untagged=got['counts0'][0], given=got['counts0'][1], own_only=got['counts0'][2],
                              given_thinned=got['counts1'][1], plan=got['info'], variant=what, rounds=rounds, calls_per_round=n,
                              ms_median=round(float(np.median(ms[i])), 4), ms_min=round(min(ms[i]), 4), ms_max=round(max(ms[i]), 4)))
            print(json.dumps(lines[-1]), flush=True)
        del dp, out, out2, index, d_names, got, preds, mask
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'a') as f:
        for ln in lines:
            f.write(json.dumps(ln) + '\n')
    print('| workload | marks | candidates | het calls | untagged | records | runs | sv_tags ms (min .. max) | plan ms (min .. max) | apply ms (min .. max) | sv_tags / apply |')
    print('|---|---|---|---|---|---|---|---|---|---|---|')
    for label in ('configs[1]', '2e7 marks'):
        m = {ln['variant']: ln for ln in lines if ln['workload'] == label}
        x = m['sv_tags']
        cell = lambda v: '%.3f (%.3f .. %.3f)' % (m[v]['ms_median'], m[v]['ms_min'], m[v]['ms_max'])
        print('| %s | %d | %d | %d | %d | %d | %d | %s | %s | %s | %.1f |' % (
            label, x['marks'], x['C'], x['het'], x['untagged'], x['plan']['n_records'], x['plan']['n_runs'], cell('sv_tags'), cell('plan'),
            cell('apply'), m['sv_tags']['ms_median'] / m['apply']['ms_median']))


if __name__ == '__main__':
    main()
