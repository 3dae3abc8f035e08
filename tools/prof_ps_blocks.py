#!/usr/bin/env python3
"""GPU-side: what the blocks of the phase-set links cost when they are built on the device (duet_ps_join_links_device,
duet_amd/csrc/duet_psblocks.hip) against the way `duet --join_ps` takes today, at two sizes: BASELINE configs[1] (bench.py's
flagship: synth.bench_contig('1', 200000, 100000, 1), ~1 M marks on one contig) and the 2e7-mark genome (synth.bench_genome(2e7, 3):
24 contigs).  Both start from the links of duet_ps_links_device, resident, and end with the remapped tag words resident and the
count of changed words on the host; min_sv 2.

    device      duet_ps_join_links_device: the table built and applied on the device, one host round trip
    host_way    the records device -> host, duet_amd/ps_links.py: blocks (a Python union-find), duet_ps_join_tags_device with the
                host table

Everything is resident in HBM and both variants run in this one process, interleaved: per round each variant once, the host clock
around work that ends in a device synchronise; the figure is the median over the rounds after one warm-up round.  The two ways'
tag words and counts, and the device table (duet_ps_blocks_device) against blocks(), are compared byte for byte before anything is
timed.  launches_per_call, the rounds and the jumps are counted from a kernel trace of one call (torch.profiler), not computed
(null where the profiler gives no kernel events).  Appends one JSON line per (size, variant) to the file given and prints a table.

    python3 tools/prof_ps_blocks.py [rounds=7] [out=profiles/prof_ps_blocks.jsonl]
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
from duet_amd.devmem import DeviceProblem

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, 'profiles', 'prof_ps_blocks.jsonl')
MIN_SV = 2
LT, BT = _lib.PS_LINK_DTYPE, _lib.PS_BLOCK_DTYPE


def traced(run):
    """One call under the profiler's kernel trace -> (launches, rounds, pointer jumps): the kernels the call really launched, the
    rounds counted by their pb_best, the jumps by their pb_jump."""
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            run()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events()
                 if str(getattr(e, 'device_type', '')).endswith('CUDA') and 'Memcpy' not in e.name and 'Memset' not in e.name]
    except RuntimeError:
        names = []
    if not names:
        return None, None, None
    return len(names), sum('pb_best' in n for n in names), sum('pb_jump' in n for n in names)


def main():
    ctx = _lib.Context(0)
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream(dev)
    lines = []
    for label, make in (('configs[1]', lambda: [synth.bench_contig('1', 200000, 100000, 1, spelled='chr1')]),
                        ('2e7 marks', lambda: synth.bench_genome(20000000, 3))):
        soa = engine.soa_from_synth(make())
        R, K = soa.n_reads, soa.n_contigs
        dp = DeviceProblem(soa, 50, 2)
        room = _lib.ps_links_room(soa.n_marks)
        links = torch.zeros(max(room, 1) * LT.itemsize, dtype=torch.uint8, device=dev)
        n_links = ctx.ps_links_device(dp.problem, links.data_ptr(), room, stream.cuda_stream)
        torch.cuda.synchronize()
        tags_dev = torch.zeros(R * 8 + 64, dtype=torch.uint8, device=dev)
        tags_host = torch.zeros(R * 8 + 64, dtype=torch.uint8, device=dev)
        got = {}

        def device():
            got['device'] = ctx.ps_join_links_device(links.data_ptr(), n_links, MIN_SV, dp.problem.read_tag, soa.read_off, R,
                                                     tags_dev.data_ptr(), stream.cuda_stream)
            torch.cuda.synchronize()

        def host_way():
            recs = links[:n_links * LT.itemsize].cpu().numpy().view(LT)
            rows, conflicts = ps_links.blocks(recs, min_sv=MIN_SV)
            got['rows'], got['conflicts'] = rows, conflicts
            got['host'] = ctx.ps_join_tags_device(dp.problem.read_tag, soa.read_off, R, ps_join.table(rows), tags_host.data_ptr(),
                                                  stream.cuda_stream)
            torch.cuda.synchronize()

        def same():
            assert torch.equal(tags_dev[:R * 8], tags_host[:R * 8]), 'the remapped words differ'
            n_changed, counts = got['device']
            assert n_changed == got['host'] and counts['n_rows'] == len(got['rows']) and counts['n_conflicts'] == len(got['conflicts'])

        variants = [('device', device), ('host_way', host_way)]
        for _, run in variants:
            run()
        same()
        # the table itself, byte for byte
        d_rows = torch.zeros(max(2 * n_links, 1) * BT.itemsize, dtype=torch.uint8, device=dev)
        d_conf = torch.zeros(max(n_links, 1) * 4, dtype=torch.uint8, device=dev)
        c = ctx.ps_blocks_device(links.data_ptr(), n_links, K, MIN_SV, d_rows.data_ptr(), 2 * n_links, d_conf.data_ptr(), n_links,
                                 stream.cuda_stream)
        torch.cuda.synchronize()
        assert d_rows[:c['n_rows'] * BT.itemsize].cpu().numpy().tobytes() == ps_join.table(got['rows']).tobytes(), 'the tables differ'
        assert d_conf[:c['n_conflicts'] * 4].cpu().numpy().view(np.uint32).tolist() == list(got['conflicts']), 'the conflicts differ'
        ms = {i: [] for i in range(len(variants))}
        for r in range(rounds):
            for i, (_, run) in enumerate(variants):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                ms[i].append((time.perf_counter() - t0) * 1e3)
        same()
        n_launches, n_rounds, n_jumps = traced(device)
        for i, (what, _) in enumerate(variants):
            lines.append(dict(workload=label, marks=soa.n_marks, reads=R, contigs=K, links=int(n_links), min_sv=MIN_SV,
                              counts=got['device'][1], n_changed=int(got['device'][0]), launches_per_call=n_launches if what == 'device' else None,
                              forest_rounds=n_rounds, pointer_jumps=n_jumps,
                              variant=what, rounds=rounds, ms_median=round(float(np.median(ms[i])), 4), ms_min=round(min(ms[i]), 4),
                              ms_max=round(max(ms[i]), 4)))
            print(json.dumps(lines[-1]), flush=True)
        del dp, links, tags_dev, tags_host, got
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'a') as f:
        for ln in lines:
            f.write(json.dumps(ln) + '\n')
    print('| workload | links | table rows | conflicts | launches | rounds | jumps | device ms (min .. max) | host way ms (min .. max) | host way / device |')
    print('|---|---|---|---|---|---|---|---|---|---|')
    for label in ('configs[1]', '2e7 marks'):
        m = {ln['variant']: ln for ln in lines if ln['workload'] == label}
        d, h = m['device'], m['host_way']
        print('| %s | %d | %d | %d | %s | %s | %s | %.3f (%.3f .. %.3f) | %.2f (%.2f .. %.2f) | %.1f |' % (
            label, d['links'], d['counts']['n_rows'], d['counts']['n_conflicts'], d['launches_per_call'], d['forest_rounds'], d['pointer_jumps'], d['ms_median'],
            d['ms_min'], d['ms_max'], h['ms_median'], h['ms_min'], h['ms_max'], h['ms_median'] / d['ms_median']))


if __name__ == '__main__':
    main()
