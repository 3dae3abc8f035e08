#!/usr/bin/env python3
"""GPU-side: what the evaluator's per-record outcome costs (duet_eval_details_host, duet_amd/csrc/duet_eval_details.hip) against
the Python path (evaluation.details_host), at the sweep workload of tools/prof_sweep.py: synth.bench_genome(1e6, 2), every
eligible candidate a call (75,049), two candidates per truth id (50,001 truth records: record u sits near candidate 2u, at most
40 bp away, with a length between half and 1.2 times the candidate's), the phase-set groups of the candidates' own (contig, PS),
list key = 2 * contig + a type drawn per truth id.  -r 30, -p 0.7.

    details     Context.eval_details_host: host arrays in, the two record arrays and the six counts out -- uploads, kernels and
                copies, to the synchronise
    counts      Context.eval_counts on the same arrays: the evaluator without the records (what --gpu costs without --details)
    python      evaluation.details_host on the same arrays

Every variant runs in this one process, interleaved: per round each variant once, the host clock around it; the figures are the
median, minimum and maximum over the rounds after one warm-up round.  The device's records and counts are compared with the
Python path's byte for byte before anything is timed, and again afterwards.  Appends one JSON line per variant to the file given
and prints a table.

    python3 tools/prof_eval_details.py [rounds=7] [out=profiles/prof_eval_details.jsonl]
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
from duet_amd import _lib, engine, synth
from duet_amd import evaluation as E

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, 'profiles', 'prof_eval_details.jsonl')
NAMES = ('call_tp', 'base_tp', 'call_gt', 'base_gt', 'call_hp', 'base_hp')


def workload(ctx):
    soa = engine.soa_from_synth(synth.bench_genome(1000000, 2))
    feat = ctx.features_host(soa, 50, 2)
    C, K = len(feat), soa.n_contigs
    rng = np.random.default_rng(1)
    elig = feat['eligible'] != 0
    ctg = np.searchsorted(soa.cand_ctg_off, np.arange(C), side='right') - 1
    n_truth = (C + 1) // 2
    first = np.arange(n_truth) * 2                                     # the candidate a truth record is made from
    typ = rng.integers(0, 2, n_truth)
    tkey = 2 * ctg[first] + typ
    tpos = np.maximum(soa.cand_pos[first].astype(np.int64) + rng.integers(-40, 41, n_truth), 0)
    tlen = np.maximum((soa.cand_svlen[first] * rng.uniform(0.5, 1.2, n_truth)).astype(np.int64), 1)
    order = np.lexsort((tpos, tkey))
    off = np.concatenate([[0], np.cumsum(np.bincount(tkey, minlength=2 * K))])
    ckey = 2 * ctg + typ[np.arange(C) // 2]
    assert (np.diff(off)[ckey[elig]] > 0).all()
    _, group = np.unique(ctg[elig].astype(np.int64) * (1 << 32) + feat['ps'][elig], return_inverse=True)
    n_calls = int(elig.sum())
    return dict(base_off=off.astype(np.uint32), base_pos=tpos[order].astype(np.uint32), base_len=tlen[order].astype(np.uint32),
                base_uid=np.arange(n_truth, dtype=np.uint32)[order], base_hp=rng.integers(0, 3, n_truth).astype(np.uint8),
                call_key=ckey[elig].astype(np.uint32), call_pos=soa.cand_pos[elig].astype(np.uint32),
                call_len=soa.cand_svlen[elig].astype(np.uint32), call_uid=np.arange(n_calls, dtype=np.uint32),
                call_group=group.astype(np.uint32), call_hp=rng.integers(0, 3, n_calls).astype(np.uint8),
                n_groups=int(group.max()) + 1, n_base_uid=n_truth, n_call_uid=n_calls, refdist=30, ratio=0.7)


def main():
    ctx = _lib.Context(0)
    a = workload(ctx)
    got = {}

    def details():
        got['details'] = ctx.eval_details_host(a)

    def counts():
        got['counts'] = ctx.eval_counts(a, a['refdist'], a['ratio'])

    def python():
        got['python'] = E.details_host(a, a['refdist'], a['ratio'])

    def compare():
        (n, calls, base), (want_n, want_calls, want_base) = got['details'], got['python']
        assert calls.tobytes() == want_calls.tobytes(), 'the call records differ from the Python path'
        assert base.tobytes() == want_base.tobytes(), 'the truth records differ from the Python path'
        assert tuple(int(getattr(n, f)) for f in NAMES) == tuple(int(getattr(got['counts'], f)) for f in NAMES) == tuple(want_n)

    variants = [('details', details), ('counts', counts), ('python', python)]
    for _, run in variants:
        run()
    compare()
    ms = {what: [] for what, _ in variants}
    for _ in range(rounds):
        for what, run in variants:
            t0 = time.perf_counter()
            run()
            ms[what].append((time.perf_counter() - t0) * 1e3)
    compare()
    n, calls, base = got['details']
    reasons = np.bincount(base['reason'][base['n_calls'] == 0], minlength=4)
    lines = []
    for what, _ in variants:
        lines.append(dict(calls=len(calls), truth=len(base), keys=len(a['base_off']) - 1, groups=a['n_groups'],
                          matched=int(np.count_nonzero(calls['bits'] & _lib.EVAL_MATCHED)), hit=int(np.count_nonzero(base['n_calls'])),
                          no_call=int(reasons[0]), far=int(reasons[1]), size=int(reasons[2]), elsewhere=int(reasons[3]),
                          variant=what, rounds=rounds, ms_median=round(float(np.median(ms[what])), 4), ms_min=round(min(ms[what]), 4),
                          ms_max=round(max(ms[what]), 4)))
        print(json.dumps(lines[-1]), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'a') as f:
        for ln in lines:
            f.write(json.dumps(ln) + '\n')
    m = {ln['variant']: ln for ln in lines}
    print('| variant | median ms | min | max |')
    print('|---|---|---|---|')
    for what, _ in variants:
        print('| %s | %.3f | %.3f | %.3f |' % (what, m[what]['ms_median'], m[what]['ms_min'], m[what]['ms_max']))
    print('python / details: %.1f' % (m['python']['ms_median'] / m['details']['ms_median']))


if __name__ == '__main__':
    main()
