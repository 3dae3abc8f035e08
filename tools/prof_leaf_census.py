#!/usr/bin/env python3
"""GPU-side: what the leaf census costs (duet_tune_leaf_census_device, duet_amd/csrc/duet_tune_leaf.hip) at tools/prof_sweep.py's
workload -- synth.bench_genome(1e6): ~1 M marks, ~1e5 candidates on 24 contigs, every eligible candidate a call, three in four
matched, two candidates per truth id inside a contig, the phase-set groups of the candidates' own (contig, PS) -- for K = 1, 256
and 4096 vectors:

    plain       duet_tune_sweep_device with the truth set (one record per vector)
    census      duet_tune_leaf_census_device, S = 1 (one record per vector and leaf)
    host_way    the way without the census kernels: the sweep with out_pred, then K x C preds and the flag, group, pair and feature
                arrays brought to the host, and there per vector the leaves (numpy, derived once), the groups' labels and
                numpy.bincount per field

Everything is resident in HBM and every variant runs in this one process, interleaved: per round each variant once, the host
clock around work that ends in a device synchronise (the host way ends on the host); the figure is the median over the rounds
after one warm-up round.  The census is compared with the host way word for word, and its sums over the leaves with the plain
sweep, before anything is timed.  Appends one JSON line per (K, variant) to the file given and prints a table.

    python3 tools/prof_leaf_census.py [rounds=7] [out=profiles/prof_leaf_census.jsonl] [host_rounds_at_4096=3]
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
from duet_amd import _lib, engine, synth, tune

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, 'profiles', 'prof_leaf_census.jsonl')
host_rounds_big = int(sys.argv[3]) if len(sys.argv) > 3 else 3
soa = engine.soa_from_synth(synth.bench_genome(1000000, 2))
ctx = _lib.Context(0)
feat = ctx.features_host(soa, 50, 2)
C = len(feat)
rng = np.random.default_rng(1)
elig = feat['eligible'] != 0
ctg = (np.searchsorted(soa.cand_ctg_off, np.arange(C), side='right') - 1).astype(np.int64)
_, group = np.unique(ctg * (1 << 32) + feat['ps'], return_inverse=True)
G = int(group.max()) + 1
matched = elig & (rng.random(C) < 0.75)
bits = rng.integers(0, 1 << 9, C).astype(np.uint16)
flags = (np.where(elig, _lib.TUNE_IN_CALLS, 0) | np.where(matched, _lib.TUNE_MATCHED, 0) | np.where(matched, bits, 0)).astype(np.uint16)
# two candidates per truth id, inside their contig
uid = (ctg * (C // 2 + 1) + (np.arange(C) - soa.cand_ctg_off[ctg].astype(np.int64)) // 2).astype(np.int64)
_, uid = np.unique(uid, return_inverse=True)
n_uid = int(uid.max()) + 1
order = np.lexsort((uid, group))
order = order[matched[order]]
pkey = group[order].astype(np.int64) * n_uid + uid[order]
first = np.concatenate([[True], pkey[1:] != pkey[:-1]])
pair = np.zeros(C, dtype=np.uint32)
pair[order] = np.cumsum(first) - 1
n_pairs = int(first.sum())
pair_group = group[order][first].astype(np.int64)
pair_uid = uid[order][first].astype(np.uint32)
gpo = np.concatenate([[0], np.cumsum(np.bincount(pair_group, minlength=G))]).astype(np.uint32)

dev = torch.device('cuda', 0)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
stream = torch.cuda.current_stream(dev)
keep = dict(cand_flags=t(flags.view(np.int16)), cand_group=t(group.astype(np.uint32).view(np.int32)), cand_uid=t(uid.astype(np.uint32).view(np.int32)),
            cand_pair=t(pair.view(np.int32)), group_pair_off=t(gpo.view(np.int32)), pair_uid=t(pair_uid.view(np.int32)))
truth = _lib.TuneTruth()
truth.n_uid, truth.n_groups, truth.n_pairs = n_uid, G, n_pairs
for name, _ in _lib.TRUTH_ARRAYS:
    setattr(truth, name, keep[name].data_ptr())
d_feat = t(feat.view(np.uint8))
item, leaf_item = _lib.COUNTS_DTYPE.itemsize, _lib.LEAF_COUNTS_DTYPE.itemsize * _lib.N_LEAVES
IN, RAISES, MATCHED = _lib.TUNE_IN_CALLS, _lib.TUNE_RAISES, _lib.TUNE_MATCHED


def derived(f):
    """What the tree compares (duet_tune_derive.hip.h), for the eligible candidates, in binary64."""
    with np.errstate(divide='ignore', invalid='ignore'):
        t1, t2 = f['t1'].astype(np.float64), f['t2'].astype(np.float64)
        a1 = np.where(f['hap1'] > 0, t1 / f['hap1'], 0.0)
        a2 = np.where(f['hap2'] > 0, t2 / f['hap2'], 0.0)
        lo, hi = np.minimum(f['t1'], f['t2']), np.maximum(f['t1'], f['t2'])
        return dict(cls=f['cls'], hr=f['allhap'] / np.maximum(f['deg'], 1).astype(np.float64),
                    sv=f['svread'] / (f['svread'].astype(np.float64) + f['refread']), totsc=np.where(lo > 0, hi / np.maximum(lo, 1).astype(np.float64), 0.0),
                    onehap=(lo == 0) & (hi != 0), diff=np.abs(a2 - a1), svread=f['svread'].astype(np.float64),
                    refread=f['refread'].astype(np.float64), hap0=f['hap0'].astype(np.float64))


def leaves(d, v):
    """The leaf of every candidate under vector v (include/duet_ef.h, "Leaf census")."""
    sv = d['sv']
    gate = ((d['hr'] <= v[7]) & (d['diff'] <= v[8])) | (d['hr'] > v[7])
    c0 = np.where((sv == 1.0) & (d['svread'] >= v[0]), 0, 1)
    c2 = np.where(~(sv >= v[1]), 2, np.where(d['diff'] <= v[2], np.where(d['svread'] >= v[3], 3, 4), np.where(d['hap0'] >= v[4], 5, 6)))
    one = np.where(sv <= v[5], 7, np.where(sv <= v[6], np.where(gate, 8, 9), np.where(gate, 10, 11)))
    two = np.where(sv <= v[9], 12, np.where(sv <= v[10], np.where(d['refread'] > v[11], 13, 14),
                                            np.where(sv <= v[12], np.where(d['totsc'] <= v[13], 15, 16), 17)))
    return np.where(d['cls'] == 0, c0, np.where(d['cls'] == 2, c2, np.where(d['onehap'], one, two)))


def on_host(vecs, pred, h_feat, fl, grp, pr):
    """Leaves, labels and numpy.bincount per field from what came down -> LEAF_COUNTS_DTYPE[K, 1, 18]"""
    K = len(vecs)
    out = np.zeros((K, 1, _lib.N_LEAVES), dtype=_lib.LEAF_COUNTS_DTYPE)
    el = h_feat['eligible'] != 0
    d = derived(h_feat)
    fl = fl.astype(np.int64)
    listed, hit0 = el & ((fl & IN) != 0), el & ((fl & (IN | MATCHED)) == (IN | MATCHED))
    for k in range(K):
        leaf, p = leaves(d, vecs[k]), pred[k].astype(np.int64)
        call = listed & (p != 0)
        hit = call & hit0
        b = (fl >> (3 * np.maximum(p - 1, 0))) & 7
        same, flip = hit & ((b & 2) != 0), hit & ((b & 4) != 0)
        sc, fc = np.bincount(grp[same], minlength=G), np.bincount(grp[flip], minlength=G)
        sb = np.bincount(pair_group[np.unique(pr[same])], minlength=G)
        fb = np.bincount(pair_group[np.unique(pr[flip])], minlength=G)
        takes_same = (sc + sb > fc + fb)[grp]
        for name, mask in (('n_cands', el), ('n_listed', listed), ('n_matched', hit0), ('n_calls', call), ('call_tp', hit),
                           ('call_gt', hit & ((b & 1) != 0)), ('call_hp', np.where(takes_same, same, flip)),
                           ('n_raise', call & ((fl & RAISES) != 0))):
            out[name][k, 0] = np.bincount(leaf[mask], minlength=_lib.N_LEAVES)
    return out


lines = []
for K in (1, 256, 4096):
    vecs = np.repeat(tune.vector()[None, :], K, axis=0)
    vecs[:, 1] = np.linspace(0.5, 0.9, K)
    vecs[:, 12] = np.linspace(0.6, 0.9, K)[::-1]
    d_vec = t(vecs)
    c_plain = torch.zeros(K * item, dtype=torch.uint8, device=dev)
    c_scratch = torch.zeros(K * item, dtype=torch.uint8, device=dev)
    c_leaf = torch.zeros(K * leaf_item, dtype=torch.uint8, device=dev)
    d_pred = torch.zeros(K * C, dtype=torch.uint8, device=dev)
    got = {}

    def plain():
        ctx.sweep_device(d_feat.data_ptr(), C, d_vec.data_ptr(), K, truth, c_plain.data_ptr(), stream.cuda_stream)
        torch.cuda.synchronize()

    def census():
        ctx.leaf_census_device(d_feat.data_ptr(), C, d_vec.data_ptr(), K, truth, None, c_leaf.data_ptr(), stream.cuda_stream)
        torch.cuda.synchronize()

    def host_way():
        rc = ctx.lib.duet_tune_sweep_device(ctx.handle, d_feat.data_ptr(), C, d_vec.data_ptr(), K, truth, c_scratch.data_ptr(),
                                            d_pred.data_ptr(), None, stream.cuda_stream)
        assert rc == 0, ctx.last_error()
        pred = d_pred.cpu().numpy().reshape(K, C)
        h_feat = d_feat.cpu().numpy().view(_lib.FEATURE_DTYPE)
        fl = keep['cand_flags'].cpu().numpy().view(np.uint16)
        grp, pr = keep['cand_group'].cpu().numpy().view(np.uint32), keep['cand_pair'].cpu().numpy().view(np.uint32)
        got['host'] = on_host(vecs, pred, h_feat, fl, grp, pr)

    variants = [('plain', plain, rounds), ('census', census, rounds), ('host_way', host_way, rounds if K < 4096 else min(rounds, host_rounds_big))]
    for _, run, _ in variants:                                                 # warm-up, and the results against each other
        run()
    whole = c_plain.cpu().numpy().view(_lib.COUNTS_DTYPE)
    leaf = c_leaf.cpu().numpy().view(_lib.LEAF_COUNTS_DTYPE).reshape(K, 1, _lib.N_LEAVES)
    for name in _lib.LEAF_COUNTS_NAMES:
        assert np.array_equal(leaf[name], got['host'][name]), (K, name)
    for name in ('n_calls', 'call_tp', 'call_gt', 'call_hp', 'n_raise'):
        assert np.array_equal(leaf[name].sum(axis=(1, 2)), whole[name]), (K, name)
    assert int(whole['call_hp'].max()) > 1000
    ms = {i: [] for i in range(len(variants))}
    for r in range(rounds):
        for i, (_, run, n) in enumerate(variants):
            if r >= n:
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            ms[i].append((time.perf_counter() - t0) * 1e3)
    for i, (what, _, n) in enumerate(variants):
        lines.append(dict(K=K, C=C, marks=soa.n_marks, eligible=int(elig.sum()), variant=what, rounds=n, ms_median=round(float(np.median(ms[i])), 4),
                          ms_min=round(min(ms[i]), 4), ms_max=round(max(ms[i]), 4), groups=G, truth_ids=n_uid, pairs=n_pairs,
                          leaves_reached=int((leaf['n_cands'].sum(axis=(0, 1)) > 0).sum())))
        print(json.dumps(lines[-1]), flush=True)
ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'a') as f:
    for ln in lines:
        f.write(json.dumps(ln) + '\n')
med = {(ln['K'], ln['variant']): ln['ms_median'] for ln in lines}
print('| K | plain sweep ms | census ms | census / plain | host way ms | host way / census |')
print('|---|---|---|---|---|---|')
for K in (1, 256, 4096):
    p, c, h = med[(K, 'plain')], med[(K, 'census')], med[(K, 'host_way')]
    print('| %d | %.3f | %.3f | %.2f | %.1f | %.1f |' % (K, p, c, c / p, h, h / c))
