#!/usr/bin/env python3
"""GPU-side: what scoring the threshold sweep per stratum costs (duet_tune_sweep_strata_device, duet_amd/csrc/duet_tune.hip) at
tools/prof_sweep.py's workload -- synth.bench_genome(1e6): ~1 M marks, ~1e5 candidates on 24 contigs, every eligible candidate a
call, three in four matched, two candidates per truth id inside a contig, the phase-set groups of the candidates' own (contig,
PS) -- for K = 256 and K = 4096 vectors:

    plain          duet_tune_sweep_device with the truth set (one record per vector)
    strata S=2     one stratified pass, the last three contigs against the rest
    strata S=25    one stratified pass, a stratum per contig (and an empty 25th)
    masked x25     the way without the stratified kernels: 25 plain sweeps, each on a flag array with DUET_TUNE_IN_CALLS cleared
                   outside one stratum (the flag arrays are made beforehand; their making is not timed)

Everything is resident in HBM and every variant runs in this one process, interleaved: per round each variant once, HIP events
around it; the figure is the median over the rounds after one warm-up round.  The stratified counts are checked against the
masked sweeps' before anything is timed.  Prints one JSON line per (K, variant).

    python3 tools/prof_sweep_strata.py [rounds=7]
"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from duet_amd import _lib, engine, synth, tune

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
soa = engine.soa_from_synth(synth.bench_genome(1000000, 2))
ctx = _lib.Context(0)
feat = ctx.features_host(soa, 50, 2)
C = len(feat)
rng = np.random.default_rng(1)
elig = feat['eligible'] != 0
ctg = (np.searchsorted(soa.cand_ctg_off, np.arange(C), side='right') - 1).astype(np.int64)
n_ctg = int(ctg.max()) + 1
assert n_ctg == 24
gkey = ctg * (1 << 32) + feat['ps']
_, group = np.unique(gkey, return_inverse=True)
G = int(group.max()) + 1
matched = elig & (rng.random(C) < 0.75)
bits = rng.integers(0, 1 << 9, C).astype(np.uint16)
flags = (np.where(elig, _lib.TUNE_IN_CALLS, 0) | np.where(matched, _lib.TUNE_MATCHED, 0) | np.where(matched, bits, 0)).astype(np.uint16)
local = (np.arange(C) - soa.cand_ctg_off[ctg].astype(np.int64)) // 2          # two candidates per truth id, inside their contig
n_local = np.bincount(ctg, minlength=n_ctg).astype(np.int64) // 2 + 1
dev = torch.device('cuda', 0)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
stream = torch.cuda.current_stream(dev)


def layout(stratum_of_contig, S):
    """Truth arrays and strata for a partition of the contigs: the truth ids stratum-major, each range from a multiple of 32."""
    cs = stratum_of_contig[ctg]
    first = np.zeros(n_ctg + 1, dtype=np.int64)                               # where a contig's ids start inside its stratum
    n_ids = np.zeros(S, dtype=np.int64)
    for k in range(n_ctg):
        first[k] = n_ids[stratum_of_contig[k]]
        n_ids[stratum_of_contig[k]] += n_local[k]
    off = np.concatenate([[0], np.cumsum((n_ids + 31) // 32 * 32)])
    uid = (off[cs] + first[ctg] + local).astype(np.uint32)
    pairs = {}
    pair = np.zeros(C, dtype=np.uint32)
    for c in np.lexsort((uid, group)):
        if matched[c]:
            pair[c] = pairs.setdefault((int(group[c]), int(uid[c])), len(pairs))
    gpo = np.zeros(G + 1, dtype=np.int64)
    pair_uid = np.zeros(len(pairs), dtype=np.uint32)
    for (g, u), p in pairs.items():
        gpo[g + 1] += 1
        pair_uid[p] = u
    np.cumsum(gpo, out=gpo)
    gs = np.zeros(G, dtype=np.uint8)
    gs[group] = cs
    keep = dict(cand_flags=t(flags.view(np.int16)), cand_group=t(group.astype(np.uint32).view(np.int32)), cand_uid=t(uid.view(np.int32)),
                cand_pair=t(pair.view(np.int32)), group_pair_off=t(gpo.astype(np.uint32).view(np.int32)), pair_uid=t(pair_uid.view(np.int32)),
                cand_stratum=t(cs.astype(np.uint8)), group_stratum=t(gs), uid_off=off.astype(np.uint32))
    tr = _lib.TuneTruth()
    tr.n_uid, tr.n_groups, tr.n_pairs = int(off[-1]), G, len(pairs)
    for k in _lib.TRUTH_ARRAYS:
        setattr(tr, k[0], keep[k[0]].data_ptr())
    st = _lib.TuneStrata()
    st.n_strata = S
    st.cand_stratum, st.group_stratum, st.uid_off = keep['cand_stratum'].data_ptr(), keep['group_stratum'].data_ptr(), keep['uid_off'].ctypes.data
    return dict(truth=tr, strata=st, keep=keep, cs=cs, S=S, pairs=len(pairs))


two = layout(np.where(np.arange(n_ctg) >= n_ctg - 3, 1, 0), 2)
per = layout(np.arange(n_ctg), 25)
# the masked way: one flag array and one truth struct per stratum, the other arrays shared with `per`
masked = []
for s in range(25):
    f = t(np.where(per['cs'] == s, flags, flags & np.uint16(~_lib.TUNE_IN_CALLS & 0xFFFF)).astype(np.uint16).view(np.int16))
    tr = _lib.TuneTruth()
    ctypes.memmove(ctypes.byref(tr), ctypes.byref(per['truth']), ctypes.sizeof(tr))
    tr.cand_flags = f.data_ptr()
    masked.append((f, tr))
d_feat = t(feat.view(np.uint8))
item = _lib.COUNTS_DTYPE.itemsize


def host(buf, shape):
    return buf.cpu().numpy().view(_lib.COUNTS_DTYPE).reshape(shape)


for K in (256, 4096):
    vecs = np.repeat(tune.vector()[None, :], K, axis=0)
    vecs[:, 1] = np.linspace(0.5, 0.9, K)
    vecs[:, 12] = np.linspace(0.6, 0.9, K)[::-1]
    d_vec = t(vecs)
    c_plain = torch.zeros(K * item, dtype=torch.uint8, device=dev)
    c_two = torch.zeros(K * 2 * item, dtype=torch.uint8, device=dev)
    c_per = torch.zeros(K * 25 * item, dtype=torch.uint8, device=dev)
    c_masked = torch.zeros(25 * K * item, dtype=torch.uint8, device=dev)

    def plain(truth=per['truth'], counts=c_plain, at=0):
        ctx.sweep_device(d_feat.data_ptr(), C, d_vec.data_ptr(), K, truth, counts.data_ptr() + at, stream.cuda_stream)

    def strata(case, counts):
        ctx.sweep_strata_device(d_feat.data_ptr(), C, d_vec.data_ptr(), K, case['truth'], case['strata'], counts.data_ptr(), stream.cuda_stream)

    def masked_25():
        for s, (_, tr) in enumerate(masked):
            plain(tr, c_masked, s * K * item)

    variants = [('plain', 1, plain), ('strata', 2, lambda: strata(two, c_two)), ('strata', 25, lambda: strata(per, c_per)),
                ('masked_plain_sweeps', 25, masked_25)]
    for _, _, run in variants:                                                 # warm-up, and the results against each other
        run()
    torch.cuda.synchronize()
    want = host(c_masked, (25, K)).T
    got, got2, whole = host(c_per, (K, 25)), host(c_two, (K, 2)), host(c_plain, (K,))
    for name in _lib.COUNTS_NAMES:
        assert np.array_equal(got[name], want[name]), name
        assert np.array_equal(got[name].sum(axis=1), whole[name]) and np.array_equal(got2[name].sum(axis=1), whole[name]), name
    assert int(whole['base_hp'].max()) > 1000 and int((got['n_calls'].max(axis=0) > 0).sum()) == 24
    ms = {i: [] for i in range(len(variants))}
    for _ in range(rounds):
        for i, (_, _, run) in enumerate(variants):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            run()
            e1.record(stream)
            torch.cuda.synchronize()
            ms[i].append(e0.elapsed_time(e1))
    for i, (what, S, _) in enumerate(variants):
        print(json.dumps(dict(K=K, C=C, marks=soa.n_marks, eligible=int(elig.sum()), variant=what, S=S, rounds=rounds,
                              ms_median=round(float(np.median(ms[i])), 4), ms_min=round(min(ms[i]), 4), ms_max=round(max(ms[i]), 4),
                              groups=G, truth_ids=int((per if S == 25 else two)['truth'].n_uid), pairs=(per if S == 25 else two)['pairs'])),
              flush=True)
ctx.close()
