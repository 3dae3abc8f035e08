# coding=utf-8
"""CPU statement of the fused SVIM-mode pipeline's contract (include/duet_ef.h: duet_svim_phase_device): the C cluster
oracle -> the adapter rules (support, reference reads, GT, contig offsets) restated in numpy -> the C E/F oracle.  The one
reference of tests/test_gpu_fused.py, tests/test_gpu_fused_edges.py, tests/test_svim_multi.py and
tests/test_svim_fuzz_cases.py.

`variant` swaps ONE adapter rule for a natural mistake, so that a test can show on the CPU that its input tells the two
apart (tests/test_svim_fuzz_cases.py); None is the contract."""
import numpy as np

from duet_amd import engine
from oracle import c_oracle

VARIANTS = ('no_clamp',        # the depth bin of a POS beyond the contig's last bin is not clamped to it (it reads on)
            'refread_wrap',    # refread = depth - support without the floor at 0 (wraps modulo 2^32)
            'ctg_off_le',      # contig k's first candidate = the first one whose contig is > k (`<=` in the search)
            'round_mean',      # POS / SVLEN = rounded mean of the members instead of the floor mean
            'dedup_support')   # support = distinct reads among the members instead of member marks


def member_means(cl, marks, rounded):
    """floor (or rounded) mean of the members' pos and span per candidate, from the cluster order"""
    off = cl['cand_off'].astype(np.int64)
    n = np.diff(off)
    out = []
    for key in ('pos', 'span'):
        v = np.asarray(marks[key]).astype(np.int64)[cl['order']]
        s = np.add.reduceat(v, off[:-1]) if len(n) else np.zeros(0, dtype=np.int64)
        out.append((s + (n // 2 if rounded else 0)) // np.maximum(n, 1))
    return out


def adapt(cl, marks, read_tag, depth, depth_off, depth_bin, variant=None):
    """cluster result -> (EfSoA, support, refread, ctg_off, depth at POS): what duet_svim_phase_device derives per candidate."""
    assert variant is None or variant in VARIANTS, variant
    K = len(depth_off) - 1
    N = len(cl['cand_pos'])
    off = cl['cand_off'].astype(np.int64)
    support = np.diff(off)
    k = cl['cand_contig'].astype(np.int64)
    depth = np.asarray(depth)
    depth_off = np.asarray(depth_off).astype(np.int64)
    mark_read = np.asarray(marks['read'], dtype=np.uint32)[cl['order']]
    pos, span = cl['cand_pos'].astype(np.int64), cl['cand_span'].astype(np.int64)
    if variant == 'round_mean':
        pos, span = member_means(cl, marks, True)
    if variant == 'dedup_support' and N:
        key = np.repeat(np.arange(N, dtype=np.int64), support) << 32 | mark_read.astype(np.int64)
        support = np.bincount((np.unique(key) >> 32), minlength=N).astype(np.int64)
    nb = np.diff(depth_off)[k]
    bins = pos // int(depth_bin)
    if variant != 'no_clamp':
        bins = np.minimum(bins, np.maximum(nb - 1, 0))
    at = np.minimum(depth_off[k] + bins, max(len(depth) - 1, 0))
    d = np.where(nb > 0, depth[at] if len(depth) else 0, 0).astype(np.int64)
    refread = (d - support) % (1 << 32) if variant == 'refread_wrap' else np.maximum(d - support, 0)
    ctg_off = np.searchsorted(k, np.arange(K + 1))
    soa = engine.EfSoA(cand_ctg_off=ctg_off, read_tag=read_tag, cand_pos=pos, cand_svlen=span, cand_svread=support,
                       cand_refread=refread, cand_gt_ok=np.ones(N, dtype=np.uint8), cand_off=off, mark_read=mark_read)
    if variant == 'ctg_off_le':                 # (behind EfSoA's validation, as the device would take it: the first occupied contig's
        ctg_off = np.searchsorted(k, np.arange(K + 1), side='right')          # candidates then belong to no contig at all)
        ctg_off[K] = N
        soa.cand_ctg_off = np.ascontiguousarray(ctg_off, dtype=np.uint32)
    return soa, support, refread, ctg_off, d


def fused(marks, read_tag, depth, depth_off, depth_bin, svlen_thres, suppread_thres, max_dist=0.9, part_gap=1000,
          part_max=100, normalizer=900.0, variant=None):
    """marks: dict(contig, type, pos, span, read); the contig count is len(depth_off) - 1.
    -> dict(rc = the E/F oracle's status, the cluster oracle's fields, support, refread, ctg_off, depth_at, pred, ps); with a variant
    that moves them, cand_pos / cand_span are the variant's."""
    cl = c_oracle.cluster(marks['contig'], marks['type'], marks['pos'], marks['span'], max_dist=max_dist, part_gap=part_gap,
                          part_max=part_max, normalizer=normalizer)
    soa, support, refread, ctg_off, d = adapt(cl, marks, read_tag, depth, depth_off, depth_bin, variant)
    rc, pred, ps = c_oracle.ef(soa, svlen_thres, suppread_thres)
    out = dict(cl, rc=rc, support=support, refread=refread, ctg_off=ctg_off, depth_at=d, pred=pred, ps=ps)
    out['cand_pos'], out['cand_span'] = soa.cand_pos, soa.cand_svlen
    return out
