# coding=utf-8
"""TEST INFRASTRUCTURE ONLY -- what stage A0's host driver DECIDES for an input, not what its kernels compute: a transcription of
the driver's plan function (cl_plan, csrc/duet_cluster_plan.h) and of rule 2 of oracle/cluster_oracle.c (the partitions), in numpy.
It is used for one thing: to show that a named case of tests/cluster_cases.py sits on the edge it is named for
(tests/test_cluster_case_edges.py).  Expected results never come from here: they come from the oracle.  The plan is not taken on
trust: tests/test_cluster_plan_host.py compiles cl_plan itself (tools/cluster_plan_check.hip) and holds plan_from_counts to it, field
for field, on every named case and on a grid of sizes, key widths and debug words."""
import numpy as np

# include/duet_ef.h
EXACT, LARGE, PAIRS, NOBOX, KC2, TIERS, SMALLCAP, LSD = 0x100, 0x200, 0x400, 0x800, 0x1000, 0x2000, 0x4000, 0x8000
KEYSORT, NOSYM, RECSORT, EVENT_FORKS, WIDE_OFF = 0x10000, 0x20000, 0x40000, 0x4000000, 0x8000000

# csrc/duet_prims.hip.h, csrc/duet_recsort.hip.h, csrc/duet_cluster.hip
SCAN_TILE, SELF_SPINE, SHARDS = 2048, 2048, 64
RS_TILE, RS_MAX_W, RS_SMALL_TILES, RS_CHUNK = 4096, 11, 1024, 16
BOX_THREADS, BOX_HALO = 256, 128
Q_ONE, K_FAR = 1 << 26, 1 << 38


def bits_for(v):
    return max(1, int(v).bit_length())


def centres(marks):
    return marks['pos'].astype(np.int64) + marks['span'].astype(np.int64) // 2


def bit_counts(marks, hints=True):
    """-> (centre_bits, type_bits, contig_bits, hinted): hints as _lib.fill_cluster_problem sets them (without them, or with
    max_pos_hint == 0, the bit counts come from the true maxima, as cl_maxima measures them)."""
    max_pos, max_span = int(marks['pos'].max()), max(int(marks['span'].max()), 1)
    hinted = bool(hints) and max_pos != 0                 # (the other three hints are never 0)
    centre_bits = bits_for(max_pos + max_span // 2) if hinted else bits_for(int(centres(marks).max()))
    return centre_bits, bits_for(int(marks['type'].max())), bits_for(int(marks['contig'].max())), hinted


def plan(marks, dbg=0, hints=True, part_max=100):
    """duet_cluster_run's switches for these marks under debug word dbg"""
    M = len(marks['pos'])
    assert M > 0
    centre_bits, type_bits, contig_bits, hinted = bit_counts(marks, hints)
    return dict(plan_from_counts(M, centre_bits, type_bits, contig_bits, dbg, part_max), hinted=hinted)


def plan_from_counts(M, centre_bits, type_bits, contig_bits, dbg=0, part_max=100):
    """cl_plan (csrc/duet_cluster_plan.h) for M marks whose keys have these widths"""
    key_bits = centre_bits + type_bits + contig_bits
    assert key_bits <= 64
    idx_bits = bits_for(M - 1)
    idx_packed = key_bits + idx_bits <= 64 and not dbg & PAIRS
    rec_mode = (contig_bits + type_bits + idx_bits <= 32 and (M >= 1250000 or bool(dbg & (RECSORT | LARGE)))
                and not dbg & (PAIRS | LSD | KEYSORT))
    T, rs_lo, rs_np, rs_w = 0, 0, 0, []
    if rec_mode:
        T = min(max(bits_for(M >> 4), 8), key_bits)
        if key_bits - T > 31:
            T = key_bits - 31
        rs_lo = key_bits - T
        rs_np = (T + RS_MAX_W - 1) // RS_MAX_W
        rs_w = [T // rs_np + (1 if i < T % rs_np else 0) for i in range(rs_np)]
    nb_rs = (M + RS_TILE - 1) // RS_TILE
    rs_chunks = (nb_rs + RS_CHUNK - 1) // RS_CHUNK
    big_sort = bool(dbg & LARGE)
    rs_small = nb_rs <= RS_SMALL_TILES and not big_sort
    small_in = M <= (4 << 20) and not dbg & LARGE
    top_bits = 16 if M <= (2 << 20) else 24
    hybrid = (not rec_mode and idx_packed and (key_bits + 7) // 8 >= top_bits // 8 + 2 and key_bits - top_bits < 32
              and not dbg & LSD)
    top_shift = key_bits - top_bits if hybrid else 0
    nb_sc = (M + SCAN_TILE - 1) // SCAN_TILE
    use_spine = nb_sc > SELF_SPINE or big_sort
    box_applies = rec_mode and (not small_in or big_sort) and use_spine
    tiers = not small_in or bool(dbg & TIERS)
    return dict(centre_bits=centre_bits, type_bits=type_bits, contig_bits=contig_bits, key_bits=key_bits, idx_bits=idx_bits,
                idx_packed=bool(idx_packed), rec_mode=bool(rec_mode), T=T, rs_lo=rs_lo, rs_np=rs_np, rs_w=rs_w, nb_rs=nb_rs,
                rs_small=rs_small, rs_chunks=rs_chunks, small_in=bool(small_in), top_bits=top_bits, hybrid=bool(hybrid),
                top_shift=top_shift, nb_sc=nb_sc, use_spine=use_spine, box_applies=bool(box_applies),
                tps=(nb_sc + SHARDS - 1) // SHARDS, tiers=tiers,
                wide=not tiers and M <= (2 << 20) and not dbg & WIDE_OFF, cap100=part_max <= 100)


def partitions(marks, part_gap=1000, part_max=100):
    """Rule 2: -> dict(order: the marks in sorted order (stable by contig, type, centre), heads: the sorted positions that start a
    natural partition, natural: the natural partitions' sizes, starts / sizes: every partition's first sorted position and number
    of marks, tile: the scan tile each partition starts in)."""
    M = len(marks['pos'])
    c = centres(marks)
    order = np.lexsort((np.arange(M), c, marks['type'].astype(np.int64), marks['contig'].astype(np.int64)))
    sc, st, sk = c[order], marks['type'][order].astype(np.int64), marks['contig'][order].astype(np.int64)
    head = np.ones(M, dtype=bool)
    head[1:] = (sk[1:] != sk[:-1]) | (st[1:] != st[:-1]) | (sc[1:] - sc[:-1] > int(part_gap))
    heads = np.nonzero(head)[0]
    natural = np.diff(np.append(heads, M))
    starts = np.concatenate([h + np.arange(0, n, int(part_max)) for h, n in zip(heads, natural)])
    sizes = np.diff(np.append(starts, M))
    # (a partition never runs over the next natural start)
    assert np.all(sizes <= part_max) and sizes.sum() == M
    return dict(order=order, heads=heads, natural=natural, starts=starts, sizes=sizes, tile=starts // SCAN_TILE)


def partition_rows(marks, parts, j):
    """(pos, span) of partition j's marks, in sorted order, as int64"""
    idx = parts['order'][parts['starts'][j]:parts['starts'][j] + parts['sizes'][j]]
    return marks['pos'][idx].astype(np.int64), marks['span'][idx].astype(np.int64)


def ends_wrap(pos, span):
    """cl_box's `bad`: some end position does not fit 32 bits"""
    return bool(np.any(pos + span >= 1 << 32))


def box_value(pos, span, normalizer=900.0, wrapped=False):
    """cl_box's bounding-box expression of one partition, in binary64:
        min(range of pos, range of end, range of centre) / normalizer + (max span - min span) / max(max span, 1).
    wrapped: ends and centres in 32-bit arithmetic, as the kernel holds them (what it would see without `bad`)."""
    pos, span = np.asarray(pos, dtype=np.int64), np.asarray(span, dtype=np.int64)
    end, centre = pos + span, pos + span // 2
    if wrapped:
        end, centre = end & 0xFFFFFFFF, centre & 0xFFFFFFFF
    r = min(int(pos.max() - pos.min()), int(end.max() - end.min()), int(centre.max() - centre.min()))
    return float(r) * (1.0 / float(normalizer)) + float(span.max() - span.min()) / float(max(int(span.max()), 1))


def box_outcomes(marks, parts, max_dist=0.9, normalizer=900.0):
    """per partition: 'one' (a single mark, or the box value is at most HALF the threshold: cl_box finishes it, or would but for
    its size), 'open' (at least TWICE the threshold, or an end that does not fit 32 bits: it goes on a work list), or
    'undecided' -- the binary32 evaluation and its 1e-5 guard band could go either way, and no case may depend on that."""
    out = []
    for j in range(len(parts['starts'])):
        pos, span = partition_rows(marks, parts, j)
        if len(pos) < 2:
            out.append('one')
            continue
        v = box_value(pos, span, normalizer)
        out.append('open' if ends_wrap(pos, span) or v >= 2.0 * max_dist else ('one' if v <= 0.5 * max_dist else 'undecided'))
    return np.array(out)


def size_class(n):
    return 0 if n <= 8 else 1 if n <= 16 else 2 if n <= 32 else 3 if n <= 64 else 4
