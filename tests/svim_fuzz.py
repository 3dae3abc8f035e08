# coding=utf-8
"""Named, seeded inputs of the fused SVIM-mode pipeline built directly as arrays (no BAMs), in the manner of
tests/soa_fuzz.py: raw marks (contig, type, pos, span, read), read tags, binned depth and thresholds, with the structure
that cl_emit's lots, the E/F plan and the adapter rules turn on placed EXACTLY -- partition counts, cluster sizes, contig
layouts, depth bins, phase sets.  tests/test_svim_fuzz_cases.py checks on the CPU that every case still has the property
it is named for; tests/test_gpu_fused_edges.py runs them on the device.

The building block is the SV group: `size` marks within 20 bp and 2 bp of span of each other, groups of one contig 3000 bp
apart.  With part_gap = 1000 a group of at most part_max marks is exactly one partition, and with max_dist = 0.9 exactly one
cluster (pair distances stay below 20 / 900 + 2 / 45), so partition, cluster and candidate counts follow from the group
list.  A contig owns whole groups: marks hashed over many contigs leave every support at 1 and every pred at 0."""
import numpy as np

from duet_amd import engine, synth

ABSENT = engine.MARK_ABSENT
U32 = 0xFFFFFFFF
SPACING = 3000
_SV_EDGE = np.array([sv for sv, _ in synth._RATIO_EDGE], dtype=np.int64)
_RF_EDGE = np.array([rf for _, rf in synth._RATIO_EDGE], dtype=np.int64)


class Case(object):
    """marks / read_tag / depth / depth_off + the parameters of one run; `kw` = the clustering keywords that differ from the
    defaults; `expect` = what tests/test_svim_fuzz_cases.py asserts of the oracle's result."""

    def __init__(self, name, marks, read_tag, depth, depth_off, depth_bin=1000, svlen_thres=50, suppread_thres=2, kw=None,
                 expect=None):
        self.name, self.marks, self.read_tag, self.depth = name, marks, read_tag, depth
        self.depth_off = np.ascontiguousarray(depth_off, dtype=np.uint32)
        self.depth_bin, self.svlen_thres, self.suppread_thres = int(depth_bin), int(svlen_thres), int(suppread_thres)
        self.kw = dict(kw or {})
        self.expect = dict(expect or {})

    @property
    def M(self):
        return len(self.marks['pos'])

    @property
    def K(self):
        return len(self.depth_off) - 1


def partitions(marks, part_gap=1000, part_max=100):
    """The partition of every mark under rule 1-2 of oracle/cluster_oracle.c, restated in numpy: -> (number of partitions,
    partition id per RAW mark)."""
    M = len(marks['pos'])
    if M == 0:
        return 0, np.zeros(0, dtype=np.int64)
    centre = marks['pos'].astype(np.int64) + marks['span'].astype(np.int64) // 2
    key = (marks['contig'].astype(np.int64) << 42) | (marks['type'].astype(np.int64) << 34) | centre
    order = np.argsort(key, kind='stable')
    ks = key[order]
    cut = np.ones(M, dtype=bool)
    cut[1:] = ((ks[1:] >> 34) != (ks[:-1] >> 34)) | (ks[1:] - ks[:-1] > part_gap)
    run = np.cumsum(cut) - 1
    in_run = np.arange(M) - np.nonzero(cut)[0][run]
    head = cut | (in_run % part_max == 0)
    pid = np.cumsum(head) - 1
    out = np.zeros(M, dtype=np.int64)
    out[order] = pid
    return int(pid[-1]) + 1, out


def sizes_to(rng, M, lo=2, hi=30):
    """group sizes, half of them support counts of synth._RATIO_EDGE (so that depth = size + its reference-read count puts the
    candidate ON a T1-T5 ratio threshold), adding up to exactly M"""
    if M == 0:
        return np.zeros(0, dtype=np.int64)
    n = max(M // lo + 1, 1)
    s = np.where(rng.chance(n, 1, 2), _SV_EDGE[rng.below(n, len(_SV_EDGE))], rng.between(n, lo, hi))
    s = np.maximum(s, min(lo, M))
    G = int(np.searchsorted(np.cumsum(s), M)) + 1
    s = s[:G].copy()
    s[-1] -= int(s.sum()) - M
    return s


def n_sizes(rng, G, lo=2, hi=30):
    """G group sizes, half of them support counts of synth._RATIO_EDGE"""
    return np.maximum(np.where(rng.chance(G, 1, 2), _SV_EDGE[rng.below(G, len(_SV_EDGE))], rng.between(G, lo, hi)), lo)


def build(name, seed, g_contig, g_size, K, depth_bin=1000, reads='phased', dup=6, beyond=(), no_bins=(), part_max=100,
          pos_jit=20, span_jit=2, g_span=None, g_type=None, svlen_thres=50, suppread_thres=2, kw=None, expect=None,
          depth_rule='edge', g_slot=None, favour=False):
    """Groups (contig ascending, size) -> Case.  reads: 'phased' | 'absent' (every mark DUET_MARK_ABSENT) | 'none' (no read
    table at all); dup: one mark in `dup` takes another member's read (0: never); beyond: contigs whose bins end in front of
    the second half of their groups; no_bins: contigs without bins; depth_rule: 'edge' (ratio thresholds, support and
    support +- 1), 'max' (2^32 - 1 on every third group), 'low' (0-3: for clusters of one mark).
    g_slot: the group's place within its contig (default: its ordinal there).  Groups that share a slot share their centre and
    their type and take spans a factor of 20 apart (50, 1000, 20000 bp ...): ONE partition of several clusters, since
    |dspan| / max(span) alone is above 0.9 for every pair.  favour: half of the groups get one phase set, one haplotype and
    low PC, no absent mark and a depth of 1.1 to 3 times their support -- candidates that end as 1|0 or 0|1, for cases of few candidates."""
    rng = synth.SplitMix(0x5F1A0000 + seed)
    g_contig = np.asarray(g_contig, dtype=np.int64)
    g_size = np.asarray(g_size, dtype=np.int64)
    G = len(g_size)
    assert len(g_contig) == G and (G == 0 or (np.all(np.diff(g_contig) >= 0) and g_contig[-1] < K and g_size.min() >= 1))
    first = np.searchsorted(g_contig, g_contig)
    idx = np.arange(G) - first
    if g_span is None:
        g_span = np.where(rng.chance(G, 1, 4), rng.between(G, 45, 55), rng.between(G, 60, 3000))
    g_span = np.asarray(g_span, dtype=np.int64)
    g_type = rng.below(G, 4) if g_type is None else np.asarray(g_type, dtype=np.int64)
    shift = 0
    if g_slot is None:
        g_slot = idx
        g_pos = 4000 + g_slot * SPACING
    else:
        g_slot = np.asarray(g_slot, dtype=np.int64)
        assert len(g_slot) == G and np.all((np.diff(g_slot) >= 0) | (np.diff(g_contig) > 0))
        sub = np.arange(G) - np.searchsorted(g_contig * (1 << 32) + g_slot, g_contig * (1 << 32) + g_slot)   # ordinal in the slot
        assert G == 0 or sub.max() <= 4
        g_span = 50 * 20 ** sub + rng.between(G, 0, 10)
        g_type = g_type[np.arange(G) - sub]
        shift = 4100000                                                        # (half the widest span, so that POS stays positive)
        g_pos = 4000 + shift + g_slot * SPACING - g_span // 2
    gi = np.repeat(np.arange(G), g_size)
    M = len(gi)
    j = np.arange(M) - np.repeat(np.cumsum(g_size) - g_size, g_size)            # the mark's ordinal in its group
    pos = g_pos[gi] + rng.between(M, 0, pos_jit)
    span = g_span[gi] + rng.between(M, 0, span_jit)
    # reads: a block of `size` reads per group; 1, 2 or 3-4 phase sets per group, phase sets of 60 kb; a dominant haplotype
    # (pure on every fourth group), hap code 3 on one read in 16; PC half on the thresholds of synth._PC_EDGE
    r0 = np.cumsum(g_size) - g_size
    R = M if reads != 'none' else 0
    mode = rng.below(G, 8)                                                      # 0-4: one phase set, 5-6: two, 7: three or four
    n_ps = np.where(mode < 5, 1, np.where(mode < 7, 2, 3 + rng.below(G, 2)))
    ps_id = g_pos[gi] // 60000 + (j * n_ps[gi] // np.maximum(g_size[gi], 1))
    fav = rng.chance(G, 1, 2) if favour else np.zeros(G, dtype=bool)
    n_ps = np.where(fav, 1, n_ps)
    dom = rng.between(G, 1, 2)
    pure = rng.chance(G, 1, 4) | fav
    hap = np.where(pure[gi] | rng.chance(M, 7, 8), dom[gi], 3 - dom[gi])
    hap = np.where(rng.chance(M, 1, 16), 0, hap)                                # packs as code 3
    pc_edge = np.array(synth._PC_EDGE, dtype=np.int64)
    pc = np.where(rng.chance(M, 1, 2), pc_edge[rng.below(M, len(pc_edge))], rng.between(M, 0, 10000))
    pc = np.where(fav[gi], rng.between(M, 0, 2000), pc)
    read_tag = engine.pack_tags(hap, pc, 17 + ps_id * 60000)[:R]
    read = r0[gi] + j
    if dup and M:
        read = np.where(rng.chance(M, 1, dup), r0[gi] + rng.below(M, 1 << 30) % g_size[gi], read)
    read = np.where(rng.chance(M, 1, 10) & ~fav[gi], ABSENT, read) if M else read
    if reads != 'phased':
        read = np.full(M, ABSENT, dtype=np.int64)
    # depth: bins up to the contig's last group (beyond: up to its middle one), a background of 8-40 reads; at every group
    # support + the reference reads of a ratio edge, or support - 1 / support / support + 1
    n_g = np.bincount(g_contig, minlength=K) if G else np.zeros(K, dtype=np.int64)
    n_slot = np.zeros(K, dtype=np.int64)
    if G:
        np.maximum.at(n_slot, g_contig, g_slot + 1)
    last = 4000 + shift + np.maximum(n_slot - 1, 0) * SPACING + pos_jit
    nb = np.where(n_g > 0, last // depth_bin + 1, 0)
    for k in beyond:
        nb[k] = (4000 + (n_g[k] // 2) * SPACING - 1500) // depth_bin + 1
    for k in no_bins:
        nb[k] = 0
    depth_off = np.concatenate([[0], np.cumsum(nb)])
    depth = rng.between(int(depth_off[-1]), 8, 40)
    sel = rng.below(G, 8)
    val = np.where(sel < 4, g_size + _RF_EDGE[rng.below(G, len(_RF_EDGE))],
                   np.where(sel < 7, np.maximum(g_size + sel - 5, 0), g_size + rng.between(G, 0, 30)))
    if depth_rule == 'max':
        val = np.where(np.arange(G) % 3 == 0, U32, val)
    if depth_rule == 'low':
        val = rng.between(G, 0, 3)
    val = np.where(fav, g_size + 1 + rng.below(G, 1 << 30) % np.maximum(2 * g_size, 1) + g_size // 10, val)
    for end in (0, pos_jit):
        b = (g_pos + end) // depth_bin
        ok = b < nb[g_contig]
        depth[depth_off[g_contig][ok] + b[ok]] = val[ok]
    perm = np.argsort(rng.u64(M), kind='stable') if M else np.zeros(0, dtype=np.int64)
    marks = dict(contig=g_contig[gi][perm].astype(np.uint16), type=g_type[gi][perm].astype(np.uint8),
                 pos=pos[perm].astype(np.uint32), span=span[perm].astype(np.uint32), read=read[perm].astype(np.uint32))
    kw = dict(kw or {})
    if part_max != 100:
        kw['part_max'] = part_max
    expect = dict(expect or {})
    expect.setdefault('phasing', reads == 'phased' and M > 0 and 'exempt' not in expect)
    expect.setdefault('silent', reads != 'phased' or M == 0)
    return Case(name, marks, read_tag, depth.astype(np.uint32), depth_off, depth_bin, svlen_thres, suppread_thres, kw, expect)


def _spread(rng, G, ids):
    """G groups dealt over the contig ids `ids` (ascending), every id at least one"""
    ids = np.asarray(ids, dtype=np.int64)
    assert G >= len(ids)
    extra = np.sort(ids[rng.below(G - len(ids), len(ids))]) if G > len(ids) else np.zeros(0, dtype=np.int64)
    return np.sort(np.concatenate([ids, extra]))


def _parts(P):
    """exactly P partitions, on three contigs when there is room: P slots of four clusters each (at most 80 marks a slot), so that
    P = 63, 64, 65 still carry some 250 candidates.  P = 1 cannot hold 20 candidates of each prediction (at most part_max marks):
    exempt, it asserts a non-zero prediction."""
    def make(seed):
        rng = synth.SplitMix(900 + seed)
        K = 3 if P >= 3 else 1
        slot_contig = _spread(rng, P, np.arange(K))
        slot = np.arange(P) - np.searchsorted(slot_contig, slot_contig)
        e = dict(n_parts=P, n_cands=4 * P)
        if P == 1:
            e.update(exempt='one partition holds at most part_max marks', some=True)
        return build('parts_%d' % P, seed, np.repeat(slot_contig, 4), n_sizes(rng, 4 * P, 2, 20), K, g_slot=np.repeat(slot, 4),
                     favour=True, expect=e)
    return make


def _sized(M):
    """exactly M marks.  Up to 65 marks there are fewer than 60 candidates of two marks or more: exempt from the 20 candidates
    of each prediction; M = 63, 64, 65 assert a non-zero prediction, M = 1, 2 only their size."""
    def make(seed):
        rng = synth.SplitMix(1700 + seed)
        s = sizes_to(rng, M, 2, 10)
        K = 2 if len(s) >= 2 else 1
        e = dict(n_marks=M)
        if 0 < M <= 65:
            e.update(exempt='fewer than 60 candidates of two marks', some=M >= 63)
        return build('marks_%d' % M, seed, _spread(rng, len(s), np.arange(K)) if len(s) else [], s, K,
                     suppread_thres=1 if M == 1 else 2, favour=True, expect=e)
    return make


def _layout(name, K, ids_of, G, **extra):
    """G groups over the contig ids ids_of(rng) out of K"""
    def make(seed):
        rng = synth.SplitMix(2600 + seed)
        ids = np.asarray(ids_of(rng), dtype=np.int64)
        e = dict(dict(occupied=len(ids), K=K), **extra.get('expect', {}))
        return build(name, seed, _spread(rng, G, ids), n_sizes(rng, G), K, expect=e,
                     **{k: v for k, v in extra.items() if k != 'expect'})
    return make


def _opening(seed):
    """contig 1 opens at candidate 128 (index = 0 mod 64), contig 2 at 191 (= 63 mod 64), contig 4 at 192 with ONE candidate,
    then ordinary contigs (a group is one candidate whatever its type: only the counts per contig matter)"""
    rng = synth.SplitMix(3100 + seed)
    per = [128, 63, 1, 0, 1, 64, 300, 1, 1, 250]
    g_contig = np.repeat(np.arange(len(per)), per)
    s = n_sizes(rng, len(g_contig))
    return build('contig_opens_at_0_and_63', seed, g_contig, s, len(per) + 2,
                 expect=dict(opens=(0, 63), single=4, n_cands=len(g_contig)))


def _cluster_sizes(part_max, sizes):
    """the named sizes between ordinary groups, and 40 more groups of those sizes (400 of them under suppread_thres = 128, where
    nothing smaller passes the filter) so that clusters of 63 marks and more end with every prediction"""
    def make(seed):
        rng = synth.SplitMix(3700 + seed + part_max)
        base = np.minimum(sizes_to(rng, 6000), part_max)
        more = np.resize(np.asarray(sizes), 40) if part_max != 128 else np.full(400, 128)
        s = np.concatenate([base[:200], np.asarray(sizes), base[200:], more])
        at = np.arange(len(s))
        g_contig = np.minimum(at * 3 // len(s), 2)
        return build('cluster_sizes_pm%d' % part_max, seed, g_contig, s, 3, part_max=part_max,
                     suppread_thres=128 if part_max == 128 else 2, favour=True,
                     expect=dict(supports=[x for x in sizes if x <= part_max], part_max=part_max))
    return make


def _dense(seed):
    """max_dist = 0: only identical marks merge, so a partition of n distinct marks gives n clusters -- 64 partitions of 12-30
    marks put about a thousand clusters into one lot of cl_emit"""
    rng = synth.SplitMix(4100 + seed)
    s = rng.between(700, 12, 30)
    return build('dense_lots', seed, _spread(rng, 700, np.arange(3)), s, 3, pos_jit=400, span_jit=40, kw=dict(max_dist=0.0),
                 suppread_thres=1, depth_rule='low', expect=dict(lot_over=64))


def _depth(name, **kw):
    def make(seed):
        rng = synth.SplitMix(4500 + seed)
        k2 = dict(kw)
        s = n_sizes(rng, 1600, k2.pop('lo', 2))
        return build(name, seed, _spread(rng, len(s), np.arange(4)), s, 4, **k2)
    return make


def _svlen(delta):
    """a third of the groups share the span 500 (+ 0-2 bp per mark): floor means of 500 and 501; svlen_thres = 501 + delta"""
    def make(seed):
        rng = synth.SplitMix(5200 + seed)
        s = n_sizes(rng, 1600)
        span = np.where(np.arange(len(s)) % 3 == 0, 500, rng.between(len(s), 60, 3000))
        return build('svlen_thres_on_a_mean_%+d' % delta, seed, _spread(rng, len(s), np.arange(2)), s, 2, g_span=span,
                     svlen_thres=501 + delta, expect=dict(span_at=501))
    return make


def _big(seed):
    """about 1.5 M marks: the record sort is the default from 1.25 M on"""
    rng = synth.SplitMix(6000 + seed)
    s = sizes_to(rng, 1500000)
    return build('one_and_a_half_million_marks', seed, _spread(rng, len(s), np.arange(24)), s, 24,
                 expect=dict(min_marks=1250000))


def _many_contigs(seed):
    """K = 65535: a third of the contigs own one group, some own several, the rest (in front, behind, in runs) none"""
    rng = synth.SplitMix(6400 + seed)
    ids = np.unique(np.concatenate([rng.below(21000, 65535 - 40) + 20, [65534 - 12]]))
    G = len(ids) + 3000
    s = n_sizes(rng, G, 2, 14)
    return build('contigs_65535', seed, _spread(rng, len(s), ids), s, 65535,
                 expect=dict(K=65535, occupied=len(ids), singles=True))


CASES = dict([('parts_%d' % P, _parts(P)) for P in (1, 63, 64, 65, 2047, 2048, 2049, 4097)] +
             [('marks_%d' % M, _sized(M)) for M in (0, 1, 2, 63, 64, 65, 4095, 4096, 4097)])
CASES.update({
    'dense_lots': _dense,
    'cluster_sizes_pm100': _cluster_sizes(100, [63, 64, 65, 100, 100, 99]),
    'cluster_sizes_pm128': _cluster_sizes(128, [63, 64, 65, 128, 127, 128]),
    'cluster_sizes_pm37': _cluster_sizes(37, [37, 36, 37, 74]),
    'contigs_1': _layout('contigs_1', 1, lambda r: [0], 600),
    'contigs_2': _layout('contigs_2', 2, lambda r: [0, 1], 600),
    'contigs_64': _layout('contigs_64', 64, lambda r: np.arange(64), 900),
    'contigs_65': _layout('contigs_65', 65, lambda r: np.arange(65), 900),
    'contigs_700': _layout('contigs_700', 700, lambda r: np.arange(700), 2000, expect=dict(singles=True)),
    'contigs_65535': _many_contigs,
    # ids 3.. in front empty; runs of two and three empty ones between; four behind
    'empty_contigs_around': _layout('empty_contigs_around', 40, lambda r: [3, 4, 7, 11, 12, 13, 17, 20, 21, 25, 30, 35], 700,
                                    expect=dict(empty_front=3, empty_behind=4, empty_run=2)),
    'contig_opens_at_0_and_63': _opening,
    'contigs_without_bins': _depth('contigs_without_bins', no_bins=(1, 3), expect=dict(no_bins=(1, 3))),
    'beyond_the_last_bin': _depth('beyond_the_last_bin', beyond=(0, 2), expect=dict(beyond=10)),
    'depth_bin_1': _depth('depth_bin_1', depth_bin=1, pos_jit=0),
    'depth_bin_max': _depth('depth_bin_max', depth_bin=U32),
    'depth_max': _depth('depth_max', depth_rule='max', expect=dict(depth_max=True)),
    'all_marks_absent': _depth('all_marks_absent', reads='absent'),
    'no_reads': _depth('no_reads', reads='none'),
    'repeated_reads': _depth('repeated_reads', dup=2, expect=dict(dup=True)),
    'suppread_thres_1': _depth('suppread_thres_1', suppread_thres=1, lo=1),
    # groups spread over 700 bp under part_gap = 100 and normalizer = 300: both cut them up, unlike the defaults
    'part_gap_100_normalizer_300': _depth('part_gap_100_normalizer_300', pos_jit=700, kw=dict(part_gap=100, normalizer=300.0),
                                          expect=dict(not_the_defaults=True)),
    'svlen_thres_on_a_mean_-1': _svlen(-1),
    'svlen_thres_on_a_mean_+0': _svlen(0),
    'svlen_thres_on_a_mean_+1': _svlen(1),
    'one_and_a_half_million_marks': _big,
})
NAMES = tuple(CASES)
SEEDS = {n: 11 + 7 * i for i, n in enumerate(NAMES)}
_made = {}


def validate(c):
    """what the device entries have to trust (include/duet_ef.h): checked here, before anything reaches a kernel"""
    m, K = c.marks, c.K
    M = c.M
    assert all(len(m[f]) == M for f in ('contig', 'type', 'pos', 'span', 'read'))
    assert 1 <= K <= 65535 and c.depth_bin >= 1 and 1 <= c.kw.get('part_max', 100) <= 128
    off = c.depth_off.astype(np.int64)
    assert off[0] == 0 and np.all(np.diff(off) >= 0) and off[-1] == len(c.depth)
    if M:
        assert int(m['contig'].max()) < K and int(m['type'].max()) <= 3
        live = m['read'][m['read'] != ABSENT]
        assert live.size == 0 or int(live.max()) < len(c.read_tag)


def case(name):
    """the named case (built once per process)"""
    if name not in _made:
        c = CASES[name](SEEDS[name])
        assert c.name == name, (c.name, name)
        validate(c)
        _made[name] = c
    return _made[name]
