# coding=utf-8
"""Threshold sweep: score many settings of the T1-T5 tree of predict_hp (src/duet/sv_phasing_fn.py:142-183) against a truth set.

    features(home, ...)                    per-candidate features of a Duet work directory (duet_ef_features_host)
    sweep(home, truth_vcf, grid, ...)      one row per threshold vector: the 14 values and evaluation.py's ten numbers
    python -m duet_amd.tune WORKDIR TRUTH.vcf --grid GRID.json [...]

The vector's 14 fields, their order and defaults are include/duet_ef.h's duet_tune_thresholds (NAMES, DEFAULTS).  A grid is
either a list of partial vectors (dicts) or a dict of name -> list of values, expanded as a Cartesian product; names left out
take the defaults, unknown names are an error.  Values may be numbers or the strings 'nan', 'inf', '-inf'.

The truth set is prepared once on the host (prepare_truth): every candidate that can be emitted is written as the row
phased_sv.vcf would hold (write_file's format), read back through duet_amd/evaluation.parse_vcf -- so the evaluator's own rules
decide which calls it sees and with which (contig, type, pos, len, phase-set group) -- and matched once to its nearest truth
record by the evaluator's rule.  The device then applies the K vectors and counts (duet_tune_sweep_host); the ten numbers are
the evaluator's binary64 quotients of those counts.  Where upstream would raise (ZeroDivisionError: no calls, or precision +
recall == 0; IndexError: an emitted call whose (contig, type) has no truth record) the row's ten numbers are nan.
"""

import argparse
import itertools
import json
import math
import os
import sys
import tempfile

import numpy as np

from duet_amd import _lib, engine, evaluation

NAMES = _lib.TUNE_NAMES
DEFAULTS = dict(zip(NAMES, _lib.TUNE_DEFAULTS))
SCORES = ('avg_sv_num', 'call_precision', 'call_recall', 'call_f1', 'gt_precision', 'gt_recall', 'gt_f1',
          'hp_precision', 'hp_recall', 'hp_f1')
HP_TEXT = ('', '1|0', '0|1', '1|1')


def _value(name, v):
    if isinstance(v, str) and v.strip().lower() in ('nan', 'inf', '+inf', '-inf', 'infinity', '-infinity'):
        return float(v)
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError('threshold %s: %r is not a number' % (name, v))
    return float(v)


def vector(partial=None):
    """A full vector (float64[14]) from a dict of some of the names; the others take the defaults."""
    partial = partial or {}
    bad = sorted(set(partial) - set(NAMES))
    if bad:
        raise ValueError('unknown threshold name(s): %s' % ', '.join(bad))
    return np.array([_value(n, partial[n]) if n in partial else DEFAULTS[n] for n in NAMES], dtype=np.float64)


def expand_grid(grid):
    """A grid (list of partial vectors, or dict of name -> values) -> float64[K, 14]."""
    if isinstance(grid, list):
        if not all(isinstance(g, dict) for g in grid):
            raise ValueError('a grid list holds partial vectors (JSON objects)')
        vecs = [vector(g) for g in grid]
    elif isinstance(grid, dict):
        bad = sorted(set(grid) - set(NAMES))
        if bad:
            raise ValueError('unknown threshold name(s): %s' % ', '.join(bad))
        keys = list(grid)
        axes = [grid[k] if isinstance(grid[k], list) else [grid[k]] for k in keys]
        vecs = [vector(dict(zip(keys, combo))) for combo in itertools.product(*axes)]
    else:
        raise ValueError('a grid is a JSON list of partial vectors or an object of name -> values')
    if not vecs:
        raise ValueError('the grid is empty')
    return np.stack(vecs)


def load_grid(path):
    with open(path) as f:
        return expand_grid(json.load(f))


def _candidates(home, svlen_thres, suppread_thres, include_all_ctgs, thread):
    """<home> -> (EfSoA, dict of per-candidate text columns chrom / ref / alt / svtype).  Native ingest where it accepts the input,
    else the Python host path (duet_amd/sv_phasing_fn.py)."""
    from duet_amd import sv_phasing
    caller_vcf = home + '/sv_calling/variants.vcf'
    ing, chrom_list = sv_phasing.load_native(home, thread, include_all_ctgs, caller_vcf, log=False)
    if ing is not None:
        try:
            rows = ing.rows()
            if rows is not None:
                pool, off = bytes(rows['pool']), rows['str_off'].astype(np.int64)
                C = ing.soa.n_cands
                cols = [[pool[off[4 * c + i]:off[4 * c + i + 1]].decode('ascii') for c in range(C)] for i in range(4)]
                s = ing.soa                                 # (views of the native object's memory: copied before it is freed)
                soa = engine.EfSoA(read_off=s.read_off.copy(), **{n: getattr(s, n).copy() for n, _ in engine.EfSoA.FIELDS})
                return soa, dict(chrom=cols[0], ref=cols[1], alt=cols[2], svtype=cols[3])
        finally:
            ing.close()
    from duet_amd.sv_phasing_fn import generate_callinfo, read_hap_bam
    tab, soa = generate_callinfo(caller_vcf, read_hap_bam(home + '/snp_phasing/', thread, include_all_ctgs), include_all_ctgs)
    return soa, dict(chrom=list(tab.chrom), ref=list(tab.ref), alt=list(tab.alt), svtype=list(tab.svtype))


def features(home, svlen_thres=50, suppread_thres=2, include_all_ctgs=False, thread=4, ctx=None):
    """Per-candidate features of a work directory (include/duet_ef.h: duet_tune_feature), callset order.
    -> dict(feat = structured array, chrom, pos, svtype, svlen (abs), ref, alt, soa)"""
    soa, txt = _candidates(home, svlen_thres, suppread_thres, include_all_ctgs, thread)
    ctx = ctx or engine.default_context()
    feat = ctx.features_host(soa, svlen_thres, suppread_thres) if soa.n_cands else np.zeros(0, dtype=_lib.FEATURE_DTYPE)
    return dict(feat=feat, pos=soa.cand_pos.copy(), svlen=soa.cand_svlen.copy(), soa=soa, **txt)


def row_text(chrom, pos, idx, ref, alt, svlen_abs, svtype, hp, ps):
    """One data row of phased_sv.vcf (duet_amd/write_file.py; SVLEN sign rule of sv_phasing_fn.py:225)."""
    signed = svlen_abs if svtype in ('INS', 'DUP') else -svlen_abs
    return '%s\t%d\tDuet.%d\t%s\t%s\t.\tPASS\tSVLEN=%d;SVTYPE=<%s>\tHP:PS\t%s:%d\n' % (chrom, pos, idx, ref, alt, signed, svtype, hp, ps)


def prepare_truth(cands, truth_vcf, refdist=1000, pctsim=0.0, bed='', skip_phasing=False):
    """The per-candidate arrays of include/duet_ef.h's duet_tune_truth, plus n_base = len(baseinfo)."""
    feat = cands['feat']
    C = len(feat)
    elig = np.nonzero(feat['eligible'])[0]
    fd, path = tempfile.mkstemp(suffix='.vcf')
    try:
        with os.fdopen(fd, 'w') as f:
            for c in elig:
                c = int(c)
                # the call id carries the candidate's index; the HP text does not change what the parser keeps
                f.write(row_text(cands['chrom'][c], int(cands['pos'][c]), c + 1, cands['ref'][c], cands['alt'][c],
                                 int(cands['svlen'][c]), cands['svtype'][c], '1|0', int(feat['ps'][c])))
        callinfo = evaluation.parse_vcf(path, skip_phasing, bed or '')
    finally:
        os.remove(path)
    baseinfo = evaluation.parse_vcf(truth_vcf, skip_phasing, bed or '')
    flags = np.zeros(C, dtype=np.uint16)
    group = np.zeros(C, dtype=np.uint32)
    uid = np.zeros(C, dtype=np.uint32)
    pair = np.zeros(C, dtype=np.uint32)
    base_uid = {}
    for r in baseinfo:
        base_uid.setdefault(r['id'], len(base_uid))
    base = {}
    for chrom in evaluation.CHROMS:
        for svtype in ('INS', 'DEL'):
            rows = sorted((s for s in baseinfo if s['chr'] == chrom and s['type'] == svtype), key=lambda r: r['pos'])
            base[(chrom, svtype)] = (rows, np.array([r['pos'] for r in rows], dtype=np.int64),
                                     np.array([r['len'] for r in rows], dtype=np.int64))
    groups, pairs = {}, {}
    het = ('1|0', '0|1')
    for rec in callinfo:
        c = int(rec['id'][5:len(rec['id']) - len(rec['chr']) - len(str(rec['pos']))]) - 1      # id = 'Duet.<c + 1>' + CHROM + POS
        assert 0 <= c < C and feat['eligible'][c], rec['id']
        flags[c] |= _lib.TUNE_IN_CALLS
        group[c] = groups.setdefault(rec['ps'], len(groups))
        key = (rec['chr'], rec['type'])
        if key not in base:
            continue                                    # not on a scored contig, or neither INS nor DEL: never matched
        rows, bpos, blen = base[key]
        if not rows:
            flags[c] |= _lib.TUNE_RAISES
            continue
        cpos = np.array([rec['pos']], dtype=np.int64)
        clen = np.array([rec['len']], dtype=np.int64)
        j = evaluation._nearest(bpos, cpos)
        ok = (np.abs(cpos - bpos[j]) <= refdist) & (np.minimum(clen, blen[j]) / np.maximum(clen, blen[j]) >= pctsim)
        if not ok[0]:
            continue
        b = rows[int(j[0])]
        flags[c] |= _lib.TUNE_MATCHED
        uid[c] = base_uid[b['id']]
        for p in (1, 2, 3):
            ch, bh = HP_TEXT[p], b['hp']
            gt = (ch in het and bh in het) or ch == bh == '1|1'
            same = ch == bh
            flip = ch == bh == '1|1' or (ch, bh) in (('0|1', '1|0'), ('1|0', '0|1'))
            flags[c] |= (int(gt) | int(same) << 1 | int(flip) << 2) << (3 * (p - 1))
    # (group, uid) pairs, numbered group-major
    matched = np.nonzero(flags & _lib.TUNE_MATCHED)[0]
    for c in sorted(matched, key=lambda c: (int(group[c]), int(uid[c]))):
        pair[c] = pairs.setdefault((int(group[c]), int(uid[c])), len(pairs))
    G = len(groups)
    group_pair_off = np.zeros(G + 1, dtype=np.int64)
    pair_uid = np.zeros(len(pairs), dtype=np.uint32)
    for (g, u), p in pairs.items():
        group_pair_off[g + 1] += 1
        pair_uid[p] = u
    np.cumsum(group_pair_off, out=group_pair_off)
    return dict(cand_flags=flags, cand_group=group, cand_uid=uid, cand_pair=pair, group_pair_off=group_pair_off, pair_uid=pair_uid,
                n_uid=len(base_uid), n_groups=G, n_pairs=len(pairs), n_base=len(baseinfo))


def scores(counts, n_base):
    """evaluation.evaluation's ten numbers from one vector's counts (binary64, the same expressions); nan where it raises."""
    n_calls, n_groups = int(counts['n_calls']), int(counts['n_groups'])
    if int(counts['n_raise']):
        return (math.nan,) * 10
    try:
        avg = n_calls / n_groups

        def prf(tp_c, tp_b):
            p, r = tp_c / n_calls, tp_b / n_base
            return p, r, 2 * p * r / (p + r)

        return (avg,) + prf(int(counts['call_tp']), int(counts['base_tp'])) + \
            prf(int(counts['call_gt']), int(counts['base_gt'])) + prf(int(counts['call_hp']), int(counts['base_hp']))
    except ZeroDivisionError:
        return (math.nan,) * 10


def sweep(home, truth_vcf, grid, refdist=1000, pctsim=0.0, bed='', skip_phasing=False, svlen_thres=50, suppread_thres=2,
          include_all_ctgs=False, thread=4, ctx=None, cands=None):
    """-> list of rows, one per vector: dict(name -> threshold for the 14 names, score name -> value for the ten numbers).
    `grid` is a grid object (see expand_grid) or an array [K, 14]."""
    vecs = grid if isinstance(grid, np.ndarray) else expand_grid(grid)
    ctx = ctx or engine.default_context()
    if cands is None:
        cands = features(home, svlen_thres, suppread_thres, include_all_ctgs, thread, ctx=ctx)
    truth = prepare_truth(cands, truth_vcf, refdist, pctsim, bed, skip_phasing)
    counts, _, _ = ctx.sweep_host(cands['feat'], vecs, truth)
    out = []
    for v, cnt in zip(vecs, counts):
        row = dict(zip(NAMES, (float(x) for x in v)))
        row.update(zip(SCORES, scores(cnt, truth['n_base'])))
        out.append(row)
    return out


def apply(cands, thresholds, ctx=None):
    """One vector applied the way the E/F kernels decide: -> (pred u8[C], ps u32[C]), duet_ef_run_device's outputs."""
    ctx = ctx or engine.default_context()
    _, pred, ps = ctx.sweep_host(cands['feat'], np.asarray(thresholds, dtype=np.float64).reshape(1, -1), want_pred=True, want_ps=True)
    return pred[0], ps


def load_vector(path):
    """--thresholds FILE.json: one partial vector (JSON object)."""
    with open(path) as f:
        obj = json.load(f)
    if not isinstance(obj, dict):
        raise ValueError('%s: a threshold file holds one JSON object of name -> value' % path)
    return vector(obj)


def _write_tsv(path, names, rows):
    with open(path, 'w') as f:
        f.write('\t'.join(names) + '\n')
        for r in rows:
            f.write('\t'.join(repr(x) if isinstance(x, float) else str(x) for x in r) + '\n')


def parse_args(argv):
    ap = argparse.ArgumentParser(description='score many T1-T5 threshold vectors of the SV phasing decision against a truth set')
    ap.add_argument('workdir', help='Duet work directory (sv_calling/variants.vcf, snp_phasing/*.bam)')
    ap.add_argument('truthset', help='VCF of the phased truth set')
    ap.add_argument('--grid', required=True, help='JSON: a list of partial vectors, or an object of name -> list of values')
    ap.add_argument('-s', '--sv_min_size', type=int, default=50, help='minimum SV size [%(default)s]')
    ap.add_argument('-r', '--min_support_read', type=int, default=2, help='minimum number of supporting reads [%(default)s]')
    ap.add_argument('-a', '--include_all_ctgs', action='store_true', help='all contigs, not only chr{1..22,X,Y}')
    ap.add_argument('-t', '--thread', type=int, default=4, help='threads of the ingest [%(default)s]')
    ap.add_argument('--refdist', type=int, default=1000, help="the evaluator's --refdist [%(default)s]")
    ap.add_argument('--pctsim', type=float, default=0, help="the evaluator's --pctsim [%(default)s]")
    ap.add_argument('--bed_file', type=str, default='', help="the evaluator's --bed_file")
    ap.add_argument('--skip_phasing', action='store_true', help="the evaluator's --skip_phasing")
    ap.add_argument('--out', default='sweep.tsv', help='one row per vector [%(default)s]')
    ap.add_argument('--features', default='', help='also write the per-candidate features here (TSV)')
    ap.add_argument('--device', type=int, default=0, help='HIP device index [%(default)s]')
    return ap.parse_args(argv)


def main(argv):
    a = parse_args(argv)
    vecs = load_grid(a.grid)
    ctx = engine.default_context(a.device)
    cands = features(a.workdir, a.sv_min_size, a.min_support_read, a.include_all_ctgs, a.thread, ctx=ctx)
    if a.features:
        f = cands['feat']
        cols = ('chrom', 'pos', 'svtype', 'svlen') + tuple(n for n in _lib.FEATURE_DTYPE.names if not n.startswith('reserved'))
        _write_tsv(a.features, cols, ([cands['chrom'][c], int(cands['pos'][c]), cands['svtype'][c], int(cands['svlen'][c])] +
                                      [int(f[n][c]) for n in cols[4:]] for c in range(len(f))))
    rows = sweep(a.workdir, a.truthset, vecs, a.refdist, a.pctsim, a.bed_file, a.skip_phasing, ctx=ctx, cands=cands)
    _write_tsv(a.out, NAMES + SCORES, ([r[n] for n in NAMES + SCORES] for r in rows))
    best = max(range(len(rows)), key=lambda i: -1.0 if math.isnan(rows[i]['hp_f1']) else rows[i]['hp_f1'])
    print('%d vectors scored -> %s; best phasing F1 %r at vector %d' % (len(rows), a.out, rows[best]['hp_f1'], best))


if __name__ == '__main__':
    main(sys.argv[1:])
