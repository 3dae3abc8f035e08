# coding=utf-8
"""Threshold sweep: score many settings of the T1-T5 tree of predict_hp (src/duet/sv_phasing_fn.py:142-183) against a truth set.

    features(home, ...)                    per-candidate features of a Duet work directory (duet_ef_features_host)
    sweep(home, truth_vcf, grid, ...)      one row per threshold vector: the 14 values and evaluation.py's ten numbers
    sweep_settings(home, truth_vcf, grid, svlen_thres=(..), suppread_thres=(..), cluster_max_distance=(..), from_bams=..)
                                           the same for every setting of -s, -r and (svim-gpu mode, from the BAMs) -c
    strata_by_contig(), strata_holdout(texts)   strata (sets of CHROM texts) for sweep_settings(holdout=.., by_contig=..): every
                                           vector scored per stratum in one pass over the candidates (duet_tune_sweep_strata_device)
    python -m duet_amd.tune WORKDIR TRUTH.vcf --grid GRID.json [-s 30,50 -r 2,3 [--from_bams -c 0.5,0.9]] [--pc_cap 4000,8100]
                                           [--holdout chr20,chr21 --by_contig FILE.tsv] [--by_leaf FILE.tsv] [...]
    fit(home, truth_vcf, objective, ...)   coordinate descent over exact lines: per axis one vector per distinct value of the feature
                                           the axis is compared with (duet_tune_line_device), scored by the same sweep
    python -m duet_amd.tune WORKDIR TRUTH.vcf --fit hp_f1 [--start VEC.json --axes a,b --rounds N --max_values N --holdout ..]
                                           [--fit_cap] --out_vector best.json [--trace fit.tsv]
                                           --fit_cap, or the name pc_cap in --axes: the PC cap is an axis too, searched along the
                                           distinct pc values of the marks that can vote (duet_tune_cap_line_device)

The vector's 14 fields, their order and defaults are include/duet_ef.h's duet_tune_thresholds (NAMES, DEFAULTS).  A grid is
either a list of partial vectors (dicts) or a dict of name -> list of values, expanded as a Cartesian product; names left out
take the defaults, unknown names are an error.  Values may be numbers or the strings 'nan', 'inf', '-inf'.

What the evaluator's parser makes of a candidate's row does not depend on -s, -r, -c or the thresholds: it is derived once per
work directory on the host (candidate_keys, contig_tables: every candidate -- or, without per-candidate text, every (contig, type)
-- written as the row phased_sv.vcf would hold and read back through duet_amd/evaluation.parse_vcf, so the evaluator's own rules
decide which calls it sees and under which (contig, type, phase-set group)).  Per setting the device then computes the features,
matches every call to its nearest truth record by the evaluator's rule and numbers the groups and pairs
(duet_tune_truth_build_device), applies the K vectors and counts (duet_tune_sweep_device); the ten numbers are the evaluator's
binary64 quotients of those counts.  prepare_truth is the same truth match on the host, in the evaluator's own terms: the
normative text the device build is tested against.  Where upstream would raise (ZeroDivisionError: no calls, or precision +
recall == 0; IndexError: an emitted call whose (contig, type) has no truth record) the row's ten numbers are nan.

Leaves.  The tree has 18 exits (include/duet_ef.h, "Leaf census"; _lib.LEAF_NAMES).  by_leaf / --by_leaf adds one pass per setting
over the resident features (duet_tune_leaf_census_device) and one row per setting, vector, stratum and leaf: how many eligible
candidates the vector sends there, how many of them the evaluator lists and matches, and what the calls among them score -- where
the calls, the wrong genotypes and the wrong haplotypes come from.  Summed over the leaves, the counts are the plain sweep's.

Fit.  With the other 13 constants fixed, every count of a sweep is a piecewise-constant function of one constant: it changes only
where the constant crosses a value of the feature it is compared with that some candidate has.  The line of an axis -- those
distinct values and one sentinel (-inf in front for the <= and > axes, +inf behind for the >= axes) -- therefore holds every
behaviour of the axis, and the best vector on it is the exact optimum of the axis, not the best of a guessed grid.  fit() walks the
axes round by round; an axis moves only to a strictly better objective, and then to the line's lowest-index value that attains it,
so the objective never decreases, and a round without a move ends the fit.  The line is made on the device from the resident
features; only count records (and the one chosen value) come back.

Strata.  A stratum is a set of CHROM texts; the ten numbers of (vector, stratum) are what the unmodified evaluator returns when the
callset and the truth set are both restricted to the rows with those CHROM texts -- it matches, fills its id sets and groups the
phase sets inside `for ch in range(24)`, so restricting the rows is all it takes, and a stratum is nan exactly where the restricted
evaluator would raise.  A truth id is the text ID + CHROM + POS, which rows of two contigs can share: truth_side(strata=..) numbers
the ids per (stratum, id text), so that such an id counts once in a stratum that holds both rows and once in each otherwise.

Voted runs.  --vote_sv_tags scores the second run of duet --vote_sv_tags for every vector of a grid, each on the tags derived from
its OWN first-run het calls: per setting one plan over the eligible candidates (duet_sv_tags_plan_device),
per vector one apply (duet_sv_tags_apply_device), the features call on the problem pointed at the words, and that vector swept
alone over its own records.  --sv_tag_min and --sv_tag_pc are the innermost settings; not with --fit or --join_ps.
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


def strata_by_contig():
    """One stratum per scored contig (evaluation.CHROMS) and `other` for any CHROM text the parser keeps that is none of them."""
    return dict(names=tuple(evaluation.CHROMS) + ('other',), index={c: i for i, c in enumerate(evaluation.CHROMS)}, default=len(evaluation.CHROMS))


def strata_holdout(texts):
    """`test`: the listed CHROM texts; `train`: every other text."""
    texts = [str(t) for t in texts]
    if not texts or not all(texts):
        raise ValueError('holdout: a non-empty list of CHROM texts, not %r' % (texts,))
    return dict(names=('train', 'test'), index=dict.fromkeys(texts, 1), default=0)


def stratum_of(strata, text):
    return strata['index'].get(text, strata['default'])


def chrom_strata(texts, strata):
    """chrom_stratum u8[n_chrom] for the dense CHROM ids _dense_ids gives the same texts (equal texts share an id)."""
    return np.array([stratum_of(strata, t) for t in dict.fromkeys(texts)], dtype=np.uint8)


def truth_side(truth_vcf, bed='', skip_phasing=False, strata=None):
    """The truth set as include/duet_ef.h's duet_eval_problem carries it (evaluation.flatten), plus n_base = len(baseinfo).
    With strata: base_uid is numbered per (stratum, id text), stratum-major, stratum s owning uid_off[s] .. uid_off[s + 1] with
    every offset a multiple of 32 (n_base_uid = uid_off[S]); n_base_strata[s] = the truth records of stratum s, those outside
    every list (CHROM not 'chr' + label) included."""
    baseinfo = evaluation.parse_vcf(truth_vcf, skip_phasing, bed or '')
    if strata is not None:
        of = [stratum_of(strata, r['chr']) for r in baseinfo]
        baseinfo = [dict(r, id=(s, r['id'])) for r, s in zip(baseinfo, of)]
    a = evaluation.flatten(baseinfo, [])
    out = dict(base_off=np.asarray(a['base_off'], dtype=np.uint32), base_pos=np.asarray(a['base_pos'], dtype=np.uint32),
               base_len=np.asarray(a['base_len'], dtype=np.uint32), base_uid=np.asarray(a['base_uid'], dtype=np.uint32),
               base_hp=np.asarray(a['base_hp'], dtype=np.uint8), n_base_uid=int(a['n_base_uid']), n_base=len(baseinfo))
    if strata is not None:
        S = len(strata['names'])
        first_seen = list(dict.fromkeys(r['id'] for r in baseinfo))         # flatten's numbering: (stratum, id text) as first seen
        n_ids = np.bincount([s for s, _ in first_seen], minlength=S)
        uid_off = np.concatenate([[0], np.cumsum((n_ids + 31) // 32 * 32)]).astype(np.int64)
        if uid_off[-1] > 0xFFFFFFFF:
            raise ValueError('too many truth ids')
        nxt, renumber = uid_off[:-1].copy(), np.zeros(len(first_seen), dtype=np.uint32)
        for i, (s, _) in enumerate(first_seen):
            renumber[i] = nxt[s]
            nxt[s] += 1
        out.update(base_uid=renumber[out['base_uid']] if len(out['base_uid']) else out['base_uid'], n_base_uid=int(uid_off[-1]),
                   uid_off=uid_off.astype(np.uint32), n_base_strata=[int(x) for x in np.bincount(of, minlength=S)])
    return out


_LIST_KEY = {(c, t): 2 * k + j for k, c in enumerate(evaluation.CHROMS) for j, t in enumerate(('INS', 'DEL'))}


def _parsed_rows(rows, bed, skip_phasing):
    """rows: (chrom, pos, ref, alt, svtype) -> per row (list key | KEY_NONE | KEY_SKIP, CHROM text), through evaluation.parse_vcf.
    The row's length is written as 50 (the parser's own length test stays with the caller: cand_len >= 50), its HP as 1|0 and its
    PS as 0: none of them changes what else the parser does with the row."""
    fd, path = tempfile.mkstemp(suffix='.vcf')
    try:
        with os.fdopen(fd, 'w') as f:
            for i, (chrom, pos, ref, alt, svtype) in enumerate(rows):
                f.write(row_text(chrom, int(pos), i + 1, ref, alt, 50, svtype, '1|0', 0))
        recs = evaluation.parse_vcf(path, skip_phasing, bed or '')
    finally:
        os.remove(path)
    key = np.full(len(rows), _lib.TUNE_KEY_SKIP, dtype=np.uint32)
    for rec in recs:
        i = int(rec['id'][5:len(rec['id']) - len(rec['chr']) - len(str(rec['pos']))]) - 1       # id = 'Duet.<i + 1>' + CHROM + POS
        key[i] = _LIST_KEY.get((rec['chr'], rec['type']), _lib.TUNE_KEY_NONE)
    return key


def _dense_ids(texts):
    ids = {}
    return np.array([ids.setdefault(t, len(ids)) for t in texts], dtype=np.uint32), max(len(ids), 1)


def candidate_keys(cands, bed='', skip_phasing=False):
    """Per candidate of a callset: cand_key, cand_chrom of include/duet_ef.h's duet_tune_truth_problem, and n_chrom.  With a
    BED file the evaluator's position test is part of it (a candidate outside the ranges is dropped: KEY_SKIP)."""
    C = len(cands['pos'])
    key = _parsed_rows([(cands['chrom'][c], cands['pos'][c], cands['ref'][c], cands['alt'][c], cands['svtype'][c]) for c in range(C)],
                       bed, skip_phasing)
    chrom, n_chrom = _dense_ids(cands['chrom'])
    return key, chrom, n_chrom


def contig_tables(chrom_texts, skip_phasing=False):
    """The table form for a cluster result (svim-gpu mode: no per-candidate text): key_table[4 * contig + type] from one row per
    (contig, type) as svim_mode.rows_text writes it, chrom_id[contig], n_chrom.  (INV comes out as KEY_SKIP.)"""
    from duet_amd.svim_mode import SV_TYPE_NAMES
    rows = [(text, 1, 'N', '<%s>' % t, t) for text in chrom_texts for t in SV_TYPE_NAMES]
    chrom_id, n_chrom = _dense_ids(chrom_texts)
    return _parsed_rows(rows, '', skip_phasing), chrom_id, n_chrom


def merge_ranges(ranges):
    """Closed integer ranges -> the same set of positions as sorted, disjoint closed ranges within 0 .. 2^32 - 1."""
    out = []
    for a, b in sorted((max(int(a), 0), min(int(b), 0xFFFFFFFF)) for a, b in ranges if int(b) >= max(int(a), 0) and int(a) <= 0xFFFFFFFF):
        if out and a <= out[-1][1] + 1:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [(a, b) for a, b in out]


def bed_tables(bed, chrom_texts):
    """-> (bed_off[K + 1], bed_lo, bed_hi): per contig the merged ranges evaluation.parse_vcf tests its positions against -- those
    of the label CHROM[3:], whatever the first three characters are."""
    spans = evaluation.parse_bed(bed)
    off, lo, hi = [0], [], []
    for text in chrom_texts:
        for a, b in merge_ranges(spans.get(text[3:], [])):
            lo.append(a)
            hi.append(b)
        off.append(len(lo))
    return np.array(off, dtype=np.uint32), np.array(lo, dtype=np.uint32), np.array(hi, dtype=np.uint32)


def _match_limits(refdist, pctsim):
    """(refdist, ratio) for the device: abs(...) <= a negative refdist never holds, which a ratio of +inf says as well."""
    return (0, math.inf) if refdist < 0 else (int(refdist), float(pctsim))


def build_truth(cands, truth_vcf, refdist=1000, pctsim=0.0, bed='', skip_phasing=False, ctx=None):
    """prepare_truth's arrays from the device build (duet_tune_truth_build_host); groups and pairs may be numbered differently."""
    ctx = ctx or engine.default_context()
    base = truth_side(truth_vcf, bed, skip_phasing)
    key, chrom, n_chrom = candidate_keys(cands, bed, skip_phasing)
    arrays = dict(base, cand_pos=cands['pos'], cand_len=cands['svlen'], cand_key=key, cand_chrom=chrom, n_chrom=n_chrom)
    out = ctx.truth_build_host(cands['feat'], arrays, *_match_limits(refdist, pctsim))
    out['n_base'] = base['n_base']
    return out


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
    truth = build_truth(cands, truth_vcf, refdist, pctsim, bed, skip_phasing, ctx=ctx)
    counts, _, _ = ctx.sweep_host(cands['feat'], vecs, truth)
    return _rows(vecs, counts, truth['n_base'])


def _rows(vecs, counts, n_base, lead=None):
    """One dict per vector: the leading setting columns (if any), the 14 thresholds, the ten numbers (counts None: nan)."""
    out = []
    for k, v in enumerate(vecs):
        row = dict(lead or {})
        row.update(zip(NAMES, (float(x) for x in v)))
        row.update(zip(SCORES, scores(counts[k], n_base) if counts is not None else (math.nan,) * 10))
        out.append(row)
    return out


def _strata_passes(truth_vcf, bed, skip_phasing, holdout, by_contig):
    """The stratified passes a sweep was asked for: (kind, strata, the truth side numbered for them)."""
    passes = []
    if holdout is not None:
        passes.append(('holdout', strata_holdout(holdout)))
    if by_contig is not None:
        passes.append(('by_contig', strata_by_contig()))
    return [(kind, st, truth_side(truth_vcf, bed, skip_phasing, strata=st)) for kind, st in passes]


COUNTS = tuple(n for n in _lib.COUNTS_NAMES if n != 'reserved')


def _strata_rows(rows, contig_rows, vecs, strata_counts, passes, lead, labels=None):
    """Per setting: train_ / test_ scores onto its K rows (holdout); one row per vector and stratum that has a call or a truth
    record to contig_rows (by_contig).  strata_counts[kind] is COUNTS_DTYPE[K, S], or None where the setting's rows are nan.
    labels[k]: the `vector` column of vector k (None: k itself)."""
    labels = range(len(vecs)) if labels is None else labels
    for kind, st, base_s in passes:
        counts, n_base = strata_counts.get(kind), base_s['n_base_strata']
        for k in range(len(vecs)):
            for s, name in enumerate(st['names']):
                rec = counts[k, s] if counts is not None else np.zeros((), dtype=_lib.COUNTS_DTYPE)
                ten = scores(rec, n_base[s]) if counts is not None else (math.nan,) * 10
                if kind == 'holdout':
                    rows[k].update(('%s_%s' % (name, n), x) for n, x in zip(SCORES, ten))
                elif int(rec['n_calls']) or n_base[s]:
                    row = dict(lead, vector=labels[k], contig=name, n_base=n_base[s])
                    row.update((n, int(rec[n])) for n in COUNTS)
                    row.update(zip(SCORES, ten))
                    contig_rows.append(row)


LEAF_PRED_TEXT = {0: '0', 1: '1|0,0|1', 3: '1|1'}
LEAF_COUNTS = _lib.LEAF_COUNTS_NAMES
LEAF_RATES = ('call_precision', 'gt_precision', 'hp_precision')         # call_tp, call_gt, call_hp over n_calls
LEAF_COLS = ('vector', 'stratum', 'leaf', 'pred') + LEAF_COUNTS + LEAF_RATES


def leaf_rows(lead, labels, census, strata=('all',)):
    """The --by_leaf rows of one census: census LEAF_COUNTS_DTYPE[K, S, 18] (None: the setting's features report a division by
    zero -- every count and quotient nan), labels[k] the vector column, strata[s] the stratum column.  A quotient is nan where
    the leaf makes no call."""
    out = []
    for k, label in enumerate(labels):
        for s, sname in enumerate(strata):
            for leaf, lname in enumerate(_lib.LEAF_NAMES):
                row = dict(lead, vector=label, stratum=sname, leaf=lname, pred=LEAF_PRED_TEXT[_lib.LEAF_PRED[leaf]])
                if census is None:
                    row.update(dict.fromkeys(LEAF_COUNTS + LEAF_RATES, math.nan))
                else:
                    rec = census[k, s, leaf]
                    row.update((n, int(rec[n])) for n in LEAF_COUNTS)
                    n_calls = row['n_calls']
                    row.update((q, row[n] / n_calls if n_calls else math.nan) for q, n in zip(LEAF_RATES, ('call_tp', 'call_gt', 'call_hp')))
                out.append(row)
    return out


def _leaf_census(ctx, dt, n_cands, resident, vectors=None):
    """The censuses --by_leaf owes for the resident features of one setting: `all` over the plain truth arrays and, with a
    holdout pass, `train` / `test` over the pass's own -> [(census, stratum names)]."""
    out = [(dt.leaf_census(ctx, n_cands, vectors), ('all',))]
    if 'holdout' in resident:
        out.append((dt.leaf_census(ctx, n_cands, vectors, strata=resident['holdout']), ('train', 'test')))
    return out


def _leaf_nan(resident):
    return [(None, ('all',))] + ([(None, ('train', 'test'))] if 'holdout' in resident else [])


def _cap_list(pc_cap):
    """pc_cap of sweep_settings / fit: None -> [None] (the entry without a cap), else a non-empty list of caps in 0 .. 2^30 - 3."""
    if pc_cap is None:
        return [None]
    vals = [pc_cap] if isinstance(pc_cap, (int, np.integer)) else list(pc_cap)
    if not vals or any(v is None for v in vals):
        raise ValueError('pc_cap: a non-empty list of integers in 0 .. 2^30 - 3, not %r' % (pc_cap,))
    return [_lib.check_pc_cap(v) for v in vals]


def _lead(c_=None, s_=None, r_=None, p_=None, j_=None, m_=None, q_=None):
    """The setting columns in front of a row, in LEAD's order."""
    vals = dict(pc_cap=p_, svlen_thres=s_, suppread_thres=r_, cluster_max_distance=c_, join_min_sv=j_, sv_tag_min=m_, sv_tag_pc=q_)
    return {n: vals[n] for n in LEAD + SV_TAG if vals[n] is not None}


JOIN = 'join_min_sv'         # the setting of --join_ps: the features over the phase sets joined by links of at least N candidates; 0: not joined


def _join_list(join_min_sv):
    """join_min_sv of sweep_settings / fit: None -> no such setting (and no column), else a non-empty list of integers >= 0."""
    return None if join_min_sv is None else _int_list(JOIN, join_min_sv)


def _int_list(name, v):
    vals = [v] if isinstance(v, (int, np.integer)) else list(v)
    if not vals or any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < 0 for x in vals):
        raise ValueError('%s: a non-empty list of non-negative integers, not %r' % (name, v))
    return [int(x) for x in vals]


SV_TAG_PC_LIMIT = (1 << 30) - 3


def _sv_tag_lists(vote_sv_tags, sv_tag_min, sv_tag_pc, join_min_sv=None):
    """vote_sv_tags / sv_tag_min / sv_tag_pc of sweep_settings: None without the flag, else (mins, pcs) -- the product's defaults
    (1,) and (0,); 0 among the mins: no second run."""
    if not vote_sv_tags:
        if sv_tag_min is not None or sv_tag_pc is not None:
            raise ValueError('sv_tag_min / sv_tag_pc need vote_sv_tags')
        return None
    if join_min_sv is not None:
        raise ValueError('vote_sv_tags: not together with join_ps')
    mins = _int_list('sv_tag_min', (1,) if sv_tag_min is None else sv_tag_min)
    pcs = _int_list('sv_tag_pc', (0,) if sv_tag_pc is None else sv_tag_pc)
    if any(q > SV_TAG_PC_LIMIT for q in pcs):
        raise ValueError('sv_tag_pc: integers in 0 .. %d, not %r' % (SV_TAG_PC_LIMIT, sv_tag_pc))
    return mins, pcs


def _sv_tag_runs(src, dt, n, setting, cap, resident, vecs, sv, want_leaf, on_features=None):
    """--vote_sv_tags for one outer setting whose first-run features, truth arrays and strata are resident in dt (n candidates):
    the first-run pred of every vector (duet_tune_sweep_device without a truth, in chunks of vectors), ONE plan with mask =
    eligible (duet_sv_tags_plan_device), and per (sv_tag_min >= 1, sv_tag_pc) and vector: the apply, the features call on the
    problem pointed at the words into a second feature tensor, the truth build, every strata build, and that vector swept ALONE
    over its own record, with its strata sweeps and its census.  The K count records of a setting come back together, with the K
    counter blocks.  -> {(m, q): dict(counts COUNTS_DTYPE[K], strata {kind: [K, S]}, leaf [(census [K, S, 18] or None per
    vector, names)], marks int[K, 3], bad bool[K])}; bad[k]: the second run of vector k divides by zero or the plan cannot serve
    its calls -- nan rows for that vector only.  sv_tag_min 0 is the plain sweep of the first run."""
    torch, ctx, K, C = dt.torch, src.ctx, dt.K, int(n)
    mins, pcs = sv
    rec, VB = _lib.COUNTS_DTYPE.itemsize, dt.VEC_BYTES
    out = {}

    def census(vectors):
        leaf = [(dt.leaf_census(ctx, C, vectors), ('all',))]
        if 'holdout' in resident:
            leaf.append((dt.leaf_census(ctx, C, vectors, strata=resident['holdout']), ('train', 'test')))
        return leaf

    todo = [(m, q) for m in mins if m >= 1 for q in pcs]
    if 0 in mins or C == 0:
        # (no candidate: nothing can be tagged, the second run IS the first -- the plain rows and marks of 0 for every sv_tag_min)
        plain = dict(counts=dt.sweep(ctx, C), strata={kind: dt.sweep_strata(ctx, C, p) for kind, p in resident.items()},
                     leaf=[([c[k:k + 1] for k in range(K)], names) for c, names in census(None)] if want_leaf else [],
                     marks=np.zeros((K, 3), dtype=np.int64), bad=np.zeros(K, dtype=bool))
        for m, q in [(0, q) for q in pcs if 0 in mins] + (todo if C == 0 else []):
            out[(m, q)] = plain
            if on_features is not None:
                on_features(dict(setting, sv_tag_min=m, sv_tag_pc=q), src.host(dt))
    if not todo or C == 0:
        return out
    st = dt.stream()
    first, second = dt.feat, torch.zeros_like(dt.feat)
    el = _lib.FEATURE_DTYPE.fields['eligible'][1]
    mask = first[:C * _lib.FEATURE_DTYPE.itemsize].view(C, _lib.FEATURE_DTYPE.itemsize)[:, el].contiguous()
    ps = torch.zeros(C, dtype=torch.int32, device=dt.device)
    chunk = max(1, min(K, (64 << 20) // C))                # (K * C bytes stay bounded)
    pred = torch.zeros(chunk * C, dtype=torch.uint8, device=dt.device)
    state = {mq: dict(counts=torch.zeros(K * rec, dtype=torch.uint8, device=dt.device),
                      four=torch.zeros(4 * K, dtype=torch.int32, device=dt.device),
                      strata={kind: torch.zeros_like(p['counts']) for kind, p in resident.items()},
                      leaf=None, bad=np.zeros(K, dtype=bool)) for mq in todo}
    planned = None
    for k0 in range(0, K, chunk):
        kn = min(chunk, K - k0)
        ctx.sweep_device(first.data_ptr(), C, dt.vec_ptr + k0 * VB, kn, None, 0, st, out_pred_ptr=pred.data_ptr(), out_ps_ptr=ps.data_ptr())
        if planned is None:                                 # (ps is the same for every vector: the first chunk brought it)
            planned = src.sv_tags_plan(dt, cap, ps, mask, st)
        for m, q in todo:
            s_ = state[(m, q)]
            for k in range(k0, k0 + kn):
                vec_k = dt.vec_ptr + k * VB
                ctx.sv_tags_apply_device(pred.data_ptr() + (k - k0) * C, planned['tags'].data_ptr(), s_['four'].data_ptr() + 16 * k,
                                         min_votes=m, pc_new=q, stream=st)
                dt.feat = second
                try:
                    src.sv_tags_features(planned, second.data_ptr(), st, cap)
                    dt.build(ctx, C, src.result)
                    ctx.sweep_device(second.data_ptr(), C, vec_k, 1, dt.truth, s_['counts'].data_ptr() + k * rec, st)
                    for kind, p in resident.items():
                        dt.build_strata(ctx, C, src.result, p)
                        S = p['strata'].n_strata
                        ctx.sweep_strata_device(second.data_ptr(), C, vec_k, 1, p.get('truth', dt.truth), p['strata'],
                                                s_['strata'][kind].data_ptr() + k * S * rec, st)
                    if want_leaf:
                        got = census(vecs[k:k + 1])
                        if s_['leaf'] is None:
                            s_['leaf'] = [([None] * K, names) for _, names in got]
                        for (per, _), (c, _) in zip(s_['leaf'], got):
                            per[k] = c
                    if on_features is not None:
                        on_features(dict(setting, sv_tag_min=m, sv_tag_pc=q), src.host(dt))
                except ZeroDivisionError:
                    s_['bad'][k] = True
                finally:
                    dt.feat = first
    for (m, q), s_ in state.items():
        four = s_['four'].cpu().numpy().view(np.uint32).reshape(K, 4)
        bad = s_['bad'] | (four[:, 3] != 0)
        out[(m, q)] = dict(counts=s_['counts'].cpu().numpy().view(_lib.COUNTS_DTYPE).copy(),
                           strata={kind: t[:K * resident[kind]['strata'].n_strata * rec].cpu().numpy().view(_lib.COUNTS_DTYPE)
                                   .reshape(K, resident[kind]['strata'].n_strata).copy() for kind, t in s_['strata'].items()},
                           leaf=s_['leaf'] or [], marks=four[:, :3].astype(np.int64), bad=bad)
    return out


_NO_CAP_LINE = np.zeros(1, dtype=np.uint32), 0, True        # the cap line of a problem without marks: the one value 0, whole


class _Callset(object):
    """Candidate source: the callset of <home>/sv_calling/variants.vcf.  Ingested, keyed (candidate_keys) and uploaded once; a
    setting's features are those of the resident DeviceProblem (ctx.features_device).  Every listed setting is computed, in the
    listed order, a repeated one again.  A source has: settings, the (c, s, r, cap) tuples in row order; ingests(), which makes
    the candidates resident and yields the settings to compute on them, in that order; and, between two steps of ingests(),
    n_max (the most candidates a setting can have), texts (the CHROM text per candidate or contig, for chrom_strata), key(dt),
    features(dt, setting, cap), result, cap_line(dt, max_values) and host(dt)."""

    def __init__(self, ctx, home, ss, rs, ps, bed, skip_phasing, include_all_ctgs, thread, js=None, names=False):
        self.ctx, self.home, self.bed, self.skip_phasing, self.ingest = ctx, home, bed, skip_phasing, (include_all_ctgs, thread)
        self.settings = [(None,) + t for t in itertools.product(ss, rs, ps, *([js] if js is not None else []))]
        self.result = None                                  # (the per-candidate form: build() reads no cluster result)
        self.names = names                                  # (--vote_sv_tags: the marks' read names too)

    def ingests(self):
        from duet_amd.devmem import DeviceProblem
        _, s_, r_, _ = self.settings[0][:4]
        if self.names:
            self.mark_name, self.n_names = _mark_names(self.home, *self.ingest)
        self.soa, txt = _candidates(self.home, s_, r_, *self.ingest)
        if self.names and len(self.mark_name) != self.soa.n_marks:
            raise RuntimeError('--vote_sv_tags needs the native ingest, which declined this input (or DUET_NATIVE_INGEST=0)')
        self.cands = dict(pos=self.soa.cand_pos, svlen=self.soa.cand_svlen, **txt)
        self.n_max, self.texts = self.soa.n_cands, self.cands['chrom']
        self.dp = DeviceProblem(self.soa, s_, r_, device='cuda:%d' % self.ctx.device_id) if self.n_max else None
        yield self.settings

    def key(self, dt):
        dt.set_candidates(self.soa.cand_pos, self.soa.cand_svlen, *candidate_keys(self.cands, self.bed, self.skip_phasing))

    def features(self, dt, setting, cap):
        """The features of `setting` under `cap` into dt.feat -> how many candidates that makes.  Raises ZeroDivisionError where
        E/F would (the records are written all the same)."""
        if self.n_max:
            p = self.dp.problem
            p.svlen_thres, p.suppread_thres = _lib.clamp_u32(setting['svlen_thres']), _lib.clamp_u32(setting['suppread_thres'])
            if setting.get(JOIN):
                # (a joined run is the ordinary run on remapped tags: the links under this -s, -r and cap, their blocks and the remap,
                # all on the device; the problem gets its own tags back whatever the features call does)
                self.joined, _ = self.dp.joined_tags(self.ctx, setting[JOIN], pc_cap=cap, stream=dt.stream())
                with self.dp.pointed_at(self.joined):
                    self.ctx.features_device(p, dt.feat.data_ptr(), dt.stream(), pc_cap=cap)
            else:
                self.ctx.features_device(p, dt.feat.data_ptr(), dt.stream(), pc_cap=cap)
        return self.n_max

    def sv_tags_plan(self, dt, cap, ps, mask, stream):
        """(--vote_sv_tags) The plan of the resident problem under the phase sets `ps` (int32[C] tensor) and `mask` (uint8[C] tensor)
        -> dict(tags, index, info): the base words, the identity index and the plan's counts.  A refusal raises."""
        from duet_amd.devmem import upload
        torch, ef, soa = dt.torch, self.dp.problem, self.soa
        if getattr(self, 'sv', None) is None:
            self.sv = dict(names=upload(torch, dt.device, self.mark_name, np.uint32),
                           tags=torch.zeros(max(soa.n_marks, 1), dtype=torch.int64, device=dt.device),
                           index=torch.zeros(max(soa.n_marks, 1), dtype=torch.int32, device=dt.device),
                           off=np.ascontiguousarray(soa.cand_ctg_off, dtype=np.uint32))
        sv = self.sv
        p = _lib.ReadTagsProblem()
        p.n_cands, p.n_marks, p.n_reads, p.n_names, p.n_contigs = soa.n_cands, soa.n_marks, soa.n_reads, self.n_names, soa.n_contigs
        p.cand_off, p.mark_read, p.read_tag, p.mark_name = ef.cand_off, ef.mark_read, ef.read_tag, sv['names'].data_ptr()
        p.cand_ctg_off, p.ps = sv['off'].ctypes.data, ps.data_ptr()
        sv['info'] = self.ctx.sv_tags_plan_device(p, sv['tags'].data_ptr(), sv['index'].data_ptr(), cand_mask_ptr=mask.data_ptr(),
                                                  pc_cap=cap, stream=stream)
        return sv

    def sv_tags_features(self, planned, out_ptr, stream, cap):
        """(--vote_sv_tags) The features of the second run: the resident problem reads the plan's words through the identity index
        (a mark is its own read); its own tags, index and read count come back whatever happens.  Raises ZeroDivisionError where
        E/F would."""
        with _pointed_at_marks(self.dp.problem, planned['tags'], planned['index'], self.soa.n_marks):
            self.ctx.features_device(self.dp.problem, out_ptr, stream, pc_cap=cap)

    def cap_line(self, dt, max_values):
        # (the same line with and without a join: the remap keeps pc bit for bit and leaves untagged words alone, so the problem's
        # own tags give the pc values of the marks that can vote)
        return dt.cap_line(self.ctx, self.dp.problem, max_values) if self.n_max else _NO_CAP_LINE

    def host(self, dt):
        """What on_features is handed: the candidates of the last features() call, on the host."""
        return dict(self.cands, feat=dt.features_host(self.n_max))


class _Bams(object):
    """Candidate source: <home>/snp_phasing/*.bam through the fused svim-gpu pipeline.  The signatures are extracted and uploaded
    once per distinct -s, ascending (max(s, 1) is the extraction's minimum size, as in svim_mode.sv_phasing_from_bams), keyed by
    per-contig tables (contig_tables, bed_tables); a setting's features are DeviceSvim.run_features', which clusters again on
    every call (the entry keeps no state between calls).  Each distinct setting is computed once, in c, r, cap order per -s."""

    def __init__(self, ctx, home, cs, ss, rs, ps, bed, skip_phasing, include_all_ctgs, thread, js=None, names=False):
        self.ctx, self.home, self.bed, self.skip_phasing, self.ingest = ctx, home, bed, skip_phasing, (include_all_ctgs, thread)
        self.settings = list(itertools.product(cs, ss, rs, ps, *([js] if js is not None else [])))
        self.names = names                                  # (--vote_sv_tags: the marks' read names too)

    def ingests(self):
        from duet_amd import svim_mode
        from duet_amd.devmem import DeviceSvim
        from duet_amd.native import NativeIngest
        from duet_amd.read_file import init_chrom_list
        include_all_ctgs, thread = self.ingest
        chroms = init_chrom_list(include_all_ctgs, self.home)
        self.texts = svim_mode.spelled_contigs(self.home, chroms)
        self.tables = contig_tables(self.texts, self.skip_phasing) + (bed_tables(self.bed, self.texts) if self.bed else None,)
        depth_bin = 1000                                    # (phase_from_bams's defaults)
        for s_ in sorted(set(t[1] for t in self.settings)):
            ing, got = NativeIngest.extract(self.home + '/snp_phasing/', chroms, thread, max(s_, 1), 20, depth_bin, names=self.names)
            if ing is None:
                raise RuntimeError('signature extraction declined the input: %s' % got)
            ing.close()
            self.n_max = len(got['pos'])
            if self.names:
                self.mark_name, self.n_names, self.sv = np.array(got['mark_name'], dtype=np.uint32), len(got['name_off']) - 1, None
            todo = list(dict.fromkeys(t for t in self.settings if t[1] == s_))
            c_, _, r_, _ = todo[0][:4]
            self.ds = DeviceSvim(got, got['read_tag'], got['depth'], got['depth_off'], depth_bin, s_, r_, max_dist=c_,
                                 device='cuda:%d' % self.ctx.device_id, read_off=got['read_off']) if self.n_max else None
            yield todo

    @property
    def result(self):
        return self.ds.result if self.n_max else None

    def key(self, dt):
        dt.set_tables(*self.tables)

    def features(self, dt, setting, cap):
        if not self.n_max:
            return 0
        p = self.ds.sv_problem
        p.marks.max_dist = setting['cluster_max_distance']
        p.svlen_thres, p.suppread_thres = _lib.clamp_u32(setting['svlen_thres']), _lib.clamp_u32(setting['suppread_thres'])
        if setting.get(JOIN):
            self.joined, _ = self.ds.joined_tags(self.ctx, setting[JOIN], pc_cap=cap)       # (as _Callset.features)
            with self.ds.pointed_at(self.joined):
                return self.ds.run_features(self.ctx, dt.feat.data_ptr(), pc_cap=cap)
        return self.ds.run_features(self.ctx, dt.feat.data_ptr(), pc_cap=cap)

    def sv_tags_plan(self, dt, cap, ps, mask, stream):
        """(--vote_sv_tags) As _Callset.sv_tags_plan, on the resident cluster result of the last features() call (its offsets, mark
        order and contig column), the raw marks' read indices and names, and the resident tags."""
        from duet_amd.devmem import upload
        torch, ds = dt.torch, self.ds
        if self.sv is None:
            self.sv = dict(names=upload(torch, dt.device, self.mark_name, np.uint32),
                           tags=torch.zeros(max(ds.M, 1), dtype=torch.int64, device=dt.device),
                           index=torch.zeros(max(ds.M, 1), dtype=torch.int32, device=dt.device))
        sv = self.sv
        sv['n_cands'] = int(ds.n_found)
        p = _lib.ReadTagsProblem()
        p.n_cands, p.n_marks, p.n_reads, p.n_names = sv['n_cands'], ds.M, ds.sv_problem.n_reads, self.n_names
        p.cand_off, p.mark_order, p.cand_contig = ds.result.cand_off, ds.result.order, ds.result.cand_contig
        p.mark_read, p.mark_name, p.read_tag = ds.keep['sv_read'].data_ptr(), sv['names'].data_ptr(), ds.keep['sv_tag'].data_ptr()
        p.ps = ps.data_ptr()
        sv['info'] = self.ctx.sv_tags_plan_device(p, sv['tags'].data_ptr(), sv['index'].data_ptr(), cand_mask_ptr=mask.data_ptr(),
                                                  pc_cap=cap, stream=stream)
        return sv

    def sv_tags_features(self, planned, out_ptr, stream, cap):
        """(--vote_sv_tags) As _Callset.sv_tags_features: the pipeline clusters again (clustering reads no tag, so the candidates
        line up; their count is checked) and reads the plan's words through the identity index."""
        with _pointed_at_marks(self.ds.sv_problem, planned['tags'], planned['index'], self.ds.M):
            n = self.ds.run_features(self.ctx, out_ptr, pc_cap=cap)
        if n != planned['n_cands']:
            raise RuntimeError('vote_sv_tags: the cluster result changed between the two runs')

    def cap_line(self, dt, max_values):
        return dt.cap_line(self.ctx, self.ds.sv_problem, max_values) if self.n_max else _NO_CAP_LINE     # (as _Callset.cap_line)

    def host(self, dt):
        from duet_amd.svim_mode import SV_TYPE_NAMES
        # (after a division by zero the records are written all the same: fetch() then asks the device for their count)
        res = self.ds.fetch() if self.n_max else dict(cand_contig=[], cand_type=[], cand_pos=[], cand_span=[])
        return dict(feat=dt.features_host(len(res['cand_pos'])), chrom=[self.texts[int(k)] for k in res['cand_contig']],
                    pos=res['cand_pos'], svlen=res['cand_span'], svtype=[SV_TYPE_NAMES[int(t) & 3] for t in res['cand_type']])


class _pointed_at_marks(object):
    def __init__(self, problem, tags, index, n_marks):
        self.problem, self.to, self.mine = problem, (tags.data_ptr(), index.data_ptr(), int(n_marks)), None

    def __enter__(self):
        p = self.problem
        self.mine = p.read_tag, p.mark_read, p.n_reads
        p.read_tag, p.mark_read, p.n_reads = self.to
        return self

    def __exit__(self, *exc):
        p = self.problem
        p.read_tag, p.mark_read, p.n_reads = self.mine
        return False


def _mark_names(home, include_all_ctgs, thread):
    """(--vote_sv_tags) The marks' read names of <home> by the native ingest -> (mark_name u32[M], n_names); refused where the
    ingest declines, as in duet."""
    from duet_amd import sv_phasing
    ing, _ = sv_phasing.load_native(home, thread, include_all_ctgs, home + '/sv_calling/variants.vcf', log=False, names=True)
    if ing is None:
        raise RuntimeError('--vote_sv_tags needs the native ingest, which declined this input (or DUET_NATIVE_INGEST=0)')
    try:
        nm = ing.mark_names()
        return np.array(nm['mark_name'], dtype=np.uint32), len(nm['name_off']) - 1
    finally:
        ing.close()


def _source(ctx, home, svlen_thres, suppread_thres, cluster_max_distance, from_bams, pc_cap, bed, skip_phasing, include_all_ctgs, thread,
            join_min_sv=None, names=False):
    """The candidate source of sweep_settings / fit for their -s, -r, -c and pc_cap arguments (nothing is read yet); its ctx is
    `ctx`, or the default context, opened once the arguments have passed."""
    ss, rs = _int_list('svlen_thres', svlen_thres), _int_list('suppread_thres', suppread_thres)
    ps, js = _cap_list(pc_cap), _join_list(join_min_sv)
    if cluster_max_distance is not None and not from_bams:
        raise ValueError('cluster_max_distance only acts on candidates clustered from the BAMs: it needs from_bams')
    cs = [float(c) for c in (cluster_max_distance if cluster_max_distance is not None else (0.9,))]
    if from_bams and not cs:
        raise ValueError('cluster_max_distance: an empty list')
    ctx = ctx or engine.default_context()
    if from_bams:
        return _Bams(ctx, home, cs, ss, rs, ps, bed, skip_phasing, include_all_ctgs, thread, js, names=names)
    return _Callset(ctx, home, ss, rs, ps, bed, skip_phasing, include_all_ctgs, thread, js, names=names)


def _make_resident(src, dt, setting, cap, passes):
    """The features of `setting` under `cap`, their plain truth arrays and those of every pass of `passes`, resident in dt
    -> the candidate count.  Raises ZeroDivisionError where the features report one (nothing is built then)."""
    n = src.features(dt, setting, cap)
    dt.build(src.ctx, n, src.result)
    for p in passes:
        dt.build_strata(src.ctx, n, src.result, p)
    return n


def _settings(src, vecs, base, passes, refdist, pctsim, on_features=None):
    """The one loop over settings, for sweep_settings and fit: every setting of `src`, in the source's compute order, as
    (lead, dt, n_cands, resident, src) -- lead: the setting's leading columns (_lead); dt: the DeviceTune that holds the setting's
    features, its plain truth arrays and, per pass of `passes`, truth arrays and strata of the pass's own (resident: kind -> the
    pass of set_strata); n_cands: the candidate count, None where the features report a division by zero (nothing is built
    then).  on_features(lead, cands) is called when the consumer is done with the setting."""
    from duet_amd.devmem import DeviceTune
    for todo in src.ingests():
        dt = DeviceTune(src.n_max, base, *_match_limits(refdist, pctsim), vectors=vecs, device='cuda:%d' % src.ctx.device_id)
        src.key(dt)
        resident = {kind: dt.set_strata(chrom_strata(src.texts, st), b['uid_off'], b['base_uid'], own_truth=True) for kind, st, b in passes}
        for t in todo:
            lead = _lead(*t)
            try:
                n = _make_resident(src, dt, lead, t[3], resident.values())
            except ZeroDivisionError:
                n = None
            yield lead, dt, n, resident, src
            if on_features is not None:
                on_features(lead, src.host(dt))


def sweep_settings(home, truth_vcf, grid, svlen_thres=(50,), suppread_thres=(2,), cluster_max_distance=None, from_bams=False,
                   refdist=1000, pctsim=0.0, bed='', skip_phasing=False, include_all_ctgs=False, thread=4, ctx=None, on_features=None,
                   holdout=None, by_contig=None, pc_cap=None, by_leaf=None, join_min_sv=None, vote_sv_tags=False, sv_tag_min=None,
                   sv_tag_pc=None):
    """sweep() for every setting of -s (svlen_thres), -r (suppread_thres) and, with from_bams, -c (cluster_max_distance; default
    (0.9,)): -> list of rows, settings outermost in the order c, s, r, each row a dict of svlen_thres, suppread_thres
    [, cluster_max_distance], the 14 thresholds and the ten numbers.  from_bams: the candidates come from <home>/snp_phasing/*.bam
    through the fused svim-gpu pipeline (duet_svim_features_device) instead of from sv_calling/variants.vcf.
    The work directory is ingested once (from_bams: once per distinct -s, whose max(s, 1) is the extraction's minimum size, as in
    svim_mode.sv_phasing_from_bams) and uploaded once; per setting the device computes the features, builds the truth arrays and
    applies the vectors -- only the K count records come back.  A setting for which E/F reports a division by zero (upstream
    raises there) yields nan rows.  on_features(setting, cands): called per setting with the features brought to the host
    (cands as features() returns them, without ref / alt / soa in the from_bams mode).
    holdout: a list of CHROM texts -- every row gains train_<score> (every other text) and test_<score> (the listed texts) for the
    ten SCORES.  by_contig: a list that receives one row per setting, vector and stratum of strata_by_contig() with a call or a
    truth record: the setting, vector, contig, the nine counts, n_base and the ten scores.  Each is one stratified pass per
    setting (truth arrays of its own with the pass's id numbering, duet_tune_sweep_strata_device) beside the plain sweep, whose
    rows do not change.
    The settings come from _settings(), the loop fit() runs too, over one of two candidate sources (_Callset, _Bams): per setting
    it leaves the features and every truth array resident; here the vectors are swept over them, the census is taken and the rows
    are made.
    pc_cap: a list of PC caps (a read with a PC tag above the cap does not vote; the reference's is 8100) -- the innermost setting,
    after c, s, r; every row then gains a leading pc_cap column.  A cap costs the features call (duet_ef_features_cap_device,
    duet_svim_features_cap_device), the truth build(s) and the sweep(s) on the resident problem: no ingest, no upload and, without
    from_bams, no host work.  None: the features of the entries without a cap, and rows without the column.
    by_leaf: a list that receives leaf_rows() per setting: one row per vector, stratum (`all`; with holdout also `train`, `test`)
    and leaf -- one more pass per setting over what is already resident (duet_tune_leaf_census_device), after the plain sweep
    and after the holdout pass's; every other row and count stays what it is without it.
    join_min_sv: a list of N >= 0 (--join_ps --join_min_sv) -- the innermost setting, behind pc_cap, because the links depend on
    -c, -s, -r and the cap; every row then gains a join_min_sv column behind the other setting columns.  N >= 1: the setting's
    features are those of the joined run -- the links under the setting (duet_ps_links_device / duet_svim_ps_links_device), their
    blocks built and applied to the read tags on the device (duet_ps_join_links_device), the features call on the remapped tags,
    whose PS column holds block names; everything downstream runs unchanged on that record.  0: not joined, the rows of a run
    without the argument.  None: no such setting and no column.
    vote_sv_tags (--vote_sv_tags), with sv_tag_min (a list of N >= 0, default (1,)) and sv_tag_pc (a list of PCs in 0 .. 2^30 - 3,
    default (0,)) -- the innermost settings, behind pc_cap: every row scores the SECOND run of duet --vote_sv_tags for its own
    vector -- the tags derived from that vector's first-run calls (_sv_tag_runs: one plan per outer setting, one apply per
    vector) -- and gains sv_tag_min, sv_tag_pc and the vector's marks_untagged, marks_given, marks_own_only behind the other
    setting columns; by_contig rows gain the two settings only.  sv_tag_min 0: no second run, the rows of a call without the
    argument and marks of 0.  A vector whose second run divides by zero has nan rows for that vector only.  Not together with
    join_min_sv.  Both candidate sources; from_bams clusters again per features call, as it does without the flag.
    on_features: one call per (setting, sv_tag_min, sv_tag_pc) with the second run's records, which differ per vector -- so
    only with a grid of exactly one vector."""
    vecs = grid if isinstance(grid, np.ndarray) else expand_grid(grid)
    sv = _sv_tag_lists(vote_sv_tags, sv_tag_min, sv_tag_pc, join_min_sv)
    if sv is not None and on_features is not None and len(vecs) != 1:
        raise ValueError('vote_sv_tags: the features of the second run differ per vector; on_features needs a grid of exactly one vector')
    src = _source(ctx, home, svlen_thres, suppread_thres, cluster_max_distance, from_bams, pc_cap, bed, skip_phasing, include_all_ctgs, thread,
                  join_min_sv, names=sv is not None)
    ctx = src.ctx
    base = truth_side(truth_vcf, bed, skip_phasing)
    passes = _strata_passes(truth_vcf, bed, skip_phasing, holdout, by_contig)
    if sv is not None:
        return _sweep_sv_tags(src, vecs, base, passes, refdist, pctsim, on_features, by_contig, by_leaf, sv)
    done = {}
    for lead, dt, n, resident, _ in _settings(src, vecs, base, passes, refdist, pctsim, on_features):
        counts, strata_counts, leaf = None, {}, _leaf_nan(resident)
        if n is not None:
            counts = dt.sweep(ctx, n)
            if by_leaf is not None:
                leaf = [(dt.leaf_census(ctx, n), ('all',))]
            for kind, p in resident.items():
                strata_counts[kind] = dt.sweep_strata(ctx, n, p)
                if by_leaf is not None and kind == 'holdout':
                    leaf.append((dt.leaf_census(ctx, n, strata=p), ('train', 'test')))
        done[tuple(lead.values())] = counts, strata_counts, leaf
    out = []
    for t in src.settings:
        lead = _lead(*t)
        counts, strata_counts, leaf = done[tuple(lead.values())]
        rows = _rows(vecs, counts, base['n_base'], lead)
        _strata_rows(rows, by_contig, vecs, strata_counts, passes, lead)
        out.extend(rows)
        if by_leaf is not None:
            for census, names in leaf:
                by_leaf.extend(leaf_rows(lead, range(len(vecs)), census, names))
    return out


def _sweep_sv_tags(src, vecs, base, passes, refdist, pctsim, on_features, by_contig, by_leaf, sv):
    """sweep_settings under vote_sv_tags: per outer setting _sv_tag_runs, then the rows -- settings outermost, sv_tag_min, sv_tag_pc,
    the vectors innermost."""
    K, done = len(vecs), {}
    for lead, dt, n, resident, _ in _settings(src, vecs, base, passes, refdist, pctsim):
        cap = lead.get('pc_cap')
        done[tuple(lead.values())] = (None if n is None else
                                      _sv_tag_runs(src, dt, n, lead, cap, resident, vecs, sv, by_leaf is not None, on_features), resident)
    out = []
    for t in src.settings:
        runs, resident = done[tuple(_lead(*t).values())]
        for m in sv[0]:
            for q in sv[1]:
                lead = _lead(*t, m_=m, q_=q)
                run = runs[(m, q)] if runs is not None else None
                rows = []
                for k in range(K):
                    ok = run is not None and not run['bad'][k]
                    row = _rows(vecs[k:k + 1], run['counts'][k:k + 1] if ok else None, base['n_base'], lead)[0]
                    marks = run['marks'][k] if ok else (math.nan,) * 3
                    row = dict(list(lead.items()) + list(zip(MARKS, (x if x != x else int(x) for x in marks))) +
                               [(name, row[name]) for name in row if name not in lead])
                    _strata_rows([row], by_contig, vecs[k:k + 1], {kind: c[k:k + 1] for kind, c in run['strata'].items()} if ok else {},
                                 passes, lead, labels=[k])
                    rows.append(row)
                out.extend(rows)
                if by_leaf is not None:
                    kinds = run['leaf'] if run is not None and run['leaf'] else [([None] * K, names) for _, names in _leaf_nan(resident)]
                    for per, names in kinds:
                        for k in range(K):
                            ok = run is not None and not run['bad'][k] and per[k] is not None
                            by_leaf.extend(leaf_rows(lead, [k], per[k] if ok else None, names))
    return out


TRACE = ('round', 'axis', 'n_distinct', 'n_vec', 'exact', 'old', 'new', 'objective_before', 'objective_after')


CAP_AXIS = 'pc_cap'         # the 15th axis of the fit: not a field of the vector -- a step on it changes the features


def _axes(axes, fit_cap=False):
    """--axes: names (or indices) of the vector's fields -> indices, in the order given; None: all 14 in field order.  The name
    pc_cap (CAP_AXIS) stands for itself, at the place given; fit_cap: appended when it is not named."""
    if axes is None:
        return list(range(len(NAMES))) + ([CAP_AXIS] if fit_cap else [])
    out = []
    for a in axes:
        if a == CAP_AXIS:
            if a not in out:
                out.append(a)
        elif isinstance(a, str) and a in NAMES:
            out.append(NAMES.index(a))
        elif isinstance(a, (int, np.integer)) and not isinstance(a, bool) and 0 <= a < len(NAMES):
            out.append(int(a))
        else:
            raise ValueError('axes: %r is not a threshold name' % (a,))
    if not out:
        raise ValueError('axes: an empty list')
    if fit_cap and CAP_AXIS not in out:
        out.append(CAP_AXIS)
    return out


def _better(x, best):
    """Is objective x strictly greater than best?  nan never wins, and anything with a number beats nan."""
    return not math.isnan(x) and (math.isnan(best) or x > best)


def _cap_step(src, dt, setting, cap, cur, max_values, score_of, n_base, hold, n_base_hold, ten):
    """One step of the fit on the pc_cap axis of `setting` (its leading columns), from `cap`: every value of the source's cap
    line, ascending, and last the current cap -- the features under it, the truth arrays, the one current vector scored.  Moves
    the cap by the rule of every axis and leaves the features and truth arrays of the cap it ends on resident.
    -> (the trace row without its round, the cap it ends on, the candidate count under that cap)"""
    ctx, passes = src.ctx, [hold] if hold is not None else []
    caps, n_distinct, whole = src.cap_line(dt, max_values)
    dt.set_line_vector(cur)

    def evaluate(c):
        """-> (objective, plain counts, strata counts or None, candidate count); a cap whose features divide by zero: nan, nothing
        built or swept"""
        try:
            n = _make_resident(src, dt, setting, c, passes)
        except ZeroDivisionError:
            return math.nan, None, None, 0
        plain = dt.sweep_line(ctx, n, 0, 1)[0]
        if hold is None:
            return ten(plain, n_base)[score_of], plain, None, n
        sc = dt.sweep_line_strata(ctx, n, 0, 1, hold)[0]
        return ten(sc[0], n_base_hold[0])[score_of], plain, sc, n

    got = [evaluate(int(c)) for c in caps]
    here = evaluate(cap)
    if here[1] is None:
        raise ZeroDivisionError('division by zero')
    best, pick = here[0], None
    for i, g in enumerate(got):
        if _better(g[0], best):
            best, pick = g[0], i
    old = cap
    if pick is not None:
        cap = int(caps[pick])
        _make_resident(src, dt, setting, cap, passes)       # (the threshold axes that follow read these)
    _, plain, sc, n_cands = here if pick is None else got[pick]
    row = dict(axis=CAP_AXIS, n_distinct=n_distinct, n_vec=len(caps), exact=int(whole), old=old, new=cap,
               objective_before=here[0], objective_after=best)
    row.update(zip(SCORES, ten(plain, n_base)))
    if hold is not None:
        for s_i, part in enumerate(('train', 'test')):
            row.update(('%s_%s' % (part, n), x) for n, x in zip(SCORES, ten(sc[s_i], n_base_hold[s_i])))
    return row, cap, n_cands


def _fit_setting(ctx, dt, n_cands, start, axes, rounds, max_values, score_of, n_base, hold=None, n_base_hold=None, src=None,
                 setting=None, cap=None):
    """Coordinate descent for one setting on the resident features and truth arrays of dt
    -> (vector, trace rows, the fitted cap, the candidate count of the features it leaves resident).
    hold: the holdout pass (its stratum 0 is `train`, whose score is the objective; stratum 1 `test` is only reported).
    src, setting, cap -- for CAP_AXIS among the axes: the candidate source, the setting's leading columns and the cap the resident
    features were computed under."""
    cur = np.array(start, dtype=np.float64)
    memo = {}

    def ten(rec, nb):
        key = (rec.tobytes(), nb)
        if key not in memo:
            memo[key] = scores(rec, nb)
        return memo[key]

    trace = []
    for rnd in range(1, rounds + 1):
        moved = False
        for ax in axes:
            if ax == CAP_AXIS:
                row, cap, n_cands = _cap_step(src, dt, setting, cap, cur, max_values, score_of, n_base, hold, n_base_hold, ten)
                moved = moved or row['new'] != row['old']
                trace.append(dict(round=rnd, **row))
                continue
            n_vec, n_distinct = dt.line(ctx, n_cands, cur, ax, max_values)
            K = n_vec + 1                                    # (the line's vectors, then the current vector)
            if hold is not None:
                sc = dt.sweep_line_strata(ctx, n_cands, 0, K, hold)
                objs = [ten(sc[k, 0], n_base_hold[0])[score_of] for k in range(K)]
            else:
                pc = dt.sweep_line(ctx, n_cands, 0, K)
                objs = [ten(pc[k], n_base)[score_of] for k in range(K)]
            before, best, pick = objs[n_vec], objs[n_vec], n_vec
            for i in range(n_vec):
                if _better(objs[i], best):
                    best, pick = objs[i], i
            old = float(cur[ax])
            if pick != n_vec:
                cur[ax] = dt.line_value(pick, ax)
                moved = True
            row = dict(round=rnd, axis=NAMES[ax], n_distinct=n_distinct, n_vec=n_vec, exact=int(n_vec == n_distinct + 1), old=old,
                       new=float(cur[ax]), objective_before=before, objective_after=objs[pick])
            plain = dt.sweep_line(ctx, n_cands, pick, 1)[0] if hold is not None else pc[pick]
            row.update(zip(SCORES, ten(plain, n_base)))
            if hold is not None:
                for s_i, part in enumerate(('train', 'test')):
                    row.update(('%s_%s' % (part, n), x) for n, x in zip(SCORES, ten(sc[pick, s_i], n_base_hold[s_i])))
            trace.append(row)
        if not moved:
            break
    return cur, trace, cap, n_cands


def _nan_row(holdout):
    row = dict(zip(TRACE, (0, '', 0, 0, 0) + (math.nan,) * 4))
    row.update(dict.fromkeys(SCORES, math.nan))
    if holdout:
        row.update(('%s_%s' % (part, n), math.nan) for part in ('train', 'test') for n in SCORES)
    return row


def fit(home, truth_vcf, objective='hp_f1', start=None, axes=None, rounds=8, max_values=0, svlen_thres=(50,), suppread_thres=(2,),
        cluster_max_distance=None, from_bams=False, refdist=1000, pctsim=0.0, bed='', skip_phasing=False, include_all_ctgs=False,
        thread=4, ctx=None, holdout=None, pc_cap=None, fit_cap=False, by_leaf=None, join_min_sv=None):
    """Fit the vector to the truth set by exact per-threshold line search (see the module text), per setting of -s, -r, -c and
    pc_cap as sweep_settings takes them.  The cap is a setting, fitted per value given; with the name pc_cap among the axes (at any
    place), or fit_cap=True (appended behind the axes in force), it is also an axis: each given value -- else the pc_cap key of a
    start dict, else 8100 -- is then the START of a fit that moves the cap along its own exact line (the distinct pc values of the
    marks that can vote, duet_tune_cap_line_device; from_bams: of the raw marks, duet_svim_cap_line_device).  A step on that axis
    costs, per line value, the features under the value, the truth build(s) and one vector swept (from_bams: every value clusters
    again); a value whose features divide by zero scores nan and never wins.  The fit dict then carries pc_cap, the fitted cap;
    setting['pc_cap'], where present, stays the start.  objective: one of SCORES (with holdout: the `train` stratum's; `test` is reported, never used);
    start: a vector, a partial vector (dict) or None for the defaults; axes: names of the fields to move, in this order (None: all,
    in field order); rounds: at most this many passes over the axes; max_values: 0 for the whole line of every axis, N >= 2 for
    at most N of its values (both ends among them).
    -> dict(fits = one dict(setting, vector (None: no fit), objective, scores, trace) per setting in c, s, r order,
            best = the fit with the greatest final objective (ties: the earlier setting; None when no setting has a fit),
            trace = every setting's rows, each the setting's columns, TRACE, the ten SCORES of the new vector and, with holdout,
            its train_ / test_ scores).
    A setting whose features or line report a division by zero, or whose objective never has a number, has no fit: its vector is
    None and (division by zero) its trace is one row of nan.
    by_leaf: a list that receives, per setting, leaf_rows() of the start vector (vector = 'start', on the features the fit starts
    from) and of the vector the fit ends on (vector = 'fitted', under the fitted cap where the cap moved): where the fit moved the
    calls.  A setting without a trace has nan rows for both.
    join_min_sv: as sweep_settings takes it -- each listed N is a setting of its own, fitted on the features of its joined run
    (0: not joined); on the cap axis every value of the line builds the links, the blocks and the remap again under that value
    before its features call (all on the device); the line itself is the same with and without a join."""
    if objective not in SCORES:
        raise ValueError('objective: %r is not one of %s' % (objective, ', '.join(SCORES)))
    rounds, max_values = int(rounds), int(max_values)
    if rounds < 1:
        raise ValueError('rounds: at least 1')
    if max_values < 0 or max_values == 1:
        raise ValueError('max_values: 0 (all) or at least 2')
    _cap_list(pc_cap)
    cap0 = None
    if isinstance(start, dict) and CAP_AXIS in start:        # (the 15th key of a fitted file: the cap axis starts there)
        start = dict(start)
        cap0 = start.pop(CAP_AXIS)
        cap0 = None if cap0 is None else _lib.check_pc_cap(cap0)
    v0 = vector(start) if start is None or isinstance(start, dict) else np.array(start, dtype=np.float64).reshape(len(NAMES))
    ax = _axes(axes, fit_cap)
    with_cap = CAP_AXIS in ax
    score_of = SCORES.index(objective)
    ctx = ctx or engine.default_context()
    base = truth_side(truth_vcf, bed, skip_phasing)
    passes = _strata_passes(truth_vcf, bed, skip_phasing, holdout, None)
    n_base, n_base_hold = base['n_base'], passes[0][2]['n_base_strata'] if passes else None
    src = _source(ctx, home, svlen_thres, suppread_thres, cluster_max_distance, from_bams, pc_cap, bed, skip_phasing, include_all_ctgs, thread,
                  join_min_sv)

    def one(setting, dt, n_cands, resident):
        """The fit of one setting (n_cands None: its features report a division by zero) -> its dict of `fits`"""
        vec, trace, cap, leaf = None, None, None, []
        hold = resident.get('holdout')
        if n_cands is not None:
            try:
                if with_cap:
                    cap = setting.get(CAP_AXIS, cap0 if cap0 is not None else _lib.PC_MAX)
                    if cap != setting.get(CAP_AXIS, _lib.PC_MAX):
                        # (the start comes from --start: the resident features are the setting's, those of 8100)
                        n_cands = _make_resident(src, dt, setting, cap, resident.values())
                if by_leaf is not None:
                    leaf = [_leaf_census(ctx, dt, n_cands, resident, v0[None, :])]
                vec, trace, cap, n_cands = _fit_setting(ctx, dt, n_cands, v0, ax, rounds, max_values, score_of, n_base, hold, n_base_hold,
                                                        src, setting, cap)
                if by_leaf is not None:
                    leaf.append(_leaf_census(ctx, dt, n_cands, resident, vec[None, :]))
            except ZeroDivisionError:
                trace = None
        if by_leaf is not None:
            for i, label in enumerate(('start', 'fitted')):
                for census, names in leaf[i] if trace is not None else _leaf_nan(resident):
                    by_leaf.extend(leaf_rows(setting, (label,), census, names))
        if trace is None:
            return dict(setting=dict(setting), vector=None, objective=math.nan, scores=dict.fromkeys(SCORES, math.nan),
                        trace=[dict(setting, **_nan_row(holdout is not None))])
        last = trace[-1]
        obj = last['objective_after']
        return dict(setting=dict(setting), vector=None if math.isnan(obj) else vec, objective=obj,
                    scores={n: last[n] for n in last if n in SCORES or n.startswith(('train_', 'test_'))},
                    trace=[dict(setting, **r) for r in trace], **({CAP_AXIS: cap} if with_cap else {}))

    fits = {}
    for lead, dt, n, resident, _ in _settings(src, v0[None, :], base, passes, refdist, pctsim):
        if tuple(lead.values()) not in fits:                # (the callset source computes a repeated setting again: it is fitted once)
            fits[tuple(lead.values())] = one(lead, dt, n, resident)
    out = [fits[k] for k in dict.fromkeys(tuple(_lead(*t).values()) for t in src.settings)]
    best = None
    for f in out:
        if f['vector'] is not None and (best is None or f['objective'] > best['objective']):
            best = f
    return dict(fits=out, best=best, trace=[r for f in out for r in f['trace']])


def apply(cands, thresholds, ctx=None):
    """One vector applied the way the E/F kernels decide: -> (pred u8[C], ps u32[C]), duet_ef_run_device's outputs."""
    ctx = ctx or engine.default_context()
    _, pred, ps = ctx.sweep_host(cands['feat'], np.asarray(thresholds, dtype=np.float64).reshape(1, -1), want_pred=True, want_ps=True)
    return pred[0], ps


def explain(cands, thresholds, ctx=None):
    """Why each candidate is called as it is under one vector: -> (leaf u8[C], pred u8[C]).  leaf is the exit of predict_hp's tree
    the candidate takes (an index into _lib.LEAF_NAMES: what the leaf census counts), _lib.LEAF_NO_SEED where its contig has no
    seed phase set, _lib.LEAF_FILTERED where the -s / -r / genotype filter drops it; pred is apply()'s."""
    ctx = ctx or engine.default_context()
    return ctx.leaves_host(cands['feat'], np.asarray(thresholds, dtype=np.float64).reshape(-1))


def load_vector(path, with_cap=False, with_join=False):
    """--thresholds FILE.json: one partial vector (JSON object) -> float64[14].  The object may carry a 15th key, pc_cap (what
    `tune --fit --pc_cap` writes): with_cap: -> (float64[14], the cap or None); without, the key is accepted and left out.
    Likewise the key join_min_sv, an integer >= 1 (what `tune --fit --join_ps` writes): with_join: the tuple gains it (or None)
    as its last element."""
    with open(path) as f:
        obj = json.load(f)
    if not isinstance(obj, dict):
        raise ValueError('%s: a threshold file holds one JSON object of name -> value' % path)
    obj = dict(obj)
    cap = obj.pop('pc_cap', None)
    if cap is not None:
        try:
            cap = _lib.check_pc_cap(cap)
        except ValueError as e:
            raise ValueError('%s: %s' % (path, e))
    join = obj.pop(JOIN, None)
    if join is not None:
        if isinstance(join, bool) or not isinstance(join, int) or join < 1:
            raise ValueError('%s: join_min_sv: an integer >= 1, not %r' % (path, join))
    vec = vector(obj)
    out = (vec,) + ((cap,) if with_cap else ()) + ((join,) if with_join else ())
    return out if len(out) > 1 else vec


def _write_tsv(path, names, rows):
    with open(path, 'w') as f:
        f.write('\t'.join(names) + '\n')
        for r in rows:
            f.write('\t'.join(repr(x) if isinstance(x, float) else str(x) for x in r) + '\n')


def _csv(kind, what):
    def parse(text):
        try:
            vals = [kind(x) for x in text.split(',')]
        except ValueError:
            raise argparse.ArgumentTypeError('%s: %r is not a comma-separated list' % (what, text))
        if not vals or any(v < 0 for v in vals):
            raise argparse.ArgumentTypeError('%s: %r holds a negative value' % (what, text))
        return vals
    return parse


def _caps(text):
    """--pc_cap: a comma-separated list of integers in 0 .. 2^30 - 3."""
    try:
        return [_lib.check_pc_cap(int(x)) for x in text.split(',')]
    except ValueError:
        raise argparse.ArgumentTypeError('--pc_cap: %r is not a comma-separated list of integers in 0 .. 2^30 - 3' % (text,))


def parse_args(argv):
    ap = argparse.ArgumentParser(description='score many T1-T5 threshold vectors of the SV phasing decision against a truth set')
    ap.add_argument('workdir', help='Duet work directory (sv_calling/variants.vcf, snp_phasing/*.bam)')
    ap.add_argument('truthset', help='VCF of the phased truth set')
    ap.add_argument('--grid', default=None, help='JSON: a list of partial vectors, or an object of name -> list of values '
                                                 '(required without --fit)')
    ap.add_argument('--fit', choices=SCORES, default=None, metavar='SCORE',
                    help='fit the vector instead of scoring a grid: coordinate descent over the exact line of every axis, maximising '
                         'this score (one of %s); with --holdout the score of the train part' % ', '.join(SCORES))
    ap.add_argument('--start', default=None, help='with --fit: JSON object, the (partial) vector the fit starts from [the defaults]')
    ap.add_argument('--axes', type=lambda t: [x for x in t.split(',')], default=None,
                    help='with --fit: comma-separated threshold names to move, in this order; pc_cap among them makes the PC cap '
                         'an axis at that place [all 14, in field order]')
    ap.add_argument('--fit_cap', action='store_true',
                    help='with --fit: the PC cap is an axis too, behind the others unless --axes names pc_cap at a place of its own; '
                         'it starts at --pc_cap (each listed value a start of its own), else at the pc_cap key of --start, else at '
                         '8100, and moves along the distinct PC values of the marks that can vote')
    ap.add_argument('--rounds', type=int, default=8, help='with --fit: at most this many passes over the axes [%(default)s]')
    ap.add_argument('--max_values', type=int, default=0,
                    help='with --fit: at most this many values of an axis per line, both ends among them; 0 = every distinct value '
                         '(exact) [%(default)s]')
    ap.add_argument('--out_vector', default='best.json', help='with --fit: the fitted vector, a JSON object that duet --thresholds '
                                                              'reads [%(default)s]')
    ap.add_argument('--trace', default='', help='with --fit: one row per setting, round and axis here (TSV)')
    ap.add_argument('-s', '--sv_min_size', type=_csv(int, '-s'), default=[50],
                    help='minimum SV size; a comma-separated list sweeps it [50]')
    ap.add_argument('-r', '--min_support_read', type=_csv(int, '-r'), default=[2],
                    help='minimum number of supporting reads; a comma-separated list sweeps it [2]')
    ap.add_argument('--from_bams', action='store_true',
                    help='take the candidates from snp_phasing/*.bam through the svim-gpu pipeline, not from sv_calling/variants.vcf')
    ap.add_argument('-c', '--cluster_max_distance', type=_csv(float, '-c'), default=None,
                    help='with --from_bams: maximum span-position distance of the clustering; a comma-separated list sweeps it [0.9]')
    ap.add_argument('--pc_cap', type=_caps, default=None,
                    help='reads with a PC tag above the cap do not vote; a comma-separated list sweeps it, innermost, and every '
                         'row gains a leading pc_cap column [8100, without the column]')
    ap.add_argument('--join_ps', action='store_true',
                    help='score the run over joined phase sets (duet --join_ps): --join_min_sv becomes the innermost setting and '
                         'every row gains a join_min_sv column')
    ap.add_argument('--join_min_sv', type=_csv(int, '--join_min_sv'), default=None,
                    help='with --join_ps: a link joins two phase sets only when at least this many SV candidates agree on it; a '
                         'comma-separated list sweeps it; 0 = not joined [2].  With --fit, --out_vector carries the best '
                         'setting\'s value when it is at least 1; when 0 (not joined) fits best the file has no such key, and '
                         'duet --thresholds FILE is then meant to run without --join_ps (with it, it joins with its default 2)')
    ap.add_argument('--vote_sv_tags', action='store_true',
                    help='score the second run of duet --vote_sv_tags, per vector: the untagged reads vote with the haplotype that the '
                         "vector's own first-run het calls give them; --sv_tag_min and --sv_tag_pc become the innermost settings and "
                         'every row gains their columns and marks_untagged, marks_given, marks_own_only')
    ap.add_argument('--sv_tag_min', type=_csv(int, '--sv_tag_min'), default=None,
                    help='with --vote_sv_tags: a read gets a tag only when the other calls favour one haplotype by at least this many '
                         'marks; a comma-separated list sweeps it; 0 = no second run [1]')
    ap.add_argument('--sv_tag_pc', type=_csv(int, '--sv_tag_pc'), default=None,
                    help='with --vote_sv_tags: the PC the derived tags carry, 0 .. 2^30 - 3; a comma-separated list sweeps it [0]')
    ap.add_argument('-a', '--include_all_ctgs', action='store_true', help='all contigs, not only chr{1..22,X,Y}')
    ap.add_argument('-t', '--thread', type=int, default=4, help='threads of the ingest [%(default)s]')
    ap.add_argument('--refdist', type=int, default=1000, help="the evaluator's --refdist [%(default)s]")
    ap.add_argument('--pctsim', type=float, default=0, help="the evaluator's --pctsim [%(default)s]")
    ap.add_argument('--bed_file', type=str, default='', help="the evaluator's --bed_file")
    ap.add_argument('--skip_phasing', action='store_true', help="the evaluator's --skip_phasing")
    ap.add_argument('--out', default='sweep.tsv', help='one row per setting and vector [%(default)s]')
    ap.add_argument('--features', default='', help='also write the per-candidate features here (TSV; with several settings one '
                                                   'file per setting, the setting in its name)')
    ap.add_argument('--holdout', type=lambda t: [x for x in t.split(',')], default=None,
                    help='comma-separated CHROM texts held out: every row gains train_<score> (all other texts) and test_<score> '
                         '(these texts) for the ten scores')
    ap.add_argument('--by_contig', default='', help='also write one row per setting, vector and contig (chr1..chrY, other) that has '
                                                    'a call or a truth record here (TSV): counts, n_base and the ten scores')
    ap.add_argument('--by_leaf', default='', help='also write one row per setting, vector, stratum (all; with --holdout also train, '
                                                  'test) and leaf of the tree here (TSV): the candidates the vector sends there, those '
                                                  'listed and matched, the calls and what they score; with --fit the start vector and '
                                                  'the fitted one')
    ap.add_argument('--device', type=int, default=0, help='HIP device index [%(default)s]')
    a = ap.parse_args(argv)
    if a.fit is not None and a.grid is not None:
        ap.error('--fit and --grid exclude each other')
    if a.fit is None and a.grid is None:
        ap.error('the following arguments are required: --grid')
    if a.fit is None and a.fit_cap:
        ap.error('--fit_cap belongs to --fit')
    if a.fit is not None and (a.by_contig or a.features):
        ap.error('--fit writes --out_vector and --trace: --by_contig and --features belong to --grid')
    if a.fit is not None and (a.rounds < 1 or a.max_values < 0 or a.max_values == 1):
        ap.error('--rounds is at least 1; --max_values is 0 (every value) or at least 2')
    if a.cluster_max_distance is not None and not a.from_bams:
        ap.error('-c / --cluster_max_distance needs --from_bams: it only acts on candidates clustered from the BAMs')
    if a.holdout is not None and (not a.holdout or not all(a.holdout)):
        ap.error('--holdout: an empty list (or an empty CHROM text in it)')
    if a.join_min_sv is not None and not a.join_ps:
        ap.error('--join_min_sv needs --join_ps')
    a.join = (a.join_min_sv if a.join_min_sv is not None else [2]) if a.join_ps else None
    if (a.sv_tag_min is not None or a.sv_tag_pc is not None) and not a.vote_sv_tags:
        ap.error('--sv_tag_min and --sv_tag_pc need --vote_sv_tags')
    if a.vote_sv_tags and a.fit is not None:
        ap.error('--vote_sv_tags does not work with --fit: the exact line of an axis rests on the feature records not moving while a '
                 'constant moves, and the second run\'s records move with the first run\'s calls')
    if a.vote_sv_tags and a.join_ps:
        ap.error('--vote_sv_tags and --join_ps do not work together')
    if a.vote_sv_tags:
        try:
            _sv_tag_lists(True, a.sv_tag_min, a.sv_tag_pc)
        except ValueError as e:
            ap.error(str(e))
    return a


LEAD = ('pc_cap', 'svlen_thres', 'suppread_thres', 'cluster_max_distance', 'join_min_sv')   # the setting columns in front of a row, in this order
SV_TAG = ('sv_tag_min', 'sv_tag_pc')            # ... and behind them the settings of --vote_sv_tags, innermost; sv_tag_min 0: no second run
MARKS = ('marks_untagged', 'marks_given', 'marks_own_only')     # ... and what the second run of a row's vector did to the marks


def features_path(path, setting):
    """--features with several settings: FILE.ext -> FILE[.c<c>].s<s>.r<r>[.p<cap>][.j<join_min_sv>][.v<sv_tag_min>.q<sv_tag_pc>].ext"""
    root, ext = os.path.splitext(path)
    tag = ''.join('.%s%s' % (t, setting[n]) for t, n in (('c', 'cluster_max_distance'), ('s', 'svlen_thres'), ('r', 'suppread_thres'),
                                                         ('p', 'pc_cap'), ('j', JOIN), ('v', 'sv_tag_min'), ('q', 'sv_tag_pc')) if n in setting)
    return root + tag + ext


def main_fit(a):
    """--fit: the fitted vector -> --out_vector, the trace -> --trace, the best setting and its scores on stdout (one line)."""
    try:
        start = None
        if a.start:
            vec, cap = load_vector(a.start, with_cap=True)
            start = dict(zip(NAMES, (float(x) for x in vec)))
            if cap is not None:
                start[CAP_AXIS] = cap
        _axes(a.axes, a.fit_cap)
    except ValueError as e:
        raise SystemExit('tune: %s' % e)
    leaf = []
    got = fit(a.workdir, a.truthset, a.fit, start, a.axes, a.rounds, a.max_values, a.sv_min_size, a.min_support_read,
              a.cluster_max_distance if a.from_bams else None, a.from_bams, a.refdist, a.pctsim, a.bed_file, a.skip_phasing,
              a.include_all_ctgs, a.thread, ctx=engine.default_context(a.device), holdout=a.holdout, pc_cap=a.pc_cap, fit_cap=a.fit_cap,
              by_leaf=leaf if a.by_leaf else None, join_min_sv=a.join)
    if a.by_leaf:
        cols = tuple(n for n in LEAD if n in leaf[0]) + LEAF_COLS
        _write_tsv(a.by_leaf, cols, ([r[n] for n in cols] for r in leaf))
    if a.trace:
        lead = tuple(n for n in LEAD if n in got['trace'][0])
        cols = lead + TRACE + SCORES
        if a.holdout is not None:
            cols += tuple('%s_%s' % (part, n) for part in ('train', 'test') for n in SCORES)
        _write_tsv(a.trace, cols, ([r[n] for n in cols] for r in got['trace']))
    best = got['best']
    if best is None:
        raise SystemExit('tune: no setting has a fit (%s is nan for every vector tried, or the features report a division by zero); '
                         '%s is not written' % (a.fit, a.out_vector))
    with open(a.out_vector, 'w') as f:
        obj = dict(zip(NAMES, (float(x) for x in best['vector'])))
        if CAP_AXIS in best:
            obj['pc_cap'] = int(best[CAP_AXIS])                     # (the fitted cap)
        elif a.pc_cap is not None:
            obj['pc_cap'] = int(best['setting']['pc_cap'])          # (the 15th key: duet --thresholds applies it)
        if a.join is not None and best['setting'][JOIN] >= 1:
            obj[JOIN] = int(best['setting'][JOIN])                  # (duet --thresholds --join_ps joins with it)
        # (join_min_sv 0 fitted best: no key -- the file's key is an integer >= 1; the printed line says join_min_sv=0, and the
        # vector is meant for a run without --join_ps)
        json.dump(obj, f, indent=1)
        f.write('\n')
    at = ' '.join('%s=%s' % (n, best['setting'][n]) for n in LEAD if n in best['setting'])
    if CAP_AXIS in best:
        at += ', fitted pc_cap=%d' % best[CAP_AXIS]
    print('fit %s=%r at %s; %s -> %s' % (a.fit, best['objective'], at, ' '.join('%s=%r' % (n, best['scores'][n]) for n in best['scores']),
                                        a.out_vector))


def main(argv):
    a = parse_args(argv)
    if a.fit is not None:
        return main_fit(a)
    vecs = load_grid(a.grid)
    if a.vote_sv_tags and a.features and len(vecs) != 1:
        raise SystemExit('tune: --features with --vote_sv_tags needs a grid of exactly one vector: the features of the second run '
                         'differ per vector')
    ctx = engine.default_context(a.device)
    cs = a.cluster_max_distance if a.from_bams else None
    single = not a.from_bams and len(a.sv_min_size) == 1 and len(a.min_support_read) == 1
    plain = single and a.pc_cap is None and a.join is None and not a.vote_sv_tags

    def write_features(setting, cands):
        f = cands['feat']
        cols = ('chrom', 'pos', 'svtype', 'svlen') + tuple(n for n in _lib.FEATURE_DTYPE.names if not n.startswith('reserved'))
        _write_tsv(a.features if plain else features_path(a.features, setting), cols,
                   ([cands['chrom'][c], int(cands['pos'][c]), cands['svtype'][c], int(cands['svlen'][c])] +
                    [int(f[n][c]) for n in cols[4:]] for c in range(len(f))))

    contig_rows, leaf = [], []
    rows = sweep_settings(a.workdir, a.truthset, vecs, a.sv_min_size, a.min_support_read, cs, a.from_bams, a.refdist, a.pctsim,
                          a.bed_file, a.skip_phasing, a.include_all_ctgs, a.thread, ctx=ctx,
                          on_features=write_features if a.features else None, holdout=a.holdout,
                          by_contig=contig_rows if a.by_contig else None, pc_cap=a.pc_cap, by_leaf=leaf if a.by_leaf else None,
                          join_min_sv=a.join, vote_sv_tags=a.vote_sv_tags, sv_tag_min=a.sv_tag_min, sv_tag_pc=a.sv_tag_pc)
    # (one -s and one -r, not from the BAMs: their columns stay away, as without --pc_cap)
    lead = tuple(n for n in LEAD + SV_TAG if n in rows[0] and (n in ('pc_cap', JOIN) + SV_TAG or not single))
    cols = lead + (MARKS if a.vote_sv_tags else ()) + NAMES + SCORES
    if a.holdout is not None:
        cols += tuple('%s_%s' % (part, n) for part in ('train', 'test') for n in SCORES)
    _write_tsv(a.out, cols, ([r[n] for n in cols] for r in rows))
    if a.by_contig:
        cols = lead + ('vector', 'contig') + COUNTS + ('n_base',) + SCORES
        _write_tsv(a.by_contig, cols, ([r[n] for n in cols] for r in contig_rows))
    if a.by_leaf:
        cols = lead + LEAF_COLS
        _write_tsv(a.by_leaf, cols, ([r[n] for n in cols] for r in leaf))
    best = max(range(len(rows)), key=lambda i: -1.0 if math.isnan(rows[i]['hp_f1']) else rows[i]['hp_f1'])
    print('%d vectors scored -> %s; best phasing F1 %r at vector %d' % (len(rows), a.out, rows[best]['hp_f1'], best))


if __name__ == '__main__':
    main(sys.argv[1:])
