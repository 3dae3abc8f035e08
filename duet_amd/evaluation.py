#!/usr/bin/env python3
# coding=utf-8
"""Accuracy evaluator for phased SV callsets (restatement of src/scripts/evaluation.py).

Same command line and the same ten numbers: precision / recall / F1 of SV calling, genotyping and phasing of a
callset against a truth set, each call matched to the NEAREST same-type truth call of its contig (ties to the
right-hand neighbour, evaluation.py:117-125) within --refdist and a length ratio of at least --pctsim, phasing
scored per phase set with the better of the two haplotype labelings (evaluation.py:143-148).

Differences in form only: records are flattened into per-(contig, type) position-sorted numpy arrays once, and
each phase set is matched with one vectorised `searchsorted` instead of Python loops over dicts.

`evaluation_gpu` is the same scoring on the MI355X (duet_eval_run_host, duet_amd/csrc/duet_eval.hip): the host flattens the
parsed records (`flatten`), the device matches, builds the id sets and picks each phase set's labelling, and the six set
sizes come back; the ten numbers are the same binary64 quotients.  `--gpu` on the command line selects it.

`details` says what was scored, per record: for every call the truth record it was compared with, the distance, each test and
the labelling its phase-set group took; for every truth record how many calls hit it, its nearest call and, when it was missed,
why (include/duet_ef.h: duet_eval_call_rec, duet_eval_base_rec).  With a context the records come from the device
(duet_eval_details_host), without one from `details_host`, the same rule in numpy and plain Python.  `--details PREFIX` writes
them as PREFIX.calls.tsv and PREFIX.truth.tsv (`details_text`).
"""

import argparse
import sys

import numpy as np

LABELS = [str(i) for i in range(1, 23)] + ['X', 'Y']
CHROMS = ['chr' + c for c in LABELS]
_ALT_TYPES = ('<INS>', '<DEL>', '<DUP:TANDEM>', '<DUP:INT>', '<DUP>')


def _tokens(path):
    with open(path, 'r') as fh:
        return [ln.strip().split() for ln in fh]


def parse_bed(path):
    """Per contig: list of closed integer ranges (evaluation.py:25-33)."""
    spans = {c: [] for c in LABELS}
    for t in _tokens(path):
        if t[0][:3] == 'chr' and t[0][3:] in spans:
            spans[t[0][3:]].append((int(t[1]), int(t[2])))
    return spans


def parse_vcf(vcf_path, skip_phasing, bed_path=''):
    """-> list of dicts {chr, pos, id, hp, ps, len, type}, file order (evaluation.py:35-97)."""
    bed = parse_bed(bed_path) if bed_path != '' else None
    out = []
    for s in _tokens(vcf_path):
        if s[0][0] == '#':
            continue
        if s[0][3:] not in LABELS:          # whatever the first three characters are (evaluation.py:43)
            continue
        if 'SVLEN=.' in s[7]:
            continue
        if not any(k in s[7] or k in s[4] for k in ('INS', 'DEL', 'DUP')):
            continue
        hp = s[-1][:3]
        if hp[0] == '.':
            hp = '0' + hp[1:]
        if hp[2] == '.':
            hp = hp[:2] + '0'
        if hp[1] == '/':
            if not skip_phasing and hp != '1/1':
                continue
            hp = hp[0] + '|' + hp[2]
            ps = s[0]
        else:
            ps = s[0] + '_' + s[-1][s[-1].rfind(':'):]
        rec = {'chr': s[0], 'pos': int(s[1]), 'id': s[2] + s[0] + s[1], 'hp': hp, 'ps': ps}
        items = s[7].split(';')
        if 'SVLEN' in s[7]:
            item = [x for x in items if 'SVLEN' in x][0]
            rec['len'] = abs(int(item[7:])) if 'SVLEN=>' in s[7] else abs(int(item[6:]))
            rec['type'] = s[4][1:-1] if s[4] in _ALT_TYPES else [x for x in items if 'SVTYPE' in x][0][7:]
            if 'DUP' in rec['type']:
                rec['type'] = 'INS'
        else:
            d = len(s[3]) - len(s[4])
            if d > 0:
                rec['len'], rec['type'] = d, 'DEL'
            if d < 0:
                rec['len'], rec['type'] = -d, 'INS'
        if bed is not None:
            p = int(s[1])
            if not any(a <= p <= b for a, b in bed[s[0][3:]]):
                continue
        if rec['len'] < 50 or rec['hp'] == '0|0':                     # KeyError for equal-length REF/ALT, as upstream
            continue
        out.append(rec)
    return out


def _nearest(base_pos, call_pos):
    """Index of the nearest base position per call; ties and the insertion point rule of evaluation.py:117-125."""
    idx = np.searchsorted(base_pos, call_pos)
    n = len(base_pos)
    if n == 0:
        raise IndexError('list index out of range')                   # upstream indexes the empty truth list
    at_end = idx == n
    left = np.maximum(idx - 1, 0)
    right = np.minimum(idx, n - 1)
    take_left = at_end | ((idx > 0) & (np.abs(call_pos - base_pos[right]) > np.abs(call_pos - base_pos[left])))
    return np.where(take_left, left, right)


def evaluation(baseinfo, callinfo, threshold_tp_range, ratio):
    call_tp, call_gt, call_hp, base_tp, base_gt, base_hp = set(), set(), set(), set(), set(), set()
    avg_sv_num = len(callinfo) / len(set(s['ps'] for s in callinfo))
    for chrom in CHROMS:
        base = {}
        for svtype in ('INS', 'DEL'):
            rows = sorted((s for s in baseinfo if s['chr'] == chrom and s['type'] == svtype), key=lambda r: r['pos'])
            base[svtype] = (rows, np.array([r['pos'] for r in rows], dtype=np.int64),
                            np.array([r['len'] for r in rows], dtype=np.int64))
        on_chrom = [s for s in callinfo if s['chr'] == chrom]
        for ps in set(s['ps'] for s in on_chrom):
            same_c, same_b, flip_c, flip_b = set(), set(), set(), set()
            for svtype in ('INS', 'DEL'):
                calls = [s for s in on_chrom if s['ps'] == ps and s['type'] == svtype]
                if not calls:
                    continue
                rows, bpos, blen = base[svtype]
                cpos = np.array([c['pos'] for c in calls], dtype=np.int64)
                clen = np.array([c['len'] for c in calls], dtype=np.int64)
                j = _nearest(bpos, cpos)
                ok = (np.abs(cpos - bpos[j]) <= threshold_tp_range) & \
                     (np.minimum(clen, blen[j]) / np.maximum(clen, blen[j]) >= ratio)
                for ci in np.nonzero(ok)[0]:
                    c, b = calls[int(ci)], rows[int(j[ci])]
                    call_tp.add(c['id'])
                    base_tp.add(b['id'])
                    het = ('1|0', '0|1')
                    if (c['hp'] in het and b['hp'] in het) or c['hp'] == b['hp'] == '1|1':
                        call_gt.add(c['id'])
                        base_gt.add(b['id'])
                    if c['hp'] == b['hp']:
                        same_c.add(c['id'])
                        same_b.add(b['id'])
                    if c['hp'] == b['hp'] == '1|1' or (c['hp'], b['hp']) in (('0|1', '1|0'), ('1|0', '0|1')):
                        flip_c.add(c['id'])
                        flip_b.add(b['id'])
            if len(same_c) + len(same_b) > len(flip_c) + len(flip_b):
                call_hp |= same_c
                base_hp |= same_b
            else:
                call_hp |= flip_c
                base_hp |= flip_b

    def prf(tp_c, tp_b):
        p, r = len(tp_c) / len(callinfo), len(tp_b) / len(baseinfo)
        return p, r, 2 * p * r / (p + r)

    return (avg_sv_num,) + prf(call_tp, base_tp) + prf(call_gt, base_gt) + prf(call_hp, base_hp)


_HP_FIXED = {'1|0': 0, '0|1': 1, '1|1': 2}


def flatten(baseinfo, callinfo):
    """The parsed records as the flat arrays of include/duet_ef.h's duet_eval_problem.  Raises IndexError where upstream
    indexes an empty truth list (a call whose (contig, type) has no truth record, evaluation.py:120-125)."""
    return flatten_rows(baseinfo, callinfo)[0]


def flatten_rows(baseinfo, callinfo):
    """-> (the arrays of `flatten`, the truth records in the order of the base arrays, the calls in the order of the call arrays)"""
    hp_code = dict(_HP_FIXED)

    def code(hp):
        if hp not in hp_code:
            hp_code[hp] = len(hp_code)
            if len(hp_code) > 255:
                raise ValueError('more than 255 distinct haplotype strings')
        return hp_code[hp]

    types = {'INS': 0, 'DEL': 1}
    contig = {c: k for k, c in enumerate(CHROMS)}
    base_uid, call_uid, groups = {}, {}, {}
    lists = [[] for _ in range(2 * len(CHROMS))]
    for r in baseinfo:
        base_uid.setdefault(r['id'], len(base_uid))
        if r['chr'] in contig and r['type'] in types:
            lists[2 * contig[r['chr']] + types[r['type']]].append(r)
    base_off = np.zeros(len(lists) + 1, dtype=np.int64)
    rows = []
    for i, lst in enumerate(lists):
        lst.sort(key=lambda r: r['pos'])                 # stable, like sorted(..., key=itemgetter('pos')) upstream
        rows.extend(lst)
        base_off[i + 1] = len(rows)
    a = dict(base_off=base_off, base_pos=[r['pos'] for r in rows], base_len=[r['len'] for r in rows],
             base_uid=[base_uid[r['id']] for r in rows], base_hp=[code(r['hp']) for r in rows])
    ck, cp, cl, cu, cg, ch, scored = [], [], [], [], [], [], []
    for r in callinfo:
        call_uid.setdefault(r['id'], len(call_uid))
        if r['chr'] not in contig:
            continue
        g = groups.setdefault((r['chr'], r['ps']), len(groups))
        if r['type'] not in types:
            continue
        key = 2 * contig[r['chr']] + types[r['type']]
        if base_off[key + 1] == base_off[key]:
            raise IndexError('list index out of range')
        ck.append(key); cp.append(r['pos']); cl.append(r['len']); cu.append(call_uid[r['id']]); cg.append(g); ch.append(code(r['hp'])); scored.append(r)
    a.update(call_key=ck, call_pos=cp, call_len=cl, call_uid=cu, call_group=cg, call_hp=ch, n_groups=len(groups),
             n_base_uid=len(base_uid), n_call_uid=len(call_uid))
    for k in ('base_pos', 'base_len', 'call_pos', 'call_len'):
        v = np.asarray(a[k], dtype=np.int64)
        if v.size and (int(v.min()) < 0 or int(v.max()) > 0xFFFFFFFF):
            raise ValueError(k + ' outside the 32-bit range of the device arrays')
    return a, rows, scored


def evaluation_gpu(baseinfo, callinfo, threshold_tp_range, ratio, ctx=None):
    """evaluation() on the GPU: same ten numbers, same exceptions."""
    from duet_amd import engine
    avg_sv_num = len(callinfo) / len(set(s['ps'] for s in callinfo))
    a = flatten(baseinfo, callinfo)
    if ctx is None:
        ctx = engine.default_context()
    if threshold_tp_range < 0:
        a['call_key'] = []                               # abs(...) <= negative never holds: nothing matches
        for k in ('call_pos', 'call_len', 'call_uid', 'call_group', 'call_hp'):
            a[k] = []
    n = ctx.eval_counts(a, max(int(threshold_tp_range), 0), ratio)

    def prf(tp_c, tp_b):
        p, r = tp_c / len(callinfo), tp_b / len(baseinfo)
        return p, r, 2 * p * r / (p + r)

    return (avg_sv_num,) + prf(n.call_tp, n.base_tp) + prf(n.call_gt, n.base_gt) + prf(n.call_hp, n.base_hp)


CALL_COLUMNS = ('CHROM', 'POS', 'ID', 'TYPE', 'LEN', 'HP', 'GROUP', 'T_POS', 'T_ID', 'T_LEN', 'T_HP', 'DIST', 'MATCHED', 'GT', 'REL',
                'LABEL', 'HP_OK')
TRUTH_COLUMNS = ('CHROM', 'POS', 'ID', 'TYPE', 'LEN', 'HP', 'N_CALLS', 'N_GT', 'N_HP', 'C_POS', 'C_ID', 'C_DIST', 'REASON')


def details_host(a, refdist, ratio):
    """The records of include/duet_ef.h's duet_eval_details_host from the flat arrays of `flatten`, on the host: the rule of
    evaluation.py:99-148 kept per record, and the nearest call of every truth record.  -> (the six counts in the order of
    duet_eval_counts, calls EVAL_CALL_DTYPE[n_calls], base EVAL_BASE_DTYPE[n_base])"""
    from duet_amd import _lib as L
    i64 = lambda k: np.asarray(a[k], dtype=np.int64)
    off, bpos, blen, buid, bhp = i64('base_off'), i64('base_pos'), i64('base_len'), i64('base_uid'), i64('base_hp')
    ckey, cpos, clen, cuid, cgrp, chp = (i64(k) for k in ('call_key', 'call_pos', 'call_len', 'call_uid', 'call_group', 'call_hp'))
    nb, nc = len(bpos), len(cpos)
    refdist, ratio = int(refdist), float(ratio)
    calls = np.zeros(nc, dtype=L.EVAL_CALL_DTYPE)
    base = np.zeros(nb, dtype=L.EVAL_BASE_DTYPE)
    listed = ckey != L.EVAL_NONE
    # the call side: the nearest record of the call's list (:117-125), the two tests (:126-127), the haplotype tests (:130-139)
    j = np.zeros(nc, dtype=np.int64)
    for key in np.unique(ckey[listed]):
        at = np.nonzero(ckey == key)[0]
        lo, hi = int(off[key]), int(off[key + 1])
        j[at] = lo + _nearest(bpos[lo:hi], cpos[at])
    dist = np.abs(cpos - bpos[j]) if nb else np.zeros(nc, dtype=np.int64)
    near = listed & (dist <= refdist)
    with np.errstate(divide='ignore', invalid='ignore'):
        size = listed & ((np.minimum(clen, blen[j]) / np.maximum(clen, blen[j]) >= ratio) if nb else np.zeros(nc, dtype=bool))
    matched = near & size
    th = bhp[j] if nb else np.zeros(nc, dtype=np.int64)
    gt = matched & (((chp < 2) & (th < 2)) | ((chp == 2) & (th == 2)))
    same = matched & (chp == th)
    flip = matched & (((chp == 2) & (th == 2)) | ((chp == 1) & (th == 0)) | ((chp == 0) & (th == 1)))
    # the labelling of every phase-set group (:140-145): sets of ids, call side plus truth side; a tie goes to "flip"
    sets = {}
    for c in np.nonzero(same | flip)[0]:
        s = sets.setdefault(int(cgrp[c]), (set(), set(), set(), set()))
        if same[c]:
            s[0].add(int(cuid[c])); s[1].add(int(buid[j[c]]))
        if flip[c]:
            s[2].add(int(cuid[c])); s[3].add(int(buid[j[c]]))
    label = np.ones(int(a['n_groups']) if nc == 0 else max(int(a['n_groups']), int(cgrp.max()) + 1), dtype=np.int64)
    for g, s in sets.items():
        if len(s[0]) + len(s[1]) > len(s[2]) + len(s[3]):
            label[g] = 0
    flipped = label[cgrp] == 1
    hp = matched & np.where(flipped, flip, same)
    calls['base'] = np.where(listed, j, L.EVAL_NONE)
    calls['dist'] = np.where(listed, dist, L.EVAL_NONE)
    for bit, on in ((L.EVAL_NEAR, near), (L.EVAL_SIZE, size), (L.EVAL_MATCHED, matched), (L.EVAL_GT, gt), (L.EVAL_SAME, same),
                    (L.EVAL_FLIP, flip), (L.EVAL_LABEL, flipped), (L.EVAL_HP, hp)):
        calls['bits'] |= np.where(on, bit, 0).astype(np.uint32)
    # the truth side: how many calls were counted at the record, and the nearest call of its list -- smallest distance, then the
    # smaller position, then the smaller index
    for field, on in (('n_calls', matched), ('n_gt', gt), ('n_hp', hp)):
        base[field] = np.bincount(j[on], minlength=nb)
    base['nearest'] = base['nearest_dist'] = L.EVAL_NONE
    for key in range(len(off) - 1):
        lo, hi = int(off[key]), int(off[key + 1])
        at = np.nonzero(ckey == key)[0]
        if hi == lo or len(at) == 0:
            continue
        at = at[np.argsort(cpos[at], kind='stable')]              # by (pos, index)
        sp, bp = cpos[at], bpos[lo:hi]
        i = np.searchsorted(sp, bp, side='left')
        right = np.minimum(i, len(sp) - 1)
        left = np.searchsorted(sp, sp[np.maximum(i - 1, 0)], side='left')        # the first call of the run below the record
        d_right = np.where(i < len(sp), np.abs(sp[right] - bp), np.int64(1) << 40)
        d_left = np.where(i > 0, np.abs(bp - sp[left]), np.int64(1) << 40)
        take_left = d_left <= d_right
        base['nearest'][lo:hi] = at[np.where(take_left, left, right)]
        base['nearest_dist'][lo:hi] = np.where(take_left, d_left, d_right)
    n = base['nearest'].astype(np.int64)
    has = n != L.EVAL_NONE
    nn = np.where(has, n, 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        fits = (np.minimum(clen[nn], blen) / np.maximum(clen[nn], blen) >= ratio) if nc else np.zeros(nb, dtype=bool)
    reason = np.where(~has, 0, np.where(base['nearest_dist'].astype(np.int64) > refdist, 1, np.where(~fits, 2, 3)))
    base['reason'] = np.where(base['n_calls'] > 0, L.EVAL_HIT, reason)
    counts = tuple(len(set(ids[on].tolist())) for ids, on in ((cuid, matched), (buid[j] if nb else cuid, matched), (cuid, gt),
                                                             (buid[j] if nb else cuid, gt), (cuid, hp), (buid[j] if nb else cuid, hp)))
    return counts, calls, base


def _details_problem(baseinfo, callinfo, refdist, ratio):
    if refdist < 0:
        raise ValueError('a negative refdist matches nothing: there is no outcome to detail')       # (evaluation() divides by zero)
    a, rows, scored = flatten_rows(baseinfo, callinfo)
    a['refdist'], a['ratio'] = int(refdist), float(ratio)
    return a, rows, scored


def details(baseinfo, callinfo, refdist, ratio, ctx=None):
    """What was scored, per record: (calls EVAL_CALL_DTYPE, base EVAL_BASE_DTYPE) in the order of flatten_rows' calls and truth
    records.  With a context the records come from the device, without one from details_host.  Raises what flatten raises."""
    a = _details_problem(baseinfo, callinfo, refdist, ratio)[0]
    return (ctx.eval_details_host(a) if ctx is not None else details_host(a, refdist, ratio))[1:]


def details_text(rows, scored, calls, base):
    """The two tables as text, header line first: one row per scored call in callset order and one per scored truth record in the
    order of the base arrays (contig, type, position).  rows, scored: flatten_rows' records; calls, base: `details`' records."""
    from duet_amd import _lib as L
    rel = {0: '.', L.EVAL_SAME: 'same', L.EVAL_FLIP: 'flip', L.EVAL_SAME | L.EVAL_FLIP: 'both'}
    flag = lambda bits, bit: '1' if bits & bit else '0'
    out_c = ['\t'.join(CALL_COLUMNS) + '\n']
    for r, rec in zip(scored, calls):
        bits, t = int(rec['bits']), rows[int(rec['base'])]
        out_c.append('\t'.join([r['chr'], str(r['pos']), r['id'], r['type'], str(r['len']), r['hp'], r['ps'], str(t['pos']), t['id'],
                                str(t['len']), t['hp'], str(int(rec['dist'])), flag(bits, L.EVAL_MATCHED), flag(bits, L.EVAL_GT),
                                rel[bits & (L.EVAL_SAME | L.EVAL_FLIP)], 'flip' if bits & L.EVAL_LABEL else 'same',
                                flag(bits, L.EVAL_HP)]) + '\n')
    out_t = ['\t'.join(TRUTH_COLUMNS) + '\n']
    for t, rec in zip(rows, base):
        if int(rec['nearest']) == L.EVAL_NONE:
            near = ['.', '.', '.']
        else:
            c = scored[int(rec['nearest'])]
            near = [str(c['pos']), c['id'], str(int(rec['nearest_dist']))]
        reason = '.' if int(rec['reason']) == L.EVAL_HIT else L.EVAL_REASON_NAMES[int(rec['reason'])]
        out_t.append('\t'.join([t['chr'], str(t['pos']), t['id'], t['type'], str(t['len']), t['hp'], str(int(rec['n_calls'])),
                                str(int(rec['n_gt'])), str(int(rec['n_hp']))] + near + [reason]) + '\n')
    return ''.join(out_c), ''.join(out_t)


def write_details(prefix, baseinfo, callinfo, refdist, ratio, ctx=None):
    """PREFIX.calls.tsv and PREFIX.truth.tsv; the records are complete before either file is created."""
    a, rows, scored = _details_problem(baseinfo, callinfo, refdist, ratio)
    calls, base = (ctx.eval_details_host(a) if ctx is not None else details_host(a, refdist, ratio))[1:]
    text = details_text(rows, scored, calls, base)
    for suffix, t in zip(('.calls.tsv', '.truth.tsv'), text):
        with open(prefix + suffix, 'w') as out:
            out.write(t)


def parse_args(argv):
    ap = argparse.ArgumentParser(description='precision / recall / F1 of SV calling, genotyping and phasing against a truth set')
    ap.add_argument('callset', type=str, help='VCF of phased SV calls to score')
    ap.add_argument('truthset', type=str, help='VCF of the phased truth set')
    ap.add_argument('-r', '--refdist', type=int, default=1000,
                    help='a call matches a truth call at most this many bp away [%(default)s]')
    ap.add_argument('-p', '--pctsim', type=float, default=0,
                    help='minimum shorter/longer SV length ratio for a match [%(default)s]')
    ap.add_argument('-b', '--bed_file', type=str, help='BED file; only calls inside its regions are scored')
    ap.add_argument('--skip_phasing', action='store_true',
                    help='score calling and genotyping only')
    ap.add_argument('--gpu', action='store_true', help='score on the MI355X (libduet_ef.so) instead of with numpy')
    ap.add_argument('--details', metavar='PREFIX', type=str,
                    help='also write PREFIX.calls.tsv and PREFIX.truth.tsv: what was scored, per call and per truth record')
    return ap.parse_args(argv)


def main(argv):
    args = parse_args(argv)
    bed = args.bed_file or ''
    truth, calls = (parse_vcf(path, args.skip_phasing, bed) for path in (args.truthset, args.callset))
    res = (evaluation_gpu if args.gpu else evaluation)(truth, calls, args.refdist, args.pctsim)
    # upstream's report lines, verbatim (evaluation.py:184-189)
    if not args.skip_phasing:
        print('Average SV number per phase set is', res[0])
    for what, at in (('calling', 1), ('genotyping', 4), ('phasing', 7)):
        if what == 'phasing' and args.skip_phasing:
            continue
        print('The precision, recall and F1 score of SV %s are' % what, res[at], res[at + 1], res[at + 2])
    if args.details:
        ctx = None
        if args.gpu:
            from duet_amd import engine
            ctx = engine.default_context()
        write_details(args.details, truth, calls, args.refdist, args.pctsim, ctx)


if __name__ == '__main__':
    main(sys.argv[1:])
