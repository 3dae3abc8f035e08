# coding=utf-8
"""Test-side restatement of the threshold sweep (duet_amd/tune.py, duet_amd/csrc/duet_tune.hip): predict_hp's tree
(src/duet/sv_phasing_fn.py:142-183) with the 14 constants taken from a vector, on top of oracle/ef_oracle.py's vote, and the
oracle pipeline's phased_sv.vcf text for a vector."""
import math

from duet_amd import engine
from oracle import ef_oracle as O

MARK_ABSENT = engine.MARK_ABSENT


def decide_vec(cls, svread, refread, deg, hap1, hap2, hap0, allhap, t1, t2, v):
    """predict_hp with vector v (14 floats in include/duet_ef.h's order), Python's own arithmetic and comparisons."""
    (c0_min_sv_num, c2_min_sv_ratio, c2_max_avgsc_diff, c2_min_sv_num, c2_min_hap0, lo_r, hi_r, hr_t, c1_diff, r1, r2, max_ref,
     r3, max_tot) = [float(x) for x in v]
    hapread_ratio = allhap / deg
    a1 = t1 / hap1 if hap1 > 0 else 0
    a2 = t2 / hap2 if hap2 > 0 else 0
    sv_ratio = svread / (svread + refread)
    lo, hi = min(t1, t2), max(t1, t2)
    totsc_ratio = hi / lo if lo > 0 else 0
    onehap_totsc = hi if lo == 0 else 0
    avgsc_diff = abs(a2 - a1)
    pred = 0
    if cls == 0:
        if sv_ratio == 1 and svread >= c0_min_sv_num:
            pred = 3
    elif cls == 2:
        if sv_ratio >= c2_min_sv_ratio:
            if avgsc_diff <= c2_max_avgsc_diff:
                if svread >= c2_min_sv_num:
                    pred = 3
            else:
                if hap0 >= c2_min_hap0:
                    pred = 3
    else:
        gate = hapread_ratio <= hr_t and avgsc_diff <= c1_diff or hapread_ratio > hr_t
        if onehap_totsc != 0:
            if sv_ratio <= lo_r:
                pred = 0
            elif sv_ratio <= hi_r:
                if gate:
                    pred = 1 if a1 > 0 else 2
            else:
                if gate:
                    pred = 3
        if onehap_totsc == 0:
            if sv_ratio <= r1:
                pred = 0
            elif sv_ratio <= r2:
                pred = 0 if refread > max_ref else (1 if t1 > t2 else 2)
            elif sv_ratio <= r3:
                pred = 3 if totsc_ratio <= max_tot else (1 if t1 > t2 else 2)
            else:
                pred = 3
    return pred


def decide_cd(cd, cls, seeds, v):
    hap1, hap2, hap0, allhap, t1, t2, ps = O.vote(cd, cls, seeds)
    return decide_vec(cls, cd.svread, cd.refread, len(cd.marks), hap1, hap2, hap0, allhap, t1, t2, v), ps


def soa_candidates(soa):
    """EfSoA -> oracle Candidates (marks as (hap, ps, pc) or None), contig index per candidate."""
    tags = soa.read_tag
    out = []
    for k in range(soa.n_contigs):
        for c in range(int(soa.cand_ctg_off[k]), int(soa.cand_ctg_off[k + 1])):
            cd = O.Candidate()
            cd.contig_index = k
            cd.pos, cd.svlen, cd.svread, cd.refread = (int(soa.cand_pos[c]), int(soa.cand_svlen[c]), int(soa.cand_svread[c]),
                                                       int(soa.cand_refread[c]))
            cd.gt = '0/1' if soa.cand_gt_ok[c] else './.'
            marks = []
            for m in soa.mark_read[soa.cand_off[c]:soa.cand_off[c + 1]]:
                if int(m) == MARK_ABSENT:
                    marks.append(None)
                else:
                    t = int(tags[int(m)])
                    marks.append((t >> 62, t & 0xFFFFFFFF, (t >> 32) & 0x3FFFFFFF))
            cd.marks = marks
            out.append(cd)
    return out


def oracle_features(soa, svlen_thres, suppread_thres):
    """Per candidate: dict(kept, eligible, cls, hap1, hap2, hap0, allhap, t1, t2, ps, deg, svread, refread), by ef_oracle's
    filter, class, seed sets and vote."""
    cds = soa_candidates(soa)
    kept = [O.passes_filter(cd, svlen_thres, suppread_thres) for cd in cds]
    cls = [O.ps_class(cd) if k else 0 for cd, k in zip(cds, kept)]
    seeds = [set() for _ in range(soa.n_contigs)]
    for cd, k, p in zip(cds, kept, cls):
        if k and p == 1:
            s = O.seed_ps(cd)
            if s is not None:
                seeds[cd.contig_index].add(s)
    out = []
    for cd, k, p in zip(cds, kept, cls):
        r = dict(kept=int(k), eligible=int(k and bool(seeds[cd.contig_index])), cls=p, hap1=0, hap2=0, hap0=0, allhap=0, t1=0, t2=0,
                 ps=0, deg=len(cd.marks), svread=cd.svread, refread=cd.refread)
        if r['eligible']:
            r['hap1'], r['hap2'], r['hap0'], r['allhap'], r['t1'], r['t2'], r['ps'] = O.vote(cd, p, seeds[cd.contig_index])
            r['ps'] = int(r['ps'])
        out.append(r)
    return out


def preds_from_features(feat, v):
    """The restated tree over a FEATURE_DTYPE array -> list of pred."""
    out = []
    for f in feat:
        if not f['eligible']:
            out.append(0)
            continue
        out.append(decide_vec(int(f['cls']), int(f['svread']), int(f['refread']), int(f['deg']), int(f['hap1']), int(f['hap2']),
                              int(f['hap0']), int(f['allhap']), int(f['t1']), int(f['t2']), v))
    return out


def phased_text(home, svlen_thres, suppread_thres, v, include_all_ctgs=False):
    """The oracle pipeline's phased_sv.vcf for vector v: ef_oracle.phase_callset with decide_cd in place of decide."""
    chroms = O.chrom_list(include_all_ctgs)
    toks = O.tokenise(home + '/sv_calling/variants.vcf')
    head = O.header_text(toks, chroms, include_all_ctgs)
    callset = O.build_callset(toks, chroms, O.load_tag_tables(home + '/snp_phasing', chroms))
    kept = [O.passes_filter(cd, svlen_thres, suppread_thres) for cd in callset]
    cls = [O.ps_class(cd) if k else None for cd, k in zip(callset, kept)]
    spell = [('chr' + c, c) for c in chroms]
    seeds = [set() for _ in chroms]
    for ctg in range(len(chroms)):
        for cd, k, p in zip(callset, kept, cls):
            if k and p == 1 and cd.chrom in spell[ctg]:
                s = O.seed_ps(cd)
                if s is not None:
                    seeds[ctg].add(s)
    rows = []
    for ctg in range(len(chroms)):
        if not seeds[ctg]:
            continue
        for want in (0, 1, 2):
            for i, cd in enumerate(callset):
                if cd.chrom not in spell[ctg] or not kept[i] or cls[i] != want:
                    continue
                pred, ps = decide_cd(cd, want, seeds[ctg], v)
                if pred == 0:
                    continue
                signed = cd.svlen if cd.svtype in ('INS', 'DUP') else -cd.svlen
                rows.append(dict(ps=ps, hp=O.HP_TEXT[pred], chrom=cd.chrom, pos=cd.pos, svlen=signed, svtype=cd.svtype, ref=cd.ref,
                                 alt=cd.alt))
    rows.sort(key=lambda r: (r['chrom'], r['pos']))
    return head + O.rows_text(rows)


def same_floats(a, b):
    return len(a) == len(b) and all((math.isnan(x) and math.isnan(y)) or x == y for x, y in zip(a, b))
