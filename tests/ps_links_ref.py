# coding=utf-8
"""The phase-set links (include/duet_ef.h: duet_ps_links_device) in plain Python: loops and dicts, one
step of the rule per block.  The one reference of tests/test_ps_links_host.py and tests/test_gpu_ps_links.py; `blocks` restates
duet_amd/ps_links.py: blocks independently (parity labels and a search per link in place of a union-find)."""
import numpy as np

ABSENT = 0xFFFFFFFF
UNTAGGED = 0xFFFFFFFFFFFFFFFF
PC_MAX = 8100
FIELDS = ('w_same', 'w_flip', 'contig', 'ps_a', 'ps_b', 'n_sv', 'n_same', 'n_flip', 'n_open', 'pos_min', 'pos_max', 'reserved')
COLUMNS = ('CHROM', 'PS_A', 'PS_B', 'N_SV', 'N_SAME', 'N_FLIP', 'N_OPEN', 'W_SAME', 'W_FLIP', 'POS_MIN', 'POS_MAX', 'VERDICT')


def groups_of(soa, c, pc_cap):
    """{ps: [h1, h2]} over the voting marks of candidate c."""
    groups = {}
    for m in range(int(soa.cand_off[c]), int(soa.cand_off[c + 1])):
        r = int(soa.mark_read[m])
        if r == ABSENT or r >= len(soa.read_tag):
            continue
        t = int(soa.read_tag[r])
        if t == UNTAGGED:
            continue
        hap, pc, ps = t >> 62, (t >> 32) & 0x3FFFFFFF, t & 0xFFFFFFFF
        if pc > pc_cap or hap not in (1, 2):
            continue
        groups.setdefault(ps, [0, 0])[hap - 1] += 1
    return groups


def observation(ga, gb):
    """(kind, weight) of two neighbouring groups [h1, h2]."""
    da, db = ga[0] - ga[1], gb[0] - gb[1]
    if da == 0 or db == 0:
        return 'open', 0
    return ('same' if (da > 0) == (db > 0) else 'flip'), min(abs(da), abs(db))


def links(soa, svlen_thres, suppread_thres, pc_cap=PC_MAX):
    """-> the records as a list of dicts (FIELDS), ascending by (contig, ps_a, ps_b)."""
    recs = {}
    for k in range(len(soa.cand_ctg_off) - 1):
        for c in range(int(soa.cand_ctg_off[k]), int(soa.cand_ctg_off[k + 1])):
            if not (int(soa.cand_svlen[c]) >= svlen_thres and int(soa.cand_svread[c]) >= suppread_thres and int(soa.cand_gt_ok[c]) != 0):
                continue
            groups = groups_of(soa, c, pc_cap)
            pss = sorted(groups)
            pos = int(soa.cand_pos[c])
            for a, b in zip(pss, pss[1:]):
                kind, w = observation(groups[a], groups[b])
                r = recs.setdefault((k, a, b), dict(w_same=0, w_flip=0, contig=k, ps_a=a, ps_b=b, n_sv=0, n_same=0, n_flip=0, n_open=0,
                                                    pos_min=pos, pos_max=pos, reserved=0))
                r['n_sv'] += 1
                r['n_' + kind] += 1
                if kind != 'open':
                    r['w_' + kind] += w
                r['pos_min'], r['pos_max'] = min(r['pos_min'], pos), max(r['pos_max'], pos)
    return [recs[key] for key in sorted(recs)]


def n_multi(soa, svlen_thres, suppread_thres, pc_cap=PC_MAX):
    """How many observations there are (candidates with G groups give G - 1)."""
    return sum(r['n_sv'] for r in links(soa, svlen_thres, suppread_thres, pc_cap))


def records(recs, dtype):
    """The list of dicts as a structured array of `dtype` (duet_amd._lib.PS_LINK_DTYPE)."""
    out = np.zeros(len(recs), dtype=dtype)
    for i, r in enumerate(recs):
        for f in FIELDS:
            out[f][i] = r[f]
    return out


def verdict(r):
    a, b = (int(r['n_same']), int(r['w_same'])), (int(r['n_flip']), int(r['w_flip']))
    return 'same' if a > b else ('flip' if b > a else '.')


def header():
    return '\t'.join(COLUMNS) + '\n'


def rows_text(recs, chrom_texts):
    out = []
    for r in recs:
        out.append('%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n' % (
            chrom_texts[int(r['contig'])], r['ps_a'], r['ps_b'], r['n_sv'], r['n_same'], r['n_flip'], r['n_open'], r['w_same'], r['w_flip'],
            r['pos_min'], r['pos_max'], verdict(r)))
    return ''.join(out)


def blocks(recs):
    """-> (rows [(contig, ps, block, flip)] ascending by (contig, ps), conflicts [row indices in the order they were met]).
    Links with a verdict, strongest first; each node carries (component label, parity); a link between two components relabels
    the second one, a link inside one component must agree with the parities or it is a conflict."""
    order = []
    for i, r in enumerate(recs):
        v = verdict(r)
        if v == '.':
            continue
        n_win, w_win = (int(r['n_same']), int(r['w_same'])) if v == 'same' else (int(r['n_flip']), int(r['w_flip']))
        order.append((-n_win, -w_win, i, 0 if v == 'same' else 1))
    order.sort()
    comp, par = {}, {}                                  # node (contig, ps) -> component id, parity relative to the component's first node
    for r in recs:
        for ps in (int(r['ps_a']), int(r['ps_b'])):
            node = (int(r['contig']), ps)
            if node not in comp:
                comp[node], par[node] = len(comp), 0
    conflicts = []
    for _, _, i, sense in order:
        r = recs[i]
        a, b = (int(r['contig']), int(r['ps_a'])), (int(r['contig']), int(r['ps_b']))
        if comp[a] == comp[b]:
            if par[a] ^ par[b] != sense:
                conflicts.append(i)
            continue
        shift, old, new = par[a] ^ par[b] ^ sense, comp[b], comp[a]
        for node in comp:
            if comp[node] == old:
                comp[node], par[node] = new, par[node] ^ shift
    rows = []
    for node in sorted(comp):
        members = [m for m in comp if comp[m] == comp[node]]
        root = min(members)
        rows.append((node[0], node[1], root[1], par[node] ^ par[root]))
    return rows, conflicts


def blocks_text(rows, chrom_texts):
    return ''.join('%s\t%d\t%d\t%d\n' % (chrom_texts[k], ps, block, flip) for k, ps, block, flip in rows)
