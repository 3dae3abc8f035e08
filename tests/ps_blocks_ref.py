# coding=utf-8
"""The round-based build of the blocks (include/duet_ef.h: duet_ps_blocks_device) in plain Python: what the
device does, stated without its kernels, to be held equal to duet_amd/ps_links.py: blocks -- the normative text -- and the seeded
random multigraph records both tests draw their cases from."""
import random

import numpy as np

from duet_amd import _lib


def verdict(r):
    same, flip = (int(r['n_same']), int(r['w_same'])), (int(r['n_flip']), int(r['w_flip']))
    return 0 if same > flip else (1 if flip > same else None)


def ranked(records, min_sv):
    """The trusted links in the strict order (-n_win, -w_win, row index) -> [(node a, node b, sense, row index)], the nodes"""
    nodes = sorted({(int(r['contig']), int(r[k])) for r in records for k in ('ps_a', 'ps_b')})
    index = {node: i for i, node in enumerate(nodes)}
    order = []
    for i, r in enumerate(records):
        v = verdict(r)
        if v is None:
            continue
        side = 'same' if v == 0 else 'flip'
        if int(r['n_' + side]) >= min_sv:
            order.append((-int(r['n_' + side]), -int(r['w_' + side]), i, v))
    order.sort()
    k = lambda i: int(records[i]['contig'])
    return [(index[(k(i), int(records[i]['ps_a']))], index[(k(i), int(records[i]['ps_b']))], s, i) for _, _, i, s in order], nodes


def has_tie(records, min_sv):
    """Two trusted links that only the row index tells apart."""
    keys = [(-int(r['n_same' if verdict(r) == 0 else 'n_flip']), -int(r['w_same' if verdict(r) == 0 else 'w_flip']))
            for r in records if verdict(r) is not None and int(r['n_same' if verdict(r) == 0 else 'n_flip']) >= min_sv]
    return len(set(keys)) < len(keys)


def blocks(records, min_sv=1):
    """-> (rows, conflicts, rounds): rounds in which every component takes its best-ranked outgoing link; a root hangs itself under
    the root at the other end with the parity the link implies, and of two roots that chose one link the smaller index stays;
    the trees are flattened before the next round; at the end every component is re-rooted at its smallest node."""
    links, nodes = ranked(records, min_sv)
    N = len(nodes)
    parent, par = list(range(N)), [0] * N       # flat between rounds: parent[x] is the root of x, par[x] the sense of x relative to it
    in_forest = [False] * len(links)
    rounds = 0
    while True:
        best = {}
        for rank, (a, b, s, _) in enumerate(links):
            if parent[a] != parent[b]:
                for root in (parent[a], parent[b]):
                    best[root] = min(best.get(root, rank), rank)
        if not best:
            break
        rounds += 1
        new_parent, new_par = list(parent), list(par)
        for v, rank in best.items():
            a, b, s, _ = links[rank]
            other = parent[b] if parent[a] == v else parent[a]
            if best.get(other) == rank and v < other:
                continue
            new_parent[v], new_par[v] = other, par[a] ^ par[b] ^ s
            in_forest[rank] = True
        parent, par = list(new_parent), list(new_par)
        for x in range(N):                     # flatten (the device jumps pointers; the result is the same)
            acc, y = 0, x
            while parent[y] != y:
                acc ^= par[y]
                y = parent[y]
            new_parent[x], new_par[x] = y, acc
        parent, par = list(new_parent), list(new_par)
    smallest = {}
    for x in range(N):
        smallest.setdefault(parent[x], x)       # (x ascends: the first one seen is the smallest)
    rows = [(nodes[x][0], nodes[x][1], nodes[smallest[parent[x]]][1], par[x] ^ par[smallest[parent[x]]]) for x in range(N)]
    conflicts = [i for rank, (a, b, s, i) in enumerate(links) if not in_forest[rank] and par[a] ^ par[b] != s]
    return rows, conflicts, rounds


def records(dicts):
    """PS_LINK_DTYPE records from dicts (fields left out are 0), in the order given."""
    out = np.zeros(len(dicts), dtype=_lib.PS_LINK_DTYPE)
    for i, d in enumerate(dicts):
        for k, v in d.items():
            out[i][k] = v
        out[i]['n_sv'] = int(out[i]['n_same']) + int(out[i]['n_flip']) + int(out[i]['n_open'])
    return out


def random_records(seed):
    """A random multigraph over 1 to 4 contigs: small counts (ties), weights above 2^33, PS values up to 2^32 - 2; ascending."""
    rng = random.Random(0xB10C5 + seed)
    K, P = rng.choice([1, 1, 2, 4]), rng.choice([2, 3, 5, 9, 17, 40])
    pool = sorted(rng.sample(range(0, 2 ** 32 - 1), P)) if rng.random() < .5 else list(range(P))
    seen, recs = set(), []
    for _ in range(rng.randrange(0, 3 * P)):
        k = rng.randrange(K)
        a, b = sorted(rng.sample(pool, 2))
        if (k, a, b) in seen:
            continue
        seen.add((k, a, b))
        big = 2 ** 33 if rng.random() < .2 else 0
        ns, nf = rng.randrange(0, 4), rng.randrange(0, 4)
        recs.append(dict(contig=k, ps_a=a, ps_b=b, n_same=ns, n_flip=nf, w_same=rng.randrange(0, 3) + big if ns else 0,
                         w_flip=rng.randrange(0, 3) + big if nf else 0))
    recs.sort(key=lambda r: (r['contig'], r['ps_a'], r['ps_b']))
    return records(recs), K


def chain(n_links, contig=0, first=0, step=1):
    """A chain of n_links + 1 phase sets with mixed verdicts, some without one, ties and every order of strengths."""
    return records([dict(contig=contig, ps_a=first + i * step, ps_b=first + (i + 1) * step, n_same=(i * 7) % 3, n_flip=(i * 5) % 4,
                         w_same=i % 5, w_flip=(i * 3) % 7) for i in range(n_links)])


def table(rows):
    return np.array([tuple(r) for r in rows], dtype=_lib.PS_BLOCK_DTYPE).reshape(-1)
