# coding=utf-8
"""-m gpu: the line of the PC cap (duet_tune_cap_line_host / _device, duet_svim_cap_line_host / _device,
duet_amd/csrc/duet_tune_capline.hip) against tests/cap_line_ref.py, word for word, at its edge shapes; and on the device the claim
the line rests on: duet_ef_features_cap_device gives identical bytes for every cap between two neighbours of the line."""
import ctypes

import numpy as np
import pytest

from duet_amd import _lib, engine
from tests import cap_line_ref as R
from tests import soa_fuzz
from tests.test_gpu_pc_cap import Resident, build, cand, cap_host

pytestmark = pytest.mark.gpu

CAP_MAX = R.CAP_MAX
SAT = CAP_MAX + 1
ABSENT = engine.MARK_ABSENT
RX_TILE, SCAN_TILE = 4096, 2048         # kRxTile, kScanTile of duet_prims.hip.h
GUARD = 0x5A5A5A5A


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def svim_problem(mark_read_ptr, read_tag_ptr, M, n_reads):
    p = _lib.SvimProblem()
    p.marks.n_marks, p.n_reads = M, n_reads
    p.mark_read, p.read_tag = mark_read_ptr or None, read_tag_ptr or None
    return p


def on_device(ctx, res, prob, M, N, svim):
    """One _device entry into a guarded buffer -> (values, D); nothing is written behind the values."""
    torch = res.torch
    room = _lib.cap_line_room(M, N)
    out = torch.full((room + 8,), GUARD, dtype=torch.int32, device='cuda:0')
    stream = torch.cuda.current_stream().cuda_stream
    n, D = (ctx.svim_cap_line_device if svim else ctx.cap_line_device)(prob, N, out.data_ptr(), stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert n <= room and np.all(got[n:] == GUARD)
    return got[:n].tolist(), D


def check(ctx, soa, s=0, r=0, Ns=(0,), res=None):
    """All four entries against the reference for every max_values -> (the whole candidate-form line, D)."""
    res = res or Resident(soa, s, r)
    res.dp.problem.svlen_thres, res.dp.problem.suppread_thres = s, r
    M = soa.n_marks
    sp = svim_problem(res.dp.problem.mark_read, res.dp.problem.read_tag, M, soa.n_reads)
    for N in Ns:
        want, D, _ = R.soa_line(soa, s, r, N)
        host, d = ctx.cap_line_host(soa, s, r, N)
        assert (host.tolist(), d) == (want, D), ('host', N, host[:8], want[:8], d, D)
        assert on_device(ctx, res, res.dp.problem, M, N, False) == (want, D), ('device', N)
        raw, Dr, _ = R.raw_line(soa.mark_read, soa.read_tag, N)
        host, d = ctx.svim_cap_line_host(soa.mark_read, soa.read_tag, N)
        assert (host.tolist(), d) == (raw, Dr), ('svim host', N, host[:8], raw[:8], d, Dr)
        assert on_device(ctx, res, sp, M, N, True) == (raw, Dr), ('svim device', N)
    full, D, L = R.soa_line(soa, s, r)
    assert len(full) == L
    return full, D


def flat(pcs, degs=None, svlen=100, svread=5, gt=1):
    """One read per mark with the given pc (hap alternating, one PS), candidates of the given degrees on one contig."""
    pcs = np.asarray(pcs, dtype=np.int64)
    M = len(pcs)
    degs = [M] if degs is None else list(degs)
    assert sum(degs) == M
    C = len(degs)
    col = lambda v: np.broadcast_to(np.asarray(v, dtype=np.int64), (C,)).copy()
    return engine.EfSoA(cand_ctg_off=[0, C], read_tag=engine.pack_tags(1 + np.arange(M) % 2, pcs, np.full(M, 7)),
                        cand_pos=np.arange(C) + 1, cand_svlen=col(svlen), cand_svread=col(svread), cand_refread=col(5),
                        cand_gt_ok=col(gt), cand_off=np.concatenate([[0], np.cumsum(degs)]), mark_read=np.arange(M))


# ---- empty and degenerate inputs -------------------------------------------------------------------------------------------------

def test_no_candidate_no_mark_and_a_candidate_without_a_mark(ctx):
    assert check(ctx, build([[]]), Ns=(0, 2, 5)) == ([0], 0)
    # M == 0 with candidates: no array is read
    soa = flat([5, 6, 7], [1, 2])
    prob, keep = _lib.problem_from_arrays(soa, 0, 0)
    prob.n_marks, prob.mark_read = 0, None
    out, n, d = np.full(4, GUARD, dtype=np.uint32), ctypes.c_uint32(9), ctypes.c_uint32(9)
    assert ctx.lib.duet_tune_cap_line_host(ctx.handle, ctypes.byref(prob), 0, _lib._ptr(out), ctypes.byref(n), ctypes.byref(d)) == 0
    assert (out.tolist(), n.value, d.value) == ([0, GUARD, GUARD, GUARD], 1, 0)
    res = Resident(soa)
    res.dp.problem.n_marks = 0
    assert on_device(ctx, res, res.dp.problem, 0, 0, False) == ([0], 0)
    assert on_device(ctx, res, svim_problem(None, None, 0, 0), 0, 0, True) == ([0], 0)
    assert ctx.svim_cap_line_host(np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint64)) [0].tolist() == [0]
    # a candidate in the middle with no mark
    soa = flat([500, 600, 700, 800], [2, 1, 1])
    soa.cand_off[:] = [0, 2, 2, 4]
    assert check(ctx, soa) == ([0, 500, 600, 700, 800], 4)


def test_no_tagged_mark(ctx):
    soa = flat([100, 200, 300, 400, 500, 600], [3, 3])
    soa.mark_read[:] = [ABSENT, soa.n_reads, 0xFFFFFFFE, ABSENT, 1, 2]
    soa.read_tag[1] = soa.read_tag[2] = R.UNTAGGED                         # an all-ones tag word
    assert check(ctx, soa, Ns=(0, 2)) == ([0], 0)
    assert check(ctx, build([[cand(5, [None, None]), cand(6, [None])]])) == ([0], 0)
    soa.read_tag[2] = engine.pack_tags([3], [321], [9])[0]                  # one participant, a hap 3 read at that
    assert check(ctx, soa, Ns=(0, 2, 3)) == ([0, 321], 1)


# ---- distinct-value counts and edge values ----------------------------------------------------------------------------------------

def test_one_value_all_distinct_and_the_zero(ctx):
    assert check(ctx, flat([777] * 300, [100, 200])) == ([0, 777], 1)
    assert check(ctx, flat([0] * 70)) == ([0], 1)                          # pc 0 present: no extra 0, L = D
    pcs = np.random.default_rng(4).permutation(3000) + 1                   # all distinct, 0 absent: L = D + 1
    assert check(ctx, flat(pcs, [1000, 1, 1999])) == ([0] + list(range(1, 3001)), 3000)
    assert check(ctx, flat(np.random.default_rng(5).permutation(3000)))[1] == 3000       # ... 0 present: L = D = 3000


def test_the_largest_values_and_all_30_key_bits(ctx):
    pcs = [CAP_MAX, SAT, SAT + 5, CAP_MAX - 1, 1 << 29, (1 << 29) + 1, (1 << 24) | 1, 0x2AAAAAAA, 0x15555555, 255, 256, 65536, 65535]
    full, D = check(ctx, flat(pcs), Ns=(0, 2, 3))
    assert full[-1] == CAP_MAX and SAT not in full and D == len(pcs) - 2   # 2^30 - 2 (and what saturates to it) is not on the line
    assert full == [0] + sorted(p for p in pcs if p <= CAP_MAX)


def test_hap_3_filters_duplicates_and_contigs(ctx):
    soa = build([[cand(10, [(1, 100, 7), (2, 300, 7), None, (1, 100, 7)]),
                  cand(20, [(1, 4000, 7)], svlen=49), cand(30, [(2, 5000, 7)], svread=2), cand(40, [(1, 6000, 7)], gt=0)],
                 [],
                 [cand(50, [(3, 700, 9), (1, SAT, 9), (2, CAP_MAX, 8)]), cand(60, [(2, 300, 5), (2, 300, 5)])]])
    soa.mark_read[3] = soa.mark_read[0]                                     # the same read twice in one candidate
    assert check(ctx, soa, 50, 3, Ns=(0, 2, 3, 4, 5, 6)) == ([0, 100, 300, 700, CAP_MAX], 4)
    assert check(ctx, soa, 49, 3)[0] == [0, 100, 300, 700, 4000, CAP_MAX]   # each filter alone
    assert check(ctx, soa, 50, 2)[0] == [0, 100, 300, 700, 5000, CAP_MAX]
    soa.cand_gt_ok[3] = 1
    assert check(ctx, soa, 50, 3)[0] == [0, 100, 300, 700, 6000, CAP_MAX]
    assert check(ctx, soa, 0, 0)[0] == [0, 100, 300, 700, 4000, 5000, 6000, CAP_MAX]


# ---- size boundaries ------------------------------------------------------------------------------------------------------------

def test_candidates_of_63_64_65_and_200_marks(ctx):
    degs = [63, 64, 65, 200, 1]
    pcs = np.random.default_rng(6).integers(0, 50000, sum(degs))
    soa = flat(pcs, degs, svread=[5, 5, 1, 5, 5])
    full, D = check(ctx, soa, 0, 2, Ns=(0, 7))
    assert D == len(set(pcs[:63 + 64].tolist() + pcs[63 + 64 + 65:].tolist()))          # the 65 marks of the unkept one left out


@pytest.mark.parametrize('M', [SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, RX_TILE - 1, RX_TILE, RX_TILE + 1, 3 * RX_TILE + 5])
def test_marks_around_the_tiles(ctx, M):
    rng = np.random.default_rng(M)
    pcs = rng.integers(0, 1 << 30, M)
    pcs[rng.integers(0, M, M // 3)] = pcs[0]                                # a long run of one value
    degs = [M - 130, 64, 66]
    soa = flat(pcs, degs)
    soa.mark_read[rng.integers(0, M, 40)] = ABSENT
    full, D = check(ctx, soa, Ns=(0, 1000))
    assert D > M // 2


# ---- the entry ------------------------------------------------------------------------------------------------------------------

def test_max_values(ctx):
    soa = soa_fuzz.random_soa(21, n_contigs=2, cands_per_contig=(30, 40), empty_contig_rate=0)
    full, D = check(ctx, soa, 50, 2)
    L = len(full)
    assert L >= 12
    check(ctx, soa, 50, 2, Ns=(2, 3, L - 1, L, L + 1, 0xFFFFFFFF))


def test_refusals(ctx):
    soa = flat([5, 6, 7], [1, 2])
    prob, keep = _lib.problem_from_arrays(soa, 0, 0)
    sp = svim_problem(soa.mark_read.ctypes.data, soa.read_tag.ctypes.data, 3, 3)
    out, n, d = np.zeros(8, dtype=np.uint32), ctypes.c_uint32(0), ctypes.c_uint32(0)
    lib = ctx.lib
    for host, dev, p in ((lib.duet_tune_cap_line_host, lib.duet_tune_cap_line_device, prob),
                         (lib.duet_svim_cap_line_host, lib.duet_svim_cap_line_device, sp)):
        full = [ctx.handle, ctypes.byref(p), 0, _lib._ptr(out), ctypes.byref(n), ctypes.byref(d)]
        assert host(*full) == 0 and (n.value, d.value, out[:4].tolist()) == (4, 3, [0, 5, 6, 7])
        for hole in (1, 3, 4, 5):
            args = list(full)
            args[hole] = None
            assert host(*args) == _lib.DUET_ERR_INVALID, hole
            assert dev(*(args + [None])) == _lib.DUET_ERR_INVALID, hole
        args = list(full)
        args[2] = 1
        assert host(*args) == _lib.DUET_ERR_INVALID and 'max_values' in ctx.last_error()
        assert dev(*(args + [None])) == _lib.DUET_ERR_INVALID
    for name in ('mark_read', 'cand_off', 'cand_svlen', 'cand_svread', 'cand_gt_ok', 'read_tag', 'cand_ctg_off'):
        bad, keep2 = _lib.problem_from_arrays(soa, 0, 0)
        setattr(bad, name, None)
        full = [ctx.handle, ctypes.byref(bad), 0, _lib._ptr(out), ctypes.byref(n), ctypes.byref(d)]
        assert lib.duet_tune_cap_line_host(*full) == _lib.DUET_ERR_INVALID, name
        assert lib.duet_tune_cap_line_device(*(full + [None])) == _lib.DUET_ERR_INVALID, name
    for name in ('mark_read', 'read_tag'):
        bad = svim_problem(soa.mark_read.ctypes.data, soa.read_tag.ctypes.data, 3, 3)
        setattr(bad, name, None)
        full = [ctx.handle, ctypes.byref(bad), 0, _lib._ptr(out), ctypes.byref(n), ctypes.byref(d)]
        assert lib.duet_svim_cap_line_host(*full) == _lib.DUET_ERR_INVALID, name
        assert lib.duet_svim_cap_line_device(*(full + [None])) == _lib.DUET_ERR_INVALID, name
    with pytest.raises(_lib.DuetLibraryError):
        ctx.cap_line_host(soa, 0, 0, 1)


def test_a_large_call_then_a_small_one_and_the_cap_features_around_them():
    large = soa_fuzz.random_soa(11, n_contigs=6, cands_per_contig=(800, 1500))
    small = soa_fuzz.random_soa(2, n_contigs=2, cands_per_contig=(20, 30), empty_contig_rate=0)
    c = _lib.Context(0)
    try:
        before = cap_host(c, small, 972)
        ef_before = c.run_host(small, 0, 0)
        check(c, large, 50, 2, Ns=(0, 9))
        check(c, small, 50, 2, Ns=(0, 9))                                    # the workspace of the large call, re-used
        check(c, large, 0, 0)
        after = cap_host(c, small, 972)
        ef_after = c.run_host(small, 0, 0)
    finally:
        c.close()
    assert before[0] == after[0] and before[1].tobytes() == after[1].tobytes()
    assert np.array_equal(ef_before[0], ef_after[0]) and np.array_equal(ef_before[1], ef_after[1])


@pytest.mark.parametrize('lowest', [0, 100])
def test_device_features_are_identical_between_neighbours_of_the_line(ctx, lowest):
    """lowest = 100: no mark carries pc 0, x_1 = 100, and every cap below it must give the records of cap 0 -- the 0 in front."""
    soa = soa_fuzz.random_soa(3, n_contigs=3, cands_per_contig=(30, 60), reads_per_contig=(10, 60), empty_contig_rate=0, no_seed_contig_rate=0)
    pool = np.array([lowest, lowest + 1, 972, 2400, 8100, 8101, 9720, 15000, CAP_MAX, SAT], dtype=np.uint64)
    pc = pool[np.random.default_rng(3).integers(0, len(pool), soa.n_reads)]
    soa.read_tag[:] = (soa.read_tag & ~(np.uint64(0x3FFFFFFF) << np.uint64(32))) | (pc << np.uint64(32))
    res = Resident(soa, 50, 2)
    full, D = check(ctx, soa, 50, 2, res=res)
    assert 4 <= len(full) <= 40 and full[0] == 0 and len(full) == D + (1 if lowest else 0)
    if lowest:
        assert full[1] == lowest
        rc0, at0 = res.run(ctx, 0)
        for cap in (1, lowest // 2, lowest - 1):
            rc, below = res.run(ctx, cap)
            assert rc == rc0 and below.tobytes() == at0.tobytes(), cap
        assert res.run(ctx, lowest)[1].tobytes() != at0.tobytes()           # ... and x_1 itself is another problem
    before = res.run(ctx, 972)
    differ = 0
    for x, nxt in zip(full, full[1:] + [None]):
        rc, at = res.run(ctx, x)
        for cap in ([c for c in (x + 1, nxt - 1) if x <= c < nxt] if nxt is not None else [min(x + 1, CAP_MAX), CAP_MAX]):
            rc2, other = res.run(ctx, cap)
            assert rc2 == rc and other.tobytes() == at.tobytes(), (x, cap)
        if nxt is not None:
            differ += res.run(ctx, nxt)[1].tobytes() != at.tobytes()
    assert differ >= 3                                                      # the line's values are different problems
    check(ctx, soa, 50, 2, res=res)                                         # a line call in between changes nothing:
    after = res.run(ctx, 972)
    assert before[0] == after[0] and before[1].tobytes() == after[1].tobytes()


# ---- the svim form ----------------------------------------------------------------------------------------------------------------

def test_svim_line_holds_the_candidate_form_line_of_the_adapted_problem(ctx, tmp_path):
    """Every tagged raw mark takes part; whatever -r keeps of the clustered marks is a subset of them."""
    from duet_amd import synth
    from duet_amd.native import NativeIngest
    from duet_amd.read_file import init_chrom_list
    from tests import helpers as H
    home = str(tmp_path / 'w')
    synth.write_svim_workdir(home, H.case_contigs('genome_small', 5), 5)
    ing, got = NativeIngest.extract(home + '/snp_phasing/', init_chrom_list(False, home), 4, 50, 20, 1000)
    assert ing is not None, got
    ing.close()
    raw, Dr, _ = R.raw_line(got['read'], got['read_tag'])
    host, d = ctx.svim_cap_line_host(got['read'], got['read_tag'])
    assert (host.tolist(), d) == (raw, Dr) and Dr > 50
    from duet_amd.devmem import DeviceSvim
    import torch
    ds = DeviceSvim(got, got['read_tag'], got['depth'], got['depth_off'], 1000, 50, 2, max_dist=0.9, device='cuda:0')
    out = torch.zeros(_lib.cap_line_room(len(got['pos'])), dtype=torch.int32, device='cuda:0')
    n, d = ctx.svim_cap_line_device(ds.sv_problem, 0, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert (out[:n].cpu().numpy().view(np.uint32).tolist(), d) == (raw, Dr)
    sizes = []
    for r in (2, 4):
        res = ctx.svim_features_host(got, got['read_tag'], got['depth'], got['depth_off'], 1000, 50, r, max_dist=0.9)
        # the adapted problem's candidate form: the marks of the clusters -r keeps (svlen and genotype as the adapter sets them)
        order = ctx.svim_host(got, got['read_tag'], got['depth'], got['depth_off'], 1000, 50, r, max_dist=0.9, want_order=True)['order']
        kept = res['feat']['kept'] != 0
        marks = np.concatenate([order[res['cand_off'][c]:res['cand_off'][c + 1]] for c in np.nonzero(kept)[0]] or [np.zeros(0, dtype=np.int64)])
        sub, _ = R.line(R.raw_participants(np.asarray(got['read'])[marks], got['read_tag']))
        # ... and the candidate-form entries on that adapted problem: the clusters as candidates, their marks in cluster order
        N = len(res['feat'])
        soa = engine.EfSoA(cand_ctg_off=[0, N], read_tag=got['read_tag'], cand_pos=res['cand_pos'], cand_svlen=res['cand_span'],
                           cand_svread=res['feat']['svread'], cand_refread=res['feat']['refread'], cand_gt_ok=np.ones(N, dtype=np.uint8),
                           cand_off=res['cand_off'], mark_read=np.asarray(got['read'])[order])
        assert np.array_equal((soa.cand_svlen >= 50) & (soa.cand_svread >= r), kept)
        line, D = ctx.cap_line_host(soa, 50, r)
        assert line.tolist() == sub and (line.tolist(), D) == R.soa_line(soa, 50, r)[:2]
        adapted = Resident(soa, 50, r)
        assert on_device(ctx, adapted, adapted.dp.problem, soa.n_marks, 0, False) == (sub, D)
        assert set(line.tolist()) <= set(host.tolist())                      # the svim line holds it
        sizes.append(len(sub))
    assert sizes[0] >= sizes[1] >= 1 and sizes[0] > 1
