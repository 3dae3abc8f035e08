# coding=utf-8
"""-m gpu: the evidence table (duet_amd/csrc/duet_evidence.hip): duet_tune_leaves_* against tests/evidence_ref.py, the sweep's
out_pred and the leaf census; duet_evidence_rows_* byte for byte against the reference's % formatting, in the text form and the
table form, with their contracts (exact size, a buffer one byte short, odd addresses, the refusals); `duet --write_evidence` in
both modes."""
import ctypes
import os
import shutil
import sys

import numpy as np
import pytest

from duet_amd import _lib, svim_mode, synth, tune
from duet_amd.native import NativeIngest
from duet_amd.read_file import init_chrom_list
from tests import cap_line_ref, evidence_ref, soa_fuzz, tune_ref
from tests import helpers as H
from tests.test_gpu_tune_score_edges import random_features, random_vectors

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 513)
NO_SEED, FILTERED = evidence_ref.NO_SEED, evidence_ref.FILTERED
U32, U64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def features(seed, C):
    """Random records in the three states: about a seventh not kept, a seventh kept without a seed set."""
    f = random_features(seed, C, eligible=1.0)
    r = np.random.default_rng(1000 + seed).random(C)
    f['kept'] = r >= 0.15
    f['eligible'] = r >= 0.3
    return f


def special_vectors():
    d = tune.vector()
    return np.stack([d, np.full(14, np.nan), np.full(14, np.inf), np.full(14, -np.inf)] +
                    [np.where(np.arange(14) % 3 == k, (np.nan, np.inf, -np.inf)[k], d) for k in range(3)])


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    t = torch.zeros(a.nbytes + 64, dtype=torch.uint8, device='cuda:0')
    if a.nbytes:
        t[:a.nbytes] = torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).to('cuda:0')
    return t


# ---- the leaves ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C', SIZES)
def test_leaves_host(ctx, C):
    feat = features(C, C)
    for v in np.concatenate([special_vectors(), random_vectors(C, 4)]):
        leaf, pred = ctx.leaves_host(feat, v)
        want_leaf, want_pred = evidence_ref.leaves(feat, v)
        assert leaf.dtype == np.uint8 and np.array_equal(leaf, want_leaf), v
        assert np.array_equal(pred, want_pred), v
        if C:
            assert np.array_equal(pred, ctx.sweep_host(feat, v[None, :], want_pred=True)[1][0])


def all_leaves_block():
    """256 candidates among which every leaf and both states occur under the default vector."""
    pool = random_features(77, 6000, eligible=1.0)
    leaf, _ = evidence_ref.leaves(pool, tune.vector())
    first = [int(np.nonzero(leaf == k)[0][0]) for k in range(18)]             # (IndexError: the pool misses a leaf)
    f = pool[np.array(first + list(range(256 - 18)))].copy()
    f['kept'][20:30] = 0
    f['eligible'][20:40] = 0
    return f


def test_one_block_with_every_leaf_and_both_states(ctx):
    feat = all_leaves_block()
    leaf, pred = ctx.leaves_host(feat, tune.vector())
    assert set(leaf.tolist()) == set(range(18)) | {NO_SEED, FILTERED}
    want = evidence_ref.leaves(feat, tune.vector())
    assert np.array_equal(leaf, want[0]) and np.array_equal(pred, want[1])
    assert set(pred.tolist()) == {0, 1, 2, 3}


@pytest.mark.parametrize('C', SIZES)
def test_leaves_device_against_the_sweep_and_the_census(ctx, C):
    """On resident arrays: out_pred is duet_tune_sweep_device's, and the leaves of the eligible candidates count up to the census's
    n_cands -- compared on the device."""
    import torch
    feat = features(3 * C + 1, C)
    d_feat = dev(feat)
    for v in special_vectors()[[0, 1, 4]]:
        d_vec = dev(v)
        leaf, pred = torch.full((C + 64,), 0xAB, dtype=torch.uint8, device='cuda:0'), torch.full((C + 64,), 0xAB, dtype=torch.uint8, device='cuda:0')
        ctx.leaves_device(d_feat.data_ptr(), C, v, leaf.data_ptr(), pred.data_ptr())
        sweep_pred, sweep_ps = torch.zeros(C + 64, dtype=torch.uint8, device='cuda:0'), torch.zeros(C + 16, dtype=torch.int32, device='cuda:0')
        ctx.apply_device(d_feat.data_ptr(), C, d_vec.data_ptr(), sweep_pred.data_ptr(), sweep_ps.data_ptr())
        census = torch.zeros(18 * 8, dtype=torch.int32, device='cuda:0')
        ctx.leaf_census_device(d_feat.data_ptr(), C, d_vec.data_ptr(), 1, None, None, census.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(pred[:C], sweep_pred[:C])
        assert bool((leaf[C:] == 0xAB).all()) and bool((pred[C:] == 0xAB).all())       # nothing behind the last candidate
        mine = leaf[:C].to(torch.int64)
        counted = torch.bincount(mine[mine < 18], minlength=18)
        assert torch.equal(counted, census.view(18, 8)[:, 0].to(torch.int64))
        assert int(counted.sum()) == int(feat['eligible'].sum())


def test_leaves_arguments(ctx):
    feat = features(1, 5)
    v = tune.vector()
    out = np.zeros(5, dtype=np.uint8)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    for args in ((None, 5, P(v), P(out), P(out)), (P(feat), 5, None, P(out), P(out)), (P(feat), 5, P(v), None, P(out)),
                 (P(feat), 5, P(v), P(out), None)):
        assert ctx.lib.duet_tune_leaves_host(ctx.handle, *args) == _lib.DUET_ERR_INVALID
        assert ctx.lib.duet_tune_leaves_device(ctx.handle, *(args + (None,))) == _lib.DUET_ERR_INVALID
        assert 'null' in ctx.last_error()
    assert ctx.lib.duet_tune_leaves_host(ctx.handle, None, 0, None, None, None) == _lib.DUET_OK
    assert ctx.lib.duet_tune_leaves_device(ctx.handle, None, 0, None, None, None, None) == _lib.DUET_OK


# ---- the rows --------------------------------------------------------------------------------------------------------------------

CHROMS = ['7', 'chr1', 'c' * 200, 'chrUn_KI270442v1', 'X']
SVTYPES = ['INS', 'DEL', '', 'DUP:TANDEM', 'BND']


def problem(seed, C):
    """Arrays of one call in both forms, and the reference's text for each."""
    rng = np.random.default_rng(seed)
    feat = features(seed, C)
    leaf, pred = evidence_ref.leaves(feat, tune.vector())
    pos = rng.integers(0, 2 ** 32, C).astype(np.uint32)
    svlen = rng.integers(0, 2 ** 20, C).astype(np.uint32)
    contig = rng.integers(0, len(CHROMS), C).astype(np.uint16)
    ctype = rng.integers(0, 4, C).astype(np.uint8)
    chrom = [CHROMS[k] for k in contig]
    svtype = [SVTYPES[int(i)] for i in rng.integers(0, len(SVTYPES), C)]
    pool, str_off = evidence_ref.pool_of(chrom, svtype)
    return dict(feat=feat, leaf=leaf, pred=pred, pos=pos, svlen=svlen, contig=contig, ctype=ctype, pool=pool, str_off=str_off,
                text=evidence_ref.rows_text(chrom, pos, svtype, svlen, feat, leaf, pred).encode(),
                table=evidence_ref.table_text(contig, ctype, pos, svlen, CHROMS, feat, leaf, pred).encode())


def host_text(ctx, q):
    return ctx.evidence_rows_host(q['feat'], q['leaf'], q['pred'], q['pos'], q['svlen'], rows=dict(pool=q['pool'], str_off=q['str_off']))


def host_table(ctx, q, chroms=CHROMS):
    return ctx.evidence_rows_host(q['feat'], q['leaf'], q['pred'], q['pos'], q['svlen'], cand_contig=q['contig'], cand_type=q['ctype'],
                                  chrom_texts=chroms)


@pytest.mark.parametrize('C', SIZES)
def test_rows_both_forms(ctx, C):
    q = problem(C + 5, C)
    assert host_text(ctx, q) == q['text']
    assert host_table(ctx, q) == q['table']
    assert q['text'].count(b'\n') == C == q['table'].count(b'\n')


def edge_problem():
    """Every number at its extremes: POS 0 and 2^32 - 1, counts of 2^32 - 1, PC sums of 0 and 2^62 + 1 (and 2^64 - 1), CHROM of 1
    and 200 bytes, an empty SVTYPE piece, a row of `.` fields beside a full-width one."""
    f = np.zeros(6, dtype=_lib.FEATURE_DTYPE)
    full = dict(hap1=U32, hap2=U32, hap0=U32, allhap=U32, deg=U32, svread=U32, refread=U32, ps=U32)
    for n, v in full.items():
        f[n][[1, 3, 5]] = v
    f['t1'] = (0, 2 ** 62 + 1, 0, U64, 1, 2 ** 62 + 1)
    f['t2'] = (0, U64, 2 ** 62 + 1, 0, 10 ** 19, 9)
    f['kept'] = (0, 1, 1, 1, 0, 1)
    f['eligible'] = (0, 1, 0, 1, 0, 1)
    f['cls'] = (0, 2, 1, 255, 2, 1)
    leaf = np.array([FILTERED, 11, NO_SEED, 9, FILTERED, 0], dtype=np.uint8)
    pred = np.array([0, 3, 0, 1, 0, 2], dtype=np.uint8)
    pos = np.array([0, U32, 1, U32, 0, 10], dtype=np.uint32)
    svlen = np.array([0, U32, 9, 10, U32, 99], dtype=np.uint32)
    contig = np.array([4, 2, 0, 2, 4, 1], dtype=np.uint16)
    ctype = np.array([0, 1, 2, 3, 0, 1], dtype=np.uint8)
    chrom = [CHROMS[k] for k in contig]
    svtype = ['', 'DUP:TANDEM', 'INS', '', '', 'DEL']
    pool, str_off = evidence_ref.pool_of(chrom, svtype, ref=['', 'ACGT', 'N', '', 'N', 'N'], alt=['<INS>', '', 'A', '', '', 'T'])
    return dict(feat=f, leaf=leaf, pred=pred, pos=pos, svlen=svlen, contig=contig, ctype=ctype, pool=pool, str_off=str_off,
                text=evidence_ref.rows_text(chrom, pos, svtype, svlen, f, leaf, pred).encode(),
                table=evidence_ref.table_text(contig, ctype, pos, svlen, CHROMS, f, leaf, pred).encode())


def test_rows_at_the_extremes(ctx):
    q = edge_problem()
    first, second = q['text'].split(b'\n')[:2]
    assert first == b'X\t0\t\t0\t0\t0\t0\tfiltered\t.\t.\t.\t.\t.\t.\t.\t.\t.'
    assert second == ('c' * 200 + '\t4294967295\tDUP:TANDEM' + '\t4294967295' * 4 + '\tc1_one_hom_gated\t2' + '\t4294967295' * 4 +
                      '\t4611686018427387905\t18446744073709551615\t4294967295\t1|1').encode()
    assert len(second) - 200 - len('DUP:TANDEM') + 1 <= _lib.EVIDENCE_ROW_MAX
    assert host_text(ctx, q) == q['text']
    assert host_table(ctx, q) == q['table']


class Resident(object):
    """One problem in HBM, in the text form (table=False) or the table form."""

    def __init__(self, q, table, chroms=CHROMS):
        self.keep = {k: dev(q[k]) for k in ('feat', 'leaf', 'pred', 'pos', 'svlen', 'contig', 'ctype', 'pool', 'str_off')}
        p = _lib.EvidenceProblem()
        p.n_cands = len(q['feat'])
        k = self.keep
        p.feat, p.leaf, p.pred, p.cand_pos, p.cand_svlen = (k[n].data_ptr() for n in ('feat', 'leaf', 'pred', 'pos', 'svlen'))
        if table:
            texts = [None if c is None else c.encode() for c in chroms]
            self.chrom = (ctypes.c_char_p * max(len(texts), 1))(*texts)
            p.n_contigs, p.cand_contig, p.cand_type, p.chrom = len(texts), k['contig'].data_ptr(), k['ctype'].data_ptr(), self.chrom
        else:
            p.pool, p.pool_bytes, p.str_off = k['pool'].data_ptr(), len(q['pool']), k['str_off'].data_ptr()
        self.p = p

    def run(self, ctx, out, at, cap):
        """-> (status, *out_len), synchronised"""
        import torch
        n = ctypes.c_uint64(0xDEAD)
        rc = ctx.lib.duet_evidence_rows_device(ctx.handle, ctypes.byref(self.p), ctypes.c_void_p(out.data_ptr() + at), ctypes.c_uint64(cap),
                                               ctypes.byref(n), None)
        torch.cuda.synchronize()
        return rc, n.value


@pytest.mark.parametrize('table', [False, True], ids=['text', 'table'])
def test_rows_device_sizes_and_addresses(ctx, table):
    import torch
    q = problem(11, 257)
    want = q['table'] if table else q['text']
    r = Resident(q, table)
    for at in (0, 1, 2, 3):
        out = torch.full((len(want) + 16,), 0xAB, dtype=torch.uint8, device='cuda:0')
        rc, n = r.run(ctx, out, at, len(want))                               # out_cap exact
        got = out.cpu().numpy()
        assert rc == _lib.DUET_OK and n == len(want)
        assert got[at:at + n].tobytes() == want
        assert np.all(got[:at] == 0xAB) and np.all(got[at + n:] == 0xAB)
    out = torch.full((len(want) + 16,), 0xAB, dtype=torch.uint8, device='cuda:0')
    rc, n = r.run(ctx, out, 1, len(want) - 1)                                # one byte short: refused, the size still exact
    assert rc == _lib.DUET_ERR_INVALID and n == len(want) and 'too small' in ctx.last_error()
    assert bool((out == 0xAB).all())
    rc, n = r.run(ctx, out, 0, 0)
    assert rc == _lib.DUET_ERR_INVALID and n == len(want) and bool((out == 0xAB).all())
    assert len(want) <= _lib.evidence_bound(257, 200, 10)


def refused(ctx, q, table, what, chroms=CHROMS):
    """Both forms of the call refuse q: DUET_ERR_INVALID, the message names the case, a sentinel-filled buffer stays as it is."""
    import torch
    out = torch.full((1 << 16,), 0xAB, dtype=torch.uint8, device='cuda:0')
    rc, n = Resident(q, table, chroms).run(ctx, out, 0, 1 << 16)
    assert rc == _lib.DUET_ERR_INVALID and what in ctx.last_error(), ctx.last_error()
    assert bool((out == 0xAB).all())
    with pytest.raises(_lib.DuetLibraryError, match=what):
        (host_table(ctx, q, chroms) if table else host_text(ctx, q))


@pytest.mark.parametrize('table', [False, True], ids=['text', 'table'])
def test_rows_refusals(ctx, table):
    base = problem(21, 300)
    for code in (18, 0x7F, 0xFC, 0xFF):
        q = dict(base, leaf=base['leaf'].copy())
        q['leaf'][299] = code
        refused(ctx, q, table, 'leaf code')
    for code in (4, 255):
        q = dict(base, pred=base['pred'].copy())
        q['pred'][64] = code
        refused(ctx, q, table, 'pred above 3')
    if table:
        for code in (4, 255):
            q = dict(base, ctype=base['ctype'].copy())
            q['ctype'][0] = code
            refused(ctx, q, True, 'type code')
        for k in (len(CHROMS), 65535):
            q = dict(base, contig=base['contig'].copy())
            q['contig'][257] = k
            refused(ctx, q, True, 'cand_contig not below n_contigs')
        refused(ctx, base, True, 'null CHROM text', CHROMS[:2] + [None] + CHROMS[3:])
        refused(ctx, base, True, 'contig count', [])
    else:
        q = dict(base, str_off=base['str_off'].copy())
        assert q['str_off'][4 * 100] > 0
        q['str_off'][4 * 100 + 1] = q['str_off'][4 * 100] - 1                                         # CHROM ends before it begins
        refused(ctx, q, False, 'string offsets')
        q = dict(base, str_off=base['str_off'].copy())
        q['str_off'][4 * 300] = len(base['pool']) + 1                                                 # SVTYPE leaves the pool
        refused(ctx, q, False, 'string offsets')
    assert (host_table(ctx, base) if table else host_text(ctx, base)) == (base['table'] if table else base['text'])


def test_rows_null_arrays(ctx):
    q = problem(2, 4)
    r = Resident(q, True)
    import torch
    out = torch.full((4096,), 0xAB, dtype=torch.uint8, device='cuda:0')
    for field in ('feat', 'leaf', 'pred', 'cand_pos', 'cand_svlen', 'cand_contig', 'cand_type', 'chrom'):
        saved = getattr(r.p, field) if field != 'chrom' else r.chrom     # (a pointer field reads as a view of the structure)
        setattr(r.p, field, None)
        rc, n = r.run(ctx, out, 0, 4096)
        assert rc == _lib.DUET_ERR_INVALID and n == 0 and 'null' in ctx.last_error(), field
        setattr(r.p, field, saved)
    n = ctypes.c_uint64(7)
    assert ctx.lib.duet_evidence_rows_device(ctx.handle, ctypes.byref(r.p), None, 4096, ctypes.byref(n), None) == _lib.DUET_ERR_INVALID
    assert ctx.lib.duet_evidence_rows_device(ctx.handle, None, None, 0, ctypes.byref(n), None) == _lib.DUET_ERR_INVALID
    t = Resident(q, False)
    t.p.str_off = None
    assert t.run(ctx, out, 0, 4096)[0] == _lib.DUET_ERR_INVALID
    assert bool((out == 0xAB).all())
    rc, n = r.run(ctx, out, 0, 4096)
    assert rc == _lib.DUET_OK and out[:n].cpu().numpy().tobytes() == q['table']
    empty = _lib.EvidenceProblem()
    n = ctypes.c_uint64(7)
    assert ctx.lib.duet_evidence_rows_device(ctx.handle, ctypes.byref(empty), None, 0, ctypes.byref(n), None) == _lib.DUET_OK and n.value == 0
    assert ctx.lib.duet_evidence_rows_host(ctx.handle, ctypes.byref(empty), None, 0, ctypes.byref(n)) == _lib.DUET_OK and n.value == 0


def test_a_large_call_then_a_small_one_and_nothing_of_ef_changes(ctx):
    soa = soa_fuzz.random_soa(3, n_contigs=4)
    before = (ctx.run_host(soa, 0, 0), ctx.features_host(soa, 0, 0))
    large, small = problem(31, 20001), problem(32, 3)
    assert host_text(ctx, large) == large['text']
    assert host_text(ctx, small) == small['text']
    assert host_table(ctx, large) == large['table']
    assert host_table(ctx, small) == small['table']
    leaf, pred = ctx.leaves_host(large['feat'], tune.vector())
    assert np.array_equal(leaf, large['leaf']) and np.array_equal(pred, large['pred'])
    leaf, pred = ctx.leaves_host(small['feat'], tune.vector())
    assert np.array_equal(leaf, small['leaf']) and np.array_equal(pred, small['pred'])
    after = (ctx.run_host(soa, 0, 0), ctx.features_host(soa, 0, 0))
    assert np.array_equal(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1])
    assert before[1].tobytes() == after[1].tobytes()
    assert int((before[0][0] != 0).sum()) > 10


def test_explain_is_the_leaves_call(ctx):
    feat = features(9, 500)
    v = random_vectors(9, 1)[0]
    leaf, pred = tune.explain(dict(feat=feat), v, ctx=ctx)
    want = evidence_ref.leaves(feat, v)
    assert np.array_equal(leaf, want[0]) and np.array_equal(pred, want[1])
    assert np.array_equal(pred, tune.apply(dict(feat=feat), v, ctx=ctx)[0])


# ---- the product -----------------------------------------------------------------------------------------------------------------

def read(path):
    with open(path, 'rb') as f:
        return f.read()


def reference_table(home, s=50, r=2, vec=None):
    """The table of a work directory with a caller's VCF, from the oracle's filter, classes, seed sets and vote."""
    soa, txt = tune._candidates(home, s, r, False, 2)
    feat = cap_line_ref.records(tune_ref.oracle_features(soa, s, r))
    leaf, pred = evidence_ref.leaves(feat, vec if vec is not None else tune.vector())
    return (evidence_ref.header() + evidence_ref.rows_text(txt['chrom'], soa.cand_pos, txt['svtype'], soa.cand_svlen, feat, leaf, pred)).encode()


@pytest.fixture(scope='module')
def golden_home(tmp_path_factory):
    from tests.test_c_oracle import materialise_bams
    home = str(tmp_path_factory.mktemp('evidence_golden') / 'w')
    shutil.copytree(os.path.join(H.GOLDEN, 'cases', 'fuzz_cutesv_s2'), home)
    materialise_bams(home)
    return home


def test_product_run_native_ingest(golden_home, tmp_path):
    from duet_amd.sv_phasing import evidence_path, sv_phasing
    from tests.test_c_oracle import materialise_bams
    from tests.test_gpu_pc_cap import demoted_copy
    home = golden_home
    pinned = read(os.path.join(H.GOLDEN, 'cases', 'fuzz_cutesv_s2', 'phased_sv.vcf'))
    sv_phasing(home, 50, 2, 4, False)
    assert read(home + '/phased_sv.vcf') == pinned
    assert not os.path.exists(evidence_path(home))                            # no table without the flag
    sv_phasing(home, 50, 2, 4, False, evidence=True)
    assert read(home + '/phased_sv.vcf') == pinned
    want = reference_table(home)
    assert read(evidence_path(home)) == want and want.count(b'\n') > 100
    rules = set(ln.split(b'\t')[7] for ln in want.splitlines()[1:])
    assert b'filtered' in rules and len(rules) > 5
    # a vector of the caller's own: the rule a candidate ends at under those constants
    v = tune.vector({'c1_max_ref_num': 3, 'c0_min_sv_num': 2})
    sv_phasing(home, 50, 2, 4, False, thresholds=v, evidence=True)
    assert read(home + '/phased_sv.vcf').decode() == tune_ref.phased_text(home, 50, 2, v)
    assert read(evidence_path(home)) == reference_table(home, vec=v) != want
    # --pc_cap 2400: the table of the work directory whose PC tags in (2400, 8100] read 8101
    demoted = str(tmp_path / 'demoted')
    assert demoted_copy(home, demoted, 2400) > 20
    materialise_bams(demoted)
    without = read(home + '/phased_sv.vcf')
    sv_phasing(home, 50, 2, 4, False, pc_cap=2400)
    capped = read(home + '/phased_sv.vcf')
    sv_phasing(home, 50, 2, 4, False, pc_cap=2400, evidence=True)
    assert read(home + '/phased_sv.vcf') == capped != without
    want_capped = reference_table(demoted)
    assert read(evidence_path(home)) == want_capped != want


def test_duet_command_native_ingest(golden_home, monkeypatch):
    """cli.main up to the last stage: the external stages and the input checks are replaced, SV phasing runs."""
    from duet_amd import cli, stages
    from duet_amd.sv_phasing import evidence_path
    home = golden_home
    for name in ('snp_calling', 'sv_calling', 'snp_phasing'):
        monkeypatch.setattr(stages, name, lambda *a: None)
    monkeypatch.setattr(cli, 'check_envs', lambda *a: None)
    monkeypatch.setattr(cli, 'set_logging', lambda *a: None)
    if os.path.exists(evidence_path(home)):
        os.remove(evidence_path(home))
    monkeypatch.setattr(sys, 'argv', ['duet', 'in.bam', 'ref.fa', home])
    cli.main(None)
    plain = read(home + '/phased_sv.vcf')
    assert not os.path.exists(evidence_path(home))
    monkeypatch.setattr(sys, 'argv', ['duet', 'in.bam', 'ref.fa', home, '--write_evidence'])
    cli.main(None)
    assert read(home + '/phased_sv.vcf') == plain
    assert read(evidence_path(home)) == reference_table(home)


@pytest.fixture(scope='module')
def svim_home(tmp_path_factory):
    """A work directory of BAMs only, and the E/F problem the fused pipeline adapts from its marks at -c 0.9, -s 50, -r 2: the
    callset the product run writes, read back (as tests/test_gpu_pc_cap.py obtains it)."""
    root = tmp_path_factory.mktemp('evidence_svim')
    home, copy = str(root / 'w'), str(root / 'copy')
    synth.write_svim_workdir(home, H.case_contigs('genome_small', 5), 5)
    shutil.copytree(home, copy)
    svim_mode.sv_phasing_from_bams(copy, 50, 2, 4, False, 0.9, 0, write_sv_calls=True)
    soa, _ = tune._candidates(copy, 50, 2, False, 4)
    ing, got = NativeIngest.extract(home + '/snp_phasing/', init_chrom_list(False, home), 4, 50, 20, 1000)
    assert ing is not None, got
    ing.close()
    return dict(home=home, soa=soa, marks=got)


def test_resident_features_are_kept_on_request_and_never_stale(ctx, svim_home):
    from duet_amd.devmem import DeviceSvim
    got = svim_home['marks']
    texts = svim_mode.spelled_contigs(svim_home['home'], init_chrom_list(False, svim_home['home']))
    ds = DeviceSvim(got, got['read_tag'], got['depth'], got['depth_off'], 1000, 50, 2, max_dist=0.9, device='cuda:0')
    ds.run_thresholds(ctx, tune.vector())
    assert ds.feat is None
    with pytest.raises(RuntimeError, match='keep_features'):
        ds.evidence_rows(ctx, texts)
    ds.run_thresholds(ctx, tune.vector(), keep_features=True)
    table = ds.evidence_rows(ctx, texts)
    assert table.tobytes().count(b'\n') == svim_home['soa'].n_cands
    ds.run_fused(ctx)                                                          # another run: its candidates have no features here
    assert ds.feat is None
    with pytest.raises(RuntimeError, match='keep_features'):
        ds.evidence_rows(ctx, texts)


def test_duet_command_svim_gpu(ctx, svim_home, monkeypatch):
    from duet_amd import cli, stages
    from duet_amd.sv_phasing import evidence_path
    from tests import pc_cap_ref
    home, soa, got = svim_home['home'], svim_home['soa'], svim_home['marks']
    for name in ('snp_calling', 'sv_calling', 'snp_phasing'):
        monkeypatch.setattr(stages, name, lambda *a: None)
    monkeypatch.setattr(cli, 'check_envs', lambda *a: None)
    monkeypatch.setattr(cli, 'set_logging', lambda *a: None)
    res = ctx.svim_features_host(got, got['read_tag'], got['depth'], got['depth_off'], 1000, 50, 2, max_dist=0.9)
    assert len(res['cand_pos']) == soa.n_cands
    texts = svim_mode.spelled_contigs(home, init_chrom_list(False, home))

    def want(cap):
        feat = cap_line_ref.records(pc_cap_ref.features(soa, 50, 2, cap) if cap is not None else tune_ref.oracle_features(soa, 50, 2))
        leaf, pred = evidence_ref.leaves(feat, tune.vector())
        return (evidence_ref.header() + evidence_ref.table_text(res['cand_contig'], res['cand_type'], res['cand_pos'], res['cand_span'],
                                                                texts, feat, leaf, pred)).encode()

    base = ['duet', 'in.bam', 'ref.fa', home, '-b', 'svim-gpu']
    monkeypatch.setattr(sys, 'argv', base)
    cli.main(None)
    plain = read(home + '/phased_sv.vcf')
    assert not os.path.exists(evidence_path(home)) and plain.count(b'\n') > 100
    monkeypatch.setattr(sys, 'argv', base + ['--write_evidence'])
    cli.main(None)
    assert read(home + '/phased_sv.vcf') == plain
    table = read(evidence_path(home))
    assert table == want(None) and table.count(b'\n') == soa.n_cands + 1
    monkeypatch.setattr(sys, 'argv', base + ['--pc_cap', '2400'])
    cli.main(None)
    capped = read(home + '/phased_sv.vcf')
    monkeypatch.setattr(sys, 'argv', base + ['--pc_cap', '2400', '--write_evidence', '--write_sv_calls'])
    cli.main(None)
    assert read(home + '/phased_sv.vcf') == capped != plain
    assert read(evidence_path(home)) == want(2400) != table
