# coding=utf-8
"""-m gpu: the fused SVIM-mode pipeline at its edge shapes -- every named case of tests/svim_fuzz.py through the three
entries (duet_svim_phase_device with and without the host round trip, duet_svim_phase_host), field for field against
tests/svim_ref.py, under the launch structures the debug bits select, with reruns on one context and the output words
behind the candidate count watched.  tests/test_svim_fuzz_cases.py shows on the CPU that the cases have the structure they
are named for.  The feature entries (duet_svim_features[_cap]_device / _host) run at the same edge shapes, and the cached depth_off
upload is driven across streams by both of its callers."""
import ctypes

import numpy as np
import pytest

from duet_amd import _lib
from duet_amd.devmem import DeviceSvim
from oracle import c_oracle
from tests import pc_cap_ref, svim_fuzz, svim_ref
from tests.test_gpu_pc_cap import assert_fields

pytestmark = pytest.mark.gpu

FIELDS = ('order', 'cand_off', 'cand_contig', 'cand_type', 'cand_pos', 'cand_span', 'pred', 'ps')
DTYPES = dict(order=np.uint32, cand_off=np.uint32, cand_contig=np.uint16, cand_type=np.uint8, cand_pos=np.uint32,
              cand_span=np.uint32, pred=np.uint8, ps=np.uint32)
ENTRIES = ('device_wait', 'device_nowait', 'host')
FILL = 0xCD
# the outputs are the same under every bit (include/duet_ef.h); each selects another kernel path or launch structure:
COMBOS = (0,
          0x40000,            # DUET_DBG_CLUSTER_RECSORT: the record sort also below 1.25 M marks
          0x200,              # DUET_DBG_CLUSTER_LARGE: the launch structure of large inputs
          0x4000000,          # DUET_DBG_CLUSTER_EVENT_FORKS: the side streams fork behind events
          0x800000,           # DUET_DBG_EF_OWN_OFF: three E/F launches at every size
          0x20 | 0x80000,     # DUET_DBG_EF_FIN_TPB2 | DUET_DBG_EF_HEAVY_ALL: two tiles per workgroup, the wave-cooperative walk
          0x80,               # DUET_DBG_EF_FIN_TPB4: four tiles per workgroup
          0x100000,           # DUET_DBG_EF_HEAVY_OFF: the lane walk up to 255 marks
          0x8000000)          # DUET_DBG_CLUSTER_WIDE_OFF: one wavefront per partition of more than 64 marks
# host-planned runs only (wait=True and the host entry), up to 64 contigs: the two E/F launches at every size
OWN_ALL = 0x1000000          # DUET_DBG_EF_OWN_ALL
OTHER = {'contigs_65': 'parts_65'}              # the case run in between: other sizes, another depth_off


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.set_debug(0)
    c.close()


_want, _resident = {}, {}


def reference(name):
    if name not in _want:
        c = svim_fuzz.case(name)
        _want[name] = svim_ref.fused(c.marks, c.read_tag, c.depth, c.depth_off, c.depth_bin, c.svlen_thres, c.suppread_thres, **c.kw)
        assert _want[name]['rc'] == 0
    return _want[name]


def resident(name, keep=False):
    """the case's DeviceSvim (kept for the cases that run in between)"""
    if name in _resident:
        return _resident[name]
    c = svim_fuzz.case(name)
    ds = DeviceSvim(c.marks, c.read_tag, c.depth, c.depth_off, c.depth_bin, c.svlen_thres, c.suppread_thres, **c.kw)
    if keep:
        _resident[name] = ds
    return ds


def device_run(ctx, ds, wait):
    """run_fused on pre-filled output buffers -> (n_cands, every output buffer whole, padding included, as bytes -> typed)"""
    bufs = dict([(f, ds.keep['out_' + f]) for f in FIELDS[:6]] + [('pred', ds.out_pred), ('ps', ds.out_ps)])
    for t in bufs.values():
        t.view(ds.torch.uint8).fill_(FILL)
    ds.keep['out_n_cands'].fill_(FILL)
    ds.run_fused(ctx, wait=wait)
    n = ds.n_cands()                                 # (synchronises)
    if wait:
        assert ds.n_found == n
    return n, {f: t.view(ds.torch.uint8).cpu().numpy() for f, t in bufs.items()}


def host_run(ctx, c):
    """duet_svim_phase_host on pre-filled host arrays (Context.svim_host's call, with the arrays kept whole)"""
    m = {k: np.ascontiguousarray(c.marks[k], dtype=dt) for k, dt in (('contig', np.uint16), ('type', np.uint8), ('pos', np.uint32),
                                                                    ('span', np.uint32), ('read', np.uint32))}
    M = c.M
    p = _lib.SvimProblem()
    p.marks.n_marks, p.marks.part_gap, p.marks.part_max = M, c.kw.get('part_gap', 1000), c.kw.get('part_max', 100)
    p.marks.max_dist, p.marks.normalizer = float(c.kw.get('max_dist', 0.9)), float(c.kw.get('normalizer', 900.0))
    if M:
        p.marks.n_contigs_hint, p.marks.n_types_hint = int(m['contig'].max()) + 1, int(m['type'].max()) + 1
        p.marks.max_pos_hint, p.marks.max_span_hint = int(m['pos'].max()), max(int(m['span'].max()), 1)
    p.marks.mark_contig, p.marks.mark_type = m['contig'].ctypes.data, m['type'].ctypes.data
    p.marks.mark_pos, p.marks.mark_span, p.mark_read = m['pos'].ctypes.data, m['span'].ctypes.data, m['read'].ctypes.data
    tag, depth = np.ascontiguousarray(c.read_tag, dtype=np.uint64), np.ascontiguousarray(c.depth, dtype=np.uint32)
    p.read_tag = tag.ctypes.data if tag.size else None
    p.depth = depth.ctypes.data if depth.size else None
    p.n_reads, p.n_contigs, p.depth_off = len(tag), c.K, c.depth_off.ctypes.data
    p.depth_bin, p.svlen_thres, p.suppread_thres = c.depth_bin, c.svlen_thres, c.suppread_thres
    out = {f: np.full((M + (f == 'cand_off')) * np.dtype(DTYPES[f]).itemsize + 64, FILL, dtype=np.uint8) for f in FIELDS}
    n = ctypes.c_uint32(0xCDCDCDCD)
    res = _lib.ClusterResult()
    for f in FIELDS[:6]:
        setattr(res, f, out[f].ctypes.data)
    res.n_cands = ctypes.addressof(n)
    rc = ctx.lib.duet_svim_phase_host(ctx.handle, ctypes.byref(p), ctypes.byref(res), out['pred'].ctypes.data, out['ps'].ctypes.data)
    assert rc == 0, ctx.last_error()
    return n.value, out


def check(tag, c, want, n, out):
    """field for field; the first differing indices; everything behind the entries written stays as it was filled"""
    N, M = len(want['pred']), c.M
    assert n == N, (tag, 'n_cands', n, N)
    for f in FIELDS:
        size = np.dtype(DTYPES[f]).itemsize
        used = M if f == 'order' else (N + 1 if f == 'cand_off' else N)
        if M == 0:
            used = 0                                  # (nothing at all is written without marks, cand_off[0] included)
        got = out[f][:used * size].view(DTYPES[f])
        ref = want[f][:used]
        bad = np.nonzero(got != ref)[0]
        assert bad.size == 0, (tag, f, bad[:5], got[bad[:5]], ref[bad[:5]])
        tail = np.nonzero(out[f][used * size:] != FILL)[0]
        assert tail.size == 0, (tag, f, 'written behind entry %d' % used, tail[:5] // size + used, out[f][used * size:][tail[:5]])


def run(ctx, name, entry, dbg, tag, ds=None):
    c, want = svim_fuzz.case(name), reference(name)
    ctx.set_debug(dbg)
    try:
        n, out = host_run(ctx, c) if entry == 'host' else device_run(ctx, ds, entry == 'device_wait')
    finally:
        ctx.set_debug(0)
    check((name, entry, hex(dbg), tag), c, want, n, out)


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('name', svim_fuzz.NAMES)
def test_edge_case_matches_the_reference(ctx, name, entry):
    other = OTHER.get(name, 'contigs_65')
    ds = ds_other = None
    if entry != 'host':
        ds, ds_other = resident(name), resident(other, keep=True)          # (one upload for all the runs of this test)
    run(ctx, name, entry, 0, 'first', ds)
    # another case in between on the same context, then this one again: every workspace is reused, the cached depth_off
    # upload is replaced twice
    run(ctx, other, entry, 0, 'in between', ds_other)
    run(ctx, name, entry, 0, 'again', ds)
    for dbg in COMBOS[1:] + ((OWN_ALL,) if entry != 'device_nowait' and svim_fuzz.case(name).K <= 64 else ()):
        run(ctx, name, entry, dbg, 'combination', ds)


# ---- the feature entries at the edge shapes ----------------------------------------------------------------------------------------

FEATURE_CASES = ('marks_0', 'marks_1', 'marks_2', 'marks_64', 'marks_65', 'contigs_2', 'contigs_65', 'empty_contigs_around',
                 'contigs_without_bins', 'all_marks_absent', 'no_reads')
# the cases whose read tags the Python feature reference takes (the others carry haplotype values only the C oracle does)
PY_REFERENCE = ('marks_0', 'marks_1', 'marks_2', 'marks_64', 'marks_65', 'all_marks_absent', 'no_reads')
CAPS = (None, 8100, 300)
NAMED = tuple(n for n in _lib.FEATURE_DTYPE.names if not n.startswith('reserved'))
COLUMNS = FIELDS[1:6]
REC = _lib.FEATURE_DTYPE.itemsize
_soa, _want_feat = {}, {}


def adapted(name):
    """the E/F problem the fused pipeline adapts from the case: svim_ref.adapt on the C cluster oracle's output"""
    if name not in _soa:
        c = svim_fuzz.case(name)
        cl = c_oracle.cluster(c.marks['contig'], c.marks['type'], c.marks['pos'], c.marks['span'], **c.kw)
        _soa[name] = svim_ref.adapt(cl, c.marks, c.read_tag, c.depth, c.depth_off, c.depth_bin)[0]
    return _soa[name]


def feature_reference(ctx, name, cap):
    """the records of duet_ef_features[_cap]_host on the adapted problem"""
    if (name, cap) not in _want_feat:
        c = svim_fuzz.case(name)
        _want_feat[name, cap] = ctx.features_host(adapted(name), c.svlen_thres, c.suppread_thres, pc_cap=cap)
    return _want_feat[name, cap]


def check_columns(tag, want, n, got):
    N = len(want['pred'])
    assert n == N, (tag, 'n_cands', n, N)
    for f in COLUMNS:
        ref = want[f][:N + (f == 'cand_off')]
        assert np.array_equal(got[f], ref), (tag, f, got[f][:5], ref[:5])


def check_records(tag, got, want):
    assert len(got) == len(want), (tag, len(got), len(want))
    for f in NAMED:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, (tag, f, bad[:5], got[f][bad[:5]], want[f][bad[:5]])


@pytest.mark.parametrize('name', FEATURE_CASES)
def test_feature_entries_at_the_edge_shapes(ctx, name):
    c, want = svim_fuzz.case(name), reference(name)
    ds = resident(name)
    torch = ds.torch
    buf = torch.zeros(max(c.M, 1) * REC + 64, dtype=torch.uint8, device=ds.device)
    seen = {}
    for cap in CAPS:
        tag = (name, 'pc_cap', cap)
        ref = feature_reference(ctx, name, cap)
        buf.fill_(FILL)
        n = ds.run_features(ctx, buf.data_ptr(), pc_cap=cap)
        torch.cuda.synchronize()
        raw = buf.cpu().numpy()
        dev = raw[:n * REC].view(_lib.FEATURE_DTYPE)
        check_columns(tag + ('device',), want, n, ds.fetch())
        check_records(tag + ('device',), dev, ref)
        tail = np.nonzero(raw[n * REC:] != FILL)[0]
        assert tail.size == 0, (tag, 'written behind record %d' % n, tail[:5])
        host = ctx.svim_features_host(c.marks, c.read_tag, c.depth, c.depth_off, c.depth_bin, c.svlen_thres, c.suppread_thres,
                                      pc_cap=cap, **c.kw)
        check_columns(tag + ('host',), want, len(host['feat']), host)
        check_records(tag + ('host',), host['feat'], ref)
        assert host['feat'].tobytes() == dev.tobytes(), tag
        if name in PY_REFERENCE:
            assert_fields(host['feat'], pc_cap_ref.features(adapted(name), c.svlen_thres, c.suppread_thres, 8100 if cap is None else cap),
                          '%s, cap %s' % (name, cap))
        seen[cap] = dev.tobytes()
    assert seen[None] == seen[8100]
    # the decisions of the default vector over those features are the C oracle's
    ds.run_thresholds(ctx, _lib.TUNE_DEFAULTS)
    got = ds.fetch()
    check_columns((name, 'thresholds'), want, ds.n_found, got)
    assert np.array_equal(got['pred'], want['pred']), (name, 'pred')
    live = got['pred'] != 0
    assert np.array_equal(got['ps'][live], want['ps'][live]), (name, 'ps')


# ---- the cached depth_off upload across streams -----------------------------------------------------------------------------------

def test_depth_off_cache_across_streams(ctx):
    """Two problems with another K and another depth_off on one context and two streams: the same contents on another stream
    (uploaded again), other contents, the first ones again, and a hit -- first through duet_svim_phase_device alone, then with
    duet_svim_features_device as every second caller of the same cache."""
    A, B = 'contigs_2', 'contigs_65'
    ds = {n: resident(n, keep=True) for n in (A, B)}
    torch = ds[A].torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    feat = torch.zeros(max(svim_fuzz.case(A).M, 1) * REC + 64, dtype=torch.uint8, device=ds[A].device)
    torch.cuda.synchronize()
    order = ((A, s1), (A, s2), (B, s2), (A, s1), (A, s1))
    for features in (False, True):
        for i, (name, stream) in enumerate(order):
            d, want, tag = ds[name], reference(name), (name, 'run %d' % i, 'features' if features else 'fused')
            if features and i % 2:
                n = d.run_features(ctx, feat.data_ptr(), stream=stream.cuda_stream)
                stream.synchronize()
                check_columns(tag, want, n, d.fetch())
                got = feat[:n * REC].cpu().numpy().view(_lib.FEATURE_DTYPE)
                check_records(tag, got, feature_reference(ctx, name, None))
                continue
            d.run_fused(ctx, stream=stream.cuda_stream, wait=False)
            stream.synchronize()
            got = d.fetch()
            check_columns(tag, want, d.n_found, got)
            for f in ('order', 'pred', 'ps'):
                assert np.array_equal(got[f], want[f]), (tag, f)
