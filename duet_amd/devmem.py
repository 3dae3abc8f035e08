# coding=utf-8
"""Device residency for E/F problems: PyTorch is used only as the allocator / stream provider;
the kernels see raw pointers through include/duet_ef.h."""

import numpy as np

from duet_amd import _lib

DEVICE_FIELDS = ('read_tag', 'cand_pos', 'cand_svlen', 'cand_svread', 'cand_refread', 'cand_gt_ok',
                 'cand_off', 'mark_read')


def upload(torch, device, a, dt=None):
    """Host array a (as dtype dt) -> a uint8 tensor of its bytes on the device, with 64 zero bytes behind them: kernels read
    past empty tables, so even an empty array has a readable address."""
    a = np.ascontiguousarray(a, dtype=dt)
    t = torch.zeros(a.nbytes + 64, dtype=torch.uint8, device=device)
    if a.nbytes:
        t[:a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(device)
    return t


class DeviceProblem(object):
    """An EfSoA uploaded once to HBM, plus output buffers, ready for repeated duet_ef_run_device."""

    def __init__(self, soa, svlen_thres, suppread_thres, device='cuda:0', misalign_marks=0, n_cands_max=None,
                 n_out=1, trailer=0, tag_guard=None):
        """tag_guard: tag words written directly behind read_tag, inside the same allocation (at most 8: the 64 bytes that
        follow every array) -- a kernel that reads the table at n_reads .. n_reads + 7 then reads these, not zeros."""
        import torch
        self.torch = torch
        self.soa = soa
        self.device = torch.device(device)
        self.buffers = {}
        ptrs = {}
        for name in DEVICE_FIELDS:
            a = getattr(soa, name)
            pad = misalign_marks if name == 'mark_read' else 0
            raw = torch.zeros(a.nbytes + pad + 64, dtype=torch.uint8, device=self.device)
            if a.nbytes:
                raw[pad:pad + a.nbytes] = torch.from_numpy(np.frombuffer(a.tobytes(), dtype=np.uint8).copy()).to(self.device)
            if name == 'read_tag' and tag_guard is not None:
                g = np.ascontiguousarray(tag_guard, dtype=np.uint64)
                assert g.nbytes <= 64
                raw[a.nbytes:a.nbytes + g.nbytes] = torch.from_numpy(g.view(np.uint8).copy()).to(self.device)
            self.buffers[name] = raw
            ptrs[name] = raw.data_ptr() + pad
        # results live in ONE block -- ps u32[n_max] then pred u8[n_max] -- so that a multi-GPU job can
        # hand the whole block to a single all-gather (duet_amd/dist.py)
        from duet_amd.dist import record_bytes
        self.n_max = max(int(n_cands_max or soa.n_cands), soa.n_cands, 1)
        # n_out > 1: rotating result blocks, so that the all-gather of one job can run beside the kernels of the next
        # (the blocks are slices of ONE allocation, so that several jobs' results can go into one collective)
        rb = record_bytes(self.n_max) + int(trailer)       # trailer: caller-defined bytes behind the records (status word)
        self.out_storage = torch.zeros(rb * max(1, n_out), dtype=torch.uint8, device=self.device)
        self.out_blocks = [self.out_storage[i * rb:(i + 1) * rb] for i in range(max(1, n_out))]
        self.out_block = self.out_blocks[0]
        self.problem = _lib.problem_from_device(soa, ptrs, svlen_thres, suppread_thres)

    def run(self, ctx, stream=None, slot=0):
        if stream is None:
            stream = self.torch.cuda.current_stream(self.device).cuda_stream
        blk = self.out_blocks[slot]
        ctx.run_device(self.problem, blk.data_ptr() + 4 * self.n_max, blk.data_ptr(), stream)
        return stream

    def joined_tags(self, ctx, min_sv, pc_cap=None, stream=None):
        """The read tags over joined phase sets, all on the device: the links under the problem's -s / -r and pc_cap (None: 8100;
        duet_ps_links_device), their blocks and the remap (duet_ps_join_links_device) into a second tag tensor -- no table visits
        the host.  -> (the tensor, dict(n_links, n_changed, n_rows, n_trusted, n_conflicts, n_components)).  The problem keeps its
        own tags: pointed_at(tensor) runs something on the remapped ones.  The tensor is the object's and is written again by the next
        call."""
        return _joined_tags(self, ctx, self.problem, self.buffers['read_tag'], self.soa.read_off, self.soa.n_marks, min_sv, stream,
                            lambda out, room, st: ctx.ps_links_device(self.problem, out, room, st, pc_cap=pc_cap))

    def pointed_at(self, tags):
        """Context manager: the problem reads `tags` (joined_tags) as its read tags; its own come back whatever happens inside."""
        return _pointed_at(self.problem, tags)

    def load_results(self, pred, ps, slot=0):
        """Put host (pred, ps) -- e.g. the merged records of a multi-GPU run -- into result block `slot`, so that the
        device-side row emission can read them."""
        torch = self.torch
        blk, C = self.out_blocks[slot], self.soa.n_cands
        if C:
            blk[:4 * C] = torch.from_numpy(np.ascontiguousarray(ps, dtype=np.uint32).view(np.uint8)).to(self.device)
            blk[4 * self.n_max:4 * self.n_max + C] = torch.from_numpy(np.ascontiguousarray(pred, dtype=np.uint8)).to(self.device)

    def results(self, slot=0):
        """-> (pred u8[C], ps u32[C]) on the host (synchronises)."""
        from duet_amd.dist import unpack_block
        return unpack_block(self.out_blocks[slot].cpu().numpy(), self.n_max, self.soa.n_cands)


def _joined_tags(obj, ctx, problem, own_tags, read_off, n_marks, min_sv, stream, links_into):
    torch = obj.torch
    if stream is None:
        stream = torch.cuda.current_stream(obj.device).cuda_stream
    if read_off is None:
        raise ValueError('joined_tags: the reads per contig (read_off) are not known to this object')
    # both tensors are kept across calls (the fit's cap axis calls this per line value): the records' room is not cleared, only
    # the records a call announces are read; the second tag tensor starts as a copy, so the words behind the reads are the same
    room = _lib.ps_links_room(n_marks)
    kept = getattr(obj, '_joined', None)
    if kept is None or kept[2] != own_tags.data_ptr():
        kept = obj._joined = (torch.empty(max(room, 1) * _lib.PS_LINK_DTYPE.itemsize, dtype=torch.uint8, device=obj.device),
                              own_tags.clone(), own_tags.data_ptr())
    links, tags = kept[0], kept[1]
    n_links = links_into(links.data_ptr(), room, stream)
    n_changed, counts = ctx.ps_join_links_device(links.data_ptr(), n_links, min_sv, own_tags.data_ptr(), read_off, problem.n_reads,
                                                 tags.data_ptr(), stream)
    return tags, dict(counts, n_links=n_links, n_changed=n_changed)


class _pointed_at(object):
    def __init__(self, problem, tags):
        self.problem, self.tags, self.mine = problem, tags, None

    def __enter__(self):
        self.mine = self.problem.read_tag
        self.problem.read_tag = self.tags.data_ptr()
        return self.tags

    def __exit__(self, *exc):
        self.problem.read_tag = self.mine
        return False


def device_rows(ctx, dp, rows, slot=0, stream=None):
    """Rows of phased_sv.vcf for the results in dp.out_blocks[slot], formatted on the device
    (duet_rows_run_device). `rows` = NativeIngest.rows().  -> (bytes of the rows, number of rows)."""
    torch = dp.torch
    if stream is None:
        stream = torch.cuda.current_stream(dp.device).cuda_stream
    soa = dp.soa
    keep = [upload(torch, dp.device, rows[k]) for k in ('pool', 'str_off', 'chrom_rank', 'plus')]
    ctg_off = np.ascontiguousarray(soa.cand_ctg_off, dtype=np.uint32)
    blk = dp.out_blocks[slot]
    p = _lib.RowsProblem()
    p.n_contigs, p.n_cands = soa.n_contigs, soa.n_cands
    p.cand_ctg_off = ctg_off.ctypes.data
    p.pred, p.ps = blk.data_ptr() + 4 * dp.n_max, blk.data_ptr()
    ef = dp.problem
    p.cand_pos, p.cand_svlen = ef.cand_pos, ef.cand_svlen
    p.cand_plus, p.cand_chrom_rank = keep[3].data_ptr(), keep[2].data_ptr()
    p.n_chrom_texts, p.max_pos = int(rows['n_chrom_texts']), int(rows['max_pos'])
    p.pool, p.pool_bytes, p.str_off = keep[0].data_ptr(), int(rows['pool_bytes']), keep[1].data_ptr()
    p.cand_off, p.mark_read, p.read_tag = ef.cand_off, ef.mark_read, ef.read_tag
    cap = int(rows['pool_bytes']) + 96 * soa.n_cands + 64
    out = torch.empty(cap, dtype=torch.uint8, device=dp.device)
    n, n_rows = ctx.rows_device(p, out.data_ptr(), cap, stream)
    return out[:n].cpu().numpy().tobytes(), n_rows


class DeviceCluster(object):
    """Raw SV marks uploaded once + result buffers, for repeated duet_cluster_run_device (stage A0)."""

    def __init__(self, marks, max_dist=0.9, part_gap=1000, part_max=100, normalizer=900.0, device='cuda:0'):
        import ctypes
        import torch
        self.torch = torch
        self.device = torch.device(device)
        M = len(marks['pos'])
        self.M = M
        self.keep = {}

        p = _lib.ClusterProblem()
        _lib.fill_cluster_problem(p, marks['contig'], marks['type'], marks['pos'], marks['span'], max_dist, part_gap, part_max, normalizer)
        for field, key, dt in (('mark_contig', 'contig', np.uint16), ('mark_type', 'type', np.uint8),
                               ('mark_pos', 'pos', np.uint32), ('mark_span', 'span', np.uint32)):
            self.keep[field] = upload(torch, self.device, marks[key], dt)
            setattr(p, field, self.keep[field].data_ptr())
        self.problem = p
        r = _lib.ClusterResult()
        sizes = dict(order=4 * M, cand_off=4 * (M + 1), cand_contig=2 * M, cand_type=M, cand_pos=4 * M, cand_span=4 * M,
                     n_cands=4)
        for k, nbytes in sizes.items():
            self.keep['out_' + k] = torch.zeros(nbytes + 64, dtype=torch.uint8, device=self.device)
            setattr(r, k, self.keep['out_' + k].data_ptr())
        self.result = r
        self._ct = ctypes

    def run(self, ctx, stream=None):
        if stream is None:
            stream = self.torch.cuda.current_stream(self.device).cuda_stream
        ct = self._ct
        rc = ctx.lib.duet_cluster_run_device(ctx.handle, ct.byref(self.problem), ct.byref(self.result),
                                             ct.c_void_p(stream))
        if rc:
            ctx._raise(rc)

    def n_cands(self):
        return int(self.keep['out_n_cands'][:4].cpu().numpy().view(np.uint32)[0])


class DeviceSvim(DeviceCluster):
    """Fused SVIM-mode pipeline on resident inputs: raw marks (+ their read indices), read tags, binned depth."""

    def __init__(self, marks, read_tag, depth, depth_off, depth_bin=1000, svlen_thres=50, suppread_thres=2,
                 max_dist=0.9, part_gap=1000, part_max=100, normalizer=900.0, device='cuda:0', read_off=None):
        """read_off: the reads of contig k are read_off[k] .. read_off[k + 1] (only joined_tags needs them)."""
        DeviceCluster.__init__(self, marks, max_dist=max_dist, part_gap=part_gap, part_max=part_max, normalizer=normalizer,
                               device=device)
        torch = self.torch
        self.read_off = None if read_off is None else np.ascontiguousarray(read_off, dtype=np.uint32)

        self.keep['sv_read'] = upload(torch, self.device, marks['read'], np.uint32)
        self.keep['sv_tag'] = upload(torch, self.device, read_tag, np.uint64)
        self.keep['sv_depth'] = upload(torch, self.device, depth, np.uint32)
        self.depth_off = np.ascontiguousarray(depth_off, dtype=np.uint32)
        p = _lib.SvimProblem()
        p.marks = self.problem
        p.mark_read = self.keep['sv_read'].data_ptr()
        p.read_tag = self.keep['sv_tag'].data_ptr()
        p.n_reads = len(read_tag)
        p.n_contigs = len(self.depth_off) - 1
        p.depth = self.keep['sv_depth'].data_ptr()
        p.depth_off = self.depth_off.ctypes.data
        p.depth_bin, p.svlen_thres, p.suppread_thres = int(depth_bin), int(svlen_thres), int(suppread_thres)
        self.sv_problem = p
        self.out_pred = torch.zeros(self.M + 64, dtype=torch.uint8, device=self.device)
        self.out_ps = torch.zeros(self.M + 16, dtype=torch.int32, device=self.device)
        self.n_found = 0
        self.feat, self.vector = None, None          # run_thresholds(keep_features=True): the candidates' features and its vector

    def run_fused(self, ctx, stream=None, wait=True):
        """wait=True: the call learns the candidate count (one host round trip inside).  wait=False: fully
        asynchronous; fetch() reads the count from the device."""
        if stream is None:
            stream = self.torch.cuda.current_stream(self.device).cuda_stream
        ct = self._ct
        n = ct.c_uint32(0)
        self.feat, self.vector = None, None          # (features of an earlier run_thresholds are not this run's)
        rc = ctx.lib.duet_svim_phase_device(ctx.handle, ct.byref(self.sv_problem), ct.byref(self.result),
                                            ct.c_void_p(self.out_pred.data_ptr()), ct.c_void_p(self.out_ps.data_ptr()),
                                            ct.byref(n) if wait else None, ct.c_void_p(stream))
        if rc:
            ctx._raise(rc)
        self.n_found = n.value if wait else None
        return stream

    def run_features(self, ctx, feat_ptr, stream=None, pc_cap=None):
        """duet_svim_features_device: clusters, adapts and writes the candidates' features to feat_ptr (room for M records);
        the cluster result stays in self.result.  -> the candidate count.  Raises ZeroDivisionError where E/F would.
        pc_cap: the features under that PC cap (duet_svim_features_cap_device)."""
        if stream is None:
            stream = self.torch.cuda.current_stream(self.device).cuda_stream
        self.n_found = None
        self.feat, self.vector = None, None
        self.n_found = ctx.svim_features_device(self.sv_problem, self.result, feat_ptr, stream, pc_cap=pc_cap)
        return self.n_found

    def run_thresholds(self, ctx, thresholds, stream=None, pc_cap=None, keep_features=False):
        """run_fused with the decision's 14 constants taken from `thresholds` (float64[14]): the candidates' features
        (duet_svim_features_device; pc_cap: under that PC cap), then the one vector applied to them (duet_tune_sweep_device) into
        out_pred / out_ps.  Raises ZeroDivisionError where the fused run would.  keep_features: the feature records stay resident
        for evidence_rows (56 bytes a candidate, until the next run of any kind on this object)."""
        torch = self.torch
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        vec = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(len(_lib.TUNE_NAMES))
        feat = torch.zeros(max(self.M, 1) * _lib.FEATURE_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
        d_vec = torch.from_numpy(vec.copy()).to(self.device)
        N = self.run_features(ctx, feat.data_ptr(), stream, pc_cap=pc_cap)
        ctx.apply_device(feat.data_ptr(), N, d_vec.data_ptr(), self.out_pred.data_ptr(), self.out_ps.data_ptr(), stream)
        torch.cuda.current_stream(self.device).synchronize()       # (d_vec, and feat unless kept, are released when this returns)
        if keep_features:
            self.feat, self.vector = feat, vec                     # (what evidence_rows reads)
        return stream

    def evidence_rows(self, ctx, chrom_texts, stream=None):
        """The data rows of the evidence table (_lib.EVIDENCE_COLUMNS) for the last run_thresholds' candidates: their leaves under
        its vector (duet_tune_leaves_device) and one row each in candidate order, formatted on the device from the resident
        features, cluster result and pred (duet_evidence_rows_device, the table form).  chrom_texts: CHROM text per contig.
        -> uint8 numpy array of the text."""
        torch = self.torch
        if self.feat is None:
            raise RuntimeError('evidence_rows needs run_thresholds(keep_features=True) as the last run on this object')
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        if self.n_found is None:
            self.n_found = self.n_cands()
        N = self.n_found
        if N == 0:
            return np.zeros(0, dtype=np.uint8)
        leaf = torch.zeros(N + 64, dtype=torch.uint8, device=self.device)
        pred = torch.zeros(N + 64, dtype=torch.uint8, device=self.device)
        ctx.leaves_device(self.feat.data_ptr(), N, self.vector, leaf.data_ptr(), pred.data_ptr(), stream)
        texts = _lib.chrom_bytes(chrom_texts)
        chrom = (self._ct.c_char_p * max(len(texts), 1))(*texts)
        p = _lib.EvidenceProblem()
        p.n_cands, p.n_contigs = N, len(texts)
        p.feat, p.leaf, p.pred = self.feat.data_ptr(), leaf.data_ptr(), pred.data_ptr()
        p.cand_pos, p.cand_svlen = self.result.cand_pos, self.result.cand_span
        p.cand_contig, p.cand_type = self.result.cand_contig, self.result.cand_type
        p.chrom = chrom
        cap = _lib.evidence_bound(N, max([len(c) for c in texts] + [0]))
        out = torch.empty(cap, dtype=torch.uint8, device=self.device)
        n = ctx.evidence_rows_device(p, out.data_ptr(), cap, stream)
        return out[:n].cpu().numpy()

    def ps_links(self, ctx, pc_cap=None, stream=None):
        """The phase-set links (_lib.PS_LINK_DTYPE, ascending by (contig, ps_a, ps_b)) of the candidates the resident marks cluster
        into (duet_svim_ps_links_device: it clusters again and leaves the same cluster result in self.result; out_pred / out_ps
        of an earlier run stay as they are).  pc_cap: the PC cap of the voters (None: 8100).  -> structured numpy array."""
        torch = self.torch
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        room = _lib.ps_links_room(self.M)
        out = torch.zeros(max(room, 1) * _lib.PS_LINK_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
        n, self.n_found = ctx.svim_ps_links_device(self.sv_problem, self.result, out.data_ptr(), room, stream, pc_cap=pc_cap)
        return out[:n * _lib.PS_LINK_DTYPE.itemsize].cpu().numpy().view(_lib.PS_LINK_DTYPE).copy()

    def read_tags(self, ctx, names, chrom_texts, pc_cap=None, stream=None):
        """The read tags of the last run's candidates and calls (duet_read_tags_device, duet_read_tags_rows_device), built on the
        resident arrays: the cluster result's cand_off / cand_contig / cand_pos, its `order` as the slots' raw marks, out_pred /
        out_ps, the marks' read indices and the read tags.  names: dict(mark_name, name_off, name_pool) of
        NativeIngest.extract(..., names=True); chrom_texts: CHROM text per contig; pc_cap: the cap of a usable tag (None: 8100).
        -> (records as a structured numpy array of _lib.READ_TAG_DTYPE, uint8 numpy array of the rows' text)."""
        torch = self.torch
        DT = _lib.READ_TAG_DTYPE
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        if self.n_found is None:
            self.n_found = self.n_cands()
        N = self.n_found
        if N == 0:
            return np.zeros(0, dtype=DT), np.zeros(0, dtype=np.uint8)
        keep = [upload(torch, self.device, names[k], dt) for k, dt in (('mark_name', np.uint32), ('name_off', np.uint64), ('name_pool', np.uint8))]
        p = _lib.ReadTagsProblem()
        p.n_cands, p.n_marks, p.n_reads, p.n_names = N, self.M, self.sv_problem.n_reads, len(names['name_off']) - 1
        p.cand_off, p.mark_order, p.cand_pos, p.cand_contig = self.result.cand_off, self.result.order, self.result.cand_pos, self.result.cand_contig
        p.mark_read, p.mark_name, p.read_tag = self.keep['sv_read'].data_ptr(), keep[0].data_ptr(), self.keep['sv_tag'].data_ptr()
        p.pred, p.ps = self.out_pred.data_ptr(), self.out_ps.data_ptr()
        recs = torch.zeros(max(self.M, 1) * DT.itemsize, dtype=torch.uint8, device=self.device)
        n = ctx.read_tags_device(p, recs.data_ptr(), self.M, stream, pc_cap=pc_cap)
        hold = []
        nm = _lib.callset_names(0, keep[1].data_ptr(), keep[2].data_ptr(), chrom_texts, hold)
        nm.n_names = p.n_names
        cap = _lib.read_tags_bound(n, names['name_off'], chrom_texts)
        text = torch.empty(max(cap, 1), dtype=torch.uint8, device=self.device)
        size = ctx.read_tags_rows_device(recs.data_ptr(), n, nm, p.read_tag, p.n_reads, text.data_ptr(), cap, stream)
        return recs[:n * DT.itemsize].cpu().numpy().view(DT).copy(), text[:size].cpu().numpy()

    def vcf_rows(self, ctx, names, chrom_texts, stream=None):
        """Rows of sv_calling/variants.vcf for the last run_fused's candidates, formatted on the device from the resident
        cluster result and depth (duet_svim_vcf_rows_device).  names: dict(mark_name, name_off, name_pool) of
        NativeIngest.extract(..., names=True); chrom_texts: CHROM text per contig.  -> uint8 numpy array of the text."""
        torch = self.torch
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        if self.n_found is None:
            self.n_found = self.n_cands()
        N = self.n_found
        if N == 0:
            return np.zeros(0, dtype=np.uint8)
        keep = [upload(torch, self.device, names[k], dt) for k, dt in (('mark_name', np.uint32), ('name_off', np.uint64), ('name_pool', np.uint8))]
        hold = []
        nm = _lib.callset_names(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), chrom_texts, hold)
        nm.n_names = len(names['name_off']) - 1
        cap = _lib.callset_bound(N, self.M, names['name_off'], chrom_texts)
        out = torch.empty(cap, dtype=torch.uint8, device=self.device)
        n = ctx.svim_vcf_rows_device(self.sv_problem, self.result, N, nm, out.data_ptr(), cap, stream)
        return out[:n].cpu().numpy()

    def joined_tags(self, ctx, min_sv, pc_cap=None, stream=None):
        """DeviceProblem.joined_tags for the fused pipeline: the links of the candidates the resident marks cluster into under the
        problem's -c / -s / -r and pc_cap (duet_svim_ps_links_device: it clusters again), their blocks and the remap
        (duet_ps_join_links_device).  Needs read_off.  -> (the second tag tensor, dict of counts)."""
        def links_into(out, room, st):
            n, self.n_found = ctx.svim_ps_links_device(self.sv_problem, self.result, out, room, st, pc_cap=pc_cap)
            return n
        return _joined_tags(self, ctx, self.sv_problem, self.keep['sv_tag'], self.read_off, self.M, min_sv, stream, links_into)

    def pointed_at(self, tags):
        """Context manager: the pipeline reads `tags` (joined_tags) as its read tags; its own come back whatever happens inside."""
        return _pointed_at(self.sv_problem, tags)

    def run_joined(self, ctx, blocks, read_off, thresholds=None, pc_cap=None, stream=None):
        """The last run again over joined phase sets (--join_ps): the read tags remapped under the table `blocks`
        (_lib.PS_BLOCK_DTYPE; duet_ps_join_tags_device) into a second tensor, the fused pipeline -- run_fused, or with thresholds /
        pc_cap run_thresholds -- on it, and the change code of every candidate between the two runs (duet_ps_join_diff_device).
        read_off: the reads of contig k are read_off[k] .. read_off[k + 1].  The object keeps the first run's (pred, ps), features and
        tags; clustering reads no tag, so the cluster result comes out byte for byte what it was (checked) and the candidates line up.
        Raises ZeroDivisionError where the joined run does.
        -> dict(pred, ps: device tensors of the joined run, change u8[N], counts u32[8], n_changed)."""
        torch = self.torch
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        if self.n_found is None:
            self.n_found = self.n_cands()
        N = self.n_found
        if thresholds is None and pc_cap is not None:
            thresholds = _lib.TUNE_DEFAULTS
        tags = torch.empty_like(self.keep['sv_tag'])
        n_changed = ctx.ps_join_tags_device(self.keep['sv_tag'].data_ptr(), read_off, self.sv_problem.n_reads, blocks, tags.data_ptr(),
                                            stream)
        names = ('order', 'cand_off', 'cand_contig', 'cand_type', 'cand_pos', 'cand_span', 'n_cands')
        before = [self.keep['out_' + k].clone() for k in names]
        mine = (self.out_pred, self.out_ps, self.feat, self.vector)
        self.out_pred, self.out_ps = torch.zeros_like(self.out_pred), torch.zeros_like(self.out_ps)
        self.sv_problem.read_tag = tags.data_ptr()
        try:
            if thresholds is not None:
                self.run_thresholds(ctx, thresholds, stream, pc_cap=pc_cap)
            else:
                self.run_fused(ctx, stream)
                ctx.check(stream)
            pred, ps = self.out_pred, self.out_ps
        finally:
            self.sv_problem.read_tag = self.keep['sv_tag'].data_ptr()
            self.out_pred, self.out_ps, self.feat, self.vector = mine
        if self.n_found != N or not all(torch.equal(a, self.keep['out_' + k]) for a, k in zip(before, names)):
            raise RuntimeError('run_joined: the cluster result changed between the two runs')
        change = torch.zeros(N + 64, dtype=torch.uint8, device=self.device)
        counts = ctx.ps_join_diff_device(N, self.out_pred.data_ptr(), self.out_ps.data_ptr(), pred.data_ptr(), ps.data_ptr(), blocks,
                                         self.sv_problem.n_contigs, change.data_ptr(), cand_contig_ptr=self.result.cand_contig,
                                         stream=stream)
        torch.cuda.current_stream(self.device).synchronize()
        return dict(pred=pred, ps=ps, change=change[:N].cpu().numpy(), counts=counts, n_changed=n_changed)

    def run_sv_tags(self, ctx, names, min_votes=1, pc_new=0, thresholds=None, pc_cap=None, stream=None):
        """The last run again with the untagged reads voting (--vote_sv_tags): one tag word per raw mark from the last run's calls
        (duet_sv_tags_device on the resident cluster result, marks and tags; names: dict(mark_name, ...) of
        NativeIngest.extract(..., names=True)), the problem pointed at those words through the identity index, the fused pipeline
        -- run_fused, or with thresholds / pc_cap run_thresholds -- on it, and the change code of every candidate between the two
        runs (duet_ps_join_diff_device under an empty table).  The object keeps the first run's (pred, ps), features and tags;
        clustering reads no tag, so the cluster result comes out byte for byte what it was (checked) and the candidates line up.
        Raises ZeroDivisionError where the second run does.
        -> dict(pred, ps: device tensors of the second run, change u8[N], counts u32[8], marks (n_untagged, n_given, n_own_only))."""
        torch = self.torch
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        if self.n_found is None:
            self.n_found = self.n_cands()
        N = self.n_found
        if thresholds is None and pc_cap is not None:
            thresholds = _lib.TUNE_DEFAULTS
        if N == 0:
            return dict(pred=torch.zeros_like(self.out_pred), ps=torch.zeros_like(self.out_ps), change=np.zeros(0, dtype=np.uint8),
                        counts=np.zeros(8, dtype=np.uint32), marks=(0, 0, 0))
        mark_name = upload(torch, self.device, names['mark_name'], np.uint32)
        p = _lib.ReadTagsProblem()
        p.n_cands, p.n_marks, p.n_reads, p.n_names = N, self.M, self.sv_problem.n_reads, len(names['name_off']) - 1
        p.cand_off, p.mark_order, p.cand_pos, p.cand_contig = self.result.cand_off, self.result.order, self.result.cand_pos, self.result.cand_contig
        p.mark_read, p.mark_name, p.read_tag = self.keep['sv_read'].data_ptr(), mark_name.data_ptr(), self.keep['sv_tag'].data_ptr()
        p.pred, p.ps = self.out_pred.data_ptr(), self.out_ps.data_ptr()
        tags = torch.zeros(max(self.M, 1) * 8, dtype=torch.uint8, device=self.device)
        index = torch.zeros(max(self.M, 1) * 4, dtype=torch.uint8, device=self.device)
        marks = ctx.sv_tags_device(p, tags.data_ptr(), index.data_ptr(), pc_cap=pc_cap, min_votes=min_votes, pc_new=pc_new, stream=stream)
        fields = ('order', 'cand_off', 'cand_contig', 'cand_type', 'cand_pos', 'cand_span', 'n_cands')
        before = [self.keep['out_' + k].clone() for k in fields]
        mine = (self.out_pred, self.out_ps, self.feat, self.vector)
        self.out_pred, self.out_ps = torch.zeros_like(self.out_pred), torch.zeros_like(self.out_ps)
        sp = self.sv_problem
        sp.read_tag, sp.mark_read, sp.n_reads = tags.data_ptr(), index.data_ptr(), self.M
        try:
            if thresholds is not None:
                self.run_thresholds(ctx, thresholds, stream, pc_cap=pc_cap)
            else:
                self.run_fused(ctx, stream)
                ctx.check(stream)
            pred, ps = self.out_pred, self.out_ps
        finally:
            sp.read_tag, sp.mark_read, sp.n_reads = self.keep['sv_tag'].data_ptr(), self.keep['sv_read'].data_ptr(), p.n_reads
            self.out_pred, self.out_ps, self.feat, self.vector = mine
        if self.n_found != N or not all(torch.equal(a, self.keep['out_' + k]) for a, k in zip(before, fields)):
            raise RuntimeError('run_sv_tags: the cluster result changed between the two runs')
        change = torch.zeros(N + 64, dtype=torch.uint8, device=self.device)
        counts = ctx.ps_join_diff_device(N, self.out_pred.data_ptr(), self.out_ps.data_ptr(), pred.data_ptr(), ps.data_ptr(),
                                         np.zeros(0, dtype=_lib.PS_BLOCK_DTYPE), self.sv_problem.n_contigs, change.data_ptr(),
                                         cand_contig_ptr=self.result.cand_contig, stream=stream)
        torch.cuda.current_stream(self.device).synchronize()
        return dict(pred=pred, ps=ps, change=change[:N].cpu().numpy(), counts=counts, marks=marks)

    def phased_rows(self, ctx, chrom_texts, stream=None, pred=None, ps=None):
        """Rows of phased_sv.vcf for the last run_fused's candidates, sorted and formatted on the device from the resident
        cluster result and (pred, ps) (duet_svim_phased_rows_device).  chrom_texts: CHROM text per contig.  pred, ps: device
        tensors of another run's calls over the same candidates (run_joined; default: the object's own).
        -> (uint8 numpy array of the text, number of rows)."""
        torch = self.torch
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        if self.n_found is None:
            self.n_found = self.n_cands()
        N = self.n_found
        if N == 0:
            return np.zeros(0, dtype=np.uint8), 0
        cap = _lib.phased_rows_bound(N, chrom_texts)
        out = torch.empty(cap, dtype=torch.uint8, device=self.device)
        pred, ps = self.out_pred if pred is None else pred, self.out_ps if ps is None else ps
        n, n_rows = ctx.svim_phased_rows_device(self.result, N, pred.data_ptr(), ps.data_ptr(), chrom_texts, out.data_ptr(), cap, stream)
        return out[:n].cpu().numpy(), n_rows

    def fetch(self):
        """-> dict of the cluster arrays + pred/ps, trimmed to the candidate count (synchronises)."""
        if self.n_found is None:
            self.n_found = self.n_cands()
        N, M = self.n_found, self.M
        g = lambda key, dt, n: self.keep['out_' + key][:n * np.dtype(dt).itemsize].cpu().numpy().view(dt)
        return dict(order=g('order', np.uint32, M), cand_off=g('cand_off', np.uint32, N + 1),
                    cand_contig=g('cand_contig', np.uint16, N), cand_type=g('cand_type', np.uint8, N),
                    cand_pos=g('cand_pos', np.uint32, N), cand_span=g('cand_span', np.uint32, N),
                    pred=self.out_pred[:N].cpu().numpy(), ps=self.out_ps[:N].cpu().numpy().view(np.uint32))


class DeviceTune(object):
    """What a sweep over settings (duet_amd/tune.py: sweep_settings) keeps in HBM: the truth side, the per-candidate key columns or
    the per-contig tables, the feature records, the six truth arrays, the vectors and the counts.  Features and truth arrays never
    leave the device; counts() brings the K count records back."""

    def __init__(self, n_max, base, refdist, ratio, vectors, device='cuda:0'):
        """n_max: the most candidates any setting can have; base: the truth side (tune.truth_side); vectors: float64[K, 14]."""
        import torch
        self.torch = torch
        self.device = torch.device(device)
        self.n_max = int(n_max)
        self.keep = {}
        p = _lib.TuneTruthProblem()
        for name, dt in _lib.TRUTH_PROBLEM_ARRAYS[-5:]:
            setattr(p, name, self._up(name, base[name], dt))
        p.n_keys, p.n_base, p.n_base_uid = len(base['base_off']) - 1, len(base['base_pos']), int(base['n_base_uid'])
        p.refdist, p.ratio = _lib.clamp_u32(refdist), float(ratio)
        self.problem = p
        n = max(self.n_max, 1)
        self.feat = torch.zeros(n * _lib.FEATURE_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
        self.truth = self._truth_arrays('')
        vec = np.ascontiguousarray(vectors, dtype=np.float64).reshape(-1, len(_lib.TUNE_NAMES))
        self.K = len(vec)
        self.vec_ptr = self._up('vectors', vec, np.float64)
        self.counts = torch.zeros(max(self.K, 1) * _lib.COUNTS_DTYPE.itemsize, dtype=torch.uint8, device=self.device)

    def _up(self, name, a, dt):
        self.keep[name] = upload(self.torch, self.device, a, dt)
        return self.keep[name].data_ptr()

    def _truth_arrays(self, tag):
        """A TuneTruth over six resident arrays of their own, sized for n_max candidates."""
        n, t = max(self.n_max, 1), _lib.TuneTruth()
        for name, dt in _lib.TRUTH_ARRAYS:
            self.keep[name + tag] = self.torch.zeros((n + 1) * np.dtype(dt).itemsize, dtype=self.torch.uint8, device=self.device)
            setattr(t, name, self.keep[name + tag].data_ptr())
        return t

    def stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def set_candidates(self, cand_pos, cand_len, cand_key, cand_chrom, n_chrom):
        """The per-candidate form: the columns of a callset, uploaded once."""
        p = self.problem
        for name, a in (('cand_pos', cand_pos), ('cand_len', cand_len), ('cand_key', cand_key), ('cand_chrom', cand_chrom)):
            setattr(p, name, self._up(name, a, np.uint32))
        p.n_chrom = int(n_chrom)

    def set_tables(self, key_table, chrom_id, n_chrom, bed=None):
        """The table form (a cluster result): per contig the four list keys and the CHROM id; bed = (bed_off, bed_lo, bed_hi)."""
        p = self.problem
        p.cand_key, p.cand_chrom = None, None
        p.key_table, p.chrom_id = self._up('key_table', key_table, np.uint32), self._up('chrom_id', chrom_id, np.uint32)
        p.n_contigs, p.n_chrom = len(chrom_id), int(n_chrom)
        if bed is not None:
            p.bed_off, p.bed_lo, p.bed_hi = (self._up(k, a, np.uint32) for k, a in zip(('bed_off', 'bed_lo', 'bed_hi'), bed))

    def build(self, ctx, n_cands, result=None, truth=None):
        """The truth arrays of the features in self.feat (duet_tune_truth_build_device).  result: the ClusterResult whose
        candidate columns the table form reads.  truth: the arrays to fill (a pass's own, see set_strata) instead of self.truth."""
        p = self.problem
        p.n_cands, p.feat = int(n_cands), self.feat.data_ptr()
        if result is not None:
            p.cand_contig, p.cand_type, p.cand_pos, p.cand_len = result.cand_contig, result.cand_type, result.cand_pos, result.cand_span
        ctx.truth_build_device(p, truth if truth is not None else self.truth, self.stream())

    def _sweep(self, ctx, n_cands, vec_ptr, K, counts):
        """K vectors at vec_ptr over the features and truth arrays of the last build, through `counts` -> COUNTS_DTYPE[K] on the host."""
        ctx.sweep_device(self.feat.data_ptr(), int(n_cands), vec_ptr, K, self.truth, counts.data_ptr(), self.stream())
        return counts[:K * _lib.COUNTS_DTYPE.itemsize].cpu().numpy().view(_lib.COUNTS_DTYPE).copy()

    def sweep(self, ctx, n_cands):
        """The K vectors over the features and truth arrays of the last build -> COUNTS_DTYPE[K] on the host."""
        return self._sweep(ctx, n_cands, self.vec_ptr, self.K, self.counts)

    def set_strata(self, chrom_stratum, uid_off, base_uid=None, own_truth=False):
        """One stratified pass (tune.truth_side(strata=...), tune.chrom_strata): chrom_stratum u8[n_chrom], uid_off u32[S + 1] and
        the truth side's base_uid numbered per (stratum, id text).  -> the pass, for build() and sweep_strata(); its arrays stay
        resident like the rest, and several passes can be set side by side.  own_truth: build_strata fills truth arrays of the
        pass's own, so that plain and stratified sweeps can alternate after one build of each (the fit)."""
        torch = self.torch
        uid_off = np.ascontiguousarray(uid_off, dtype=np.uint32)
        S, n = len(uid_off) - 1, max(self.n_max, 1)
        i = len([k for k in self.keep if k.startswith('chrom_stratum')])
        st = _lib.TuneStrata()
        st.n_strata = S
        for name in ('cand_stratum', 'group_stratum'):
            self.keep['%s%d' % (name, i)] = t = torch.zeros(n + 64, dtype=torch.uint8, device=self.device)
            setattr(st, name, t.data_ptr())
        st.uid_off = uid_off.ctypes.data
        p = dict(strata=st, uid_off=uid_off, n_base_uid=int(uid_off[-1]),
                 chrom_stratum=self._up('chrom_stratum%d' % i, chrom_stratum, np.uint8),
                 base_uid=self._up('base_uid%d' % i, base_uid, np.uint32) if base_uid is not None else self.problem.base_uid,
                 counts=torch.zeros(max(self.K * S, 1) * _lib.COUNTS_DTYPE.itemsize, dtype=torch.uint8, device=self.device))
        if own_truth:
            p['truth'] = self._truth_arrays('_strata%d' % i)
        self.strata = p
        return p

    def build_strata(self, ctx, n_cands, result=None, strata=None):
        """build() with the pass's truth-id numbering, then the strata of the candidates and groups
        (duet_tune_strata_build_device).  The truth arrays are the pass's from here on: a plain sweep() goes before it -- unless
        the pass has truth arrays of its own (set_strata(own_truth=True))."""
        s, p = strata or self.strata, self.problem
        truth = s.get('truth', self.truth)
        plain = p.base_uid, p.n_base_uid
        p.base_uid, p.n_base_uid = s['base_uid'], s['n_base_uid']
        try:
            self.build(ctx, n_cands, result, truth)
        finally:
            p.base_uid, p.n_base_uid = plain
        ctx.strata_build_device(p, truth, s['chrom_stratum'], s['strata'].n_strata, s['strata'].cand_stratum,
                                s['strata'].group_stratum, self.stream())

    def _sweep_strata(self, ctx, n_cands, vec_ptr, K, s, counts):
        """K vectors at vec_ptr over the features and the truth arrays of the last build_strata of pass s, through `counts`
        -> COUNTS_DTYPE[K, S] on the host."""
        S = s['strata'].n_strata
        ctx.sweep_strata_device(self.feat.data_ptr(), int(n_cands), vec_ptr, K, s.get('truth', self.truth), s['strata'],
                                counts.data_ptr(), self.stream())
        return counts[:K * S * _lib.COUNTS_DTYPE.itemsize].cpu().numpy().view(_lib.COUNTS_DTYPE).reshape(K, S).copy()

    def sweep_strata(self, ctx, n_cands, strata=None):
        """The K vectors over the features and the truth arrays of the last build_strata -> COUNTS_DTYPE[K, S] on the host."""
        s = strata or self.strata
        return self._sweep_strata(ctx, n_cands, self.vec_ptr, self.K, s, s['counts'])

    def leaf_census(self, ctx, n_cands, vectors=None, strata=None):
        """The leaf census (duet_tune_leaf_census_device) over the resident features: `vectors` (float64[K, 14], uploaded; None:
        the resident grid) over the truth arrays of the last build -- or, with strata (a pass of set_strata), over those of the
        last build_strata of that pass, one record per stratum -> LEAF_COUNTS_DTYPE[K, S, N_LEAVES] on the host."""
        torch, rec = self.torch, _lib.LEAF_COUNTS_DTYPE.itemsize * _lib.N_LEAVES
        if vectors is None:
            K, vec_ptr = self.K, self.vec_ptr
        else:
            vec = np.ascontiguousarray(vectors, dtype=np.float64).reshape(-1, len(_lib.TUNE_NAMES))
            K, vec_ptr = len(vec), self._up('leaf_vectors', vec, np.float64)
        S = strata['strata'].n_strata if strata is not None else 1
        if getattr(self, 'leaf_counts', None) is None or self.leaf_counts.numel() < K * S * rec:
            self.leaf_counts = torch.zeros(max(K * S, 1) * rec, dtype=torch.uint8, device=self.device)
        truth = strata.get('truth', self.truth) if strata is not None else self.truth
        ctx.leaf_census_device(self.feat.data_ptr(), int(n_cands), vec_ptr, K, truth, strata['strata'] if strata is not None else None,
                               self.leaf_counts.data_ptr(), self.stream())
        return self.leaf_counts[:K * S * rec].cpu().numpy().view(_lib.LEAF_COUNTS_DTYPE).reshape(K, S, _lib.N_LEAVES).copy()

    # -- the line of one axis (tune.fit): a block of n_max + 2 vectors next to the grid's, made on the device --------------------
    VEC_BYTES = 8 * len(_lib.TUNE_NAMES)

    def _line_block(self):
        """The line block and its counts, allocated on first use."""
        if getattr(self, 'line_vec', None) is None:
            n = self.n_max + 2
            self.line_vec = self.torch.zeros(n * self.VEC_BYTES, dtype=self.torch.uint8, device=self.device)
            self.line_counts = self.torch.zeros(n * _lib.COUNTS_DTYPE.itemsize, dtype=self.torch.uint8, device=self.device)
        return self.line_vec

    def line(self, ctx, n_cands, base, axis, max_values=0):
        """The line of `axis` through `base` (float64[14], host) from the resident features (duet_tune_line_device) into the
        line block, and `base` itself behind its n_vec vectors, so that one sweep scores the current vector in the same batch.
        -> (n_vec, n_distinct).  Raises ZeroDivisionError where a compared feature is not finite."""
        base = np.ascontiguousarray(base, dtype=np.float64).reshape(len(_lib.TUNE_NAMES))
        n_vec, n_distinct = ctx.line_device(self.feat.data_ptr(), int(n_cands), base, axis, max_values, self._line_block().data_ptr(),
                                            self.stream())
        self.set_line_vector(base, n_vec)
        return n_vec, n_distinct

    def line_value(self, i, axis):
        """The value of field `axis` (index) in vector i of the line block."""
        at = i * self.VEC_BYTES + 8 * int(axis)
        return float(self.line_vec[at:at + 8].cpu().numpy().view(np.float64)[0])

    def sweep_line(self, ctx, n_cands, first, K):
        """Vectors first .. first + K of the line block over the features and truth arrays of the last build
        -> COUNTS_DTYPE[K] on the host."""
        return self._sweep(ctx, n_cands, self.line_vec.data_ptr() + first * self.VEC_BYTES, K, self.line_counts)

    def sweep_line_strata(self, ctx, n_cands, first, K, strata=None):
        """The same per stratum, over the truth arrays of the last build_strata -> COUNTS_DTYPE[K, S] on the host."""
        s = strata or self.strata
        if s.get('line_counts') is None:
            s['line_counts'] = self.torch.zeros((self.n_max + 2) * s['strata'].n_strata * _lib.COUNTS_DTYPE.itemsize, dtype=self.torch.uint8,
                                                device=self.device)
        return self._sweep_strata(ctx, n_cands, self.line_vec.data_ptr() + first * self.VEC_BYTES, K, s, s['line_counts'])

    # -- the line of the PC cap (tune.fit's pc_cap axis) -------------------------------------------------------------------------
    def cap_line(self, ctx, prob, max_values=0):
        """The line of the PC cap of a resident problem -- an EfProblem (duet_tune_cap_line_device) or a SvimProblem
        (duet_svim_cap_line_device: its raw marks) -- brought to the host: -> (caps u32[n_caps] ascending, D, whether they are
        the whole line).  max_values as for line()."""
        torch = self.torch
        svim = isinstance(prob, _lib.SvimProblem)
        entry = ctx.svim_cap_line_device if svim else ctx.cap_line_device

        def run(N, fetch=True):
            room = _lib.cap_line_room(prob.marks.n_marks if svim else prob.n_marks, N)
            if getattr(self, 'cap_vals', None) is None or self.cap_vals.numel() < room:
                self.cap_vals = torch.zeros(room, dtype=torch.int32, device=self.device)
            n, D = entry(prob, N, self.cap_vals.data_ptr(), self.stream())
            return (self.cap_vals[:n].cpu().numpy().view(np.uint32).copy() if fetch else n), D

        N = int(max_values)
        caps, D = run(N)
        if N < 2 or len(caps) < N or D + 1 == N:
            return caps, D, True
        if D > N:
            return caps, D, False
        # N values came back and D == N: the whole line when it has no 0 in front (L = D), a sample of D + 1 values otherwise --
        # both start with 0 and end with x_D, and the entry reports D, not L: the one case in which they cannot be told apart asks
        # once more, for one value more, and reads only how many came (nothing is downloaded)
        return caps, D, run(N + 1, fetch=False)[0] == N

    def set_line_vector(self, base, i=0):
        """`base` (float64[14], host) as vector i of the line block; i = 0: what sweep_line(ctx, n, 0, 1) then scores."""
        base = np.ascontiguousarray(base, dtype=np.float64).reshape(len(_lib.TUNE_NAMES))
        self._line_block()[i * self.VEC_BYTES:(i + 1) * self.VEC_BYTES] = self.torch.from_numpy(base.view(np.uint8).copy()).to(self.device)

    def features_host(self, n_cands):
        """(--features) the feature records of the last setting, on the host."""
        return self.feat[:int(n_cands) * _lib.FEATURE_DTYPE.itemsize].cpu().numpy().view(_lib.FEATURE_DTYPE).copy()
