# coding=utf-8
"""The read names of the caller VCF's marks (duet_ingest_keep_mark_names before duet_ingest_parse_vcf*; NativeIngest.load(...,
names=True)) against the RNAMES / READS lists of the Python host path, mark for mark.  No GPU."""
import ctypes
import shutil

import numpy as np
import pytest

from duet_amd import native, read_tags
from duet_amd import sv_phasing_fn as F
from duet_amd.read_file import init_chrom_list
from tests import helpers as H
from tests.test_c_oracle import materialise_bams
from tests.test_native_ingest import REC, SAM, _tiny_case

CHROMS = init_chrom_list(False, '')


def load(home, names=True, thread=4):
    ing = native.NativeIngest.load(home + '/sv_calling/variants.vcf', home + '/snp_phasing/', CHROMS, thread, names=names)
    assert ing is not None and ing.handle, getattr(ing, 'why', 'library missing')
    return ing


@pytest.mark.parametrize('name,src,params', H.full_cases(), ids=[c[0] for c in H.full_cases()])
def test_names_of_the_golden_work_dirs(name, src, params, tmp_path):
    home = str(tmp_path / name)
    shutil.copytree(src, home)
    materialise_bams(home)
    ing = load(home)
    tab, soa = F.generate_callinfo(home + '/sv_calling/variants.vcf', F.read_hap_bam(home + '/snp_phasing/', 4, False), False)
    nm = ing.mark_names()
    texts = read_tags.names_of(nm['name_off'], nm['name_pool'])
    want = [n.encode() for names in tab.names for n in names]
    assert len(nm['mark_name']) == soa.n_marks == len(want) and len(want) > 0
    assert [texts[i] for i in nm['mark_name']] == want                  # mark for mark, the order of mark_read
    assert np.array_equal(ing.soa.mark_read, soa.mark_read)
    # interned per contig: inside a contig one name has one index, and so one read index; the pool holds each entry once
    mark_contig = np.repeat(np.repeat(np.arange(soa.n_contigs), np.diff(soa.cand_ctg_off)), np.diff(soa.cand_off))
    seen = {}
    for k, i, r in zip(mark_contig.tolist(), nm['mark_name'].tolist(), soa.mark_read.tolist()):
        assert seen.setdefault(i, (k, r)) == (k, r)
    assert len(set((k, texts[i]) for i, (k, _) in seen.items())) == len(seen) == len(texts)
    assert any(r == 0xFFFFFFFF for _, r in seen.values())               # an untagged read has a name
    assert max(np.bincount(nm['mark_name'])) > 1                        # the same read in two marks has one index
    assert int(nm['name_off'][-1]) == len(nm['name_pool']) == sum(len(t) for t in texts)
    # the parse itself is what it is without the names
    plain = load(home, names=False)
    for field, _ in type(soa).FIELDS:
        assert np.array_equal(getattr(plain.soa, field), getattr(ing.soa, field)), field
    with pytest.raises(RuntimeError, match='no names were kept'):
        plain.mark_names()
    plain.close()
    ing.close()


def test_untagged_reads_and_repeats(tmp_path):
    second = REC.replace('\t100\t', '\t300\t').replace('RNAMES=a,b', 'RNAMES=b,c,a,b,')
    home = _tiny_case(tmp_path, [REC, second], SAM)
    ing = load(home, thread=1)
    nm = ing.mark_names()
    assert nm['mark_name'].tolist() == [0, 1, 1, 2, 0, 1, 3]            # in order of first mark; b twice in one candidate
    assert read_tags.names_of(nm['name_off'], nm['name_pool']) == [b'a', b'b', b'c', b'']      # ','.split keeps the empty name
    assert ing.soa.mark_read.tolist() == [0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0xFFFFFFFF, 0xFFFFFFFF]
    ing.close()


def test_opt_in_comes_before_the_parse(tmp_path):
    home = _tiny_case(tmp_path, [REC], SAM)
    lib = native.load()
    labels = (ctypes.c_char_p * len(CHROMS))(*[c.encode() for c in CHROMS])
    h = lib.duet_ingest_create(len(CHROMS), labels)
    try:
        out = native.IngestMarkNames()
        assert lib.duet_ingest_get_mark_names(h, ctypes.byref(out)) != native.OK             # nothing parsed
        assert lib.duet_ingest_parse_vcf(h, (home + '/sv_calling/variants.vcf').encode(), 1) == native.OK
        assert lib.duet_ingest_get_mark_names(h, ctypes.byref(out)) != native.OK             # no opt-in: nothing was kept
        assert lib.duet_ingest_keep_mark_names(h, 1) != native.OK                            # ... and it is too late for it
        assert b'after the caller VCF was parsed' in lib.duet_ingest_error(h)
    finally:
        lib.duet_ingest_destroy(h)
    h = lib.duet_ingest_create(len(CHROMS), labels)
    try:
        assert lib.duet_ingest_keep_mark_names(h, 1) == native.OK
        assert lib.duet_ingest_parse_vcf(h, (home + '/sv_calling/variants.vcf').encode(), 1) == native.OK
        out = native.IngestMarkNames()
        assert lib.duet_ingest_get_mark_names(h, ctypes.byref(out)) == native.OK
        assert (out.n_marks, out.n_names, out.pool_bytes) == (2, 2, 2)                         # a, b: no BAM was added, both untagged
        # a second parse on the same object starts the names afresh
        assert lib.duet_ingest_parse_vcf(h, (home + '/sv_calling/variants.vcf').encode(), 1) == native.OK
        assert lib.duet_ingest_get_mark_names(h, ctypes.byref(out)) == native.OK
        assert (out.n_marks, out.n_names, out.pool_bytes) == (2, 2, 2)
    finally:
        lib.duet_ingest_destroy(h)
