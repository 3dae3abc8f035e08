# coding=utf-8
"""Hostile inputs for the native ingest (libduet_ingest.so), as data: every case's bytes are put together from the formats
themselves (RFC 1952 / SAMv1 4.1 for BGZF, SAMv1 4.2 for BAM, the caller VCF's lines), with the hand-written helpers of
tests/test_bam_spec.py and nothing of the repository's own BAM writer.  No test lives here: tests/test_ingest_hostile.py runs the
cases against the normal library, one child process per case, and tools/ingest_hostile_check.cpp runs them under the host
sanitizers from the manifest this module writes:

    python -m tests.ingest_hostile OUTDIR          the files of every case + OUTDIR/manifest.tsv (name, path, mode, status)

A case is (name, files, expectation): files = [(file name, bytes)], expectation = decline(<substring of the reason>) -- the native
path returns DUET_INGEST_UNSUPPORTED (or the stated status) and says why -- or ACCEPT: the native path builds what the Python
reader builds.  Where a case holds several files, the expectation is every file's (one family, e.g. a member cut at each of its
first 18 bytes).  cases() yields them; they are built on demand (REGISTRY keeps name, mode and a builder).

Modes (the manifest's third column):  bam:threads=T  one BAM as contig 1's;  extract:bin=W  the same with SVIM-mode extraction;
bams:threads=T:contigs=a,b,..  several files in one duet_ingest_add_bams call (`-` = a path that does not exist);
vcf:threads=T  a caller VCF."""
import collections
import os
import struct
import sys
import zlib

from tests.test_bam_spec import CIG_CODE, EOF_MEMBER, REFS, aux, bgzf_member, record

OK, UNSUPPORTED, IO = 0, 1, -1
PC_SAT = (1 << 30) - 2                             # kPcSat of duet_ingest.cpp / engine.pack_tags
ACCEPT = ('accept', '', OK)


def decline(why, status=UNSUPPORTED):
    return ('decline', why, status)


Entry = collections.namedtuple('Entry', 'name group mode build expect names')
REGISTRY = collections.OrderedDict()


def case(name, group, build, expect, mode='bam:threads=1', names=('r1',)):
    assert name not in REGISTRY, name
    REGISTRY[name] = Entry(name, group, mode, build, expect, tuple(names))


def cases():
    for e in REGISTRY.values():
        yield e.name, e.build(), e.expect


# ---------------------------------------------------------------------------------------------------------------------------
# pieces
# ---------------------------------------------------------------------------------------------------------------------------
u16 = lambda v: struct.pack('<H', v)
u32 = lambda v: struct.pack('<I', v)


def deflate(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def gz(extra, body, data=b'', isize=None, flg=4, xlen=None):
    """One gzip member around `body`: FLG, the extra field as given (XLEN as given, else its length), CRC32 and ISIZE of `data`."""
    x = (u16(len(extra) if xlen is None else xlen) + extra) if flg & 4 else b''
    return bytes([31, 139, 8, flg, 0, 0, 0, 0, 0, 255]) + x + body + u32(zlib.crc32(data) & 0xFFFFFFFF) + u32(len(data) if isize is None else isize)


def bc(bsize, slen=2):
    return b'BC' + u16(slen) + u16(bsize)


def member(data, isize=None, bsize_add=0, extra_before=b'', level=6):
    body = deflate(data, level)
    total = 12 + len(extra_before) + 6 + len(body) + 8
    return gz(extra_before + bc(total - 1 + bsize_add), body, data, isize)


def header(refs=REFS, text=b'@HD\tVN:1.6\tSO:coordinate\n'):
    h = b'BAM\1' + u32(len(text)) + text + u32(len(refs))
    for name, ln in refs:
        h += u32(len(name) + 1) + name.encode() + b'\0' + u32(ln)
    return h


def bam(payload, cuts=()):
    """The payload in BGZF members cut at the given offsets (and every 60000 bytes), then the end-of-file marker."""
    at = [0] + sorted(c for c in set(cuts) | set(range(60000, len(payload), 60000)) if 0 < c < len(payload)) + [len(payload)]
    return b''.join(bgzf_member(payload[a:b]) for a, b in zip(at, at[1:])) + EOF_MEMBER


def hp(v, t='C'):
    return aux('HP', t, struct.pack('<' + {'c': 'b', 'C': 'B', 's': 'h', 'S': 'H', 'i': 'i', 'I': 'I'}[t], v))


PC300 = aux('PC', 'S', u16(300))
PS1E5 = aux('PS', 'I', u32(100000))
TAGS = hp(1) + PC300 + PS1E5


def rec(name='r1', tags=TAGS, flag=0, pos1=1000, cigar=((8, 'M'),), seq='ACGTACGT', qual='*', ref_id=0, mapq=60):
    return record(name, flag, ref_id, pos1, mapq, list(cigar), seq, qual, tags)


def one(blob, fname='chr1.bam'):
    return lambda: [(fname, blob() if callable(blob) else blob)]


def family(blobs):
    """-> builder of one file per blob, chr1.bam in a folder of its own each (see the runner)"""
    return lambda: [('%02d/chr1.bam' % i, b) for i, b in enumerate(blobs() if callable(blobs) else blobs)]


GOOD = header() + rec()


# ---------------------------------------------------------------------------------------------------------------------------
# BGZF layer
# ---------------------------------------------------------------------------------------------------------------------------
def _defect1(extra_bytes):
    # XLEN = 10: a complete BC subfield, then the 4-byte header of a second one (SLEN = 2) that ends exactly at the extra field's end
    return bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255]) + u16(10) + bc(21) + b'BC' + u16(2) + b'\0' * extra_bytes


def _valid():
    return member(GOOD)


def _one_corrupt(n, bad):
    """n data members (the record stream cut into n pieces) with the deflate body of member `bad` damaged"""
    payload = header() + b''.join(rec('q%d' % i) for i in range(4 * n))
    step = len(payload) // n
    ms = [bytearray(bgzf_member(payload[i * step:(i + 1) * step if i < n - 1 else len(payload)])) for i in range(n)]
    ms[bad][18] |= 0x07                                # BTYPE = 3, the reserved block type: no inflate gets past it
    return b''.join(bytes(m) for m in ms) + EOF_MEMBER


def _empty_member(isize):
    m = bytearray(EOF_MEMBER)
    m[-4:] = u32(isize)
    return bytes(m)


G = 'bgzf'
case('bgzf_subfield_header_at_extra_end', G, one(_defect1(0)), decline('truncated BGZF block'))
case('bgzf_subfield_header_at_extra_end_plus1', G, one(_defect1(1)), decline('truncated BGZF block'))
case('bgzf_subfield_header_at_extra_end_plus2', G, one(_defect1(2)), decline('truncated BGZF block'))
case('bgzf_xlen_past_eof', G, one(lambda: gz(bc(27), deflate(b''), xlen=60000)), decline('gzip member without BGZF block size'))
case('bgzf_xlen_zero', G, one(lambda: gz(b'', deflate(GOOD), GOOD)), decline('gzip member without BGZF block size'))
case('bgzf_extra_without_bc', G, one(lambda: gz(b'XY' + u16(2) + u16(40), deflate(GOOD), GOOD)), decline('gzip member without BGZF block size'))
case('bgzf_bc_slen_1', G, one(lambda: gz(b'BC' + u16(1) + b'\x28', deflate(GOOD), GOOD)), decline('gzip member without BGZF block size'))
case('bgzf_bc_slen_3', G, one(lambda: gz(b'BC' + u16(3) + b'\x28\0\0', deflate(GOOD), GOOD)), decline('gzip member without BGZF block size'))
case('bgzf_bsize_below_header', G, one(lambda: gz(bc(24), deflate(GOOD), GOOD)), decline('truncated BGZF block'))
case('bgzf_bsize_one_past_eof', G, one(lambda: member(GOOD, bsize_add=1)), decline('truncated BGZF block'))
case('bgzf_cut_in_first_18_bytes', G, family(lambda: [_valid()[:k] for k in range(1, 19)]), decline('BGZF'))
case('bgzf_cut_in_deflate_body', G, one(lambda: _valid()[:18 + 20]), decline('truncated BGZF block'))
case('bgzf_cut_in_trailer', G, family(lambda: [_valid()[:-k] for k in range(1, 8)]), decline('truncated BGZF block'))
case('bgzf_isize_65537', G, one(lambda: member(GOOD, isize=65537) + EOF_MEMBER), decline('ISIZE above 65536'))
case('bgzf_isize_smaller', G, one(lambda: member(GOOD, isize=len(GOOD) - 1) + EOF_MEMBER), decline('BGZF inflate failed'))
case('bgzf_isize_larger', G, one(lambda: member(GOOD, isize=len(GOOD) + 1) + EOF_MEMBER), decline('BGZF inflate failed'))
case('bgzf_isize_zero_on_a_full_body', G, one(lambda: member(GOOD, isize=0) + EOF_MEMBER), decline('BGZF inflate failed'))
case('bgzf_100000_members_isize_ffffffff', G, one(lambda: _empty_member(0xFFFFFFFF) * 100000), decline('ISIZE above 65536'))
case('bgzf_2000_members_isize_ffffffff', G, one(lambda: _empty_member(0xFFFFFFFF) * 2000), decline('ISIZE above 65536'))
case('bgzf_2000_members_isize_65536', G, one(lambda: _empty_member(65536) * 2000), decline('ISIZE above what its body can inflate to'))
for _n, _bad, _where in ((9, 0, 'first'), (9, 4, 'middle'), (9, 8, 'last')):
    for _t in (1, 4):
        case('bgzf_9_members_%s_corrupt_t%d' % (_where, _t), G, one(lambda n=_n, bad=_bad: _one_corrupt(n, bad)),
             decline('BGZF inflate failed'), mode='bam:threads=%d' % _t)
case('bgzf_plain_gzip_member', G, one(lambda: gz(b'', deflate(GOOD), GOOD, flg=0)), decline('not a BGZF stream'))
case('bgzf_empty_file', G, one(b''), ACCEPT)
case('bgzf_9_members_sound_t4', G, one(lambda: bam(header() + b''.join(rec('q%d' % i) for i in range(36)), cuts=range(100, 1800, 200))),
     ACCEPT, mode='bam:threads=4', names=('q0', 'q35', 'zz'))

# ---------------------------------------------------------------------------------------------------------------------------
# BAM header
# ---------------------------------------------------------------------------------------------------------------------------
G = 'header'
case('header_inflated_0_to_11_bytes', G, family(lambda: [bam(GOOD[:k]) if k else bgzf_member(b'') + EOF_MEMBER for k in range(12)]),
     decline('not a BAM file'))
case('header_wrong_magic', G, one(lambda: bam(b'BAM\2' + GOOD[4:])), decline('not a BAM file'))
case('header_l_text_past_end', G, one(lambda: bam(b'BAM\1' + u32(5000) + b'@HD\n' + u32(0))), decline('truncated BAM header'))
case('header_n_ref_ffffffff', G, one(lambda: bam(b'BAM\1' + u32(0) + u32(0xFFFFFFFF))), decline('truncated BAM header'))
case('header_ref_l_name_past_end', G, one(lambda: bam(b'BAM\1' + u32(0) + u32(1) + u32(500) + b'chr1\0' + u32(1000))),
     decline('truncated BAM header'))
case('header_ends_after_n_ref', G, one(lambda: bam(b'BAM\1' + u32(0) + u32(0))), ACCEPT)


# ---------------------------------------------------------------------------------------------------------------------------
# record framing
# ---------------------------------------------------------------------------------------------------------------------------
def _fixed(block_size=None, l_name=3, n_cig=0, l_seq=0, body=b'r1\0'):
    """A record whose 32 fixed bytes are written out here, followed by `body` (name, CIGAR, SEQ, QUAL, aux as the case wants)"""
    core = struct.pack('<iiBBHHHIiii', 0, 999, l_name, 60, 0, n_cig, 0, l_seq, -1, -1, 0)
    return u32(len(core) + len(body) if block_size is None else block_size) + core + body


def _ends_at(field, over):
    """l_read_name / n_cigar_op / l_seq chosen so that name + CIGAR + SEQ + QUAL end `over` bytes past the record's end (no aux)"""
    if field == 'l_read_name':
        return _fixed(l_name=40 + over, body=b'n' * 39 + b'\0')
    if field == 'n_cigar_op':
        return _fixed(n_cig=5 + (1 if over else 0), body=b'r1\0' + u32((8 << 4) | 0) * 5 + (b'\0' * 3 if over else b''))
    return _fixed(l_seq=10 + (1 if over else 0), body=b'r1\0' + b'\x11' * 5 + b'\xff' * 10 + (b'' if not over else b'\0'))


G = 'framing'
case('rec_block_size_0', G, one(lambda: bam(header() + u32(0) + rec())), decline('truncated BAM record'))
case('rec_block_size_31', G, one(lambda: bam(header() + _fixed(block_size=31, l_name=0, body=b'')[:35])), decline('truncated BAM record'))
case('rec_block_size_32', G, one(lambda: bam(header() + _fixed(block_size=32, l_name=0, body=b''))), decline('without a read name'))
case('rec_block_size_one_past_end', G, one(lambda: bam(header() + rec() + u32(len(rec()) - 4 + 1) + rec()[4:])), decline('truncated BAM record'))
case('rec_stray_bytes_after_last', G, family(lambda: [bam(GOOD + b'\x07' * k) for k in (1, 2, 3)]), ACCEPT)
case('rec_l_read_name_0', G, one(lambda: bam(header() + _fixed(l_name=0, body=TAGS))), decline('without a read name'))
case('rec_l_read_name_1', G, one(lambda: bam(header() + _fixed(l_name=1, body=b'\0' + TAGS))), ACCEPT, names=('', 'r1'))
for _f in ('l_read_name', 'n_cigar_op', 'l_seq'):
    case('rec_%s_ends_at_record_end' % _f, G, one(lambda f=_f: bam(header() + _ends_at(f, 0) + rec())), ACCEPT, names=('r1', 'n' * 39))
    case('rec_%s_ends_past_record_end' % _f, G, one(lambda f=_f: bam(header() + _ends_at(f, 1) + rec())), decline('corrupt BAM record'))

# ---------------------------------------------------------------------------------------------------------------------------
# aux fields
# ---------------------------------------------------------------------------------------------------------------------------
_FULL = collections.OrderedDict((
    ('A', b'Q'), ('c', b'\xfb'), ('C', b'\xfa'), ('s', b'\x01\x02'), ('S', b'\x01\x02'), ('i', b'\x01\x02\x03\x04'),
    ('I', b'\x01\x02\x03\x04'), ('f', b'\0\0\x80\x3e'), ('Z', b'ab\0'), ('H', b'1A\0'), ('B', b'S' + u32(2) + b'\x01\0\x02\0')))

G = 'aux'
case('aux_every_type_cut_one_byte_short', G, family(lambda: [bam(header() + rec(tags=TAGS + aux('XX', t, v[:-1]))) for t, v in _FULL.items()]),
     decline('corrupt aux field'))
case('aux_every_type_whole', G, family(lambda: [bam(header() + rec(tags=aux('XX', t, v) + TAGS)) for t, v in _FULL.items()]), ACCEPT)
case('aux_z_and_h_without_terminator', G, family(lambda: [bam(header() + rec(tags=TAGS + aux('XX', t, b'abcd'))) for t in 'ZH']),
     decline('corrupt aux field'))
case('aux_b_count_one_past_end', G, one(lambda: bam(header() + rec(tags=TAGS + aux('XB', 'B', b'S' + u32(3) + b'\x01\0\x02\0')))),
     decline('corrupt aux field'))
case('aux_b_count_ffffffff', G, family(lambda: [bam(header() + rec(tags=TAGS + aux('XB', 'B', s + u32(0xFFFFFFFF) + b'\x01\0\x02\0'))) for s in (b'C', b'S', b'I')]),
     decline('corrupt aux field'))
case('aux_b_unknown_subtype', G, one(lambda: bam(header() + rec(tags=aux('XB', 'B', b'x' + u32(1) + b'\x01\0\x02\0') + TAGS))),
     decline('corrupt aux field'))
case('aux_unknown_type', G, one(lambda: bam(header() + rec(tags=aux('XQ', 'q', b'\x01') + TAGS))), decline('corrupt aux field'))


def _cg(n_stored=2, count=None, sub='I', twice=False, placed=True):
    """The CG convention of SAMv1 4.2.2 around read r1: the placeholder <l_seq>S<ref_len>N (padded to n_stored operations) in the
    record, the five real operations in CG:B (`count` overrides the array's count word only).  The CG tag is the LAST aux field,
    behind HP, PC, PS: folded away, the line ends in HP, PC, PS and r1 is a tagged read; printed, token [-2] is PS and r1 is not
    (with two CG tags the first is folded and the second printed).  So the tag path's result depends on the fold, and in SVIM mode
    (the *_extract twins) the folded CIGAR gives the 45I and 52D marks where the placeholder gives none."""
    real = [(10, 'M'), (45, 'I'), (10, 'M'), (52, 'D'), (10, 'M')]
    words = [(n << 4) | CIG_CODE.index(op) for n, op in real]
    l_seq, ref_len = 65, 82
    stored = ([(l_seq, 'S'), (ref_len, 'N')] + [(1, 'P')] * 4)[:n_stored]
    body = b''.join(struct.pack('<' + {'I': 'I', 'i': 'i', 'f': 'f'}[sub], w) for w in words)
    cgtag = aux('CG', 'B', sub.encode() + u32(len(words) if count is None else count) + body)
    tags = aux('NM', 'C', b'\0') + TAGS + cgtag + (cgtag if twice else b'')
    return bam(header() + record('r1', 0, 0 if placed else -1, 50000 if placed else 0, 60, stored, 'A' * l_seq, '*', tags) + rec('r2'))


# what the SAM text says, written out (the runner checks it beside the comparison with the Python reader): the names that carry
# a tag in the tag path, and the (type, pos, span) marks of the *_extract twin
EXPECT_TAGGED, EXPECT_MARKS = {}, {}
_FOLDED = [(1, 50010, 45), (0, 50020, 52)]
for _name, _kw, _folded, _tagged in (
        ('cg_count_equals_n_cigar_op', dict(n_stored=5), True, True),
        ('cg_count_n_cigar_op_minus_1', dict(n_stored=6), False, False),
        ('cg_subtype_i', dict(sub='i'), True, True),
        ('cg_subtype_f', dict(sub='f'), False, False),
        ('cg_two_tags', dict(twice=True), True, False),
        ('cg_on_unplaced_record', dict(placed=False), False, False)):
    case(_name, G, one(lambda kw=_kw: _cg(**kw)), ACCEPT, names=('r1', 'r2'))
    case(_name + '_extract', G, one(lambda kw=_kw: _cg(**kw)), ACCEPT, mode='extract:bin=10', names=('r1', 'r2'))
    EXPECT_TAGGED[_name] = {'r2', 'r1'} if _tagged else {'r2'}
    EXPECT_MARKS[_name + '_extract'] = _FOLDED if _folded else []
case('cg_count_2_pow_29', G, one(lambda: _cg(count=1 << 29)), decline('corrupt aux field'))


# ---------------------------------------------------------------------------------------------------------------------------
# tag values
# ---------------------------------------------------------------------------------------------------------------------------
def _int_aux(tag, v):
    """the narrowest signed or unsigned integer type that holds v (SAMv1 4.2.4)"""
    for t, f, lo, hi in (('C', 'B', 0, 255), ('c', 'b', -128, 127), ('S', 'H', 0, 65535), ('s', 'h', -32768, 32767),
                         ('I', 'I', 0, 0xFFFFFFFF), ('i', 'i', -(1 << 31), (1 << 31) - 1)):
        if lo <= v <= hi:
            return aux(tag, t, struct.pack('<' + f, v))
    raise ValueError(v)


def _hp_files():
    out = []
    for t, lo, hi in (('c', -128, 127), ('C', 0, 255), ('s', -32768, 32767), ('S', 0, 65535), ('i', -(1 << 31), (1 << 31) - 1), ('I', 0, 0xFFFFFFFF)):
        recs = b''.join(rec('h%d' % i, tags=hp(v, t) + PC300 + PS1E5) for i, v in enumerate((0, 1, 2, 3, 255, -1)) if lo <= v <= hi)
        out.append(bam(header() + recs))
    return out


G = 'tags'
_HP_NAMES = tuple('h%d' % i for i in range(6))
case('tag_hp_six_types_six_values', G, family(_hp_files), ACCEPT, names=_HP_NAMES)
case('tag_pc_edges', G, one(lambda: bam(header() + b''.join(rec('p%d' % i, tags=hp(1) + _int_aux('PC', v) + PS1E5)
                                                              for i, v in enumerate((0, PC_SAT - 1, PC_SAT, PC_SAT + 1, (1 << 31) - 1))))),
     ACCEPT, names=tuple('p%d' % i for i in range(5)))
case('tag_pc_minus_1', G, one(lambda: bam(header() + rec(tags=hp(1) + _int_aux('PC', -1) + PS1E5))), decline('PC/PS out of range'))
case('tag_ps_0_and_fffffffe', G, one(lambda: bam(header() + rec('s0', tags=hp(1) + PC300 + _int_aux('PS', 0)) +
                                                  rec('s1', tags=hp(2) + PC300 + _int_aux('PS', 0xFFFFFFFE)))), ACCEPT, names=('s0', 's1'))
case('tag_ps_ffffffff', G, one(lambda: bam(header() + rec(tags=hp(1) + PC300 + _int_aux('PS', 0xFFFFFFFF)))), decline('PC/PS out of range'))
case('tag_ps_minus_1', G, one(lambda: bam(header() + rec(tags=hp(1) + PC300 + _int_aux('PS', -1)))), decline('PC/PS out of range'))
case('tag_name_byte_7f', G, one(lambda: bam(header() + _fixed(l_name=4, body=b'a\x7fb\0' + TAGS))), ACCEPT, names=('a\x7fb', 'r1'))
case('tag_name_byte_80', G, one(lambda: bam(header() + _fixed(l_name=4, body=b'a\x80b\0' + TAGS))), decline('non-ASCII read name'))
case('tag_name_byte_80_untagged', G, one(lambda: bam(header() + _fixed(l_name=4, body=b'a\x80b\0' + aux('NM', 'C', b'\0')))), decline('non-ASCII read name'))
case('tag_name_254_bytes', G, one(lambda: bam(header() + rec('n' * 254) + rec())), ACCEPT, names=('n' * 254, 'r1'))
case('tag_same_name_three_times', G, one(lambda: bam(header() + rec(tags=hp(1) + PC300 + _int_aux('PS', 5)) + rec(tags=hp(2) + _int_aux('PC', 7) + _int_aux('PS', 6)) +
                                                      rec(tags=hp(2) + _int_aux('PC', 9000) + _int_aux('PS', 70000)))), ACCEPT)
case('tag_pc_as_z_string', G, one(lambda: bam(header() + rec(tags=hp(1) + aux('PC', 'Z', b'PC:i:5\0') + PS1E5))), decline("string aux value containing 'PC:i:'"))


# ---------------------------------------------------------------------------------------------------------------------------
# extraction mode (duet_ingest_set_extraction) against oracle/svim_oracle.py
# ---------------------------------------------------------------------------------------------------------------------------
def _reach(pos0, end, tail=()):
    """M operations of at most 2^28 - 1 bases from pos0 to `end`, then `tail`"""
    ops, left = [], end - pos0
    while left > 0:
        n = min(left, (1 << 28) - 1)
        ops.append((n, 'M'))
        left -= n
    return ops + list(tail)


def _far(end, tail=(), name='far'):
    return bam(header() + rec(name, pos1=1 << 30, cigar=_reach((1 << 30) - 1, end, tail), seq='', tags=TAGS) + rec('r2'))


G = 'extract'
_X = 'extract:bin=1000'
case('extract_ref_end_2_pow_32_minus_2', G, one(lambda: _far((1 << 32) - 2)), ACCEPT, mode=_X)
case('extract_ref_end_2_pow_32_minus_1', G, one(lambda: _far((1 << 32) - 1)), ACCEPT, mode=_X)
case('extract_ref_end_2_pow_32', G, one(lambda: _far(1 << 32)), decline('alignment ends past reference position 2^32 - 1'), mode=_X)
case('extract_insertion_at_fffffffd', G, one(lambda: _far(0xFFFFFFFD, [(50, 'I'), (1, 'M')])), ACCEPT, mode=_X)
case('extract_insertion_at_fffffffe', G, one(lambda: _far(0xFFFFFFFE, [(50, 'I'), (1, 'M')])), decline('SV mark at or past reference position 2^32 - 1'), mode=_X)
case('extract_ref_end_1e13_bin_1', G, one(lambda: _far(10 ** 13)), decline('alignment ends past reference position 2^32 - 1'), mode='extract:bin=1')
case('extract_depth_bins_past_2_pow_28_bin_1', G, one(lambda: _far((1 << 30) + (1 << 28) + 5)), decline('more than 2^28 depth bins'), mode='extract:bin=1')


# ---------------------------------------------------------------------------------------------------------------------------
# several contigs in one call (duet_ingest_add_bams); file k is contig k's, `None` a path that does not exist
# ---------------------------------------------------------------------------------------------------------------------------
def _contig_bam(k, n=40, pc0=0):
    return bam(header() + b''.join(rec('c%d_%d' % (k, i), tags=hp(1 + i % 2) + _int_aux('PC', pc0 + 10 * i + k) + _int_aux('PS', 1000 * (k + 1))) for i in range(n)))


def _bad_pc(k, n=20):       # declines in mid-stream, after records that were applied already
    return bam(header() + b''.join(rec('c%d_%d' % (k, i)) for i in range(n)) + rec('bad', tags=hp(1) + _int_aux('PC', -1) + PS1E5))


def _bad_aux(k, n=30):
    return bam(header() + b''.join(rec('c%d_%d' % (k, i)) for i in range(n)) + rec('bad', tags=aux('XQ', 'q', b'\x01') + TAGS))


G = 'multi'
_M = 'bams:threads=4:contigs=0,1,2,3'
_MN = tuple('c%d_%d' % (k, i) for k in range(4) for i in (0, 1, 19, 39))
case('multi_two_contigs_decline_differently', G, lambda: [('chr1.bam', _contig_bam(0)), ('chr2.bam', _bad_pc(1)), ('chr3.bam', _contig_bam(2)), ('chr4.bam', _bad_aux(3))],
     decline('PC/PS out of range'), mode=_M, names=_MN)
# (3000 records in front of the one that declines: the four workers are then sure to be at work side by side)
case('multi_four_contigs_all_decline', G, lambda: [('chr1.bam', _bad_pc(0, 3000)), ('chr2.bam', _bad_aux(1, 3000)), ('chr3.bam', _bad_pc(2, 3000)), ('chr4.bam', _bad_aux(3, 3000))],
     decline('PC/PS out of range'), mode=_M, names=_MN)
case('multi_io_failure_then_decline', G, lambda: [('chr1.bam', _contig_bam(0)), ('chr2.bam', None), ('chr3.bam', _contig_bam(2)), ('chr4.bam', _bad_aux(3))],
     decline('cannot read', IO), mode=_M, names=_MN)
case('multi_decline_then_io_failure', G, lambda: [('chr1.bam', _contig_bam(0)), ('chr2.bam', _bad_aux(1)), ('chr3.bam', _contig_bam(2)), ('chr4.bam', None)],
     decline('corrupt aux field'), mode=_M, names=_MN)
case('multi_one_contig_named_twice', G, lambda: [('a.bam', _contig_bam(0)), ('b.bam', _contig_bam(0, n=25, pc0=7000)), ('chr3.bam', _contig_bam(2))],
     ACCEPT, mode='bams:threads=4:contigs=0,0,2', names=_MN)
case('multi_n_0', G, lambda: [], ACCEPT, mode='bams:threads=4:contigs=', names=_MN)
case('multi_threads_0', G, lambda: [('chr1.bam', _contig_bam(0)), ('chr2.bam', _contig_bam(1)), ('chr3.bam', _contig_bam(2)), ('chr4.bam', _contig_bam(3))],
     ACCEPT, mode='bams:threads=0:contigs=0,1,2,3', names=_MN)

# ---------------------------------------------------------------------------------------------------------------------------
# caller VCF lines, 1 MiB and above (the threaded line index), read with 1 thread and with 8
# ---------------------------------------------------------------------------------------------------------------------------
# Already pinned on small files, not repeated here: a blank line in mid-file and a non-ASCII byte in a record
# (tests/test_native_ingest.py::test_declines_what_it_cannot_vouch_for, tests/test_host_errors.py blank_line).
VCF_REC = 'chr1\t%d\tid\tN\t<DEL>\t.\tPASS\tPRECISE;SVTYPE=DEL;SVLEN=-80;END=180;RE=5;RNAMES=r1,zz;STRAND=+-\tGT:DR:DV:PL:GQ\t0/1:3:5:1,2,3:9'
MIB = 1 << 20


def _vcf(tail, long_line=0):
    """'##' lines up to 1 MiB (optionally one of `long_line` bytes), a few records, more '##' lines, then `tail` (the last stretch)"""
    head = '##fileformat=VCFv4.2\n##contig=<ID=chr1,length=249250621>\n'
    filler = '##filler=' + 'x' * 110 + '\n'
    body = head + ('##long=' + 'y' * long_line + '\n' if long_line else '')
    body += filler * ((MIB - len(body)) // len(filler) + 1)
    body += ''.join(VCF_REC % (100 + i) + '\n' for i in range(5)) + filler * 40
    return (body + tail).encode('latin-1')


G = 'vcf'
_LAST = VCF_REC % 900
for _name, _build, _exp in (
        ('vcf_last_line_with_newline', lambda: _vcf(_LAST + '\n'), ACCEPT),
        ('vcf_last_line_without_newline', lambda: _vcf(_LAST), ACCEPT),
        ('vcf_line_longer_than_a_stretch', lambda: _vcf(_LAST + '\n', long_line=300000), ACCEPT),
        ('vcf_one_crlf_in_last_stretch', lambda: _vcf('##note=a\r\n' + _LAST + '\n'), ACCEPT),
        ('vcf_one_lone_cr_in_last_stretch', lambda: _vcf('##note=a\r##note=b\n' + _LAST + '\n'), ACCEPT),
        ('vcf_nul_in_last_stretch', lambda: _vcf('##note=a\0b\n' + _LAST + '\n'), decline('NUL byte in the VCF')),
        ('vcf_byte_80_in_header_line_of_last_stretch', lambda: _vcf('##note=a\x80b\n' + _LAST + '\n'), decline('non-ASCII byte in the VCF')),
        ('vcf_blank_last_line', lambda: _vcf(_LAST + '\n\n'), decline('blank line in the VCF'))):
    for _t in (1, 8):
        case('%s_t%d' % (_name, _t), G, one(_build, 'variants.vcf'), _exp, mode='vcf:threads=%d' % _t)


# ---------------------------------------------------------------------------------------------------------------------------
# manifest
# ---------------------------------------------------------------------------------------------------------------------------
def write_case(e, outdir):
    """The files of one case under outdir/<name>/ -> their paths (None for a path that must not exist)."""
    paths = []
    for fname, blob in e.build():
        p = os.path.join(outdir, e.name, fname)
        if blob is None:
            paths.append(p + '.missing')
            continue
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, 'wb') as f:
            f.write(blob)
        paths.append(p)
    return paths


def write_all(outdir):
    os.makedirs(outdir, exist_ok=True)
    with open(os.path.join(outdir, 'manifest.tsv'), 'w') as man:
        for e in REGISTRY.values():
            paths = write_case(e, outdir)
            if e.mode.startswith('bams:'):
                man.write('%s\t%s\t%s\t%d\n' % (e.name, ','.join(paths) if paths else '-', e.mode, e.expect[2]))
            else:
                for p in paths:
                    man.write('%s\t%s\t%s\t%d\n' % (e.name, p, e.mode, e.expect[2]))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    write_all(sys.argv[1])
