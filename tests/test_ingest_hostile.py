# coding=utf-8
"""The native ingest (libduet_ingest.so) on hostile BAM and VCF inputs: it declines with a reason or builds exactly what the Python
reader builds -- it never crashes and never reports one contig's failure as another's.  The cases are data
(tests/ingest_hostile.py); every one runs in a fresh child process (`python -m tests.test_ingest_hostile --case NAME DIR`), so an
abort or a stray signal shows as a failed assertion on the child's exit status, not as a dead suite.  CPU only.

  * decline cases: duet_ingest_add_bam (or _add_bams / _parse_vcf) returns the stated status, duet_ingest_error contains the stated
    substring, and through native.NativeIngest.load `handle is None` with `why` set;
  * accept cases: the arrays of engine.EfSoA.FIELDS equal those of F.generate_callinfo(..., F.read_hap_bam(...)) field by field, and
    the tag triples equal what bamio.iter_bam_records + tail_tokens give under the rule of sv_phasing_fn.py:25-29;
  * extraction cases: NativeIngest.extract against oracle/svim_oracle.py;
  * one differential corpus with a fixed seed (test_mutation_corpus; counts in DESIGN.md, "The ingest on hostile inputs").
"""
import ctypes
import json
import os
import random
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from tests import ingest_hostile as HO

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _spawn(args, tmp_path):
    p = subprocess.run([sys.executable, '-m', 'tests.test_ingest_hostile'] + args + [str(tmp_path)], cwd=REPO,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    return p.returncode, p.stdout.decode('utf-8', 'replace')


@pytest.mark.parametrize('name', list(HO.REGISTRY))
def test_case(name, tmp_path):
    rc, out = _spawn(['--case', name], tmp_path)
    assert rc == 0, 'child exit status %d\n%s' % (rc, out)


def test_manifest_lists_every_case(tmp_path):
    """`python -m tests.ingest_hostile OUTDIR` (what tools/ingest_hostile_check.cpp reads): one line per file of a one-file mode, one
    line per several-contig case, every path but the deliberately missing ones present."""
    HO.write_all(str(tmp_path))
    rows = [l.rstrip('\n').split('\t') for l in open(str(tmp_path / 'manifest.tsv'))]
    assert all(len(r) == 4 for r in rows)
    assert set(r[0] for r in rows) == set(HO.REGISTRY)
    for name, path, mode, status in rows:
        assert int(status) == HO.REGISTRY[name].expect[2]
        for p in (path.split(',') if mode.startswith('bams:') else [path]):
            assert p == '-' or p.endswith('.missing') or os.path.exists(p), p


# Reasons for which the native path declines an input that the Python reader may well accept (DESIGN.md lists them): the corpus
# below lets the native path decline a mutant the Python reader accepts for one of these only.
DOCUMENTED_DECLINES = (
    'alignment with fewer than three aux fields and a PC-like column',
    "string aux value containing 'PC:i:'",
    'HP/PS neighbours of PC are not integers',
)
# ... and for these only where the mutant holds a field that was malformed on purpose (an integer value cut short at the record's
# end, which the Python reader reads out of the next record): on a well-formed mutant they would be a regression
MALFORMED_DECLINES = ('corrupt aux field', 'corrupt BAM record')
CORPUS_SEED, CORPUS_N = 20240611, 320


def test_mutation_corpus(tmp_path):
    """Field-level mutants of the hand-written BAM of tests/test_bam_spec.py (long CIGAR shortened to 121 operations), wrapped in
    members cut at random offsets.  For every mutant: native accepts => Python accepts and agrees; Python raises => native declines.
    A corpus that declines everything proves nothing: at least a third must be accepted by the Python reader, and the native path
    must accept every one of those unless it states one of DOCUMENTED_DECLINES (or, on a mutant with a field malformed on purpose, one
    of MALFORMED_DECLINES)."""
    rc, out = _spawn(['--corpus'], tmp_path)
    assert rc == 0, 'child exit status %d\n%s' % (rc, out)
    counts = json.loads(out.strip().split('\n')[-1])
    print(counts)
    assert counts['generated'] == CORPUS_N
    assert 3 * counts['python_accepted'] >= counts['generated'], counts
    assert counts['violations'] == [], counts


# ---------------------------------------------------------------------------------------------------------------------------
# the child process
# ---------------------------------------------------------------------------------------------------------------------------
def _mode(mode):
    kind, _, rest = mode.partition(':')
    return kind, dict(kv.split('=') for kv in rest.split(':') if kv)


def _lib():
    from duet_amd import native
    lib = native.load()
    assert lib is not None, 'libduet_ingest.so is missing'
    return lib


def _create(lib, chroms):
    labels = (ctypes.c_char_p * len(chroms))(*[c.encode() for c in chroms])
    h = lib.duet_ingest_create(len(chroms), labels)
    assert h
    return h


def _vcf_text(names, chrom='chr1'):
    return ('##contig=<ID=%s,length=249250621>\n%s\t1000\tid\tN\t<DEL>\t.\tPASS\tPRECISE;SVTYPE=DEL;SVLEN=-80;END=1080;RE=9;RNAMES=%s;STRAND=+-\t'
            'GT:DR:DV:PL:GQ\t0/1:3:9:1,2,3:9\n' % (chrom, chrom, ','.join(names)))


def _home(root, blob, names, vcf=None):
    os.makedirs(root + '/sv_calling')
    os.makedirs(root + '/snp_phasing')
    if blob is not None:
        with open(root + '/snp_phasing/chr1.bam', 'wb') as f:
            f.write(blob)
    with open(root + '/sv_calling/variants.vcf', 'wb') as f:
        f.write(vcf if vcf is not None else _vcf_text(names).encode('latin-1'))
    return root


def _python_triples(path):
    """name -> (hap, pc, ps) by the rule of sv_phasing_fn.py:25-29 on the Python reader's tokens (later lines win)"""
    from duet_amd import bamio
    want = {}
    for name, mandatory, aux_fields in bamio.iter_bam_records(path):
        tail = bamio.tail_tokens(mandatory, aux_fields)
        if 'PC:i:' in tail[-2]:
            want[name] = (int(tail[-3][5:]), int(tail[-2][5:]), int(tail[-1][5:]))
    return want


def _agree_with_python(ing, home, names, threads):
    from duet_amd import engine
    from duet_amd import sv_phasing_fn as F
    vcf, sams = home + '/sv_calling/variants.vcf', home + '/snp_phasing/'
    tab, soa = F.generate_callinfo(vcf, F.read_hap_bam(sams, threads, False), False)
    for field, _ in engine.EfSoA.FIELDS:
        assert np.array_equal(getattr(ing.soa, field), getattr(soa, field)), field
    if names and os.path.exists(sams + 'chr1.bam'):
        want = _python_triples(sams + 'chr1.bam')
        got = {}
        for name, m in zip(names, ing.soa.mark_read):
            if m != engine.MARK_ABSENT:
                t = int(ing.soa.read_tag[m])
                got[name] = (t >> 62, (t >> 32) & 0x3FFFFFFF, t & 0xFFFFFFFF)
        coded = {n: (h if h in (1, 2) else 3, min(pc, HO.PC_SAT), ps) for n, (h, pc, ps) in want.items() if n in names}
        assert got == coded, (got, coded)
        return set(got)
    return None


def _run_bam(e, opts, root, i, blob):
    from duet_amd import native
    from duet_amd.read_file import init_chrom_list
    chroms = init_chrom_list(False, '')
    threads = int(opts['threads'])
    home = _home('%s/%02d' % (root, i), blob, e.names)
    vcf, sams = home + '/sv_calling/variants.vcf', home + '/snp_phasing/'
    kind, why, status = e.expect
    if kind == 'decline':
        lib = _lib()
        h = _create(lib, chroms)
        rc = lib.duet_ingest_add_bam(h, 0, (sams + 'chr1.bam').encode(), threads)
        msg = lib.duet_ingest_error(h).decode('utf-8', 'replace')
        lib.duet_ingest_destroy(h)
        assert rc == status and why in msg, (i, rc, msg)
        ing = native.NativeIngest.load(vcf, sams, chroms, threads)
        assert ing is not None and ing.handle is None and ing.why and why in ing.why, (i, ing.why)
    else:
        ing = native.NativeIngest.load(vcf, sams, chroms, threads)
        assert ing is not None and ing.handle, (i, ing.why)
        tagged = _agree_with_python(ing, home, e.names, threads)
        if e.name in HO.EXPECT_TAGGED:
            assert tagged == HO.EXPECT_TAGGED[e.name], tagged
        ing.close()


def _run_extract(e, opts, root, i, blob):
    from duet_amd import bamio, native
    from duet_amd.read_file import init_chrom_list
    from oracle import svim_oracle
    chroms = init_chrom_list(False, '')
    home = _home('%s/%02d' % (root, i), blob, e.names)
    sams = home + '/snp_phasing/'
    kind, why, status = e.expect
    ing, got = native.NativeIngest.extract(sams, chroms, thread=2, depth_bin=int(opts['bin']))
    if kind == 'decline':
        assert ing is None and why in got, got
        return
    assert ing is not None, got
    with open(sams + 'chr1.bam.sam', 'w') as f:            # the text the oracle reads: the Python reader's lines
        for name, mandatory, aux_fields in bamio.iter_bam_records(sams + 'chr1.bam'):
            f.write('\t'.join(mandatory() + aux_fields) + '\n')
    rule = svim_oracle.extract_workdir(home, chroms, depth_bin=int(opts['bin']))
    for f in ('contig', 'type', 'pos', 'span'):
        assert np.array_equal(got[f], rule[f]), (f, got[f], rule[f])
    if e.name in HO.EXPECT_MARKS:
        assert list(zip(got['type'].tolist(), got['pos'].tolist(), got['span'].tolist())) == HO.EXPECT_MARKS[e.name], got
    d = got['depth'][got['depth_off'][0]:got['depth_off'][1]]
    assert np.array_equal(d, np.array(rule['depth'][0], dtype=np.uint32))
    assert int(got['depth_off'][-1]) == len(d)
    ing.close()


def _tables(lib, h, chroms, vcf):
    """(read_off, read_tag, mark_read) of a handle after the caller VCF is joined against its tables"""
    from duet_amd import native
    rc = lib.duet_ingest_parse_vcf(h, vcf.encode(), 2)
    assert rc == 0, lib.duet_ingest_error(h)
    a = native.IngestArrays()
    assert lib.duet_ingest_get_arrays(h, ctypes.byref(a)) == 0
    return (native._view(a.read_off, a.n_contigs + 1, np.uint32).copy(), native._view(a.read_tag, a.n_reads, np.uint64).copy(),
            native._view(a.mark_read, a.n_marks, np.uint32).copy())


def _run_bams(e, opts, root):
    from duet_amd.read_file import init_chrom_list
    chroms = init_chrom_list(False, '')
    lib = _lib()
    paths = HO.write_case(e, root)
    contigs = [int(c) for c in opts['contigs'].split(',') if c]
    assert len(contigs) == len(paths)
    vcf = root + '/variants.vcf'
    with open(vcf, 'w') as f:
        for k in range(4):
            f.write(_vcf_text([n for n in e.names if n.startswith('c%d_' % k)] + ['zz'], 'chr%d' % (k + 1)))
    kind, why, status = e.expect
    ks = (ctypes.c_int * max(1, len(contigs)))(*contigs)
    ps = (ctypes.c_char_p * max(1, len(paths)))(*[p.encode() for p in paths])
    for _ in range(3):                                      # (a race does not show every time)
        h = _create(lib, chroms)
        rc = lib.duet_ingest_add_bams(h, len(contigs), ks, ps, int(opts['threads']))
        msg = lib.duet_ingest_error(h).decode('utf-8', 'replace')
        assert rc == status and why in msg, (rc, msg)
        # the contigs that loaded hold what they hold when loaded alone, one by one; the failing ones hold nothing
        alone = _create(lib, chroms)
        for k, p in zip(contigs, paths):
            one = _create(lib, chroms)
            ok = lib.duet_ingest_add_bam(one, k, p.encode(), 1) == 0
            lib.duet_ingest_destroy(one)
            if ok or kind == 'accept':
                assert lib.duet_ingest_add_bam(alone, k, p.encode(), 1) == 0
        got, want = _tables(lib, h, chroms, vcf), _tables(lib, alone, chroms, vcf)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), (got, want)
        if contigs and kind == 'accept':
            assert len(want[1]) > 0
        lib.duet_ingest_destroy(h)
        lib.duet_ingest_destroy(alone)


def _run_vcf(e, opts, root):
    from duet_amd import native
    from duet_amd.read_file import init_chrom_list
    chroms = init_chrom_list(False, '')
    (fname, blob), = e.build()
    assert len(blob) >= HO.MIB
    home = _home(root + '/w', HO.bam(HO.GOOD), (), vcf=blob)
    threads = int(opts['threads'])
    ing = native.NativeIngest.load(home + '/sv_calling/variants.vcf', home + '/snp_phasing/', chroms, threads)
    kind, why, status = e.expect
    if kind == 'decline':
        assert ing is not None and ing.handle is None and why in ing.why, ing.why
    else:
        assert ing is not None and ing.handle, ing.why
        assert ing.soa.n_cands == 6 and int((ing.soa.mark_read != 0xFFFFFFFF).sum()) == 6
        _agree_with_python(ing, home, (), threads)
        ing.close()


def run_case(name, root):
    e = HO.REGISTRY[name]
    kind, opts = _mode(e.mode)
    if kind == 'bams':
        _run_bams(e, opts, root)
    elif kind == 'vcf':
        _run_vcf(e, opts, root)
    else:
        for i, (fname, blob) in enumerate(e.build()):
            (_run_bam if kind == 'bam' else _run_extract)(e, opts, root, i, blob)
    return 0


# ---------------------------------------------------------------------------------------------------------------------------
# the differential corpus
# ---------------------------------------------------------------------------------------------------------------------------
_INT = {'c': 'b', 'C': 'B', 's': 'h', 'S': 'H', 'i': 'i', 'I': 'I'}
_RANGE = {'c': (-128, 127), 'C': (0, 255), 's': (-32768, 32767), 'S': (0, 65535), 'i': (-(1 << 31), (1 << 31) - 1), 'I': (0, 0xFFFFFFFF)}
_WIDTH = {'A': 1, 'c': 1, 'C': 1, 's': 2, 'S': 2, 'i': 4, 'I': 4, 'f': 4}
_POOL = ['r1', 'r2', 'r5', 'r9', 'x', '', 'a\x7fb', 'n' * 60]


def _base_payload():
    """The payload of tests/test_bam_spec.build() with the long CIGAR cut to 121 operations -> (header bytes, list of records)"""
    from tests import test_bam_spec as S
    full = S.long_cigar_ops
    S.long_cigar_ops = lambda: full()[:120] + [(10, 'M')]
    try:
        blob = S.build()[0]
    finally:
        S.long_cigar_ops = full
    buf, pos = b'', 0
    while pos < len(blob):
        d = zlib.decompressobj(31)
        buf += d.decompress(blob[pos:]) + d.flush()
        pos = len(blob) - len(d.unused_data)
    p = 8 + struct.unpack_from('<I', buf, 4)[0]
    n_ref = struct.unpack_from('<I', buf, p)[0]
    p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from('<I', buf, p)[0]
    head, recs = buf[:p], []
    while p < len(buf):
        bs = struct.unpack_from('<I', buf, p)[0]
        recs.append(_split(buf[p + 4:p + 4 + bs]))
        p += 4 + bs
    return head, recs


def _split(body):
    """One well-formed record -> dict(core list, name, cigar words, seq+qual bytes, aux list of [tag, type, value bytes])"""
    core = list(struct.unpack_from('<iiBBHHHIiii', body, 0))
    l_name, n_cig, l_seq = core[2], core[5], core[7]
    q = 32
    name = body[q:q + l_name - 1]
    q += l_name
    cig = list(struct.unpack_from('<%dI' % n_cig, body, q))
    q += 4 * n_cig
    sq = body[q:q + (l_seq + 1) // 2 + l_seq]
    q += len(sq)
    auxs = []
    while q < len(body):
        tag, typ = body[q:q + 2], chr(body[q + 2])
        q += 3
        if typ in _WIDTH:
            w = _WIDTH[typ]
        elif typ in 'ZH':
            w = body.index(b'\0', q) + 1 - q
        else:
            sub, cnt = chr(body[q]), struct.unpack_from('<I', body, q + 1)[0]
            w = 5 + cnt * (4 if sub == 'f' else _WIDTH[sub])
        auxs.append([tag, typ, body[q:q + w]])
        q += w
    return dict(core=core, name=name, cig=cig, sq=sq, aux=auxs)


def _join(r):
    core = list(r['core'])
    core[2], core[5] = (len(r['name']) + 1) & 0xFF, len(r['cig'])
    body = (struct.pack('<iiBBHHHIiii', *core) + r['name'] + b'\0' + struct.pack('<%dI' % len(r['cig']), *r['cig']) + r['sq'] +
            b''.join(t + y.encode('latin-1') + v for t, y, v in r['aux']))
    return struct.pack('<I', len(body)) + body


def _mutate(rng, recs):
    """1 to 3 field-level mutations; most leave the file well formed -> (records, whether a field was malformed on purpose)"""
    malformed = False
    recs = [dict(r, core=list(r['core']), cig=list(r['cig']), aux=[list(a) for a in r['aux']]) for r in recs]
    for _ in range(rng.randint(1, 3)):
        r = rng.choice(recs)
        what = rng.random()
        ints = [a for a in r['aux'] if a[1] in _INT]
        if what < 0.30 and ints:                   # an integer tag's type and value
            a = rng.choice(ints)
            v = rng.choice([0, 1, 2, 3, 7, 255, 256, 8100, 8101, 65535, 65536, HO.PC_SAT, HO.PC_SAT + 1, (1 << 31) - 1, 0xFFFFFFFE,
                            0xFFFFFFFF, -1, -7] if rng.random() < 0.8 else [rng.randrange(0, 1 << 20)])
            fits = [t for t in _INT if _RANGE[t][0] <= v <= _RANGE[t][1]]
            a[1] = rng.choice(fits)
            a[2] = struct.pack('<' + _INT[a[1]], v)
        elif what < 0.42 and len(r['aux']) >= 2:   # order of the tags
            i, j = rng.sample(range(len(r['aux'])), 2)
            r['aux'][i], r['aux'][j] = r['aux'][j], r['aux'][i]
        elif what < 0.50 and r['aux']:             # one tag less / one twice
            i = rng.randrange(len(r['aux']))
            if rng.random() < 0.5:
                del r['aux'][i]
            else:
                r['aux'].insert(rng.randrange(len(r['aux']) + 1), list(r['aux'][i]))
        elif what < 0.62:                          # the name
            r['name'] = rng.choice(_POOL).encode('latin-1') if rng.random() < 0.9 else b'r\x80'
        elif what < 0.72:                          # flag, position, reference
            r['core'][6] ^= 1 << rng.randrange(12)
            if rng.random() < 0.5:
                r['core'][1] = rng.choice([-1, 0, 5, 1 << 20, (1 << 31) - 1])
            if rng.random() < 0.3:
                r['core'][0] = rng.choice([-1, 0, 1, 2])
        elif what < 0.86 and r['cig']:             # a CIGAR operation
            i = rng.randrange(len(r['cig']))
            r['cig'][i] = (rng.choice([0, 1, 39, 40, 45, 1000, (1 << 28) - 1]) << 4) | rng.randrange(9)
        elif what < 0.92:                          # a string tag: with a blank, with the PC pattern, or typed Z in place of PC
            r['aux'].insert(rng.randrange(len(r['aux']) + 1), [b'XZ', 'Z', rng.choice([b'a b\0', b'PC:i:5\0', b'\0', b'plain\0'])])
        elif what < 0.96:                          # malformed on purpose: unknown type letter / B subtype, value cut short
            r['aux'].append(rng.choice([[b'XQ', 'q', b'\x01'], [b'XB', 'B', b'x' + struct.pack('<I', 1) + b'\0\0\0\0'], [b'XI', 'I', b'\x01\x02']]))
            malformed = True
        else:                                      # a record with no name at all
            r['name'] = b''
    return recs, malformed


def run_corpus(root):
    from duet_amd import engine, native
    from duet_amd import sv_phasing_fn as F
    from duet_amd.read_file import init_chrom_list
    import logging
    logging.disable(logging.CRITICAL)
    chroms = init_chrom_list(False, '')
    lib = _lib()
    rng = random.Random(CORPUS_SEED)
    head, base = _base_payload()
    names = sorted(set(_POOL) | set(r['name'].decode() for r in base))
    home = _home(root + '/w', None, names)
    vcf, sams = home + '/sv_calling/variants.vcf', home + '/snp_phasing/'
    counts = dict(generated=0, python_accepted=0, native_accepted=0, both_accepted=0, violations=[])
    for m in range(CORPUS_N):
        recs, malformed = _mutate(rng, base)
        payload = head + b''.join(_join(r) for r in recs)
        cuts = [rng.randrange(1, len(payload)) for _ in range(rng.randint(0, 9))]
        with open(sams + 'chr1.bam', 'wb') as f:
            f.write(HO.bam(payload, cuts))
        counts['generated'] += 1
        try:
            tab, soa = F.generate_callinfo(vcf, F.read_hap_bam(sams, 1, False), False)
            py = None
        except Exception as ex:                    # noqa: the Python reader's way of declining
            py = '%s: %s' % (type(ex).__name__, ex)
        ing = native.NativeIngest.load(vcf, sams, chroms, 1 + m % 4)
        assert ing is not None
        counts['python_accepted'] += py is None
        counts['native_accepted'] += ing.handle is not None
        if ing.handle is not None:
            if py is not None:
                counts['violations'].append((m, 'native accepts, Python raises ' + py))
            else:
                counts['both_accepted'] += 1
                bad = [f for f, _ in engine.EfSoA.FIELDS if not np.array_equal(getattr(ing.soa, f), getattr(soa, f))]
                if bad:
                    counts['violations'].append((m, 'both accept, they differ in %s' % bad))
            ing.close()
        elif py is None and not any(d in ing.why for d in DOCUMENTED_DECLINES + (MALFORMED_DECLINES if malformed else ())):
            counts['violations'].append((m, 'Python accepts, native declines: ' + ing.why))
    print(json.dumps(counts))
    return 0


if __name__ == '__main__':
    if sys.argv[1] == '--case':
        sys.exit(run_case(sys.argv[2], sys.argv[3]))
    sys.exit(run_corpus(sys.argv[2]))
