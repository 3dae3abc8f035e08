# coding=utf-8
"""evaluation.details / details_text / --details on the Python path (no GPU): the tables against the ten numbers the repository pins
from the reference's evaluator (tests/golden/eval/expected.json), their own totals, hand-written cases with every column spelled
out (tests/eval_details_cases.py), an independent restatement on random problems, and the command line."""
import json
import os

import numpy as np
import pytest

from duet_amd import _lib as L
from duet_amd import evaluation as E
from tests import eval_details_cases as C
from tests import helpers as H

EVAL = os.path.join(H.GOLDEN, 'eval')


def golden_cases():
    with open(os.path.join(EVAL, 'expected.json')) as f:
        cases = json.load(f)
    assert len(cases) == 24
    return cases


def tables(truth, calls, refdist, ratio):
    """-> (rows of the calls table as dicts, rows of the truth table as dicts), through details and details_text"""
    a, rows, scored = E.flatten_rows(truth, calls)
    recs = E.details(truth, calls, refdist, ratio)
    text = E.details_text(rows, scored, *recs)
    out = []
    for t, cols in zip(text, (E.CALL_COLUMNS, E.TRUTH_COLUMNS)):
        lines = t.splitlines()
        assert lines[0] == '\t'.join(cols) and t.endswith('\n')
        out.append([dict(zip(cols, ln.split('\t'))) for ln in lines[1:]])
        assert all(len(ln.split('\t')) == len(cols) for ln in lines[1:])
    assert len(out[0]) == len(scored) and len(out[1]) == len(rows)
    return out


@pytest.fixture(scope='module')
def golden_tables():
    out = []
    for c in golden_cases():
        pair = os.path.join(EVAL, 'pair%d' % c['pair'])
        bed = os.path.join(pair, 'regions.bed') if c['bed'] else ''
        truth = E.parse_vcf(os.path.join(pair, 'truth.vcf'), c['skip_phasing'], bed)
        calls = E.parse_vcf(os.path.join(pair, 'call.vcf'), c['skip_phasing'], bed)
        out.append((c, truth, calls) + tuple(tables(truth, calls, c['refdist'], c['pctsim'])))
    return out


def test_distinct_ids_are_the_six_counts_of_the_reference(golden_tables):
    """The ten pinned numbers are quotients of the six set sizes and the two list lengths (evaluation.py:147-151): distinct ids
    of the tables' rows, divided the same way, give the same binary64 values -- which no other count does."""
    for c, truth, calls, crows, trows in golden_tables:
        got = [len(calls) / len(set(s['ps'] for s in calls))]
        for on_call, on_truth in (('MATCHED', 'N_CALLS'), ('GT', 'N_GT'), ('HP_OK', 'N_HP')):
            n_c = len(set(r['ID'] for r in crows if r[on_call] == '1'))
            n_t = len(set(r['ID'] for r in trows if int(r[on_truth]) > 0))
            p, r = n_c / len(calls), n_t / len(truth)
            got += [p, r, 2 * p * r / (p + r)]
        assert got == c['result'], c
        # ... and evaluation() itself
        assert got == [float(x) for x in E.evaluation(truth, calls, c['refdist'], c['pctsim'])]


def test_totals(golden_tables):
    seen = set()
    for c, truth, calls, crows, trows in golden_tables:
        assert sum(int(r['N_CALLS']) for r in trows) == sum(r['MATCHED'] == '1' for r in crows)
        assert sum(int(r['N_GT']) for r in trows) == sum(r['GT'] == '1' for r in crows)
        assert sum(int(r['N_HP']) for r in trows) == sum(r['HP_OK'] == '1' for r in crows)
        by_call = {(r['CHROM'], r['POS'], r['ID'], r['TYPE']): r for r in crows}
        for r in trows:
            # every miss has exactly one reason, every hit none
            assert (r['REASON'] in L.EVAL_REASON_NAMES) == (int(r['N_CALLS']) == 0) and (r['REASON'] == '.') == (int(r['N_CALLS']) > 0)
            assert (r['C_POS'] == '.') == (r['C_ID'] == '.') == (r['C_DIST'] == '.') == (r['REASON'] == 'no_call')
            if r['REASON'] == 'elsewhere':
                assert by_call[(r['CHROM'], r['C_POS'], r['C_ID'], r['TYPE'])]['T_ID'] != r['ID']
            if r['REASON'] == 'far':
                assert int(r['C_DIST']) > c['refdist']
            seen.add(r['REASON'])
        for r in crows:
            assert r['REL'] in ('same', 'flip', 'both', '.') and r['LABEL'] in ('same', 'flip')
            assert int(r['DIST']) == abs(int(r['POS']) - int(r['T_POS']))
            assert r['MATCHED'] == '1' or (r['GT'], r['REL'], r['HP_OK']) == ('0', '.', '0')
            assert (r['HP_OK'] == '1') == (r['REL'] in ('both', r['LABEL']))
        # one labelling per phase-set group
        for g in set((r['CHROM'], r['GROUP']) for r in crows):
            assert len(set(r['LABEL'] for r in crows if (r['CHROM'], r['GROUP']) == g)) == 1
    assert seen >= {'.', 'far', 'size'}, seen


@pytest.mark.parametrize('name', sorted(C.CASES))
def test_hand_written_case(name):
    truth, calls, refdist, ratio, want_calls, want_truth = C.CASES[name]
    crows, trows = tables(truth, calls, refdist, ratio)
    assert [[r[k] for k in E.CALL_COLUMNS] for r in crows] == want_calls
    assert [[r[k] for k in E.TRUTH_COLUMNS] for r in trows] == want_truth


def test_the_hand_written_cases_together_give_every_value_of_every_column():
    seen_rel, seen_reason, seen_label = set(), set(), set()
    for truth, calls, refdist, ratio, _, _ in C.CASES.values():
        crows, trows = tables(truth, calls, refdist, ratio)
        seen_rel |= set(r['REL'] for r in crows)
        seen_label |= set(r['LABEL'] for r in crows)
        seen_reason |= set(r['REASON'] for r in trows)
    assert seen_rel == {'same', 'flip', 'both', '.'} and seen_label == {'same', 'flip'}
    assert seen_reason == {'.', 'no_call', 'far', 'size', 'elsewhere'}
    one, two = tables(*C.CASES['one_id_twice_and_three_hits'][:4])[0][:2]
    assert one['ID'] == two['ID'] and one['MATCHED'] != two['MATCHED']


def same_records(got, want):
    for g, w in zip(got[1:], want[1:]):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    assert tuple(got[0]) == tuple(want[0])


@pytest.mark.parametrize('n_calls,n_base,n_keys', [(1, 1, 1), (2, 2, 1), (7, 3, 2), (40, 25, 1), (65, 64, 6), (300, 120, 48), (257, 9, 3)])
def test_random_problems_against_the_plain_restatement(n_calls, n_base, n_keys):
    for seed in range(6):
        a = C.random_problem(1000 * n_calls + seed, n_calls, n_base, n_keys)
        same_records(E.details_host(a, a['refdist'], a['ratio']), C.brute(a))


@pytest.mark.parametrize('n_calls,n_base,n_keys', [(2, 1, 1), (40, 25, 1), (300, 120, 48), (257, 9, 3)])
def test_calls_without_a_list_key(n_calls, n_base, n_keys):
    """base and dist all-ones, LABEL alone in bits; no truth record counts such a call or has it as its nearest"""
    for seed in range(4):
        a = C.random_problem(77000 + 10 * n_calls + seed, n_calls, n_base, n_keys, unlisted=5)
        none = a['call_key'] == L.EVAL_NONE
        assert none[0] and none[-1]
        got = E.details_host(a, a['refdist'], a['ratio'])
        same_records(got, C.brute(a))
        calls, base = got[1:]
        assert set(calls['base'][none].tolist()) == set(calls['dist'][none].tolist()) == {L.EVAL_NONE}
        assert not (calls['bits'][none] & ~np.uint32(L.EVAL_LABEL)).any()
        assert not np.isin(base['nearest'], np.nonzero(none)[0]).any()


def test_all_calls_or_all_records_of_a_list_on_one_position():
    a = C.random_problem(5, 200, 90, 3, call_pos=17)
    assert len(set(a['call_pos'][a['call_key'] == a['call_key'].min()].tolist())) == 1
    same_records(E.details_host(a, a['refdist'], a['ratio']), C.brute(a))
    a = C.random_problem(6, 200, 90, 3, base_pos=17)
    assert len(set(a['base_pos'][:int(a['base_off'][1])].tolist())) <= 1
    same_records(E.details_host(a, a['refdist'], a['ratio']), C.brute(a))


def test_record_layouts():
    assert L.EVAL_CALL_DTYPE.itemsize == 12 and L.EVAL_BASE_DTYPE.itemsize == 24
    assert L.EVAL_BASE_DTYPE.fields['reason'][1] == 20
    calls, base = E.details(*C.CASES['four_reasons'][:4])
    assert calls.dtype == L.EVAL_CALL_DTYPE and base.dtype == L.EVAL_BASE_DTYPE and not base['reserved'].any()
    with pytest.raises(ValueError):
        E.details(*C.CASES['four_reasons'][:2], -1, 0.0)


# ---- the command line -------------------------------------------------------------------------------------------------------

PAIR = os.path.join(EVAL, 'pair1')
FILES = [os.path.join(PAIR, 'call.vcf'), os.path.join(PAIR, 'truth.vcf')]


@pytest.mark.parametrize('extra', [[], ['-b', os.path.join(PAIR, 'regions.bed')], ['--skip_phasing'], ['-r', '500', '-p', '0.7'],
                                   ['-b', os.path.join(PAIR, 'regions.bed'), '--skip_phasing', '-r', '500', '-p', '0.7']],
                         ids=['plain', 'bed', 'skip_phasing', 'r_p', 'all'])
def test_cli_writes_both_tables_and_prints_what_it_printed(tmp_path, capsys, extra):
    # every fifth call unphased: dropped unless it is 1/1 or --skip_phasing is given, and then its group is the contig
    (tmp_path / 'in').mkdir()
    (tmp_path / 'out').mkdir()
    with open(FILES[0]) as f, open(str(tmp_path / 'in' / 'call.vcf'), 'w') as out:
        for i, ln in enumerate(f):
            s = ln.split('\t')
            out.write(ln if ln.startswith('#') or i % 5 else '\t'.join(s[:-1] + [s[-1].replace('|', '/')]))
    files = [str(tmp_path / 'in' / 'call.vcf'), FILES[1]]
    E.main(files + extra)
    plain = capsys.readouterr().out
    assert os.listdir(str(tmp_path / 'out')) == []
    prefix = str(tmp_path / 'out' / 'x')
    E.main(files + extra + ['--details', prefix])
    assert capsys.readouterr().out == plain and plain
    assert sorted(os.listdir(str(tmp_path / 'out'))) == ['x.calls.tsv', 'x.truth.tsv']
    args = E.parse_args(files + extra)
    truth, calls = (E.parse_vcf(p, args.skip_phasing, args.bed_file or '') for p in (args.truthset, args.callset))
    a, rows, scored = E.flatten_rows(truth, calls)
    want = E.details_text(rows, scored, *E.details(truth, calls, args.refdist, args.pctsim))
    for name, text in zip(('x.calls.tsv', 'x.truth.tsv'), want):
        with open(str(tmp_path / 'out' / name)) as f:
            assert f.read() == text
    lines = [ln.split('\t') for ln in want[0].splitlines()[1:]]
    assert len(lines) == len(scored) > 50 and all(ln[15] in ('same', 'flip') for ln in lines)     # the phasing columns are always written
    on_contig = [ln for ln in lines if ln[6] == ln[0]]
    if '--skip_phasing' in extra:
        assert any(ln[5] != '1|1' for ln in on_contig)
    else:
        assert on_contig and all(ln[5] == '1|1' for ln in on_contig)


def filtered(src, dst, keep):
    with open(src) as f, open(dst, 'w') as out:
        for ln in f:
            if ln.startswith('#') or keep(ln.split('\t')):
                out.write(ln)
    return dst


def test_cli_error_leaves_no_file(tmp_path, capsys):
    d = tmp_path / 'in'
    d.mkdir()
    out = tmp_path / 'out'
    out.mkdir()
    prefix = str(out / 'x')
    empty = filtered(FILES[0], str(d / 'empty.vcf'), lambda s: False)
    no_chr2_truth = filtered(FILES[1], str(d / 'truth.vcf'), lambda s: s[0] != 'chr2')
    for argv, err in (([empty, FILES[1]], ZeroDivisionError),                   # an empty callset: len(callinfo) / 0 phase sets
                      ([FILES[0], no_chr2_truth], IndexError),                  # a call whose list has no truth record
                      (FILES + ['-p', '2'], ZeroDivisionError),                 # nothing matches: precision + recall is 0
                      (FILES + ['-r', '-1'], ZeroDivisionError)):
        with pytest.raises(err) as plain:
            E.main(argv)
        with pytest.raises(err) as detailed:
            E.main(argv + ['--details', prefix])
        assert str(plain.value) == str(detailed.value)
        assert os.listdir(str(out)) == []
    capsys.readouterr()
