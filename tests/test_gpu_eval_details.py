# coding=utf-8
"""-m gpu: duet_eval_details_host (duet_amd/csrc/duet_eval_details.hip) through Context.eval_details_host against the records of
the Python path (evaluation.details_host, pinned by tests/test_eval_details_host.py), byte for byte: the hand-written cases and
the golden configurations, seeded random problems at the sizes where the kernels' blocks, the sort's tiles and the lists begin
and end, and the command line with --gpu.  On every problem `counts` is what duet_eval_run_host gives."""
import json
import os

import numpy as np
import pytest

from duet_amd import _lib
from duet_amd import evaluation as E
from tests import eval_details_cases as C
from tests import helpers as H

pytestmark = pytest.mark.gpu

EVAL = os.path.join(H.GOLDEN, 'eval')
NAMES = ('call_tp', 'base_tp', 'call_gt', 'base_gt', 'call_hp', 'base_hp')


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def check(ctx, a):
    want_counts, want_calls, want_base = E.details_host(a, a['refdist'], a['ratio'])
    counts, calls, base = ctx.eval_details_host(a)
    assert calls.dtype == want_calls.dtype and calls.tobytes() == want_calls.tobytes(), np.nonzero(calls != want_calls)[0][:8]
    assert base.dtype == want_base.dtype and base.tobytes() == want_base.tobytes(), np.nonzero(base != want_base)[0][:8]
    got = tuple(int(getattr(counts, f)) for f in NAMES)
    plain = ctx.eval_counts(a, a['refdist'], a['ratio'])
    assert got == tuple(int(getattr(plain, f)) for f in NAMES) == tuple(want_counts)
    return calls, base


@pytest.mark.parametrize('name', sorted(C.CASES))
def test_hand_written_case(ctx, name):
    truth, calls, refdist, ratio = C.CASES[name][:4]
    a = E.flatten(truth, calls)
    a['refdist'], a['ratio'] = refdist, ratio
    check(ctx, a)
    # through evaluation.details, and as text: the rows the case spells out
    a, rows, scored = E.flatten_rows(truth, calls)
    text = E.details_text(rows, scored, *E.details(truth, calls, refdist, ratio, ctx=ctx))
    assert [ln.split('\t') for ln in text[0].splitlines()[1:]] == C.CASES[name][4]
    assert [ln.split('\t') for ln in text[1].splitlines()[1:]] == C.CASES[name][5]


def test_golden_configurations(ctx):
    with open(os.path.join(EVAL, 'expected.json')) as f:
        cases = json.load(f)
    for c in cases:
        pair = os.path.join(EVAL, 'pair%d' % c['pair'])
        bed = os.path.join(pair, 'regions.bed') if c['bed'] else ''
        a = E.flatten(E.parse_vcf(os.path.join(pair, 'truth.vcf'), c['skip_phasing'], bed),
                      E.parse_vcf(os.path.join(pair, 'call.vcf'), c['skip_phasing'], bed))
        a['refdist'], a['ratio'] = c['refdist'], c['pctsim']
        check(ctx, a)


@pytest.mark.parametrize('n_calls', [1, 2, 63, 64, 65, 255, 256, 257, 5000])
def test_random_problems(ctx, n_calls):
    hits = 0
    for n_base in (1, 2, 256, 257, 5000):
        for n_keys in (1, 48):
            a = C.random_problem(100000 * n_keys + 10 * n_calls + n_base, n_calls, n_base, n_keys)
            used = np.unique(np.repeat(np.arange(n_keys), np.diff(a['base_off'].astype(np.int64))))
            assert len(used) == 1 or used[-1] not in a['call_key']            # a list with truth records and no call
            calls, base = check(ctx, a)
            hits += int(np.count_nonzero(calls['bits'] & _lib.EVAL_MATCHED))
            assert len(used) == 1 or np.count_nonzero(base['reason'] == 0) > 0
    assert hits > 0


@pytest.mark.parametrize('n_calls,n_base,n_keys', [(2, 1, 1), (65, 300, 1), (257, 256, 48), (5000, 5000, 48), (5000, 40, 3)])
def test_calls_without_a_list_key(ctx, n_calls, n_base, n_keys):
    """They sort behind every list (the bucket n_keys): the last list's records must not take one for a neighbour."""
    a = C.random_problem(77000 + n_calls + n_base, n_calls, n_base, n_keys, unlisted=5)
    none = a['call_key'] == _lib.EVAL_NONE
    assert none[0] and none[-1]
    calls, base = check(ctx, a)
    assert set(calls['base'][none].tolist()) == {_lib.EVAL_NONE} and not (calls['bits'][none] & ~np.uint32(_lib.EVAL_LABEL)).any()
    assert not np.isin(base['nearest'], np.nonzero(none)[0]).any()
    if n_calls > 2:
        # all of them without a key: every record is a no_call
        a['call_key'][:] = _lib.EVAL_NONE
        calls, base = check(ctx, a)
        assert set(base['reason'].tolist()) == {0}


def test_an_id_or_group_out_of_range_is_refused_for_every_call(ctx):
    a = C.random_problem(12, 20, 40, 3, unlisted=5)
    for field, bound in (('call_group', 'n_groups'), ('call_uid', 'n_call_uid')):
        for c in (0, int(np.nonzero(a['call_key'] != _lib.EVAL_NONE)[0][0])):      # a call without a list key, and one with
            b = dict(a)
            b[field] = a[field].copy()
            b[field][c] = a[bound]
            with pytest.raises(_lib.DuetLibraryError, match='out of range'):
                ctx.eval_details_host(b)


def test_every_call_of_a_list_on_one_position(ctx):
    a = C.random_problem(5, 600, 300, 3, call_pos=17)
    first = a['call_key'] == a['call_key'].min()
    assert np.count_nonzero(first) > 100 and set(a['call_pos'][first].tolist()) == {17}
    calls, base = check(ctx, a)
    # all records of that list have one nearest call: the first of the list in the callset
    assert set(base['nearest'][:int(a['base_off'][int(a['call_key'].min()) + 1])].tolist()) == {int(np.nonzero(first)[0][0])}


def test_every_truth_record_of_a_list_on_one_position(ctx):
    a = C.random_problem(6, 600, 300, 3, base_pos=17)
    n = int(a['base_off'][1])
    assert n > 50 and set(a['base_pos'][:n].tolist()) == {17}
    calls, base = check(ctx, a)
    # the calls take the first of the equal records (or, from above, the last); every record has the same nearest call
    assert len(set(base['nearest'][:n].tolist())) == 1
    assert set(calls['base'][a['call_key'] == 0].tolist()) <= {0, n - 1}


def test_no_call_at_all(ctx):
    a = C.random_problem(7, 1, 40, 3)
    for k in ('call_key', 'call_pos', 'call_len', 'call_uid', 'call_group', 'call_hp'):
        a[k] = a[k][:0]
    calls, base = check(ctx, a)
    assert len(calls) == 0 and set(base['reason'].tolist()) == {0} and set(base['nearest'].tolist()) == {_lib.EVAL_NONE}


def test_a_call_without_truth_records_is_refused(ctx):
    a = C.random_problem(8, 20, 40, 48)
    empty = [k for k in range(48) if a['base_off'][k] == a['base_off'][k + 1]]
    a['call_key'][3] = empty[0]
    with pytest.raises(_lib.DuetLibraryError, match='no truth record'):
        ctx.eval_details_host(a)
    a['call_key'][3] = 48
    with pytest.raises(_lib.DuetLibraryError, match='no truth record'):
        ctx.eval_details_host(a)


def test_workspace_re_use(ctx):
    """One context: a large problem, a small one, the plain evaluator in between -- nothing stale in the shared arena."""
    big = C.random_problem(9, 5000, 5000, 48)
    small = C.random_problem(10, 3, 2, 1)
    for _ in range(2):
        check(ctx, big)
        check(ctx, small)


def test_cli_with_gpu_writes_the_same_files(tmp_path, capsys):
    pair = os.path.join(EVAL, 'pair2')
    argv = [os.path.join(pair, 'call.vcf'), os.path.join(pair, 'truth.vcf'), '-r', '500', '-p', '0.7', '-b', os.path.join(pair, 'regions.bed')]
    E.main(argv + ['--details', str(tmp_path / 'host')])
    host_out = capsys.readouterr().out
    E.main(argv + ['--gpu', '--details', str(tmp_path / 'gpu')])
    assert capsys.readouterr().out == host_out
    for suffix in ('.calls.tsv', '.truth.tsv'):
        with open(str(tmp_path / 'host') + suffix) as f, open(str(tmp_path / 'gpu') + suffix) as g:
            text = f.read()
            assert g.read() == text and text.count('\n') > 50
