# coding=utf-8
"""No GPU: the model of stage A0's plan (tests/cluster_model.py: plan_from_counts) against the driver's own plan function (cl_plan,
duet_amd/csrc/duet_cluster_plan.h -- the one duet_cluster_run calls), compiled into the stand-alone tools/cluster_plan_check.hip:
field for field, on every field the model has.  tests/test_cluster_case_edges.py places the named cases on their edges with the
model; this is what keeps the model the driver's."""
import os
import shutil
import subprocess

import pytest

from tests import cluster_cases as C
from tests import cluster_model as Mo
from tests.test_gpu_cluster import MODES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'

GRID_M = (1, 2, 15, 16, 4095, 4096, 4097, 65536, 1249999, 1250000, 2097152, 2097153, 4194304, 4194305)
GRID_BITS = ((8, 1, 1), (22, 1, 1), (23, 1, 1), (28, 3, 5), (32, 8, 16), (40, 8, 16))
GRID_PART_MAX = (1, 100, 101, 128)


@pytest.fixture(scope='module')
def driver_plan(tmp_path_factory):
    """-> f(rows of (M, centre_bits, type_bits, contig_bits, dbg, part_max)) -> the driver's plan of every row, as text fields"""
    exe = str(tmp_path_factory.mktemp('plan') / 'cluster_plan_check')
    cmd = [HIPCC, '--offload-arch=gfx950', '-O1', '-std=c++17', '-Wno-unused-function', '-I' + os.path.join(REPO, 'include'),
           '-I' + os.path.join(REPO, 'duet_amd', 'csrc'), os.path.join(REPO, 'tools', 'cluster_plan_check.hip'), '-o', exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(rows):
        text = ''.join('%d %d %d %d %d %d 1\n' % row for row in rows)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(rows)
        return [dict(f.split('=') for f in ln.split()) for ln in lines]
    return run


def as_model(text, like):
    """a printed field in the type the model holds it in"""
    if isinstance(like, bool):
        assert text in ('0', '1')
        return text == '1'
    if isinstance(like, list):
        return [int(w) for w in text.split(',')] if text else []
    return int(text)


def compare(driver_plan, rows):
    for row, got in zip(rows, driver_plan(rows)):
        want = Mo.plan_from_counts(*row)
        assert len(want) >= 25
        for name, v in want.items():
            assert as_model(got[name], v) == v and type(as_model(got[name], v)) is type(v), (row, name, got[name], v)


def test_the_model_is_the_drivers_plan_on_every_named_case(driver_plan):
    rows = []
    for name in C.NAMES:
        marks, kw = C.case(name)
        for hints in (True, False):
            counts = Mo.bit_counts(marks, hints)[:3]
            rows += [(len(marks['pos']),) + counts + (dbg, kw.get('part_max', 100)) for h, dbg in MODES if h == hints]
    assert len(rows) == len(C.NAMES) * len(MODES)
    compare(driver_plan, rows)
    # ... and through plan(marks, ...), the form the edge tests call
    marks, kw = C.case(C.NAMES[0])
    for hints, dbg in MODES[:4]:
        full = Mo.plan(marks, dbg, hints, kw.get('part_max', 100))
        assert full.pop('hinted') in (True, False)
        assert full == Mo.plan_from_counts(len(marks['pos']), *Mo.bit_counts(marks, hints)[:3], dbg=dbg, part_max=kw.get('part_max', 100))


def test_the_model_is_the_drivers_plan_on_a_grid_of_counts(driver_plan):
    rows = [(M, c, t, k, dbg, pm) for M in GRID_M for c, t, k in GRID_BITS for dbg in sorted(set(d for _, d in MODES)) for pm in GRID_PART_MAX]
    compare(driver_plan, rows)
    # the grid has both sides of what it is there for
    plans = [Mo.plan_from_counts(*row) for row in rows]
    for name in ('idx_packed', 'rec_mode', 'rs_small', 'small_in', 'hybrid', 'use_spine', 'box_applies', 'tiers', 'wide', 'cap100'):
        assert {p[name] for p in plans} == {True, False}, name
    assert {p['key_bits'] for p in plans} >= {10, 64} and {p['rs_np'] for p in plans} >= {0, 1, 2, 3}
