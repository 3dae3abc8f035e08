# coding=utf-8
"""-m gpu: a plain bench.py run (no --full) is the headline alone -- set-up, warm-up, the timed steps, --dump-outputs and
the line -- and what it computed is still bit for bit what the C oracle computes on the same seeded input."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from duet_amd import engine, synth
from oracle import c_oracle

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what only --full measures or checks: none of it may appear on a plain run's line
FULL_ONLY = ('parity_vs_oracle', 'kernels_us_isolated', 'cpu_baseline', 'cpu_baseline_ncore', 'cpu_baseline_python',
             'value_clustered_and_phased', 'roofline_clustered_and_phased', 'roofline_bandwidth_bound', 'scaling_point_1gpu',
             'summed_kernels_frac_B_EF', 'extra', 'same_problem_on_1_gpu', 'value_vs_1gpu_same_problem', 'detail_file')


def plain_line(args, env, out_dir):
    out = subprocess.check_output([sys.executable, os.path.join(REPO, 'bench.py')] + args + ['--dump-outputs', str(out_dir)],
                                  env=env, timeout=600).decode()
    line = [l for l in out.splitlines() if l.startswith('{')][-1]
    d = json.loads(line)
    assert d['metric'] == bench.METRIC and d['unit'] == 'marks/s' and d['higher_is_better'] is True and d['dtype'] == bench.DTYPE
    for k in FULL_ONLY:
        assert k not in d, k
    return d


def assert_dump_matches_oracle(out_dir, soa):
    pred = np.load(os.path.join(str(out_dir), 'pred.npy'))
    ps = np.load(os.path.join(str(out_dir), 'ps.npy'))
    rc, want_pred, want_ps = c_oracle.ef(soa, 50, 2)
    assert rc == 0 and len(pred) == soa.n_cands
    assert np.array_equal(pred.astype(np.uint8), want_pred) and np.array_equal(ps.astype(np.uint32), want_ps)


def test_plain_single_gpu_run(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    d = plain_line(['--gpus', '1', '--steps', '20', '--warmup', '5'], env, tmp_path)
    assert d['n_gpus'] == 1 and d['steps'] == 20 and d['warmup'] == 5 and d['config']['device_preheat_steps'] > 0
    # value = marks per step / time per step (the line keeps 6 significant digits)
    assert abs(d['value'] * d['ms_per_step'] * 1e-3 / d['config']['marks_per_gpu'] - 1) < 1e-4
    # 20 steps hold two sampled ef_classify launches: too few for the roofline, whose fallback loop is --full's
    assert 'roofline' not in d
    assert_dump_matches_oracle(tmp_path, engine.soa_from_synth([synth.bench_contig('1', 200000, 100000, 1, spelled='chr1')]))


def test_plain_sharded_run_one_gpu_plumbing(tmp_path):
    """N > 1 without --full: the sharded timed steps and the gathered, merged call set; no 1-GPU reference, no isolated
    figures.  DUET_BENCH_ONE_GPU=1: both ranks on device 0, gloo -- plumbing, not a measurement."""
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    env['DUET_BENCH_ONE_GPU'] = '1'
    d = plain_line(['--gpus', '2', '--steps', '3', '--warmup', '1', '--genome-marks', '400000'], env, tmp_path)
    assert d['n_gpus'] == 2 and d['scaling'] == 'strong' and d['steps'] == 3 and d['warmup'] == 1
    assert d['gather'] == {'collectives_per_problem': 1, 'bytes_contributed_per_rank': d['sharding']['record_bytes_per_rank']}
    assert sum(d['per_rank']['marks']) == d['config']['marks'] and 'kernels_only_us' not in d['per_rank']
    assert d['topology']['world_size'] == 2
    assert_dump_matches_oracle(tmp_path, engine.soa_from_synth(synth.bench_genome(400000, 3)))
