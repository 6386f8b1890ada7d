"""GPU: bench.py's timed path on the small C1 workload -- --steps K is the number of timed steps (ONE call of K
iterations; ms_per_step is its time / K), and --dump-outputs writes what that call computed in its last step, bit for
bit the same in two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')


@pytest.mark.gpu
def test_bench_times_exactly_steps_and_dumps_the_same_outputs_every_run(tmp_path):
    dumps = []
    for run in range(2):
        out = tmp_path / ('dump%d' % run)
        detail = tmp_path / ('detail%d.json' % run)
        p = subprocess.run([sys.executable, BENCH, '--gpus', '1', '--steps', '3', '--warmup', '2', '--workload', 'c1',
                            '--no-cpu-baseline', '--shard-of', '1', '--detail', str(detail), '--dump-outputs', str(out)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
        assert len(lines) == 1
        line = json.loads(lines[0])
        rec = json.load(open(str(detail)))['workloads']['c1']
        assert line['steps'] == 3 and line['ms_per_step'] > 0 and line['timing']['repeats'] == 1
        assert rec['repeats'] == 1 and rec['ms_per_step'] == pytest.approx(rec['timed_s'] * 1e3 / 3)
        names = sorted(os.listdir(str(out)))
        assert names == sorted('c1_%s.npy' % n for n in ('columns', 'X', 'V', 'EX', 'EV', 'dwell', 'transitions', 'stats'))
        assert sum(os.path.getsize(str(out / n)) for n in names) <= 64 << 20
        arrays = {n[:-len('.npy')]: np.load(str(out / n)) for n in names}
        assert all(a.dtype == np.float64 for a in arrays.values())
        assert arrays['c1_X'].shape == (2, 100) and np.isfinite(arrays['c1_X']).all()
        stats = arrays['c1_stats']
        assert stats[0] + stats[1] + stats[2] == 100        # l + f + r moves of the last step: every particle once
        dumps.append(arrays)
    for n in dumps[0]:
        assert np.array_equal(dumps[0][n], dumps[1][n], equal_nan=True), n


@pytest.mark.gpu
def test_a_plain_run_measures_the_head_only_and_full_adds_the_rest(tmp_path):
    """Without --full the run times the head workload and stops there: no CPU baseline, no boundary or
    one-iteration-per-call figures.  --full measures those as before, around the same kind of timed call."""
    lines = {}
    for mode in ('plain', 'full'):
        extra = ['--full', '--detail', str(tmp_path / 'detail.json')] if mode == 'full' else []
        p = subprocess.run([sys.executable, BENCH, '--gpus', '1', '--steps', '3', '--warmup', '2', '--workload', 'c1'] + extra,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        out = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
        assert len(out) == 1
        lines[mode] = json.loads(out[0])
    plain, full = lines['plain'], lines['full']
    for line in (plain, full):
        assert line['steps'] == 3 and line['warmup'] == 2 and line['ms_per_step'] > 0 and line['value'] > 0
        assert line['metric'] == 'particle-steps/sec (ndims x nparticles x L)' and line['higher_is_better'] is True
        assert list(line['summary']) == ['c1']
    assert plain['unit'] == full['unit'] and plain['dtype'] == full['dtype']
    assert 'cpu_baseline' not in plain and 'boundary' not in plain and 'c1_one_iter_ms' not in plain['config']
    assert full['cpu_baseline']['value'] > 0 and full['boundary']['samples'] > 0 and full['config']['c1_one_iter_ms'] > 0
    assert 'c1' in json.load(open(str(tmp_path / 'detail.json')))['workloads']
