"""GPU: bench.py as a command -- the plain run's result line and --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_bench_run_prints_its_line_and_dumps_the_timed_end_states(gpu, tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` (a short schedule: 1 000 RK4 steps per slice) ends
    with the one JSON line, times K steps, runs none of the --full legs, and --dump-outputs writes
    the end states of the timed sweep: float64, bitwise the oracle's sweep of the same seeded inputs."""
    import oracle as O
    n, nf, steps = 128, 1000, 2
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps),
                        '--warmup', '1', '--steps-per-slice', str(nf), '--dump-outputs', str(tmp_path / 'out')],
                       capture_output=True, text=True, timeout=240, env=env, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    rec = json.loads(p.stdout.splitlines()[-1])
    assert rec['steps'] == steps and rec['n_gpus'] == 1 and rec['dtype'] == 'f64' and rec['higher_is_better']
    assert rec['unit'] == 'fine RK steps/s' and rec['ms_per_step'] > 0
    assert rec['value'] == pytest.approx(n * nf / (rec['ms_per_step'] / 1e3), rel=1e-9)
    assert 'fhn_pde_strong' not in rec and 'cpu_baseline' not in rec and 'published_k' not in rec
    assert sorted(os.listdir(tmp_path / 'out')) == ['fine_end_states.npy']
    got = np.load(tmp_path / 'out' / 'fine_end_states.npy')
    assert got.dtype == np.float64 and got.shape == (n, 3) and rec['outputs'] == {'fine_end_states': [n, 3]}
    t = np.linspace(-20, 500, n + 1)
    U = np.random.default_rng(1234).uniform(-0.5, 0.5, size=(n, 3))
    ref = O.System('hopf', param=(500.0,)).rk_batch(4, t[:-1], t[1:], nf, U)
    assert np.array_equal(got, ref), np.max(np.abs(got - ref))
