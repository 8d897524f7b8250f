"""Cost of the sampled-trajectory launch (nngp_rk_traj) next to the end-state launch (nngp_rk_batch)
on two fine schedules, and the wall time of SolverRK.run_F_full.

    python tools/traj_probe.py [--root DIR] end  hopf|fhn [--reps R]
    python tools/traj_probe.py              traj hopf|fhn EVERY [EVERY ...] [--reps R]
    python tools/traj_probe.py [--root DIR] full [--reps R]

  hopf: Hopf '-11', N = 128 slices, RK4, 10^6 steps per slice (the lane-group kernel)
  fhn:  FHN-PDE d = 800 (20 x 20), 512 slices, RK8, 2 * 10^3 steps (the point-pair kernel)
  full: Lorenz '-11', RK4, run_F_full over 2000 steps (numpy in and out)
EVERY may be the word `steps` (only u0 and the end state are written).  --root imports the package
from another checkout of this repository (with its library built), so that two commits are measured
in one session by the same script; `end` and `full` use only what every commit has.
Each launch is timed with events after two warm-up launches; every time is printed, then the median.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

SCHEDULES = {'hopf': ('RK4', 128, 1_000_000), 'fhn': ('RK8', 512, 2_000)}


def setup(g, name):
    tab, n, steps = SCHEDULES[name]
    rng = np.random.default_rng(0)
    dev = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')
    if name == 'hopf':
        ode = g.Hopf(normalization='-11')
        U0 = dev(rng.uniform(-0.3, 0.3, (n, 3)))
        T0 = dev(np.linspace(0, 1, n))
        T1 = T0 + 1e-3
    else:
        ode = g.FHN_PDE(d_x=20)
        u0 = ode.get_init_cond()
        U0 = dev(np.clip(u0[None, :] + 0.01 * rng.standard_normal((n, len(u0))), -1, 1))
        T0 = dev(np.linspace(0, 1, n))
        T1 = T0 + 1e-2
    s = g.SolverRK(ode.get_vector_field(), Ng=4, Nf=steps, F=tab, G='RK1')
    return s, T0, T1, U0, steps, f'{name} {tab} n={n} steps={steps}'


def timed(fn, reps, steps, label):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    print(f'{label}: median {med:.3f} ms = {med * 1e3 / steps:.5f} us/step  min {min(ms):.3f} max {max(ms):.3f}  '
          f'all [{", ".join(f"{x:.3f}" for x in ms)}]', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('what', choices=['end', 'traj', 'full'])
    ap.add_argument('args', nargs='*')
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import nngp_amd as g
    torch.cuda.set_device(0)
    tag = f'[{os.path.relpath(os.path.abspath(a.root))}]'
    if a.what == 'full':
        ode = g.Lorenz(normalization='-11')
        s = g.SolverRK(ode.get_vector_field(), Ng=4, Nf=2000, F='RK4', G='RK1')
        u0 = ode.get_init_cond()
        s.run_F_full(0.0, 0.5, u0)
        wall = []
        for _ in range(a.reps):
            t = time.perf_counter()
            out = s.run_F_full(0.0, 0.5, u0)
            wall.append(time.perf_counter() - t)
        print(f'{tag} run_F_full lorenz RK4 steps=2000 -> {out.shape}: median {statistics.median(wall) * 1e3:.2f} ms  '
              f'all [{", ".join(f"{x * 1e3:.2f}" for x in wall)}]', flush=True)
        return
    s, T0, T1, U0, steps, label = setup(g, a.args[0])
    if a.what == 'end':
        out = torch.empty_like(U0)
        timed(lambda: s.run_F_batch(T0, T1, U0, out=out), a.reps, steps, f'{tag} end-state {label}')
        return
    end = s.run_F_batch(T0, T1, U0)
    for ev in a.args[1:]:
        every = steps if ev == 'steps' else int(ev)
        rows = s.traj_rows(steps, every)
        out = torch.empty((U0.shape[0], rows, U0.shape[1]), dtype=torch.float64, device='cuda')
        timed(lambda: s.run_F_traj_batch(T0, T1, U0, every=every, out=out), a.reps, steps,
              f'{tag} traj every={every} ({out.numel() * 8 / 2**20:.1f} MiB) {label}')
        assert torch.equal(out[:, -1].view(torch.int64), end.view(torch.int64)), 'last row != end state'
        del out
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
