"""Cost of the polynomial vector field (PolyODE, NNGP_SYS_POLY) per RK step.

    python tools/poly_probe.py [--lib PATH] lane  [--reps R] [--steps S]
    python tools/poly_probe.py [--lib PATH] field [--reps R] [--steps S]

  lane:  Brusselator and Lorenz, '-11', 128 slices, RK4: the built-in lane kernel (NNGP_RK_GROUP=0),
         the built-in default (the lane-group kernel) and the same system as a PolyODE (lane form)
  field: Lorenz-96 as a PolyODE at d = 40 and d = 1024, 64 and 512 slices, RK8 (field form)
--lib loads another build of the library (same C-ABI), so that two forms of a kernel are measured
in one session by the same script.  Each launch is timed with events after two warm-up launches;
every time is printed, then the median.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRUS = [[(1.0, ()), (1.0, (0, 0, 1)), (-4.0, (0,))], [(3.0, (0,)), (-1.0, (0, 0, 1))]]
LORENZ = [[(10.0, (1,)), (-10.0, (0,))], [(28.0, (0,)), (-1.0, (1,)), (-1.0, (0, 2))],
          [(1.0, (0, 1)), (-(8.0 / 3), (2,))]]


def lorenz96(d, forcing=8.0):
    return [[(1.0, ((i + 1) % d, (i - 1) % d)), (-1.0, ((i - 2) % d, (i - 1) % d)), (-1.0, (i,)), (forcing, ())]
            for i in range(d)]


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')


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
    ap.add_argument('--lib', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=None)
    ap.add_argument('what', choices=['lane', 'field'])
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import nngp_amd as g
    from nngp_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    torch.cuda.set_device(0)
    tag = f'[{os.path.relpath(_lib.LIB_PATH, ROOT)}]'
    rng = np.random.default_rng(0)
    if a.what == 'lane':
        n, steps = 128, a.steps or 100_000
        T0 = dev(np.linspace(0, 1, n))
        T1 = T0 + 1e-3
        for name, rows, built in (('Brusselator', BRUS, g.Brusselator(normalization='-11')),
                                  ('Lorenz', LORENZ, g.Lorenz(normalization='-11'))):
            U0 = dev(built.get_init_cond()[None, :] + 0.01 * rng.standard_normal((n, built.d)))
            sb = g.SolverRK(built.get_vector_field(), Ng=4, Nf=steps, F='RK4', G='RK1')
            os.environ['NNGP_RK_GROUP'] = '0'
            timed(lambda: sb.run_F_batch(T0, T1, U0), a.reps, steps, f'{tag} {name} built-in lane kernel RK4 n={n}')
            del os.environ['NNGP_RK_GROUP']
            timed(lambda: sb.run_F_batch(T0, T1, U0), a.reps, steps, f'{tag} {name} built-in default    RK4 n={n}')
            poly = g.PolyODE(rows, built.normalizer.inverse(built.get_init_cond()), mn=built.normalizer.mn,
                             mx=built.normalizer.mx, normalization='-11')
            sp = g.SolverRK(poly.get_vector_field(), Ng=4, Nf=steps, F='RK4', G='RK1')
            timed(lambda: sp.run_F_batch(T0, T1, U0), a.reps, steps, f'{tag} {name} as PolyODE (lane)   RK4 n={n}')
    else:
        steps = a.steps or 2_000
        for d in (40, 1024):
            poly = g.PolyODE(lorenz96(d), np.full(d, 2.0), mn=-12.0, mx=16.0, normalization='-11')
            s = g.SolverRK(poly.get_vector_field(), Ng=4, Nf=steps, F='RK8', G='RK1')
            for n in (64, 512):
                U0 = dev(poly.get_init_cond()[None, :] + 0.05 * rng.standard_normal((n, d)))
                T0 = dev(np.linspace(0, 1, n))
                T1 = T0 + 1e-2
                timed(lambda: s.run_F_batch(T0, T1, U0), a.reps, steps,
                      f'{tag} Lorenz-96 d={d} as PolyODE (field) RK8 n={n}')


if __name__ == '__main__':
    main()
