"""Cost of a field with elementary-function atoms (FuncODE, NNGP_SYS_FUNC) per RK step.

    python tools/func_probe.py [--lib PATH] lane  [--reps R] [--steps S]
    python tools/func_probe.py [--lib PATH] field [--reps R] [--steps S]

  lane:  ThomasLabyrinth, '-11', 128 slices, RK4 and RK8: the built-in lane kernel (NNGP_RK_GROUP=0),
         the built-in default (the lane-group kernel) and the same system as a FuncODE of three sine
         atoms (lane form)
  field: sine-Gordon by lines at d = 1024 (512 sine atoms) and Bratu at d = 40 (40 exp atoms) as
         FuncODE, each beside a PolyODE with the same rows in which every atom index is replaced by a
         state index -- the same term count and the same walk, without the atoms and their second
         barrier; 64 slices, RK4 and RK8
--lib loads another build of the library (same C-ABI).  Each launch is timed with events after two
warm-up launches; every time is printed, then the median.  One process, nothing asserted.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THOMAS_ATOMS = [('sin', (1.0, 1)), ('sin', (1.0, 2)), ('sin', (1.0, 0))]
THOMAS_ROWS = [[(-0.5, (0,)), (10.0, (3,))], [(-0.5, (1,)), (10.0, (4,))], [(-0.5, (2,)), (10.0, (5,))]]


def sine_gordon(points, length):
    """u_tt = u_xx - sin u, periodic, by lines: state u | v, d = 2 points (tests/func_ref.py)"""
    n = points
    c = 1.0 / (length / n) ** 2
    atoms = [('sin', (1.0, i)) for i in range(n)]
    rows = [[(1.0, (n + i,))] for i in range(n)]
    rows += [[(c, ((i - 1) % n,)), (-2.0 * c, (i,)), (c, ((i + 1) % n,)), (-1.0, (2 * n + i,))] for i in range(n)]
    x = length * np.arange(n) / n
    u0 = np.concatenate([4.0 * np.arctan(np.exp(-0.5 * (x - length / 2) ** 2 + 1.0)), 0.2 * np.sin(2 * np.pi * x / length)])
    return atoms, rows, u0, -8.0, 8.0


def bratu(d, lam=2.0):
    """u_t = u_xx + lambda exp(u) on (0, 1), zero at both ends (tests/func_ref.py)"""
    c = float((d + 1) ** 2)
    atoms = [('exp', (1.0, i)) for i in range(d)]
    rows = []
    for i in range(d):
        row = [(c, (i - 1,))] if i > 0 else []
        row.append((-2.0 * c, (i,)))
        if i + 1 < d:
            row.append((c, (i + 1,)))
        row.append((lam, (d + i,)))
        rows.append(row)
    u0 = 0.3 * np.sin(np.pi * np.arange(1, d + 1) / (d + 1)) + 0.05
    return atoms, rows, u0, -1.0, 2.0


def without_atoms(rows, d):
    """the same rows with atom index d + q replaced by the state index q mod d: a PolyODE of the same
    term count (another system: only its cost is of interest)"""
    return [[(coef, tuple(i if i < d else (i - d) % d for i in ind)) for coef, ind in row] for row in rows]


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
        n, steps = 128, a.steps or 20_000
        T0 = dev(np.linspace(0, 1, n))
        T1 = T0 + 1e-3
        built = g.ThomasLabyrinth(normalization='-11')
        func = g.FuncODE(atoms=THOMAS_ATOMS, terms=THOMAS_ROWS, u0=built.normalizer.inverse(built.get_init_cond()),
                         mn=built.normalizer.mn, mx=built.normalizer.mx, normalization='-11')
        U0 = dev(built.get_init_cond()[None, :] + 0.01 * rng.standard_normal((n, 3)))
        for tab in ('RK4', 'RK8'):
            sb = g.SolverRK(built.get_vector_field(), Ng=4, Nf=steps, F=tab, G='RK1')
            os.environ['NNGP_RK_GROUP'] = '0'
            timed(lambda: sb.run_F_batch(T0, T1, U0), a.reps, steps, f'{tag} Thomas built-in lane kernel {tab} n={n}')
            del os.environ['NNGP_RK_GROUP']
            timed(lambda: sb.run_F_batch(T0, T1, U0), a.reps, steps, f'{tag} Thomas built-in default     {tab} n={n}')
            sf = g.SolverRK(func.get_vector_field(), Ng=4, Nf=steps, F=tab, G='RK1')
            timed(lambda: sf.run_F_batch(T0, T1, U0), a.reps, steps, f'{tag} Thomas as FuncODE (lane)    {tab} n={n}')
            assert torch.equal(sf.run_F_batch(T0, T1, U0), sb.run_F_batch(T0, T1, U0))   # the same bits
    else:
        steps, n = a.steps or 2_000, 64
        for name, (atoms, rows, u0, mn, mx), span in (('sine-Gordon d=1024', sine_gordon(512, 64.0), 1e-2),
                                                      ('Bratu d=40', bratu(40), 1e-4)):
            d = len(u0)
            func = g.FuncODE(atoms=atoms, terms=rows, u0=u0, mn=mn, mx=mx, normalization='-11')
            poly = g.PolyODE(without_atoms(rows, d), u0, mn=mn, mx=mx, normalization='-11')
            U0 = dev(func.get_init_cond()[None, :] + 1e-3 * rng.standard_normal((n, d)))
            T0 = dev(np.linspace(0, 1, n))
            T1 = T0 + span
            for tab in ('RK4', 'RK8'):
                sf = g.SolverRK(func.get_vector_field(), Ng=4, Nf=steps, F=tab, G='RK1')
                sp = g.SolverRK(poly.get_vector_field(), Ng=4, Nf=steps, F=tab, G='RK1')
                timed(lambda: sf.run_F_batch(T0, T1, U0), a.reps, steps,
                      f'{tag} {name} as FuncODE ({len(atoms)} atoms, field) {tab} n={n}')
                timed(lambda: sp.run_F_batch(T0, T1, U0), a.reps, steps,
                      f'{tag} {name} rows as PolyODE (no atoms, field)  {tab} n={n}')


if __name__ == '__main__':
    main()
