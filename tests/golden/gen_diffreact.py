"""Generate tests/golden/diffreact.npz by running the REFERENCE's DiffReact system itself.

Development container only, like gen_golden.py (the reference tree and this script never travel
to the GPU box; only the .npz is committed):

    PYTHONPATH=tests/golden/jaxshim:<reference tree> python tests/golden/gen_diffreact.py

Every number written is computed by reference code (systems.py:463-577, RK.py, solver.py,
parareal.py) with use_jax=False, the deterministic scipy DIA path; this script only chooses inputs
and records outputs.
"""
import os
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

import systems as rsys          # noqa: E402  (reference)
import RK as rrk                # noqa: E402
import solver as rsolver        # noqa: E402
import parareal as rpara        # noqa: E402


def make(d_x, norm):
    kw = dict(normalization='-11') if norm else {}
    return rsys.DiffReact(d_x=d_x, use_jax=False, **kw)


def part_init(arrs):
    for d_x in (4, 10):
        for norm in (False, True):
            ode = make(d_x, norm)
            tag = f'init__{d_x}{"_n" if norm else ""}'
            arrs[tag + '__u0'] = ode.get_init_cond()
            arrs[tag + '__dim'] = np.array(ode.get_dim())
            arrs[tag + '__name'] = np.array(ode.name)
            arrs[tag + '__mn'] = np.asarray(ode.normalizer.mn, dtype=float)
            arrs[tag + '__mx'] = np.asarray(ode.normalizer.mx, dtype=float)


def part_rhs(arrs):
    rng = np.random.default_rng(1234)
    for d_x, norm in ((4, False), (4, True), (10, False), (10, True), (16, False), (17, False)):
        ode = make(d_x, norm)
        f = ode.get_vector_field()
        U = rng.uniform(-0.9, 0.9, size=(4, ode.get_dim()))
        F = np.stack([np.asarray(f(0.0, u), dtype=float) for u in U])
        tag = f'rhs__{d_x}{"_n" if norm else ""}'
        arrs[tag + '__u'] = U
        arrs[tag + '__f'] = F


def part_rk(arrs):
    rng = np.random.default_rng(99)
    t0, t1, steps = 0.0, 0.5, 10
    for d_x, norm in ((4, False), (10, True), (17, False)):
        ode = make(d_x, norm)
        f = ode.get_vector_field()
        u0 = ode.get_init_cond() + rng.uniform(-0.02, 0.02, size=ode.get_dim())
        for tab in ('RK1', 'RK2', 'RK4', 'RK8'):
            r = rrk.RK(f, tab)
            key = f'rk__{d_x}{"_n" if norm else ""}__{tab}'
            arrs[key + '__u0'] = u0
            arrs[key + '__span'] = np.array([t0, t1, steps], dtype=float)
            arrs[key + '__fixed'] = np.asarray(r.run_get_last(t0, t1, steps, u0), dtype=float)
            arrs[key + '__linspace'] = np.asarray(r.run(t0, t1, steps, u0), dtype=float)[-1]


def part_para(arrs):
    """Classic Parareal, '-11', G = RK1 2/slice, F = RK4 40/slice, eps 5e-7, and the serial fine
    solution at the slice boundaries."""
    for d_x, N, T in ((4, 8, 4), (8, 16, 8)):
        ode = make(d_x, True)
        f = ode.get_vector_field()
        s = rsolver.SolverRK(f, Ng=2, Nf=40, F='RK4', G='RK1')
        p = rpara.Parareal(ode, s, tspan=[0, T], N=N, epsilon=5e-7, verbose=None)
        st = time.time()
        res = p.run(model='parareal')
        print('parareal d_x', d_x, 'K=', res['k'], f'{time.time() - st:.1f}s', flush=True)
        tag = f'para__{d_x}'
        arrs[tag + '__cfg'] = np.array([0, T, N, 2, 40, 5e-7])
        arrs[tag + '__k'] = np.array(res['k'])
        arrs[tag + '__conv_int'] = np.array(res['conv_int'])
        arrs[tag + '__u'] = res['u']
        arrs[tag + '__err'] = res['err']
        r = rrk.RK(f, 'RK4')
        t = np.linspace(0, T, N + 1)
        u = ode.get_init_cond()
        fine = [u]
        for i in range(N):
            u = np.asarray(r.run_get_last(t[i], t[i + 1], 40, u), dtype=float)
            fine.append(u)
        arrs[tag + '__fine'] = np.array(fine)


if __name__ == '__main__':
    arrs = {}
    for part in (part_init, part_rhs, part_rk, part_para):
        st = time.time()
        part(arrs)
        print(part.__name__, f'{time.time() - st:.1f}s', flush=True)
    path = os.path.join(HERE, 'diffreact.npz')
    np.savez_compressed(path, **arrs)
    print('wrote', path, os.path.getsize(path), 'bytes', flush=True)
