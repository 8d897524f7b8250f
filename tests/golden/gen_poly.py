"""Generate tests/golden/poly.npz by running the REFERENCE on two user-defined systems, added the
way the reference's own extension point asks for: a subclass of systems.ODE with its _f_np
(systems.py:23-61).

Development container only, like gen_diffreact.py (the reference tree and this script never travel
to the GPU box; only the .npz is committed):

    PYTHONPATH=tests/golden/jaxshim:<reference tree> python tests/golden/gen_poly.py

Every number written is computed by reference code (systems.ODE.get_vector_field, RK.py, solver.py,
parareal.py) with use_jax=False.  The two _f_np below are written in the operation order of the
polynomial contract: each term coef * u_i * u_j left to right, the terms added
in list order -- the rows tests/poly_ref.py gives the same systems (VDP, lorenz96(40)).
"""
import os
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

import systems as rsys          # noqa: E402  (reference)
import RK as rrk                # noqa: E402
import solver as rsolver        # noqa: E402
import parareal as rpara        # noqa: E402


class VanDerPol(rsys.ODE):
    """x' = y, y' = y - x^2 y - x  (mu = 1)"""

    def __init__(self, **kwargs):
        mn, mx = np.array([[-2.5, -3.0], [2.5, 3.0]])
        super().__init__('VanDerPol', mn, mx, np.array([2.0, 0.0]), **kwargs)

    @staticmethod
    def _f_np(t, u):
        x, y = u
        return np.array([1.0 * y, (1.0 * y + ((-1.0 * x) * x) * y) + -1.0 * x])


class Lorenz96(rsys.ODE):
    """u_i' = (u_{i+1} - u_{i-2}) u_{i-1} - u_i + 8 on d = 40 periodic points, as four monomials"""

    def __init__(self, d=40, **kwargs):
        mn, mx = np.array([[-12.0] * d, [16.0] * d])
        u0 = 8.0 + 0.5 * np.sin(1.0 + 2.0 * np.arange(d))
        super().__init__(f'Lorenz96_{d}', mn, mx, u0, **kwargs)

    @staticmethod
    def _f_np(t, u):
        up, um, um2 = np.roll(u, -1), np.roll(u, 1), np.roll(u, 2)   # u_{i+1}, u_{i-1}, u_{i-2}
        return (((1.0 * up) * um + (-1.0 * um2) * um) + -1.0 * u) + 8.0


SYSTEMS = {'vdp': VanDerPol, 'l96': Lorenz96}
# classic Parareal, '-11', F = RK4, eps 5e-7: (tspan end, N, Ng, Nf, G).  Forward Euler is unstable on
# Lorenz-96 (its spectrum lies along the imaginary axis), so its coarse solver is RK4 with 4 steps.
PARA = {'vdp': (8.0, 16, 4, 40, 'RK1'), 'l96': (2.0, 8, 4, 40, 'RK4')}


def make(key, norm, **kw):
    return SYSTEMS[key](use_jax=False, **(dict(normalization='-11') if norm else {}), **kw)


def part_rhs(arrs):
    rng = np.random.default_rng(4321)
    for key in SYSTEMS:
        for norm in (False, True):
            ode = make(key, norm)
            f = ode.get_vector_field()
            d = ode.get_dim()
            U = ode.get_init_cond()[None, :] + (0.05 if norm else 0.5) * rng.uniform(-1, 1, size=(4, d))
            tag = f'rhs__{key}{"_n" if norm else ""}'
            arrs[tag + '__u'] = U
            arrs[tag + '__f'] = np.stack([np.asarray(f(0.0, u), dtype=float) for u in U])
            arrs[f'init__{key}{"_n" if norm else ""}__u0'] = ode.get_init_cond()


def part_rk(arrs):
    rng = np.random.default_rng(99)
    t0, t1, steps = 0.0, 0.25, 10
    for key in SYSTEMS:
        for norm in (False, True):
            ode = make(key, norm)
            f = ode.get_vector_field()
            u0 = ode.get_init_cond() + rng.uniform(-0.01, 0.01, size=ode.get_dim())
            for tab in ('RK1', 'RK2', 'RK4', 'RK8'):
                r = rrk.RK(f, tab)
                k = f'rk__{key}{"_n" if norm else ""}__{tab}'
                arrs[k + '__u0'] = u0
                arrs[k + '__span'] = np.array([t0, t1, steps], dtype=float)
                arrs[k + '__fixed'] = np.asarray(r.run_get_last(t0, t1, steps, u0), dtype=float)
                arrs[k + '__linspace'] = np.asarray(r.run(t0, t1, steps, u0), dtype=float)[-1]


def _final(u):
    cols = [c for c in range(u.shape[2]) if not np.any(np.isnan(u[:, :, c]))]
    return u[:, :, cols[-1]]


def _para(key, shift):
    T, N, Ng, Nf, G = PARA[key]
    ode = make(key, True)
    if shift:
        ode.set_default_init_cond(ode.normalizer.inverse(ode.get_init_cond()) + shift)
    s = rsolver.SolverRK(ode.get_vector_field(), Ng=Ng, Nf=Nf, F='RK4', G=G)
    p = rpara.Parareal(ode, s, tspan=[0, T], N=N, epsilon=5e-7, verbose=None)
    return ode, p.run(model='parareal')


def part_para(arrs):
    """One classic run each and the serial fine solution at the slice boundaries; and the same run
    from u0 + 1e-13, to show that the comparison bound (1e-9) is not decided by chaos: K and
    conv_int must stay and u must move by less than 1e-10."""
    for key in SYSTEMS:
        T, N, Ng, Nf, G = PARA[key]
        st = time.time()
        ode, res = _para(key, 0.0)
        _, res2 = _para(key, 1e-13)
        moved = float(np.nanmax(np.abs(res['u'] - res2['u'])))
        same = res['k'] == res2['k'] and list(res['conv_int']) == list(res2['conv_int'])
        print('parareal', key, 'K=', res['k'], 'conv_int', list(res['conv_int']), 'perturbed: same K/conv_int', same,
              'u moved', moved, f'{time.time() - st:.1f}s', flush=True)
        assert same and moved < 1e-10, (key, same, moved)
        tag = f'para__{key}'
        arrs[tag + '__cfg'] = np.array([0, T, N, Ng, Nf, 5e-7, int(G[2:])])
        arrs[tag + '__k'] = np.array(res['k'])
        arrs[tag + '__conv_int'] = np.array(res['conv_int'])
        arrs[tag + '__u'] = res['u']
        arrs[tag + '__err'] = res['err']
        arrs[tag + '__perturbed'] = np.array([1e-13, moved, float(same)])
        r = rrk.RK(ode.get_vector_field(), 'RK4')
        t = np.linspace(0, T, N + 1)
        u = ode.get_init_cond()
        fine = [u]
        for i in range(N):
            u = np.asarray(r.run_get_last(t[i], t[i + 1], Nf, u), dtype=float)
            fine.append(u)
        arrs[tag + '__fine'] = np.array(fine)
        print('   classic final vs fine', float(np.max(np.abs(_final(res['u']) - np.array(fine)))), flush=True)


if __name__ == '__main__':
    arrs = {}
    for part in (part_rhs, part_rk, part_para):
        st = time.time()
        part(arrs)
        print(part.__name__, f'{time.time() - st:.1f}s', flush=True)
    path = os.path.join(HERE, 'poly.npz')
    np.savez_compressed(path, **arrs)
    print('wrote', path, os.path.getsize(path), 'bytes', flush=True)
