"""Generate tests/golden/func.npz by running the REFERENCE on seven user-defined systems whose
right-hand sides are not polynomials, added the way the reference's own extension point asks for: a
subclass of systems.ODE with its _f_np (systems.py:23-61).

Development container only, like gen_poly.py (the reference tree and this script never travel to the
GPU box; only the .npz is committed):

    PYTHONPATH=tests:tests/golden/jaxshim:<reference tree> python tests/golden/gen_func.py

Every number written is computed by reference code (systems.ODE.get_vector_field, RK.py, solver.py,
parareal.py) with use_jax=False and NumPy's own sin / exp / log / sqrt and division.  The seven _f_np
below are written by hand from the equations, in vectorised NumPy, with the parameters of
tests/func_ref.py (which gives the same systems as atoms and rows); they share no code with
func_ref.FuncNP, which the fixture is there to check.  Together they use all six atom functions:
pendulum and Kuramoto and sine-Gordon sin, chemostat recip, Gompertz log, the tanks sqrt, Bratu exp --
and, as a seventh, the pendulum measured from the horizontal (`pendulum_cos`) for cos.
"""
import os
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

import systems as rsys          # noqa: E402  (reference)
import RK as rrk                # noqa: E402
import solver as rsolver        # noqa: E402
import parareal as rpara        # noqa: E402

import func_ref as FR           # noqa: E402  (the project's: parameters, initial conditions, test states)


def _base(name, **kwargs):
    S = FR.GOLDEN_SYSTEMS[name]()
    return (name, np.array(S['mn']), np.array(S['mx']), np.array(S['u0'])), kwargs


class Pendulum(rsys.ODE):
    def __init__(self, **kwargs):
        a, k = _base('pendulum', **kwargs)
        super().__init__(*a, **k)

    @staticmethod
    def _f_np(t, u):
        th, om = u
        return np.array([om, -np.sin(th) - 0.1 * om])


class PendulumCos(rsys.ODE):
    """the pendulum measured from the horizontal: omega' = -cos(theta - 1.25) - 0.1 omega"""

    def __init__(self, **kwargs):
        a, k = _base('pendulum_cos', **kwargs)
        super().__init__(*a, **k)

    @staticmethod
    def _f_np(t, u):
        th, om = u
        return np.array([om, -np.cos(th - 1.25) - 0.1 * om])


class Chemostat(rsys.ODE):
    def __init__(self, **kwargs):
        a, k = _base('chemostat', **kwargs)
        super().__init__(*a, **k)

    @staticmethod
    def _f_np(t, u):
        p = FR.CHEMO
        s, x = u
        growth = p['mu'] * s * x / (p['K'] + s)
        return np.array([p['D'] * (p['s0'] - s) - growth, p['Y'] * growth - p['D'] * x])


class GompertzTanks(rsys.ODE):
    def __init__(self, **kwargs):
        a, k = _base('gompertz', **kwargs)
        super().__init__(*a, **k)

    @staticmethod
    def _f_np(t, u):
        p = FR.GOMP
        x, h1, h2 = u
        return np.array([-p['r'] * x * np.log(x * p['invK']), p['q'] - p['k'] * np.sqrt(h1),
                         p['k'] * np.sqrt(h1) - p['k'] * np.sqrt(h2)])


class Kuramoto(rsys.ODE):
    def __init__(self, **kwargs):
        a, k = _base('kuramoto', **kwargs)
        super().__init__(*a, **k)

    @staticmethod
    def _f_np(t, u):
        s = np.sin(u[None, :] - u[:, None])          # s[i][j] = sin(theta_j - theta_i); the diagonal is 0
        return FR.kuramoto_omega() + (FR.KURA_K / FR.KURA_N) * np.sum(s, axis=1)


class SineGordon(rsys.ODE):
    LENGTH = 16.0

    def __init__(self, **kwargs):
        a, k = _base('sinegordon', **kwargs)
        super().__init__(*a, **k)

    @staticmethod
    def _f_np(t, w):
        n = w.shape[0] // 2
        u, v = w[:n], w[n:]
        c = 1.0 / (SineGordon.LENGTH / n) ** 2
        return np.concatenate([v, c * (np.roll(u, 1) - 2.0 * u + np.roll(u, -1)) - np.sin(u)])


class Bratu(rsys.ODE):
    def __init__(self, **kwargs):
        a, k = _base('bratu', **kwargs)
        super().__init__(*a, **k)

    @staticmethod
    def _f_np(t, u):
        d = u.shape[0]
        c = float((d + 1) ** 2)
        p = np.concatenate([[0.0], u, [0.0]])
        return c * (p[:-2] - 2.0 * u + p[2:]) + FR.BRATU_LAM * np.exp(u)


SYSTEMS = {'pendulum': Pendulum, 'pendulum_cos': PendulumCos, 'chemostat': Chemostat, 'gompertz': GompertzTanks, 'kuramoto': Kuramoto,
           'sinegordon': SineGordon, 'bratu': Bratu}
N_RHS, RK_STEPS = 16, 32


def make(key, norm):
    return SYSTEMS[key](use_jax=False, **(dict(normalization='-11') if norm else {}))


def check_ranges(key, U):
    """the issue's ranges: every atom argument within |x| <= 50, every log / sqrt / recip argument >= 0.05"""
    S = FR.GOLDEN_SYSTEMS[key]()
    for atom in S['atoms']:
        fn, (a, i), second, b = FR.parse_atom(atom)
        x = a * U[..., i]
        if second is not None:
            x = x + second[0] * U[..., second[1]]
        if b is not None:
            x = x + b
        assert np.all(np.abs(x) <= 50), (key, atom)
        if fn in ('log', 'sqrt', 'recip'):
            assert np.all(x >= 0.05), (key, atom, float(np.min(x)))


def part_rhs(arrs):
    for key in SYSTEMS:
        f = make(key, False).get_vector_field()
        U = FR.golden_states(key, N_RHS, 4321, False)
        check_ranges(key, U)
        arrs[f'rhs__{key}__u'] = U
        arrs[f'rhs__{key}__f'] = np.stack([np.asarray(f(0.0, u), dtype=float) for u in U])


def part_rk(arrs):
    for key in SYSTEMS:
        S = FR.GOLDEN_SYSTEMS[key]()
        f = make(key, False).get_vector_field()
        u0 = FR.golden_states(key, 1, 99, False)[0]
        t0, t1 = 0.0, RK_STEPS * S['dt']
        for tab in ('RK1', 'RK4', 'RK8'):
            r = rrk.RK(f, tab)
            k = f'rk__{key}__{tab}'
            arrs[k + '__u0'] = u0
            arrs[k + '__span'] = np.array([t0, t1, RK_STEPS], dtype=float)
            arrs[k + '__fixed'] = np.asarray(r.run_get_last(t0, t1, RK_STEPS, u0), dtype=float)
            traj = np.asarray(r.run(t0, t1, RK_STEPS, u0), dtype=float)
            check_ranges(key, traj)
            arrs[k + '__linspace'] = traj[-1]


def _final(u):
    cols = [c for c in range(u.shape[2]) if not np.any(np.isnan(u[:, :, c]))]
    return u[:, :, cols[-1]]


def part_para(arrs):
    """classic Parareal ('-11', F = RK4, G as func_ref.GOLDEN_PARA names it) and the serial fine solution at the slice boundaries"""
    for key, (T, N, Ng, Nf, G) in FR.GOLDEN_PARA.items():
        st = time.time()
        ode = make(key, True)
        s = rsolver.SolverRK(ode.get_vector_field(), Ng=Ng, Nf=Nf, F='RK4', G=G)
        res = rpara.Parareal(ode, s, tspan=[0, T], N=N, epsilon=5e-7, verbose=None).run(model='parareal')
        tag = f'para__{key}'
        arrs[tag + '__cfg'] = np.array([0, T, N, Ng, Nf, 5e-7, int(G[2:])])
        arrs[tag + '__k'] = np.array(res['k'])
        arrs[tag + '__conv_int'] = np.array(res['conv_int'])
        arrs[tag + '__final'] = _final(res['u'])
        arrs[tag + '__u0'] = ode.get_init_cond()
        r = rrk.RK(ode.get_vector_field(), 'RK4')
        t = np.linspace(0, T, N + 1)
        u = ode.get_init_cond()
        fine = [u]
        for i in range(N):
            u = np.asarray(r.run_get_last(t[i], t[i + 1], Nf, u), dtype=float)
            fine.append(u)
        arrs[tag + '__fine'] = np.array(fine)
        check_ranges(key, ode.normalizer.inverse(np.array(fine)))
        print('parareal', key, 'K=', res['k'], 'conv_int', list(res['conv_int']), 'final vs fine',
              float(np.max(np.abs(_final(res['u']) - np.array(fine)))), f'{time.time() - st:.1f}s', flush=True)


if __name__ == '__main__':
    arrs = {}
    for part in (part_rhs, part_rk, part_para):
        st = time.time()
        part(arrs)
        print(part.__name__, f'{time.time() - st:.1f}s', flush=True)
    path = os.path.join(HERE, 'func.npz')
    np.savez_compressed(path, **arrs)
    print('wrote', path, os.path.getsize(path), 'bytes', flush=True)
