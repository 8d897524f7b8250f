"""Generate tests/golden/burgers_sizes.npz by running the REFERENCE's Burgers system itself at the
sizes that rhs.npz / rk.npz (d = 16, 128) do not cover.

Development container only, like gen_golden.py and gen_diffreact.py (the reference tree and this
script never travel to the GPU box; only the .npz is committed):

    PYTHONPATH=tests/golden/jaxshim:<reference tree> python tests/golden/gen_burgers_sizes.py

Every number written is computed by reference code (systems.py:402-459 Burgers: the dense Dxx / Dx
matrices; RK.py) with use_jax=False; this script only chooses inputs and records outputs.

Sizes: 3 (every row touches the wrap-around), 5, 64 / 192 / 256 (the wave kernel's 1, 3 and 4
elements per lane), 65 and 300 (LDS field kernel, no multiple of 16); identity and '-11'.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

import systems as rsys          # noqa: E402  (reference)
import RK as rrk                # noqa: E402

SIZES = (3, 5, 64, 65, 192, 256, 300)
STEPS = 5


def step(d, nu=0.01):
    dx = 2.0 / (d - 1)
    return min(0.1 * dx * dx / nu, 0.1 * dx)


if __name__ == '__main__':
    arrs = {}
    rng = np.random.default_rng(4242)
    for d in SIZES:
        for norm in (False, True):
            ode = rsys.Burgers(d_x=d, use_jax=False, **(dict(normalization='-11') if norm else {}))
            f = ode.get_vector_field()
            tag = f'{d}{"_n" if norm else ""}'
            U = np.stack([ode.get_init_cond(), rng.uniform(-0.9, 0.9, d), rng.uniform(-0.9, 0.9, d)])
            arrs[f'rhs__{tag}__u'] = U
            arrs[f'rhs__{tag}__f'] = np.stack([np.asarray(f(0.0, u), dtype=float) for u in U])
            u0 = ode.get_init_cond() + rng.uniform(-0.02, 0.02, size=d)
            t0, t1 = 0.0, STEPS * step(d)
            for tab in ('RK1', 'RK4', 'RK8'):
                r = rrk.RK(f, tab)
                key = f'rk__{tag}__{tab}'
                arrs[key + '__u0'] = u0
                arrs[key + '__span'] = np.array([t0, t1, STEPS], dtype=float)
                arrs[key + '__fixed'] = np.asarray(r.run_get_last(t0, t1, STEPS, u0), dtype=float)
                arrs[key + '__linspace'] = np.asarray(r.run(t0, t1, STEPS, u0), dtype=float)[-1]
    path = os.path.join(HERE, 'burgers_sizes.npz')
    np.savez_compressed(path, **arrs)
    print('wrote', path, os.path.getsize(path), 'bytes', flush=True)
