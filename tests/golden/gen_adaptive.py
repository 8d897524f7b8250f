"""Generate tests/golden/adaptive.npz by running the REFERENCE's SolverScipy itself.

Development container only, like gen_golden.py (the reference tree and this script never travel to
the GPU box; only the .npz is committed):

    PYTHONPATH=tests/golden/jaxshim:<reference tree>:tests:oracle python tests/golden/gen_adaptive.py

For every case the end state is what the reference's SolverScipy.run_F returns (solver.py:138-145),
and nfev / the accepted-step count come from a direct solve_ivp call with the same arguments and no
t_eval.  The script walks a grid of candidate tolerances and step caps per system and method and
keeps, per class, the first candidate on which the restatement (tests/adaptive_ref.py) takes
exactly scipy's number of evaluations and accepted steps:
    max   every step is max_step (the reference's default use): no rejection and at most nf + 1
          steps, the one more being the selected initial step where that is shorter than max_step
          (the last step is then the remainder up to t1)
    rej   at least one rejected step
    clip  the controller, not the cap, sizes the steps (more than nf + 1 of them) and the last one
          is cut short by t1
It prints the largest relative end-state deviation of the restatement over the kept cases: ten
times that is the bound tests/test_adaptive_host.py asserts.
"""
import os
import sys

import numpy as np
from scipy.integrate import solve_ivp
from scipy.integrate._ivp.rk import RK23, RK45

HERE = os.path.dirname(os.path.abspath(__file__))

import systems as rsys          # noqa: E402  (reference)
import solver as rsolver        # noqa: E402

import adaptive_ref as AR       # noqa: E402  (tests/)
import oracle as O              # noqa: E402
from diffreact_ref import DiffReactNP   # noqa: E402

# name: (reference ODE, restated f(u), slice length)
SYSTEMS = {
    'lorenz': (lambda: rsys.Lorenz(normalization='-11'), lambda: O.System('lorenz').rhs, 0.5),
    'lorenz_id': (lambda: rsys.Lorenz(), lambda: O.System('lorenz', normalized=False).rhs, 0.5),
    'fhn_ode': (lambda: rsys.FHN_ODE(normalization='-11'), lambda: O.System('fhn_ode').rhs, 2.0),
    'brus': (lambda: rsys.Brusselator(normalization='-11'), lambda: O.System('brus').rhs, 2.0),
    'tomlab': (lambda: rsys.ThomasLabyrinth(normalization='-11'), lambda: O.System('tomlab').rhs, 0.5),
    'burgers16': (lambda: rsys.Burgers(d_x=16, normalization='-11'),
                  lambda: O.System('burgers', d=16, param=(0.01,), mn=0, mx=1).rhs, 0.5),
    'fhnpde4': (lambda: rsys.FHN_PDE(d_x=4), lambda: O.System('fhn_pde', nx=4, normalized=False).rhs, 6.0),
    'diffreact3': (lambda: rsys.DiffReact(d_x=3, use_jax=False), lambda: DiffReactNP(3), 6.0),
}
METHODS = {'RK23': ('RK2', RK23), 'RK45': ('RK4', RK45)}   # the reference's names (solver.py:130-135)
CANDIDATES = [(rtol, rtol * 1e-3, nf) for nf in (40, 12, 5, 2, 1, 400)
              for rtol in (1e-3, 1e-4, 1e-5, 1e-6, 1e-8, 1e-10)]
T0 = 0.25


def classify(cls, f, t0, t1, u0, nf, rtol, atol):
    """(rejections, class max, class clip) of scipy's own stepping"""
    s = cls(f, t0, u0, t1, max_step=(t1 - t0) / nf, rtol=rtol, atol=atol)
    steps, clipped = 0, False
    while s.status == 'running':
        want = min(s.h_abs, s.max_step)
        s.step()
        steps += 1
        clipped = s.h_previous < want * (1 - 1e-9)
    assert s.status == 'finished'
    n_stage = s.n_stages
    rej = (s.nfev - 2) // n_stage - steps
    return rej, (steps <= nf + 1 and rej == 0), (clipped and steps > nf + 1)


def main():
    arrs, worst, kept = {}, 0.0, []
    rng = np.random.default_rng(2024)
    for name, (make, make_f, length) in SYSTEMS.items():
        ode = make()
        f = ode.get_vector_field()
        fr = make_f()
        u0 = ode.get_init_cond()
        u0 = u0 + 1e-3 * rng.uniform(-1, 1, u0.shape)
        t0, t1 = T0, T0 + length
        for method, (ref_name, cls) in METHODS.items():
            found = {}
            for rtol, atol, nf in CANDIDATES:
                rej, is_max, clipped = classify(cls, f, t0, t1, u0, nf, rtol, atol)
                kinds = [k for k, ok in (('max', is_max), ('rej', rej > 0), ('clip', clipped)) if ok]
                kinds = [k for k in kinds if k not in found]
                if not kinds:
                    continue
                res = solve_ivp(f, [t0, t1], u0, method=method, max_step=(t1 - t0) / nf, rtol=rtol, atol=atol)
                s = rsolver.SolverScipy(f, Ng=1, Nf=nf, G='RK1', F=ref_name, rtol=rtol, atol=atol)
                y = np.asarray(s.run_F(t0, t1, u0), dtype=float)
                yr, nfev, acc, rrej, status = AR.solve(fr, method, t0, t1, nf, u0, rtol=rtol, atol=atol)
                if status != 0 or nfev != res.nfev or acc != len(res.t) - 1:
                    print(f'  drop {name} {method} rtol={rtol:g} nf={nf}: restatement {nfev}/{acc}, scipy '
                          f'{res.nfev}/{len(res.t) - 1}')
                    continue
                dev = float(np.max(np.abs(yr - y) / np.maximum(np.abs(y), 1e-300)))
                for k in kinds:
                    found[k] = True
                    key = f'{name}__{method}__{k}'
                    arrs[key + '__u0'] = u0
                    arrs[key + '__span'] = np.array([t0, t1, nf], dtype=float)
                    arrs[key + '__tol'] = np.array([rtol, atol])
                    arrs[key + '__y'] = y
                    arrs[key + '__counts'] = np.array([res.nfev, len(res.t) - 1, rej], dtype=np.int64)
                    kept.append(key)
                    worst = max(worst, dev)
                    print(f'{key}: rtol={rtol:g} nf={nf} nfev={res.nfev} accepted={len(res.t) - 1} rejected={rej} '
                          f'dev={dev:.3e}')
            missing = [k for k in ('max', 'rej', 'clip') if k not in found]
            if missing:
                print(f'  {name} {method}: no candidate for {missing}')
            assert 'rej' in found, (name, method)
    arrs['keys'] = np.array(kept)
    arrs['max_rel_dev'] = np.array(worst)
    path = os.path.join(HERE, 'adaptive.npz')
    np.savez_compressed(path, **arrs)
    print(f'{len(kept)} cases, largest relative end-state deviation of the restatement: {worst:.3e}')
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    sys.exit(main())
