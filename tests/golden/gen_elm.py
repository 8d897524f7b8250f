"""Generate tests/golden/elm.npz and tests/golden/elm_wide.npz by running the REFERENCE's ELM model
itself.

Development container only, like gen_diffreact.py (the reference tree and this script never travel
to the GPU box; only the .npz files are committed):

    PYTHONPATH=tests/golden/jaxshim:<reference tree> python tests/golden/gen_elm.py          # elm.npz
    PYTHONPATH=tests/golden/jaxshim:<reference tree> python tests/golden/gen_elm.py wide     # elm_wide.npz

Each invocation writes one fixture and leaves the other alone.  elm_wide.npz holds predictions only,
at wide hidden layers: the reference's default res_size = 500 at degree 2, and two degree-1 sets, one
with more hidden units than m - 1 can use up (200) and one nearer to it (100), at m up to 16.

Every number written is computed by reference code (models.py:476-554 ELM_base / ELM, parareal.py,
solver.py, systems.py) or, for the recorded condition numbers, by numpy on the reference's own
hidden features; this script only chooses inputs and records outputs.
"""
import os
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

import systems as rsys          # noqa: E402  (reference)
import solver as rsolver        # noqa: E402
import models as rmodels        # noqa: E402
import parareal as rpara        # noqa: E402

warnings.filterwarnings('ignore')   # Ridge(alpha=0) on a singular centred Gram warns on every fit

WEIGHTS = ((2, 20, 2), (3, 20, 2), (3, 7, 1), (16, 50, 2))   # (d, res_size, degree)
MS = (1, 2, 4, 7)
N_CASES, N_TRAIN = 10, 20
WIDE_WEIGHTS = ((3, 500, 2), (16, 200, 1), (3, 100, 1))   # elm_wide.npz
WIDE_MS = (5, 10, 16)
WIDE_N_TRAIN = 40


def gram_cond(mdl, xm):
    """Condition number of the non-null part of the centred Gram of the m neighbours' hidden rows
    (what Ridge(alpha=0).fit solves): centring removes one rank, so the m-1 largest eigenvalues."""
    X = mdl.loss(mdl.bias + (mdl.R * mdl.C) @ mdl.poly.fit_transform(xm).T).T
    Xc = X - X.mean(0)
    ev = np.sort(np.linalg.eigvalsh(Xc @ Xc.T))[::-1][:max(xm.shape[0] - 1, 0)]
    if len(ev) == 0:
        return 1.0
    return float(ev[0] / ev[-1]) if ev[-1] > 0 else np.inf


def part_predict(arrs, weights=WEIGHTS, ms=MS, n_train=N_TRAIN, seed0=1000):
    for d, res, deg in weights:
        tag = f'w__{d}_{res}_{deg}'
        rng = np.random.default_rng(seed0 + 10 * d + deg)
        X = rng.uniform(-1, 1, (N_CASES, n_train, d))
        Y = rng.uniform(-1, 1, (N_CASES, n_train, d))
        Q = rng.uniform(-1, 1, (N_CASES, d))
        arrs[tag + '__X'], arrs[tag + '__Y'], arrs[tag + '__Q'] = X, Y, Q
        for m in ms:
            mdl = rmodels.ELM_base(d=d, seed=47, res_size=res, degree=deg, m=m)
            arrs[tag + '__bias'], arrs[tag + '__C'] = mdl.bias, mdl.C
            preds, conds = [], []
            for c in range(N_CASES):
                p = mdl.fit_predict(X[c], Y[c], Q[c][None, :], 0)
                preds.append(np.asarray(p, dtype=float).reshape(d))
                s_idx = np.argsort(((X[c] - Q[c]) ** 2).sum(1))[:m]
                conds.append(gram_cond(mdl, X[c][s_idx]))
            arrs[tag + f'__pred_m{m}'] = np.array(preds)
            arrs[tag + f'__cond_m{m}'] = np.array(conds)


def part_runs(arrs):
    """The two whole runs at the ELM defaults ('-11', eps 5e-7), and classic Parareal's K."""
    runs = {'lorenz': (rsys.Lorenz(normalization='-11'), dict(Ng=6, Nf=450, F='RK4', G='RK4'), [0, 18], 32),
            'fhn_ode': (rsys.FHN_ODE(normalization='-11'), dict(Ng=4, Nf=400, F='RK4', G='RK2'), [0, 40], 40)}
    for name, (ode, skw, tspan, N) in runs.items():
        s = rsolver.SolverRK(ode.get_vector_field(), **skw)
        for model in ('elm', 'parareal'):
            p = rpara.Parareal(ode, s, tspan=tspan, N=N, epsilon=5e-7, verbose=None)
            st = time.time()
            res = p.run(model=model)
            print(name, model, 'K=', res['k'], f'{time.time() - st:.1f}s', flush=True)
            tag = f'run__{name}__{model}'
            arrs[tag + '__k'] = np.array(res['k'])
            if model == 'elm':
                arrs[tag + '__cfg'] = np.array([tspan[0], tspan[1], N, skw['Ng'], skw['Nf'], 5e-7])
                arrs[tag + '__conv_int'] = np.array(res['conv_int'])
                arrs[tag + '__u'] = np.asarray(res['u'])[:, :, :3]


def part_predict_wide(arrs):
    """The same quantities as part_predict at the wide weight sets (seeds 2000 + 10 d + degree)."""
    part_predict(arrs, WIDE_WEIGHTS, WIDE_MS, WIDE_N_TRAIN, 2000)


if __name__ == '__main__':
    import sys
    wide = sys.argv[1:] == ['wide']
    if sys.argv[1:] and not wide:
        raise SystemExit('usage: gen_elm.py [wide]')
    arrs = {}
    for part in ((part_predict_wide,) if wide else (part_predict, part_runs)):
        st = time.time()
        part(arrs)
        print(part.__name__, f'{time.time() - st:.1f}s', flush=True)
    path = os.path.join(HERE, 'elm_wide.npz' if wide else 'elm.npz')
    np.savez_compressed(path, **arrs)
    print('wrote', path, os.path.getsize(path), 'bytes', flush=True)
