"""Generate tests/golden/nntype.npz by running the REFERENCE's NNGP_alt (the nntype variants of
nnGPara_with_time.py) under the reference's own Parareal driver.

Development container only, like gen_knnmean.py (the reference tree and this script never travel to
the GPU box; only the .npz is committed):

    PYTHONPATH=tests/golden/jaxshim:<reference tree> python tests/golden/gen_nntype.py

nnGPara_with_time.py defines NNGP_alt inside an `if False:` block and unpickles results at module
scope, so it cannot be imported: the class node is found by walking the `ast` and executed over the
reference's modern models.NNGP_p.  Its predict calls get_preds with four arguments (it predates the
parent's fifth, the interval); a subclass here passes the interval on and records the selected xm.
Nothing of the reference is written out, only arrays: every number is computed by reference code.

Configuration: gen_knnmean.py's -- Rossler '-11', tspan [0, 10], N = 10, Ng = 50 RK1, Nf = 500 RK4,
eps 5e-7 -- with nn = 6.  Per nntype T:
  T__data_x    [N][n][K]   the table of starting values (NaN: converged)
  T__k, T__conv_int, T__u  the run's K, converged-interval counts and iterates
  T__ki        [P][2]      (iteration, interval) of every prediction, in call order
  T__len       [P]         neighbours of each prediction
  T__cells     [sum len][2] their cells (interval, iteration), found by exact row match in data_x;
                            -1, -1 where a row matches no cell or more than one
"""
import ast
import os
import sys
import time

import numpy as np
import scipy
import scipy.spatial

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

import systems as rsys          # noqa: E402  (reference)
import solver as rsolver        # noqa: E402
import models as rmodels        # noqa: E402
import parareal as rpara        # noqa: E402

NNTYPES = ('nn', 'col+rnd', 'col_only', 'row_col', 'row', 'col_full')
CFG = dict(tspan=[0, 10], N=10, Ng=50, Nf=500, G='RK1', F='RK4', eps=5e-7, nn=6)


def alt_class():
    with open(os.path.join(os.path.dirname(rpara.__file__), 'nnGPara_with_time.py')) as f:
        tree = ast.parse(f.read())
    node = next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == 'NNGP_alt')
    ns = dict(np=np, scipy=scipy, NNGP_p=rmodels.NNGP_p)
    exec(compile(ast.Module(body=[node], type_ignores=[]), 'nnGPara_with_time', 'exec'), ns)
    Alt = ns['NNGP_alt']

    class Recording(Alt):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.recorded = []

        def get_preds(self, xm, ym, n, new_x, intrvl_i=None):
            self.recorded.append((self.k, self.i, np.array(xm, dtype=float)))
            return super().get_preds(xm, ym, n, new_x, self.i)

    return Recording


def cells_of(xm, data_x, k):
    out = []
    for row in xm:
        hit = np.argwhere(np.all(data_x[:, :, :k + 1] == row[None, :, None], axis=1))
        out.append(hit[0] if len(hit) == 1 else (-1, -1))
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def run(Alt, nntype, arrs):
    ode = rsys.Rossler(normalization='-11')
    s = rsolver.SolverRK(ode.get_vector_field(), Ng=CFG['Ng'], Nf=CFG['Nf'], F=CFG['F'], G=CFG['G'])
    p = rpara.Parareal(ode, s, CFG['tspan'], CFG['N'], epsilon=CFG['eps'], verbose=None)
    mdl = Alt(n=ode.get_dim(), N=CFG['N'], worker_pool=rpara.MyPool(), nntype=nntype, nn=CFG['nn'])
    st = time.time()
    r = p._parareal(mdl, pool=rpara.MyPool())
    print(nntype, 'K=', r['k'], 'conv_int=', list(r['conv_int']), f'{time.time() - st:.1f}s', flush=True)
    data_x = np.asarray(r['data_x'], dtype=float)
    arrs[f'{nntype}__data_x'] = data_x
    arrs[f'{nntype}__k'] = np.array(r['k'])
    arrs[f'{nntype}__conv_int'] = np.array(r['conv_int'])
    arrs[f'{nntype}__u'] = np.asarray(r['u'], dtype=float)
    arrs[f'{nntype}__ki'] = np.array([(k, i) for k, i, _ in mdl.recorded], dtype=np.int64).reshape(-1, 2)
    arrs[f'{nntype}__len'] = np.array([len(xm) for _, _, xm in mdl.recorded], dtype=np.int64)
    full = np.asarray(mdl.data_x, dtype=float)   # the driver's whole table (the result's is cut at K)
    arrs[f'{nntype}__cells'] = np.concatenate([cells_of(xm, full, k) for k, _, xm in mdl.recorded])
    return ode


if __name__ == '__main__':
    Alt = alt_class()
    arrs = {}
    for t in NNTYPES:
        ode = run(Alt, t, arrs)
    arrs['cfg'] = np.array([CFG['tspan'][0], CFG['tspan'][1], CFG['N'], CFG['Ng'], CFG['Nf'], CFG['eps'], CFG['nn']])
    arrs['u0'] = np.asarray(ode.get_init_cond(), dtype=float)
    path = os.path.join(HERE, 'nntype.npz')
    np.savez_compressed(path, **arrs)
    print('wrote', path, os.path.getsize(path), 'bytes', flush=True)
