"""Generate tests/golden/knnmean.npz by running the REFERENCE's k-NN Parareal model and its
Figure 2 comparison loop themselves.

Development container only, like gen_adaptive.py (the reference tree and this script never travel
to the GPU box; only the .npz is committed):

    PYTHONPATH=tests/golden/jaxshim:<reference tree> python tests/golden/gen_knnmean.py

Figure_2.py runs and plots at module scope, so it cannot be imported: its class definitions NN and
Paramod are taken with `ast` and executed in a namespace holding the reference's Parareal,
ModelAbstr, SolverAbstr, numpy, scipy, time, os and a do-nothing plt.  Nothing of the reference is
written out, only arrays: every number is computed by reference code, this script only chooses
inputs and records outputs -- except `max_abs_dev`, the largest |10**e_ref - 10**e_restated| over the
comparison lists of group (b), where e_restated comes from tests/knnmean_ref.py's loop.

Groups:
  a__*   seeded predict cases (X, Y, q, nn) and the reference NN.predict output
  b__*   the comparison run: Rossler '-11', tspan [0, 10], N = 10, Ng = 50 RK1, Nf = 500 RK4,
         eps 5e-7, driver 'parareal', comp_mdls = NN(nn = 1, 2, 4, 10), debug=True
  c__*   the same configuration driven by NN(nn=3)
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

PRED_D, PRED_NN, PRED_ROWS = (2, 3, 33), (1, 2, 8, 9, 30, 64), (5, 40, 300)
COMP_NN = (1, 2, 4, 10)
CFG = dict(tspan=[0, 10], N=10, Ng=50, Nf=500, G='RK1', F='RK4', eps=5e-7)


class _Ax:
    def __getattr__(self, k):
        return lambda *a, **kw: None


class _Plt:
    def subplots(self, *a, **kw):
        return _Ax(), _Ax()


def figure2_classes():
    with open(os.path.join(os.path.dirname(rpara.__file__), 'Figure_2.py')) as f:
        tree = ast.parse(f.read())
    nodes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in ('Paramod', 'NN')]
    ns = dict(np=np, scipy=scipy, time=time, os=os, plt=_Plt(), Parareal=rpara.Parareal,
              ModelAbstr=rmodels.ModelAbstr, SolverAbstr=rsolver.SolverAbstr)
    exec(compile(ast.Module(body=nodes, type_ignores=[]), 'fig2', 'exec'), ns)
    return ns['Paramod'], ns['NN']


def part_predict(arrs, NN):
    for d in PRED_D:
        for rows in PRED_ROWS:
            rng = np.random.default_rng(7000 + 100 * d + rows)
            X = rng.standard_normal((rows, d))
            Y = 0.01 * np.sin(3 * X) + 1e-4 * rng.standard_normal((rows, d))
            q = X[rows // 2] + 1e-2 * rng.standard_normal(d)
            tag = f'a__d{d}_r{rows}'
            arrs[tag + '__X'], arrs[tag + '__Y'], arrs[tag + '__q'] = X, Y, q
            for nn in PRED_NN:
                mdl = NN(N=4, nn=nn)
                mdl.fit(X, Y, 0, data_x=None, data_y=None)
                arrs[tag + f'__pred_nn{nn}'] = np.asarray(mdl.predict(q[None, :], None, None, i=0), dtype=float)


def setup(Paramod):
    ode = rsys.Rossler(normalization='-11')
    s = rsolver.SolverRK(ode.get_vector_field(), Ng=CFG['Ng'], Nf=CFG['Nf'], F=CFG['F'], G=CFG['G'])
    return ode, Paramod(ode, s, CFG['tspan'], CFG['N'], epsilon=CFG['eps'], verbose=None)


def part_compare(arrs, Paramod, NN):
    ode, p = setup(Paramod)
    N = CFG['N']
    st = time.time()
    r = p.run(comp_mdls=[NN(N=N, nn=k) for k in COMP_NN], debug=True)
    print('compare run K=', r['k'], f'{time.time() - st:.1f}s', flush=True)
    arrs['cfg'] = np.array([CFG['tspan'][0], CFG['tspan'][1], N, CFG['Ng'], CFG['Nf'], CFG['eps']])
    arrs['u0'] = np.asarray(ode.get_init_cond(), dtype=float)
    arrs['b__k'] = np.array(r['k'])
    arrs['b__conv_int'] = np.array(r['conv_int'])
    arrs['b__u'] = np.asarray(r['u'])
    names = [f'{k}-NN' for k in COMP_NN] + ['para']
    for name in names:
        its = sorted(r['err_store_mdls'][name])
        arrs[f'b__iters__{name}'] = np.array(its)
        for k in its:
            arrs[f'b__err__{name}__{k}'] = np.array(r['err_store_mdls'][name][k], dtype=float)
    # the restated loop against the reference's lists
    sys.path[:0] = [os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle')]
    import oracle as O
    import knnmean_ref as KR
    so = O.System('rossler')
    o = KR.parareal_compare(so, CFG['tspan'], N, CFG['Ng'], CFG['Nf'], CFG['G'], CFG['F'], epsilon=CFG['eps'],
                            u0=arrs['u0'], model='parareal', comp=[KR.NNRef(k) for k in COMP_NN], debug=True)
    assert o['k'] == r['k'] and o['conv_int'] == list(r['conv_int']), (o['k'], r['k'])
    dev = 0.0
    for name in names:
        for k in r['err_store_mdls'][name]:
            a = np.array(r['err_store_mdls'][name][k], dtype=float)
            b = np.array(o['err_store_mdls'][name][k], dtype=float)
            assert a.shape == b.shape, (name, k)
            dev = max(dev, float(np.max(np.abs(10.0 ** a - 10.0 ** b))) if a.size else 0.0)
    print('max_abs_dev', dev, flush=True)
    arrs['max_abs_dev'] = np.array(dev)


def part_driver(arrs, Paramod, NN):
    _, p = setup(Paramod)
    st = time.time()
    r = p._parareal(NN(N=CFG['N'], nn=3), pool=rpara.MyPool())
    print('nn=3 driver K=', r['k'], f'{time.time() - st:.1f}s', flush=True)
    arrs['c__k'] = np.array(r['k'])
    arrs['c__conv_int'] = np.array(r['conv_int'])
    arrs['c__u'] = np.asarray(r['u'])


if __name__ == '__main__':
    Paramod, NN = figure2_classes()
    arrs = {}
    part_predict(arrs, NN)
    part_compare(arrs, Paramod, NN)
    part_driver(arrs, Paramod, NN)
    path = os.path.join(HERE, 'knnmean.npz')
    np.savez_compressed(path, **arrs)
    print('wrote', path, os.path.getsize(path), 'bytes', flush=True)
